"""The hipGraph replay rules (engine.hip_step.GraphReplay), checked on CPU.

``torch.cuda.CUDAGraph`` / ``torch.cuda.graph`` are replaced by fakes: what
a recording extension sees launched inside the ``with`` block is the graph,
and ``replay()`` launches it again.  A fused step and the data-parallel
trainer over it are then driven through batch-size changes (and, for
BatchTopK, a replaced buffer tree) and every call is classified as eager,
captured (capture + first replay) or replayed."""

import tempfile

import pytest
import torch
import torch.distributed as dist

from tests import test_hip_step_trace as T
from tests.test_batch_topk_cpu import RecordingExt as BatchTopKExt
from tests.test_batch_topk_cpu import _ensemble as _btk_ensemble

# (batch size, repeats) and what each call must be
SEQUENCE = [(64, 4), (60, 3), (64, 3)]
EXPECTED = ["eager", "eager", "captured", "replayed",
            "eager", "eager", "captured",
            "eager", "eager", "captured"]


class FakeGraphs:
    """Stand-ins for torch.cuda.CUDAGraph / graph / synchronize."""

    def __init__(self, monkeypatch, ext, fail=False):
        self.events = []
        fakes = self

        class Graph:
            launches = None

            def replay(self):
                assert self.launches, "replay of a graph that captured nothing"
                fakes.events.append("replay")
                ext.calls.extend(self.launches)

        class capture:
            def __init__(self, g):
                self.g = g

            def __enter__(self):
                if fail:
                    raise RuntimeError("no capture today")
                fakes.events.append("capture")
                self.start = len(ext.calls)

            def __exit__(self, *exc):
                self.g.launches = ext.calls[self.start:]
                del ext.calls[self.start:]  # capture does not execute

        monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
        monkeypatch.setattr(torch.cuda, "graph", capture)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)

    def classify(self, call):
        """Run call(); eager / captured / replayed from the graph events."""
        self.events.clear()
        call()
        return {(): "eager", ("capture", "replay"): "captured", ("replay",): "replayed"}[tuple(self.events)]


def _step(kind):
    from sparse_coding_amd.engine import hip_step as hs
    from sparse_coding_amd.models.batch_topk import BatchTopKEncoder

    torch.manual_seed(0)
    if kind == "tied":
        sig, models, make = T._targets()["tied"]
        ens, ext = T._ensemble(sig, models()), T.RecordingExt()
    else:
        ens = _btk_ensemble([BatchTopKEncoder.init(T.D, T.N, k) for k in (4, 8)], no_stacking=True)
        ext, make = BatchTopKExt(), hs.HipBatchTopKStep
    step = make(ens, ext)
    ext.step = step
    ext.x = torch.randn(64, T.D)
    ens._hip_step = step
    return ens, step, ext


def _drive(fakes, ext, call):
    """The outcome of every call of SEQUENCE; each must launch a whole step."""
    got, per_step = [], None
    for B, times in SEQUENCE:
        for _ in range(times):
            before = len(ext.calls)
            got.append(fakes.classify(lambda: call(torch.randn(B, T.D))))
            per_step = per_step or len(ext.calls) - before
            assert len(ext.calls) - before == per_step > 0, (B, got)
    return got


@pytest.mark.parametrize("kind", ["tied", "batch_topk"])
def test_step_graph_rules(kind, monkeypatch):
    monkeypatch.delenv("SPARSE_CODING_AMD_NO_GRAPH", raising=False)
    ens, step, ext = _step(kind)
    fakes = FakeGraphs(monkeypatch, ext)
    assert step.use_graph
    assert _drive(fakes, ext, step.step) == EXPECTED
    assert step._graph is not None
    if kind == "batch_topk":
        # a replaced buffer tree drops the graph but keeps the eager count:
        # the next step captures again at once, on the new buffers
        ens.buffers = {k: v.clone() for k, v in ens.buffers.items()}
        assert fakes.classify(lambda: step.step(torch.randn(64, T.D))) == "captured"
        assert fakes.classify(lambda: step.step(torch.randn(64, T.D))) == "replayed"


@pytest.mark.parametrize("kind", ["tied", "batch_topk"])
def test_no_graph_env_keeps_every_call_eager(kind, monkeypatch):
    monkeypatch.setenv("SPARSE_CODING_AMD_NO_GRAPH", "1")
    _, step, ext = _step(kind)
    fakes = FakeGraphs(monkeypatch, ext)
    assert not step.use_graph
    assert _drive(fakes, ext, step.step) == ["eager"] * len(EXPECTED)
    assert step._graph is None


def test_failed_capture_disables_capture_for_good(monkeypatch, capsys):
    monkeypatch.delenv("SPARSE_CODING_AMD_NO_GRAPH", raising=False)
    _, step, ext = _step("tied")
    fakes = FakeGraphs(monkeypatch, ext, fail=True)
    assert _drive(fakes, ext, step.step) == ["eager"] * len(EXPECTED)
    assert not step.use_graph and step._graph is None
    assert capsys.readouterr().out.count("hipGraph capture failed (no capture today); staying eager") == 1


@pytest.fixture
def one_rank_group():
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{tmp}/store", rank=0, world_size=1)
        try:
            yield
        finally:
            dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["tied", "batch_topk"])
def test_trainer_graph_follows_the_steps_rules(kind, monkeypatch, one_rank_group):
    """The trainer's graph over the DP body: same sequence, same outcome, and
    it goes when the step's key changes (BatchTopK's replaced buffer tree)."""
    from sparse_coding_amd.parallel.dp import DataParallelEnsembleTrainer

    ens, step, ext = _step(kind)
    fakes = FakeGraphs(monkeypatch, ext)
    trainer = DataParallelEnsembleTrainer(ens, force_dp_path=True, graph_capture=True)
    trainer._replay.enabled = True  # graph_capture engages on a GPU only: forced on for the fakes
    assert _drive(fakes, ext, trainer.step) == EXPECTED
    assert trainer._graph is not None and step._graph is None
    if kind == "batch_topk":
        ens.buffers = {k: v.clone() for k, v in ens.buffers.items()}
        assert fakes.classify(lambda: trainer.step(torch.randn(64, T.D))) == "captured"


def test_trainer_stays_eager_without_graph_capture(monkeypatch, one_rank_group):
    from sparse_coding_amd.parallel.dp import DataParallelEnsembleTrainer

    monkeypatch.delenv("SC_AMD_DP_GRAPH", raising=False)
    ens, step, ext = _step("tied")
    fakes = FakeGraphs(monkeypatch, ext)
    trainer = DataParallelEnsembleTrainer(ens, force_dp_path=True)
    assert _drive(fakes, ext, trainer.step) == ["eager"] * len(EXPECTED)

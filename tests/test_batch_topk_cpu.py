"""BatchTopK on the CPU: the oracle signature against the helper reference,
the comparator against injected selection faults, the inference-threshold
recursion, the torch backend's buffer hook, the eval dict, the fused step's
launch trace under a recording stand-in for the extension, and the sweep
entry points."""

import copy
import io
import pickle
from contextlib import redirect_stdout

import pytest
import torch

from tests import batch_topk_reference as BR
from tests import test_hip_step_trace as T
from tests.hip_reference import Mismatch

from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models.batch_topk import BatchTopKEncoder, BatchTopKLearnedDict

M, B, D, N = 2, 256, 64, 128
KS = (4, 16)


def _normed(W):
    return W / torch.norm(W, dim=-1)[:, None]


@pytest.fixture(scope="module")
def case():
    """The step test's inputs (seed 11): scores, reference selection."""
    torch.manual_seed(11)
    models = [BatchTopKEncoder.init(D, N, k) for k in KS]
    x = torch.randn(B, D)
    W = torch.stack([p["dict"] for p, _ in models])
    s = torch.stack([x @ _normed(W[m]).T for m in range(M)])
    c, fired, t = BR.batch_topk_ref(s, KS)
    return {"models": models, "x": x, "s": s, "c": c, "fired": fired, "t": t}


def test_case_shows_batch_level_selection(case):
    """What the issue states about the seed-11 case: exactly k*B kept per
    model, per-row counts that vary, no exact ties, and the same selection
    from fp64 scores."""
    W = torch.stack([p["dict"] for p, _ in case["models"]]).double()
    for m, k in enumerate(KS):
        kept = case["c"][m] > 0
        assert int(kept.sum()) == k * B
        rows = kept.sum(dim=1)
        assert rows.min() < k < rows.max()
        assert int((case["s"][m] == case["t"][m]).sum()) == 1  # no tie at t
        s64 = case["x"].double() @ _normed(W[m]).T
        t64 = torch.topk(s64.flatten(), k * B).values[-1]
        assert torch.equal((s64 >= t64) & (s64 > 0), kept)


def test_oracle_signature_matches_reference(case):
    for m, (params, buffers) in enumerate(case["models"]):
        loss, (ld, aux) = BatchTopKEncoder.loss(params, buffers, case["x"])
        BR.check_batch_topk(f"oracle[{m}]", case["s"][m:m + 1], aux["c"][None],
                            (aux["c"] > 0).float().sum(dim=0)[None], aux["threshold"][None], KS[m:m + 1])
        x_hat = case["c"][m] @ _normed(params["dict"])
        assert torch.allclose(loss, (case["x"] - x_hat).pow(2).mean(), rtol=1e-6, atol=0)
        assert set(aux) == {"c", "threshold"} and set(ld) == {"loss"}


def test_oracle_gradient_flows_through_kept_entries_only(case):
    """d loss / d scores is zero wherever c is zero: t is a constant."""
    params, buffers = case["models"][0]
    normed = _normed(params["dict"])
    s = (case["x"] @ normed.T).requires_grad_(True)
    K = KS[0] * B
    t = torch.topk(s.detach().flatten(), K).values[-1]
    c = torch.where((s >= t) & (s > 0), s, torch.zeros_like(s))
    ((c @ normed - case["x"]) ** 2).mean().backward()
    assert (s.grad[case["c"][0] == 0] == 0).all()
    assert (s.grad[case["c"][0] > 0] != 0).any()


def test_comparator_accepts_reference_and_k_edges(case):
    BR.check_batch_topk("ref", case["s"], case["c"], case["fired"], case["t"], KS)
    s = case["s"]
    c, fired, t = BR.batch_topk_ref(s, (0, N + 3))
    assert (c[0] == 0).all() and t[0] == float("inf")
    assert torch.equal(c[1] != 0, s[1] > 0)  # K = B*n: every positive score
    assert t[1] == s[1].min()
    BR.check_batch_topk("edges", s, c, fired, t, (0, N + 3))


def _per_row(s, ks):
    c = torch.zeros_like(s)
    for m, k in enumerate(ks):
        vals, idx = torch.topk(s[m], k, dim=-1)
        c[m].scatter_(-1, idx, torch.clamp(vals, min=0.0))
    return c


def _per_slice(s, ks, n_slices=4):
    """Each quarter of the flattened matrix thresholds at its own K/4-th
    value: a select whose blocks never combined their histograms."""
    c = torch.zeros_like(s)
    for m, k in enumerate(ks):
        flat = s[m].flatten()
        out = torch.zeros_like(flat)
        step = flat.numel() // n_slices
        for i in range(n_slices):
            part = flat[i * step:(i + 1) * step]
            t = torch.topk(part, k * s.shape[1] // n_slices).values[-1]
            out[i * step:(i + 1) * step] = torch.where((part >= t) & (part > 0), part, torch.zeros_like(part))
        c[m] = out.view_as(s[m])
    return c


def test_comparator_rejects_injected_faults(case):
    s, c, t = case["s"], case["c"], case["t"]
    count = lambda c_: (c_ > 0).float().sum(dim=1)

    bad = _per_row(s, KS)
    assert not torch.equal(bad, c)
    with pytest.raises(Mismatch, match="c"):
        BR.check_batch_topk("per-row", s, bad, count(bad), t, KS)

    bad = _per_slice(s, KS)
    assert (bad > 0).sum() == (c > 0).sum() and not torch.equal(bad, c)
    with pytest.raises(Mismatch, match="c"):
        BR.check_batch_topk("per-slice", s, bad, count(bad), t, KS)

    # a selected value off by one ulp
    bad = c.clone()
    idx = tuple(int(i) for i in (c > 0).nonzero()[7])
    bad[idx] = torch.nextafter(bad[idx], torch.tensor(float("inf")))
    with pytest.raises(Mismatch, match="c"):
        BR.check_batch_topk("ulp", s, bad, count(bad), t, KS)

    # fired counted from S > 0 instead of c > 0
    with pytest.raises(Mismatch, match="fired"):
        BR.check_batch_topk("fired", s, c, count(s), t, KS)

    # t of the neighbouring rank
    bad_t = t.clone()
    bad_t[1] = torch.topk(s[1].flatten(), KS[1] * B + 1).values[-1]
    with pytest.raises(Mismatch, match="t"):
        BR.check_batch_topk("t", s, c, case["fired"], bad_t, KS)


def test_comparator_rejects_a_dropped_tie():
    """Scores from five positive values: hundreds tie at t, all are kept (more
    than K), and dropping one of them is a mismatch."""
    gen = torch.Generator().manual_seed(5)
    vals = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])
    s = vals[torch.randint(0, 5, (1, 64, 100), generator=gen)]
    ks = (20,)
    c, fired, t = BR.batch_topk_ref(s, ks)
    ties = (s[0] == t[0]).sum()
    assert ties > 200 and (c > 0).sum() > 20 * 64
    BR.check_batch_topk("ties", s, c, fired, t, ks)
    bad = c.clone()
    idx = tuple(int(i) for i in (s == t[0]).nonzero()[3])
    bad[idx] = 0.0
    with pytest.raises(Mismatch):
        BR.check_batch_topk("tie dropped", s, bad, (bad > 0).float().sum(dim=1), t, ks)


def test_reference_t_orders_the_two_zeros():
    s = torch.tensor([[[-1.0, -0.0, 0.0, -0.0]]])
    for k, want in ((1, 0.0), (2, -0.0), (3, -0.0), (4, -1.0)):
        c, _, t = BR.batch_topk_ref(s, (k,))
        assert t.view(torch.int32).item() == torch.tensor(want).view(torch.int32).item()
        assert (c == 0).all()


# ---------------------------------------------------------------------------
# the inference threshold
# ---------------------------------------------------------------------------

def _buffers(ks, lr=0.01):
    bufs = [BatchTopKEncoder.init(4, 8, k, threshold_lr=lr)[1] for k in ks]
    return {k: torch.stack([b[k] for b in bufs]) for k in bufs[0]}


def test_threshold_recursion():
    """First step copies max(t, 0); later steps move by threshold_lr; K == 0
    (t = +inf) leaves value and count alone."""
    b = _buffers((3, 0, 5), lr=0.25)
    ts = [torch.tensor([2.0, float("inf"), -1.0]),
          torch.tensor([4.0, float("inf"), 3.0]),
          torch.tensor([-2.0, float("inf"), 1.0])]
    want = [[0.0, 0], [0.0, 0], [0.0, 0]]
    for t in ts:
        BatchTopKEncoder.update_buffers(b, {"threshold": t})
        for m in (0, 2):
            want[m] = list(BR.theta_ref(want[m][0], want[m][1], max(float(t[m]), 0.0), 0.25))
        for m in range(3):
            assert b["threshold"][m].item() == pytest.approx(want[m][0], rel=1e-6, abs=0)
            assert b["threshold_n"][m].item() == want[m][1]
    assert b["threshold"].tolist() == [2.0 + 0.25 * 2.0 - 0.25 * 2.5, 0.0, 0.75 + 0.25 * 0.25]
    assert b["threshold_n"].tolist() == [3, 0, 3]
    assert BR.theta_ref(1.0, 0, 3.0, 0.5) == (3.0, 1) and BR.theta_ref(1.0, 2, 3.0, 0.5) == (2.0, 3)


def _ensemble(models, sig=BatchTopKEncoder, **kw):
    return FunctionalEnsemble(models, sig, adam, {"lr": 1e-3}, device="cpu", backend="torch", **kw)


def test_torch_backend_maintains_threshold(case):
    ens = _ensemble(copy.deepcopy(case["models"]), no_stacking=True)
    assert ens.buffers["threshold_n"].tolist() == [0, 0]
    loss, aux = ens.step_batch(case["x"])
    # step 0 ran on the fixture's dictionary: its thresholds are the reference's
    assert torch.equal(aux["threshold"], case["t"])
    assert torch.equal(ens.buffers["threshold"], torch.clamp(case["t"], min=0.0))
    theta = [[float(v), 1] for v in ens.buffers["threshold"]]
    for _ in range(2):
        loss, aux = ens.step_batch(case["x"])
        for m in range(M):
            theta[m] = list(BR.theta_ref(*theta[m], max(float(aux["threshold"][m]), 0.0), 0.01))
    assert ens.buffers["threshold_n"].tolist() == [3, 3]
    for m in range(M):
        assert ens.buffers["threshold"][m].item() == pytest.approx(theta[m][0], rel=1e-6)
    assert ens.buffers["sparsity"].tolist() == list(KS)
    assert torch.isfinite(loss["loss"]).all()


def test_torch_dp_path_maintains_threshold(case):
    """The data-parallel trainer's torch path (compute_grads / apply_grads)
    runs the buffer hook: after three steps parameters and threshold state
    equal a twin's stepped with step_batch, bit for bit."""
    from sparse_coding_amd.parallel.dp import DataParallelEnsembleTrainer

    ens = _ensemble(copy.deepcopy(case["models"]), no_stacking=True)
    twin = _ensemble(copy.deepcopy(case["models"]), no_stacking=True)
    trainer = DataParallelEnsembleTrainer(ens, force_dp_path=True)
    for _ in range(3):
        trainer.step(case["x"])
        twin.step_batch(case["x"])
    assert twin.buffers["threshold_n"].tolist() == [3, 3]
    for k in ("threshold", "threshold_n"):
        assert torch.equal(ens.buffers[k], twin.buffers[k]), k
    for k in twin.params:
        assert torch.equal(ens.params[k], twin.params[k]), k


def test_hook_leaves_other_signatures_alone():
    from sparse_coding_amd.models.sae_signatures import FunctionalTiedSAE
    from sparse_coding_amd.models.topk import TopKEncoder

    torch.manual_seed(0)
    x = torch.randn(32, 16)
    for sig, models, kw in (
            (FunctionalTiedSAE, [FunctionalTiedSAE.init(16, 32, l1) for l1 in (1e-3, 3e-3)], {}),
            (TopKEncoder, [TopKEncoder.init(16, 32, k) for k in (2, 4)], {"no_stacking": True})):
        assert not hasattr(sig, "update_buffers")
        ens = _ensemble(models, sig, **kw)
        before = {k: v.clone() for k, v in ens.buffers.items()}
        ens.step_batch(x)
        assert set(ens.buffers) == set(before)
        for k, v in before.items():
            assert torch.equal(ens.buffers[k], v), k


def test_learned_dict_encode_and_pickle(case):
    params, buffers = copy.deepcopy(case["models"][1])
    buffers["threshold"].fill_(1.75)
    ld = BatchTopKEncoder.to_learned_dict(params, buffers)
    assert isinstance(ld, BatchTopKLearnedDict)
    assert ld.sparsity == KS[1] and ld.threshold == 1.75
    assert type(ld).__module__ == "sparse_coding_amd.models.batch_topk"
    s = case["x"] @ _normed(params["dict"]).T
    want = torch.where((s >= 1.75) & (s > 0), s, torch.zeros_like(s))
    got = ld.encode(case["x"])
    assert torch.equal(got, want) and 0 < (got != 0).sum() < got.numel()
    # a threshold of 0 (an untrained dict) keeps the positive scores only
    ld0 = BatchTopKLearnedDict(ld.dict, 4, 0.0)
    assert torch.equal(ld0.encode(case["x"]), torch.clamp(s, min=0.0) + 0.0)
    ld2 = pickle.loads(pickle.dumps(ld))
    assert torch.equal(ld2.encode(case["x"]), got) and ld2.threshold == 1.75
    assert torch.equal(ld2.get_learned_dict(), ld.get_learned_dict())
    assert ld.predict(case["x"]).shape == case["x"].shape


# ---------------------------------------------------------------------------
# launch trace of the fused step
# ---------------------------------------------------------------------------

BINDINGS = dict(T.BINDINGS)
BINDINGS["batch_topk_select"] = [
    ("scores", T._REQ), ("c_out", T._REQ), ("fired", T._REQ), ("ks", T._REQ), ("thr_out", T._REQ),
    ("work", T._REQ), ("threshold", None), ("threshold_n", None), ("threshold_lr", None)]


class RecordingExt(T.RecordingExt):
    """test_hip_step_trace's recorder, knowing the new launcher as well."""

    WORK_PER_MODEL = 7

    def batch_topk_workspace_size(self, n_models):
        return self.WORK_PER_MODEL * n_models

    def __getattr__(self, fn):
        # the recorder looks a launcher's argument list up once, here
        saved, T.BINDINGS = T.BINDINGS, BINDINGS
        try:
            return super().__getattr__(fn)
        finally:
            T.BINDINGS = saved


def _traced_step(with_on_grads=False):
    from sparse_coding_amd.engine import hip_step as hs

    torch.manual_seed(0)
    ens = _ensemble([BatchTopKEncoder.init(T.D, T.N, k) for k in (4, 8)], no_stacking=True)
    ext = RecordingExt()
    step = hs.HipBatchTopKStep(ens, ext)
    ext.step = step
    ext.x = x = torch.randn(T.B, T.D)
    seen = []
    n = step.grads_phase(x, on_grads=seen.extend) if with_on_grads else step.grads_phase(x)
    step.update_phase(n)
    return ens, step, ext, seen


def test_step_launch_trace():
    ens, step, ext, _ = _traced_step()
    names = [fn for fn, _ in ext.calls]
    assert names == ["row_norms", "enc_fwd", "batch_topk_select", "dec_fwd", "gc", "grad_w", "grad_w",
                     "project_adam"]
    calls = {i: a for i, (_, a) in enumerate(ext.calls)}
    Mm, Bb, Nn, Dd = 2, T.B, T.N, T.D
    code = ["c", 0, [Mm, Bb, Nn]]
    scores = ["scores", 0, [Mm, Bb, Nn]]
    assert calls[1]["c_out"] == scores and calls[1]["mode"] == 1
    sel = calls[2]
    assert sel == {
        "scores": scores, "c_out": code, "fired": ["fired", 0, [Mm, Nn]], "ks": ["ks_i32", 0, [Mm]],
        "thr_out": ["thr_batch", 0, [Mm]], "work": ["btk_work", 0, [RecordingExt.WORK_PER_MODEL * Mm]],
        "threshold": ["buffers.threshold", 0, [Mm]], "threshold_n": ["buffers.threshold_n", 0, [Mm]],
        "threshold_lr": ["buffers.threshold_lr", 0, [Mm]]}
    assert step.btk_work.dtype == torch.int32
    assert calls[3]["c"] == code and calls[4]["c"] == code and calls[5]["P"] == code
    assert calls[5]["gw"] == calls[6]["gw"] == calls[7]["gw"] == ["gw", 0, [Mm, Nn, Dd]]
    assert calls[6]["P"] == ["gpre", 0, [Mm, Bb, Nn]] and calls[6]["beta"] == 1.0
    assert calls[7]["W"] == ["params.dict", 0, [Mm, Nn, Dd]] and calls[7]["project"] is True
    loss = step._loss_data(Bb)
    assert set(loss) == {"loss", "threshold"} and loss["threshold"] is step.thr_batch
    assert [t is step.gw for t in step.dp_grad_tensors()] == [True]


def test_step_trace_is_the_topk_chain_with_the_selection_replaced():
    """Apart from the selection launch the trace equals HipTopKStep's."""
    _, _, ext, seen = _traced_step(with_on_grads=True)
    topk, _, _ = T.run_case("topk", "t", False)
    assert len(seen) == 1
    for (fn, got), (fn_t, want) in zip(ext.calls, topk):
        if fn_t == "topk_select":
            assert fn == "batch_topk_select"
            assert {k: got[k] for k in want} == want
        else:
            assert (fn, got) == (fn_t, want)


def test_step_reads_threshold_state_at_launch_time():
    """A resumed sweep replaces ens.buffers: the next launch must see the new
    tensors, and a captured graph holding the old addresses must go."""
    ens, step, ext, _ = _traced_step()
    replay = step._replay
    replay.enabled = True
    replay._check_key()  # the key a capture at this point would be tied to
    replay.graph, held = object(), step.graph_key()
    ens.buffers = {k: v.clone() for k, v in ens.buffers.items()}
    assert held != step.graph_key() and held[0] is step.graph_key()[0]
    replay._check_key()
    assert step._graph is None
    step.use_graph = False  # CPU: the launch below runs eagerly
    ext.calls.clear()
    step.step(ext.x)
    assert step._graph is None
    sel = dict(ext.calls)["batch_topk_select"]
    assert sel["threshold"] == ["buffers.threshold", 0, [2]]


def test_maybe_make_step_knows_the_signature():
    import inspect

    from sparse_coding_amd.engine import hip_step as hs

    assert "BatchTopKEncoder: HipBatchTopKStep" in inspect.getsource(hs.maybe_make_step)
    doc = hs.HipBatchTopKStep.__doc__
    assert "data parallelism" in doc and "each rank" in doc


# ---------------------------------------------------------------------------
# sweep entry points
# ---------------------------------------------------------------------------

def test_batch_topk_init_builds_an_ensemble(monkeypatch):
    from sparse_coding_amd.config import EnsembleArgs
    from sparse_coding_amd.sweep import experiments as E

    monkeypatch.setattr(E, "default_devices", lambda n=None: ["cpu"])
    cfg = EnsembleArgs()
    cfg.activation_width, cfg.learned_dict_ratio, cfg.batch_size, cfg.lr = 16, 2.0, 32, 1e-3
    ensembles, ens_hp, buf_hp, ranges = E.batch_topk_init(cfg, ks=(2, 4, 8))
    (ens, args, name), = ensembles
    assert name == "batch_topk" and buf_hp == ["sparsity"] and ens_hp == ["dict_size"]
    assert ranges == {"sparsity": [2, 4, 8], "dict_size": [32]}
    assert ens.sig is BatchTopKEncoder and ens.no_stacking and ens.n_models == 3
    assert ens.params["dict"].shape == (3, 32, 16)
    assert args == {"batch_size": 32, "device": "cpu", "dict_size": 32}
    loss, aux = ens.step_batch(torch.randn(32, 16))
    assert (aux["c"] > 0).sum(dim=(1, 2)).tolist() == [2 * 32, 4 * 32, 8 * 32]
    assert ens.buffers["threshold_n"].tolist() == [1, 1, 1]
    dicts = ens.to_learned_dicts()
    assert [d.sparsity for d in dicts] == [2, 4, 8]
    assert all(d.threshold > 0 for d in dicts)


def test_cli_lists_run_batch_topk():
    import big_sweep_experiments

    out = io.StringIO()
    with redirect_stdout(out):
        big_sweep_experiments.main(["list"])
    assert "run_batch_topk" in out.getvalue().split()
    assert "run_topk" in out.getvalue().split()


def test_resampler_accepts_the_signature(case):
    from sparse_coding_amd.engine.resample import EnsembleResampler

    ens = _ensemble(copy.deepcopy(case["models"]), no_stacking=True)
    rs = EnsembleResampler(ens, n_track=8)
    assert rs.w_key == "dict"
    _, aux = ens.step_batch(case["x"])
    rs.observe(case["x"], aux)
    assert torch.equal(rs.fired, case["fired"])

"""Launch traces of the data-parallel trainer over the fused HIP steps, on CPU.

``tests/test_hip_step_trace.py`` pins what one ``grads_phase`` +
``update_phase`` launches.  This file pins what
``DataParallelEnsembleTrainer.step`` launches on top of a step: the same
recording stand-in for the extension is attached as ``ens._hip_step`` and the
trainer is driven under gloo, so "which launches, in which order, on which
operands" of both ``dp_mode``s is checked without a GPU.

The expected traces (``tests/golden/dp_step_trace.json``) were recorded with
this recorder from the commit before the trainer's sharded update moved into
``HipSAEStep``; a refactor of the trainer must reproduce them entry for entry.
The trainer's own row-shard buffers appear as ``<unowned>``.  Workspaces are
uninitialised CPU memory: only operands and order are compared.

Re-record (from the repository root) with
``python -m tests.test_dp_step_trace --record tests/golden/dp_step_trace.json``.
"""

import json
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_hip_step_trace import B, D, M, N, RecordingExt, _ensemble, _targets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dp_step_trace.json")

MODES = ("allreduce", "rs_ag")
W1_TARGETS = ("tied", "untied", "centered", "thresholding", "topk", "lista")
W2_TARGETS = ("tied", "untied")
W2_PORT = 29597
STEPS = 2  # the second step reuses the rs_ag shard buffers


def trainer_trace(target, dp_mode, rank=0, world=1):
    """STEPS trainer steps over a fresh CPU ensemble with a recording step
    attached; the caller has initialised the process group."""
    from sparse_coding_amd.ops.kconfig import DEFAULTS, kernel_config, set_kernel_config
    from sparse_coding_amd.parallel.dp import DataParallelEnsembleTrainer, shard_batch

    old = kernel_config()
    set_kernel_config(**DEFAULTS)
    try:
        torch.manual_seed(0)
        sig, models, make = _targets()[target]
        ext = RecordingExt()
        ens = _ensemble(sig, models())
        step = make(ens, ext)
        step.use_graph = False
        ens._hip_step = step
        ext.step = step
        ext.x = x = shard_batch(torch.randn(B * world, D), rank, world).contiguous()
        trainer = DataParallelEnsembleTrainer(ens, force_dp_path=True, dp_mode=dp_mode)
        for _ in range(STEPS):
            trainer.step(x)
        return json.loads(json.dumps(ext.calls))
    finally:
        set_kernel_config(**old)


def world1_traces():
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{tmp}/store", rank=0, world_size=1)
        try:
            return {f"w1/{t}/{m}": trainer_trace(t, m) for t in W1_TARGETS for m in MODES}
        finally:
            dist.destroy_process_group()


def _world2_worker(rank, port, out_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=2)
        try:
            out = {f"w2/{t}/{m}/rank{rank}": trainer_trace(t, m, rank, 2)
                   for t in W2_TARGETS for m in MODES}
        finally:
            dist.destroy_process_group()
        out_q.put(out)
    except Exception:  # noqa: BLE001
        import traceback

        out_q.put({"_error": f"rank {rank}: {traceback.format_exc()}"})
        raise


def world2_traces():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_world2_worker, args=(r, W2_PORT, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = {}
    for _ in procs:
        res = q.get(timeout=100)
        assert "_error" not in res, res.get("_error")
        out.update(res)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def w1():
    return world1_traces()


@pytest.fixture(scope="module")
def w2():
    return world2_traces()


def _assert_equal(key, got, want):
    assert len(got) == len(want), (key, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} of {key} differs:\n got  {g}\n want {w}"


@pytest.mark.parametrize("dp_mode", MODES)
@pytest.mark.parametrize("target", W1_TARGETS)
def test_world1_trace_matches_recorded(golden, w1, target, dp_mode):
    key = f"w1/{target}/{dp_mode}"
    _assert_equal(key, w1[key], golden[key])


def test_world1_rs_ag_falls_back_to_allreduce_where_unsupported(w1):
    for target in ("centered", "thresholding", "topk", "lista"):
        assert w1[f"w1/{target}/rs_ag"] == w1[f"w1/{target}/allreduce"], target
    assert w1["w1/tied/rs_ag"] != w1["w1/tied/allreduce"]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("dp_mode", MODES)
@pytest.mark.parametrize("target", W2_TARGETS)
def test_world2_trace_matches_recorded(golden, w2, target, dp_mode, rank):
    key = f"w2/{target}/{dp_mode}/rank{rank}"
    _assert_equal(key, w2[key], golden[key])


# weight-gradient chunks in the order the step announces them, as
# (parameter, first model, end model): the tied step chunks over model
# quarters (here one model each), the untied one announces gw then gw_enc whole
RS_AG_CHUNKS = {
    "tied": [("encoder", 0, 1), ("encoder", 1, 2)],
    "untied": [("decoder", 0, M), ("encoder", 0, M)],
}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("target", W2_TARGETS)
def test_world2_rs_ag_addresses_the_ranks_own_rows(w2, target, rank):
    """Rank r updates rows [lo*n + r*k, lo*n + (r+1)*k) of the flattened
    parameter for a chunk of models [lo, hi), k = (hi-lo)*n/world."""
    adams = [a for fn, a in w2[f"w2/{target}/rs_ag/rank{rank}"] if fn == "project_adam"]
    chunks = RS_AG_CHUNKS[target] * STEPS
    assert len(adams) == len(chunks)
    for a, (pname, lo, hi) in zip(adams, chunks):
        k = (hi - lo) * N // 2
        g0 = lo * N + rank * k
        assert a["W"] == [f"params.{pname}", g0 * D, [k, D]], a["W"]
        assert a["mu"] == [f"mu.{pname}", g0 * D, [k, D]], a["mu"]
        assert a["nu"] == [f"nu.{pname}", g0 * D, [k, D]], a["nu"]
        assert a["norms"] == ["norms", g0, [k]], a["norms"]
        assert a["lr_mult"] == ["lr_mult", g0, [k]], a["lr_mult"]
        assert a["gw"][1:] == [0, [k, D]], a["gw"]
        assert a["step_no"][2] == [1] and a["n_per_model"] == k


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    out = dict(world1_traces())
    w2_out = world2_traces()
    out.update({k: w2_out[k] for k in sorted(w2_out)})
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        f.write("{\n")
        for ki, (key, calls) in enumerate(out.items()):
            f.write(f" {json.dumps(key)}: [\n")
            f.write(",\n".join("  " + json.dumps(c) for c in calls))
            f.write("\n ]" + ("," if ki + 1 < len(out) else "") + "\n")
        f.write("}\n")
    print(f"recorded {len(out)} traces to {sys.argv[2]}")

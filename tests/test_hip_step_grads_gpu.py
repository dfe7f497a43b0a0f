"""Every fused step's gradients against fp64 autograd of its signature's loss.

The ensembles are built with ``lr = 0``: the parameters stay bit for bit what
they were, every step sees the same gradient ``g``, and Adam's moments after
``t`` steps from zero state are ``mu = (1-b1^t) g`` and ``nu = (1-b2^t) g^2``
with ``g`` the gradient Adam consumed (projection through the row
normalisation, clamp mask, bias decay and rho gate included).  ``mu`` has the
tree of ``ens.params``, so it is compared leaf for leaf and model for model with
``torch.func.grad`` of the signature's ``loss`` in float64 on the CPU
(tests/step_reference.py), under ``err <= 8 e32 + 16 U scale`` in the max norm,
``e32`` being the error of the same autograd in float32 on the CPU.  The third
call is the first one GraphReplay captures and replays, so the captured chain
is checked too.  The loss dict and the codes are checked after the first call.

Cases x shapes: every case at the tile-aligned (2, 128, 64, 128), which takes
the guard-free kernels; the shallow chains at (2, 130, 68, 260): two row tiles,
column tails at both widths, K tails at both depths in every GEMM; LISTA
(L = 3), residual-denoising (L = 2) and semilinear at (2, 36, 20, 132); tied,
untied and masked tied under staging="pre" at (2, 132, 68, 132).  The seeds
come from the CPU (test_step_reference_cpu.py): inputs on which no nonsmooth
decision of the float64 forward is near its knee, so a failure here is not a
flipped mask.

Worst ratio err / bound per case over its shapes, leaves and both moments
(1.0 is the bound; measured on an MI355X, see the table the module prints with
-s as ``[step64]`` lines):

    case            worst err/bound
    tied            0.131
    untied          0.121
    masked_tied     0.128
    masked_untied   0.130
    reverse         0.115
    centered        0.400
    whitened        0.175
    positive        0.112
    thresholding    0.160
    lista           0.206
    residual        0.133
    semilinear      0.141
    topk            0.136
    batch_topk      0.108
"""

import pytest
import torch

from tests import step_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _to_dev(tree):
    return R.tree_apply(lambda t: t.to(DEV), tree)


def _report(entry, what, ratios):
    for leaf, ratio in ratios.items():
        print(f"[step64] {R.grid_id(entry)} {what} {leaf} {ratio:.3f}")


@pytest.fixture
def staging():
    from sparse_coding_amd.ops.kconfig import kernel_config, set_kernel_config

    old = kernel_config()

    def use(value):
        if value is not None:
            set_kernel_config(staging=value)
    yield use
    set_kernel_config(**old)


@pytest.mark.parametrize("entry", R.GRID, ids=[R.grid_id(e) for e in R.GRID])
def test_step_gradients_match_fp64_autograd(entry, staging):
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam

    name, shape, stg = entry
    M, B, d, n = shape
    c = R.case(name)
    assert R.decisions(name, shape)["near"] == 0  # before touching the GPU
    ref = R.reference(name, shape)
    models, x = R.build(name, shape)
    masked = (n, c.dict_sizes(n)) if c.dict_sizes else None

    staging(stg)
    ens = FunctionalEnsemble([(_to_dev(p), _to_dev(b)) for p, b in models], c.sig, adam, {"lr": 0.0},
                             device=DEV, backend="hip")
    hs = ens._hip_step
    assert type(hs).__name__ == c.step_class
    if c.step_class == "HipSAEStep":  # one class, told apart by its flags
        for flag in ("tied", "masked", "reverse"):
            assert bool(getattr(hs, flag)) == (flag in c.flags), flag
    assert hs.captures_graph == c.captures_graph
    params0 = R.tree_apply(lambda t: t.detach().cpu().clone(), ens.params)
    for (path, p0), (_, p) in zip(R.tree_items(params0), R.tree_items(R.tree_stack([p for p, _ in models]))):
        assert torch.equal(p0, p), path  # the ensemble trains what the reference differentiated
    xg = x.to(DEV)

    # ---- call 1: losses, codes, moments -----------------------------------
    losses, aux = ens.step_batch(xg)
    torch.cuda.synchronize()
    if stg is not None:
        assert hs.kc["staging"] == stg
    worst = {}
    worst["loss"] = R.compare_losses(losses, ref, R.loss_depths(c, B, d, n))
    assert set(worst["loss"]) >= set(ref["loss64"]) - {"threshold"}
    worst["c"] = R.compare_codes(aux["c"], ref, masked[1] if masked else None)
    st = ens.optim_states
    assert (st["step"] == 1).all()
    worst["mu1"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 1, masked)
    worst["nu1"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 1, masked)

    # ---- call 3: the first replay of the captured graph --------------------
    ens.step_batch(xg)
    assert hs._graph is None
    ens.step_batch(xg)
    torch.cuda.synchronize()
    if c.captures_graph:
        assert hs._graph is not None
    else:
        assert hs._graph is None
    assert (st["step"] == 3).all()
    worst["mu3"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 3, masked)
    worst["nu3"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 3, masked)
    for (path, p0), (_, p) in zip(R.tree_items(params0), R.tree_items(ens.params)):
        p = p.detach().cpu()
        assert p.dtype == p0.dtype and torch.equal(p0.view(torch.int32), p.view(torch.int32)), \
            f"{path} moved at lr = 0"

    for what, ratios in worst.items():
        _report(entry, what, ratios)
    print(f"[step64] {R.grid_id(entry)} worst {max(max(r.values()) for r in worst.values()):.3f}")

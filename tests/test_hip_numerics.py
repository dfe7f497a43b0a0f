"""Numerics of the gfx950 HIP kernels vs the plain-PyTorch fp32 oracle.

Every test is @gpu: runs on the MI355X box (`pytest -m gpu`).  Tolerances
are fp32-accumulation-order level (the MFMA f32 path is exact f32 but sums
in a different order than rocBLAS/torch).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from sparse_coding_amd import ops

    return ops.get_extension()


def _rel_err(a, b):
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


@pytest.fixture(scope="module")
def shapes():
    # deliberately NOT multiples of the 128x128 tile: exercises edge guards
    return dict(M=3, B=192, d=96, n=160)


# every test in this module runs under each compiled kernel variant:
# (staging, tile depth TBK, younger-half s_setprio) — see ops/kconfig.py
@pytest.fixture(autouse=True, params=[("t", 32, False, 128), ("t", 16, True, 128),
                                      ("pre", 32, True, 128), ("pre", 16, False, 128),
                                      ("t", 16, False, 256)],
                ids=lambda p: f"{p[0]}-bk{p[1]}-p{int(p[2])}-bn{p[3]}")
def kcfg(request):
    from sparse_coding_amd.ops.kconfig import kernel_config, set_kernel_config

    old = kernel_config()
    staging, bk, prio, bn = request.param
    set_kernel_config(staging=staging, bk=bk, prio=prio, bn=bn)
    yield {"bk": bk, "prio": prio, "staging": staging, "bn": bn}
    set_kernel_config(**old)


def test_row_norms(shapes):
    ext = _ext()
    M, n, d = shapes["M"], shapes["n"], shapes["d"]
    torch.manual_seed(0)
    W = torch.randn(M, n, d, device=DEV)
    W[0, 0] = 0.0  # degenerate row: clamped, not inf
    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)
    ref = torch.norm(W, 2, dim=-1)
    assert _rel_err(norms, ref) < 1e-6
    ref_inv = 1.0 / torch.clamp(ref, min=1e-8)
    assert _rel_err(inv, ref_inv) < 1e-6


def test_enc_fwd_untied(shapes, kcfg):
    ext = _ext()
    M, B, d, n = shapes["M"], shapes["B"], shapes["d"], shapes["n"]
    torch.manual_seed(1)
    x = torch.randn(B, d, device=DEV)
    W = torch.randn(M, n, d, device=DEV) * 0.2
    bias = torch.randn(M, n, device=DEV) * 0.1
    c = torch.empty(M, B, n, device=DEV)
    loss_parts = torch.zeros(M, 2, device=DEV)
    fired = torch.zeros(M, n, device=DEV)
    ext.enc_fwd(x, W, bias, None, c, loss_parts, fired, 0, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    ref = torch.clamp(torch.einsum("mnd,bd->mbn", W, x) + bias[:, None, :], min=0)
    assert _rel_err(c, ref) < 1e-5
    assert _rel_err(loss_parts[:, 1], ref.sum(dim=(1, 2))) < 1e-4
    ref_fired = (ref > 0).float().sum(dim=1)
    assert torch.equal(fired, ref_fired)


def test_enc_fwd_tied_scaled(shapes, kcfg):
    ext = _ext()
    M, B, d, n = shapes["M"], shapes["B"], shapes["d"], shapes["n"]
    torch.manual_seed(2)
    x = torch.randn(B, d, device=DEV)
    W = torch.randn(M, n, d, device=DEV)
    bias = torch.zeros(M, n, device=DEV)
    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)
    c = torch.empty(M, B, n, device=DEV)
    lp = torch.zeros(M, 2, device=DEV)
    fired = torch.zeros(M, n, device=DEV)
    ext.enc_fwd(x, W, bias, inv, c, lp, fired, 0, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    What = W / torch.clamp(torch.norm(W, dim=-1, keepdim=True), 1e-8)
    ref = torch.clamp(torch.einsum("mnd,bd->mbn", What, x), min=0)
    assert _rel_err(c, ref) < 1e-5


def test_dec_fwd(shapes, kcfg):
    ext = _ext()
    M, B, d, n = shapes["M"], shapes["B"], shapes["d"], shapes["n"]
    torch.manual_seed(3)
    x = torch.randn(B, d, device=DEV)
    W = torch.randn(M, n, d, device=DEV)
    c = torch.rand(M, B, n, device=DEV)
    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)
    r = torch.empty(M, B, d, device=DEV)
    lp = torch.zeros(M, 2, device=DEV)
    ext.dec_fwd(c, W, inv, x, r, lp, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    What = W / torch.clamp(torch.norm(W, dim=-1, keepdim=True), 1e-8)
    ref_r = torch.einsum("mnd,mbn->mbd", What, c) - x
    assert _rel_err(r, ref_r) < 1e-5
    assert _rel_err(lp[:, 0], ref_r.pow(2).sum(dim=(1, 2))) < 1e-4


def test_gc(shapes, kcfg):
    ext = _ext()
    M, B, d, n = shapes["M"], shapes["B"], shapes["d"], shapes["n"]
    torch.manual_seed(4)
    r = torch.randn(M, B, d, device=DEV)
    W = torch.randn(M, n, d, device=DEV)
    c = torch.clamp(torch.randn(M, B, n, device=DEV), min=0)  # ~half zeros
    l1 = torch.tensor([1e-3, 1e-2, 0.0], device=DEV)
    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)
    gpre = torch.empty(M, B, n, device=DEV)
    g_bias = torch.zeros(M, n, device=DEV)
    ext.gc(r, W, inv, c, l1, gpre, g_bias, kcfg["bk"], kcfg["prio"], bn=kcfg["bn"])
    What = W / torch.clamp(torch.norm(W, dim=-1, keepdim=True), 1e-8)
    gscale = 2.0 / (B * d)
    g = gscale * torch.einsum("mnd,mbd->mbn", What, r) + l1[:, None, None] / B
    ref = torch.where(c > 0, g, torch.zeros_like(g))
    assert _rel_err(gpre, ref) < 1e-5
    assert _rel_err(g_bias, ref.sum(dim=1)) < 1e-4


def test_gc_bias_grad_reproducible(kcfg):
    """The bias gradient is summed in a fixed order (per-32-row column sums,
    then one ordered add): repeated calls give bitwise-identical g_bias, and
    the sum is ADDED to what g_bias held.  B is no multiple of the 32-row
    group nor of the 128-row tile, n no multiple of the column tile."""
    ext = _ext()
    M, B, d, n = 2, 300, 64, 200
    torch.manual_seed(14)
    r = torch.randn(M, B, d, device=DEV)
    W = torch.randn(M, n, d, device=DEV)
    c = torch.clamp(torch.randn(M, B, n, device=DEV), min=0)
    l1 = torch.tensor([1e-3, 1e-2], device=DEV)
    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)
    outs = []
    for _ in range(3):
        gpre = torch.empty(M, B, n, device=DEV)
        g_bias = torch.ones(M, n, device=DEV)
        ext.gc(r, W, inv, c, l1, gpre, g_bias, kcfg["bk"], kcfg["prio"], bn=kcfg["bn"])
        outs.append(g_bias)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # fp32 sum of 300 terms of magnitude ~gpre.abs().max(): a few ulp of the column's abs-sum
    ref = 1.0 + gpre.double().sum(dim=1)
    bound = 300 * 2.0 ** -24 * gpre.double().abs().sum(dim=1).max().item() + 2.0 ** -23
    assert (outs[0].double() - ref).abs().max().item() <= bound
    # accumulate=False overwrites whatever g_bias held
    g_over = torch.full((M, n), 7.0, device=DEV)
    ext.gc(r, W, inv, c, l1, gpre, g_over, kcfg["bk"], kcfg["prio"], bn=kcfg["bn"], accumulate=False)
    assert (g_over.double() - (ref - 1.0)).abs().max().item() <= bound


def test_grad_w(shapes, kcfg):
    ext = _ext()
    M, B, d, n = shapes["M"], shapes["B"], shapes["d"], shapes["n"]
    torch.manual_seed(5)
    P = torch.randn(M, B, n, device=DEV)
    Q = torch.randn(M, B, d, device=DEV)
    gw = torch.zeros(M, n, d, device=DEV)
    ext.grad_w(P, Q, gw, 0.5, 0.0, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    ref = 0.5 * torch.einsum("mbn,mbd->mnd", P, Q)
    assert _rel_err(gw, ref) < 1e-5
    # beta accumulate + shared Q
    x = torch.randn(B, d, device=DEV)
    ext.grad_w(P, x, gw, 1.0, 1.0, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    ref = ref + torch.einsum("mbn,bd->mnd", P, x)
    assert _rel_err(gw, ref) < 1e-5


def test_project_adam_matches_autograd(shapes):
    """Projection kernel == autograd through w/clamp(norm, eps) + torch Adam."""
    ext = _ext()
    M, n, d = shapes["M"], shapes["n"], shapes["d"]
    torch.manual_seed(6)
    W = torch.randn(M, n, d, device=DEV)
    gw = torch.randn(M, n, d, device=DEV)
    mu = torch.zeros_like(W)
    nu = torch.zeros_like(W)
    step_no = torch.ones(M, device=DEV)
    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)

    # autograd reference for the projected gradient (grad mode explicitly on:
    # a prior sweep() in the same process must not poison this)
    with torch.enable_grad():
        W_ref = W.clone().requires_grad_()
        What = W_ref / torch.clamp(torch.norm(W_ref, dim=-1, keepdim=True), 1e-8)
        (What * gw).sum().backward()
    g_ref = W_ref.grad

    W_out = W.clone()
    ext.project_adam(W_out, gw, norms, mu, nu, step_no, n, 1e-3, 0.9, 0.999, 1e-8, 1e-8, True)
    # step 1 adam: update = -lr * g/|g| (bias-corrected), so recover direction
    upd_ref = 1e-3 * g_ref / (g_ref.abs() + 1e-8)
    assert _rel_err(W_out, W - upd_ref) < 1e-4
    assert _rel_err(mu, 0.1 * g_ref) < 1e-4


def test_full_step_matches_torch_backend():
    """Several fused steps track the vmap+functional-Adam oracle."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalSAE, FunctionalTiedSAE

    for sig, tied in ((FunctionalTiedSAE, True), (FunctionalSAE, False)):
        torch.manual_seed(7)
        M, B, d, n = 2, 256, 64, 128
        models = [sig.init(d, n, l1, device=DEV) for l1 in (1e-3, 3e-3)]
        ens_hip = FunctionalEnsemble(models, sig, adam, {"lr": 1e-3}, device=DEV, backend="hip")
        # clone params for the oracle BEFORE any stepping
        models2 = []
        for p, b in ens_hip.unstack():
            models2.append(({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()}))
        ens_ref = FunctionalEnsemble(models2, sig, adam, {"lr": 1e-3}, device=DEV, backend="torch")

        assert ens_hip._hip_step is not None, "HIP step not active on GPU!"

        x = torch.randn(B, d, device=DEV)
        for i in range(5):
            l_hip, aux_hip = ens_hip.step_batch(x)
            l_ref, aux_ref = ens_ref.step_batch(x)
            assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, (sig.__name__, i)
            assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, (sig.__name__, i)
        for k in ens_ref.params:
            assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, (sig.__name__, k)


def test_full_step_large_shapes_flagship():
    """Flagship-shaped step (d=512, n=4096, M=2, B=512): finite + decreasing."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalTiedSAE

    torch.manual_seed(8)
    M, B, d, n = 2, 512, 512, 4096
    models = [FunctionalTiedSAE.init(d, n, l1, device=DEV) for l1 in (1e-4, 1e-3)]
    ens = FunctionalEnsemble(models, FunctionalTiedSAE, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    x = torch.randn(B, d, device=DEV)
    l0, _ = ens.step_batch(x)
    for _ in range(10):
        losses, _ = ens.step_batch(x)
    assert torch.isfinite(losses["loss"]).all()
    assert (losses["loss"] < l0["loss"]).all()


def test_bias_decay_gradient():
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalSAE

    torch.manual_seed(9)
    M, B, d, n = 2, 128, 64, 128
    models = [FunctionalSAE.init(d, n, 1e-3, bias_decay=0.01, device=DEV) for _ in range(M)]
    ens_hip = FunctionalEnsemble(models, FunctionalSAE, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalSAE, adam, {"lr": 1e-3}, device=DEV, backend="torch")
    x = torch.randn(B, d, device=DEV)
    # give the bias a nonzero value so the decay grad is active
    with torch.no_grad():
        ens_hip.params["encoder_bias"].normal_(0, 0.1)
        ens_ref.params["encoder_bias"].copy_(ens_hip.params["encoder_bias"])
    for _ in range(3):
        l_hip, _ = ens_hip.step_batch(x)
        l_ref, _ = ens_ref.step_batch(x)
    assert _rel_err(ens_hip.params["encoder_bias"], ens_ref.params["encoder_bias"]) < 2e-3
    assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4


def test_thresholding_step_matches_torch():
    """Fused threshold-gate step (k_enc_fwd mode 2 + k_gc_thresh) vs the vmap
    oracle: gate forward, g'(u) backward, and the gain/scale column-sum
    grads all have to line up."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalThresholdingSAE

    torch.manual_seed(10)
    M, B, d, n = 2, 256, 64, 128
    models = [FunctionalThresholdingSAE.init(d, n, l1, device=DEV) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, FunctionalThresholdingSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipThresholdStep"
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalThresholdingSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="torch")
    # scale up inputs so the gate's u regularly crosses the 0.9/1.0 knees
    x = 2.0 * torch.randn(B, d, device=DEV)
    for i in range(5):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, i
    for k in ens_ref.params:
        assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, k


def test_centered_step_matches_torch():
    """Fused tied-centered step: per-model x' = x - t[m] through the tied
    pipeline; learnable-center grad = gscale*sum_b r - g_bias @ What."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalTiedCenteredSAE

    torch.manual_seed(15)
    M, B, d, n = 2, 256, 64, 128
    models = [FunctionalTiedCenteredSAE.init(d, n, l1, device=DEV) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, FunctionalTiedCenteredSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipCenteredStep"
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalTiedCenteredSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="torch")
    with torch.no_grad():  # nonzero center so x' differs per model
        ens_hip.params["center"].normal_(0, 0.3)
        ens_ref.params["center"].copy_(ens_hip.params["center"])
    x = torch.randn(B, d, device=DEV) + 0.5
    for i in range(4):
        l_hip, _ = ens_hip.step_batch(x)
        l_ref, _ = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
    for k in ens_ref.params:
        assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, k


def test_positive_step_matches_torch():
    """Fused positive-tied step: pipeline on Wc = clamp(W,0) and x + 0.18,
    clamp-masked projected gradient updating the raw encoder."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.positive import FunctionalPositiveTiedSAE

    torch.manual_seed(16)
    M, B, d, n = 2, 256, 64, 128
    models = [FunctionalPositiveTiedSAE.init(d, n, l1, bias_decay=0.01, device=DEV)
              for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, FunctionalPositiveTiedSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipPositiveStep"
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalPositiveTiedSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="torch")
    # drive some weights negative so the clamp mask matters
    with torch.no_grad():
        ens_hip.params["encoder"].sub_(0.05)
        ens_ref.params["encoder"].copy_(ens_hip.params["encoder"])
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, _ = ens_hip.step_batch(x)
        l_ref, _ = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
    for k in ens_ref.params:
        assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, k


def test_reverse_step_matches_torch():
    """Fused reverse-SAE step (enc mode 3 + gc_mode 1): bias-subtracted
    codes (possibly negative), |code| L1, and NO bias grad from the code
    path — vs the vmap oracle."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalReverseSAE

    torch.manual_seed(14)
    M, B, d, n = 2, 256, 64, 128
    models = [FunctionalReverseSAE.init(d, n, l1, bias_decay=0.01, device=DEV) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, FunctionalReverseSAE, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    assert getattr(ens_hip._hip_step, "reverse", False)
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalReverseSAE, adam, {"lr": 1e-3}, device=DEV, backend="torch")
    # nonzero bias so the bias-subtract path actually differs from tied
    with torch.no_grad():
        ens_hip.params["encoder_bias"].normal_(0, 0.2)
        ens_ref.params["encoder_bias"].copy_(ens_hip.params["encoder_bias"])
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, i
        assert (aux_hip["c"] < 0).any()  # reverse codes go negative
    for k in ens_ref.params:
        assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, k


def test_masked_step_matches_torch():
    """Fused masked steps (K9): different dict sizes stacked to one width;
    coefficient columns >= dict_size[m] stay zero and get no grads."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import (
        FunctionalMaskedSAE,
        FunctionalMaskedTiedSAE,
    )

    for sig in (FunctionalMaskedTiedSAE, FunctionalMaskedSAE):
        torch.manual_seed(13)
        B, d, n_stack = 256, 64, 192
        dict_sizes = (64, 192)
        models = [sig.init(d, nd, n_stack, 1e-3, device=DEV) for nd in dict_sizes]
        ens_hip = FunctionalEnsemble(models, sig, adam, {"lr": 1e-3}, device=DEV, backend="hip")
        assert type(ens_hip._hip_step).__name__ == "HipSAEStep" and ens_hip._hip_step.masked
        models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
                   for p, b in ens_hip.unstack()]
        ens_ref = FunctionalEnsemble(models2, sig, adam, {"lr": 1e-3}, device=DEV, backend="torch")
        x = torch.randn(B, d, device=DEV)
        for i in range(4):
            l_hip, aux_hip = ens_hip.step_batch(x)
            l_ref, aux_ref = ens_ref.step_batch(x)
            assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, (sig.__name__, i)
            # masked coefficients exactly zero
            assert (aux_hip["c"][0, :, dict_sizes[0]:] == 0).all()
        for k in ens_ref.params:
            assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, (sig.__name__, k)


def test_topk_step_matches_torch():
    """Fused TopK step vs the reference-semantics no_stacking vmap oracle."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.topk import TopKEncoder

    torch.manual_seed(11)
    M, B, d, n = 2, 256, 64, 128
    ks = (4, 16)
    models = [TopKEncoder.init(d, n, k) for k in ks]
    ens_hip = FunctionalEnsemble(models, TopKEncoder, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipTopKStep"
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, TopKEncoder, adam, {"lr": 1e-3},
                                 device=DEV, no_stacking=True, backend="torch")
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        # sparsity respected
        for m, k in enumerate(ks):
            assert (aux_hip["c"][m] != 0).sum(dim=-1).max() <= k
    assert _rel_err(ens_hip.params["dict"], ens_ref.params["dict"]) < 2e-3


def test_lista_step_matches_torch():
    """HipLISTAStep (hand-derived backward through the unrolled LISTA
    layers) vs the torch.func.grad oracle: decoder, per-layer W/theta/rho
    and the loss must all track over several steps."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.lista import FunctionalLISTADenoisingSAE

    torch.manual_seed(17)
    M, B, d, n, L = 2, 256, 64, 128, 3
    models = [FunctionalLISTADenoisingSAE.init(d, n, L, l1) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, FunctionalLISTADenoisingSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipLISTAStep"
    models2 = [({k: (v.clone() if torch.is_tensor(v) else [{kk: vv.clone() for kk, vv in lay.items()} for lay in v])
                 for k, v in p.items()},
                {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalLISTADenoisingSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="torch")
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, i
    assert _rel_err(ens_hip.params["decoder"], ens_ref.params["decoder"]) < 2e-3
    for l in range(L):
        for k in ("W", "theta", "rho"):
            err = _rel_err(ens_hip.params["encoder_layers"][l][k],
                           ens_ref.params["encoder_layers"][l][k])
            assert err < 2e-3, (l, k, err)


def test_resampler_gpu():
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.engine.resample import EnsembleResampler
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalTiedSAE

    torch.manual_seed(12)
    M, B, d, n = 2, 256, 64, 256
    models = [FunctionalTiedSAE.init(d, n, 1e-3, device=DEV) for _ in range(M)]
    ens = FunctionalEnsemble(models, FunctionalTiedSAE, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    rs = EnsembleResampler(ens, n_track=64)
    # kill half the features so they never fire
    with torch.no_grad():
        ens.params["encoder_bias"][:, : n // 2] = -1e6
    x = torch.randn(B, d, device=DEV)
    for _ in range(3):
        _, aux = ens.step_batch(x)
        rs.observe(x, aux)
    assert (rs.fired[:, : n // 2] == 0).all()
    before = ens.params["encoder"][:, : n // 2].clone()
    counts = rs.resample()
    assert (counts == 64).all()  # n_track-limited
    after = ens.params["encoder"][:, :64]
    assert not torch.allclose(before[:, :64], after)
    assert (ens.optim_states["mu"]["encoder"][0, :64] == 0).all()


def test_residual_denoising_step_matches_torch():
    """HipResidualDenoisingStep vs the vmap oracle."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.lista import FunctionalResidualDenoisingSAE

    torch.manual_seed(18)
    M, B, d, n, L = 2, 256, 64, 128, 2
    models = [FunctionalResidualDenoisingSAE.init(d, n, L, l1) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, FunctionalResidualDenoisingSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipResidualDenoisingStep"
    models2 = [({k: (v.clone() if torch.is_tensor(v) else [{kk: vv.clone() for kk, vv in lay.items()} for lay in v])
                 for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, FunctionalResidualDenoisingSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="torch")
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, i
    assert _rel_err(ens_hip.params["decoder"], ens_ref.params["decoder"]) < 2e-3
    assert _rel_err(ens_hip.params["encoder_bias"], ens_ref.params["encoder_bias"]) < 2e-3
    for l in range(L):
        for k in ("W", "theta"):
            err = _rel_err(ens_hip.params["encoder_layers"][l][k],
                           ens_ref.params["encoder_layers"][l][k])
            assert err < 2e-3, (l, k, err)


def test_semilinear_step_matches_torch():
    """HipSemilinearStep (2-layer MLP encoder) vs the vmap oracle."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.semilinear import SemiLinearSAE

    torch.manual_seed(19)
    M, B, d, n = 2, 256, 64, 128
    models = [SemiLinearSAE.init(d, n, l1, device=DEV) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, SemiLinearSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="hip")
    assert type(ens_hip._hip_step).__name__ == "HipSemilinearStep"
    models2 = [({k: (v.clone() if torch.is_tensor(v) else [{kk: vv.clone() for kk, vv in lay.items()} for lay in v])
                 for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, SemiLinearSAE, adam, {"lr": 1e-3},
                                 device=DEV, backend="torch")
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, i
    assert _rel_err(ens_hip.params["decoder"], ens_ref.params["decoder"]) < 2e-3
    for li in (0, 1):
        for k in ("weight", "bias"):
            err = _rel_err(ens_hip.params["encoder_layers"][li][k],
                           ens_ref.params["encoder_layers"][li][k])
            assert err < 2e-3, (li, k, err)


def test_extreme_dict_ratios():
    """SURVEY.md scale range: dict ratios 0.25x-96x.  The 96x grid at d=512
    (n=49152), the 0.25x grid (n=128, one column tile) and a d=2048 grid
    must track the oracle's LOSS TRAJECTORY over several steps.

    Elementwise post-Adam param comparison is meaningless at huge sparse
    ratios: rows that barely fire have |g| at roundoff scale, and Adam's
    m/sqrt(v) normalization turns any fp32 summation-order difference into
    a full +-lr sign flip — so correctness is asserted through the losses,
    which integrate the updates over steps."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalTiedSAE

    for d, ratio, B in ((512, 96, 256), (512, 0.25, 256), (2048, 8, 256)):
        n = int(d * ratio)
        torch.manual_seed(23)
        models = [FunctionalTiedSAE.init(d, n, 1e-3, device=DEV) for _ in range(2)]
        ens_hip = FunctionalEnsemble(models, FunctionalTiedSAE, adam, {"lr": 1e-3},
                                     device=DEV, backend="hip")
        models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
                   for p, b in ens_hip.unstack()]
        ens_ref = FunctionalEnsemble(models2, FunctionalTiedSAE, adam, {"lr": 1e-3},
                                     device=DEV, backend="torch")
        x = torch.randn(B, d, device=DEV)
        for step in range(3):
            l_hip, _ = ens_hip.step_batch(x)
            l_ref, _ = ens_ref.step_batch(x)
            assert _rel_err(l_hip["loss"], l_ref["loss"]) < 5e-4, (d, ratio, step)
        for k in ens_ref.params:
            assert torch.isfinite(ens_hip.params[k]).all(), (d, ratio, k)
        del ens_hip, ens_ref
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", range(10))
def test_shape_fuzz_gemm_kernels(case, kcfg):
    """Seeded random shapes (d,n multiples of 4; arbitrary B, M) through
    enc/dec/gc/grad_w vs einsum — edge-guard fuzzing beyond the two fixed
    odd shapes."""
    ext = _ext()
    g = torch.Generator().manual_seed(1000 + case)

    def r(lo, hi, mult=1):
        return int(torch.randint(lo, hi, (1,), generator=g)) * mult

    M, B, d, n = r(1, 5), r(3, 70), r(1, 80, 4), r(1, 90, 4)
    torch.manual_seed(case)
    x = torch.randn(B, d, device=DEV)
    W = torch.randn(M, n, d, device=DEV) * 0.3
    bias = torch.randn(M, n, device=DEV) * 0.1
    c = torch.empty(M, B, n, device=DEV)
    lp = torch.zeros(M, 2, device=DEV)
    fired = torch.zeros(M, n, device=DEV)
    ext.enc_fwd(x, W, bias, None, c, lp, fired, 0, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    ref_c = torch.clamp(torch.einsum("mnd,bd->mbn", W, x) + bias[:, None, :], min=0)
    assert _rel_err(c, ref_c) < 1e-4, (M, B, d, n)

    norms = torch.empty(M, n, device=DEV)
    inv = torch.empty(M, n, device=DEV)
    ext.row_norms(W, norms, inv, 1e-8)
    rr = torch.empty(M, B, d, device=DEV)
    ext.dec_fwd(c, W, inv, x, rr, lp, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    What = W / torch.clamp(torch.norm(W, dim=-1, keepdim=True), 1e-8)
    ref_r = torch.einsum("mnd,mbn->mbd", What, ref_c) - x
    assert _rel_err(rr, ref_r) < 1e-4, (M, B, d, n)

    gw = torch.zeros(M, n, d, device=DEV)
    ext.grad_w(c, rr, gw, 1.0, 0.0, kcfg["bk"], kcfg["prio"], kcfg["bn"])
    ref_gw = torch.einsum("mbn,mbd->mnd", ref_c, ref_r)
    assert _rel_err(gw, ref_gw) < 1e-4, (M, B, d, n)

"""The fp64 references and comparators of tests/hip_reference.py, checked on
the CPU: fp32 CPU computations stand in for the kernels and must be accepted;
each of a list of injected kernel faults must be rejected; every hand-written
reference must equal fp64 autograd through the signature code to 1e-12.  The
last test covers the staging fix that goes with the GPU suite's ragged steps."""

import pytest
import torch

from tests import hip_reference as R

M, B, D, N = 2, 130, 68, 260  # the GPU suite's main shape: tails on every axis


def _inv32(W):
    return 1.0 / torch.clamp(W.norm(dim=-1), min=1e-8)


def _enc32(x, W, bias):
    """fp32 CPU einsum standing in for k_enc_fwd_t mode 0 (tied: scaled rows)."""
    Wh = W * _inv32(W)[..., None]
    return torch.clamp(torch.einsum("bd,mnd->mbn", x, Wh) + bias[:, None, :], min=0.0)


@pytest.fixture(scope="module")
def enc():
    inp = R.gemm_inputs(M, B, D, N, seed=1)
    ref = R.enc_relu(inp["x"], inp["W"], inp["bias"], True)
    return inp, ref, _enc32(inp["x"], inp["W"], inp["bias"])


@pytest.fixture(scope="module")
def gcase():
    inp = R.gemm_inputs(M, B, D, N, seed=2)
    gen = inp["gen"]
    r = inp["xm"]
    c = torch.clamp(torch.randn(M, B, N, generator=gen), min=0.0)
    l1 = torch.tensor([1e-3, 1e-2])
    ref = R.gc(r, inp["W"], c, l1, 0)
    Wh = inp["W"] * _inv32(inp["W"])[..., None]
    g = (2.0 / (B * D)) * torch.einsum("mbd,mnd->mbn", r, Wh) + (l1 / B)[:, None, None]
    return ref, torch.where(c > 0, g, torch.zeros_like(g))


def test_comparator_accepts_fp32_einsum(enc, gcase):
    inp, ref, got = enc
    stats = R.check("enc", got, ref["c"], ref["e"])
    assert 0 < stats["worst"] <= 1
    lo, hi = R.fired_range(ref["on"], ref["undecided"], torch.full((M, N), 3.0))
    R.check_counts("fired", 3.0 + (got > 0).float().sum(dim=1), lo, hi)
    R.sum_check("l1", 5.0 + got.sum(dim=(1, 2)), torch.full((M,), 5.0), ref["c"], ref["e"],
                R.epi_sum_depth(B, N), (1, 2))
    gref, ggot = gcase
    R.check("gpre", ggot, gref["gpre"], gref["e"])
    R.sum_check("g_bias", ggot.sum(dim=1), torch.zeros(M, N), gref["gpre"], gref["e"],
                R.col_sum_depth(B), 1)


def test_rejects_small_relative_error_in_a_small_tail_row(enc):
    """2^-12 relative to itself, in a row 2^-10 and less of the large ones: far
    below any max-norm tolerance, far above the componentwise bound."""
    inp, ref, got = enc
    assert inp["x"][B - 1].abs().max() < 2.0 ** -6 and inp["x"].abs().max() > 2.0 ** 9
    j = int((ref["c"][1, B - 1] / ref["e"][1, B - 1].clamp_min(1e-300)).argmax())
    assert ref["c"][1, B - 1, j] * 2.0 ** -12 > 4 * ref["e"][1, B - 1, j]
    bad = got.clone()
    bad[1, B - 1, j] *= 1.0 + 2.0 ** -12
    assert (bad - got).abs().max() / got.abs().max() < 1e-7  # invisible to the max-norm measure
    with pytest.raises(R.Mismatch):
        R.check("enc", bad, ref["c"], ref["e"])


def test_rejects_dropped_last_k_term(enc):
    inp, ref, _ = enc
    Wh = inp["W"] * _inv32(inp["W"])[..., None]
    bad = torch.clamp(torch.einsum("bd,mnd->mbn", inp["x"][:, :-1], Wh[..., :-1])
                      + inp["bias"][:, None, :], min=0.0)
    with pytest.raises(R.Mismatch):
        R.check("enc", bad, ref["c"], ref["e"])


def test_rejects_swapped_tail_rows(enc):
    _, ref, got = enc
    bad = got.clone()
    bad[:, [B - 1, B - 2]] = got[:, [B - 2, B - 1]]
    with pytest.raises(R.Mismatch):
        R.check("enc", bad, ref["c"], ref["e"])


@pytest.mark.parametrize("group", [0, 3, 4])
def test_rejects_column_sum_missing_a_row_group(gcase, group):
    """A bias gradient that lost one 32-row group's partial (group 4 is the
    2-row tail group)."""
    gref, ggot = gcase
    keep = torch.ones(B, dtype=torch.bool)
    keep[32 * group:32 * (group + 1)] = False
    with pytest.raises(R.Mismatch):
        R.sum_check("g_bias", ggot[:, keep].sum(dim=1), torch.zeros(M, N), gref["gpre"], gref["e"],
                    R.col_sum_depth(B), 1)


def test_rejects_topk_with_one_wrong_member():
    gen = torch.Generator().manual_seed(3)
    s = torch.randn(2, 7, 1000, generator=gen)
    ks = (7, 40)
    c, fired = R.topk_ref(s, ks)
    R.check_bits("c", R.canon_zero(c), R.canon_zero(c.clone()))
    # the 7th member of one row replaced by the runner-up
    order = torch.argsort(s[0, 3], descending=True)
    bad = c.clone()
    bad[0, 3, order[6]] = 0.0
    bad[0, 3, order[7]] = torch.clamp(s[0, 3, order[7]], min=0.0)
    with pytest.raises(R.Mismatch):
        R.check_bits("c", R.canon_zero(bad), R.canon_zero(c))
    # the tie rule: any choice among the tied scores passes, a wrong member does not
    t = (torch.randn(2, 7, 1000, generator=gen) * 4).round() / 4 + 8.0
    t = t.clamp_min(0.25)
    ct, _ = R.topk_ref(t, ks)
    R.check_topk_properties("ties", t, ct, ks)
    order = torch.argsort(t[1, 2], descending=True, stable=True)
    lowest = order[-1]
    assert t[1, 2, lowest] < t[1, 2, order[39]]
    bad = ct.clone()
    bad[1, 2, order[0]] = 0.0
    bad[1, 2, lowest] = t[1, 2, lowest]
    with pytest.raises(R.Mismatch):
        R.check_topk_properties("ties", t, bad, ks)
    bad = ct.clone()
    bad[1, 2, order[0]] = 0.0  # one slot short
    with pytest.raises(R.Mismatch):
        R.check_topk_properties("ties", t, bad, ks)


def _resample_inputs(n=600, d=12, Mr=2, n_track=64, seed=4):
    gen = torch.Generator().manual_seed(seed)
    fired = torch.randint(1, 9, (Mr, n), generator=gen).float()
    fired[torch.rand(Mr, n, generator=gen) < 0.3] = 0.0
    fired[:, [0, 63, 64, 255, 256, 599]] = 0.0
    t = lambda *s: torch.randn(*s, generator=gen)
    return dict(fired=fired, new_rows=t(Mr, n_track, d), enc_scale=torch.tensor([0.2, 0.7]),
                W=t(Mr, n, d), mu_w=t(Mr, n, d), nu_w=t(Mr, n, d).abs())


def test_rejects_resample_ranked_per_segment():
    inp = _resample_inputs(n_track=700)
    good = R.resample_ref(**inp)
    again = R.resample_ref(**inp)
    seg = R.resample_ref(**inp, per_segment=256)
    for k in ("W", "mu_w", "nu_w"):
        R.check_bits(k, again[k], good[k])
    with pytest.raises(R.Mismatch):
        R.check_bits("W", seg["W"], good["W"])
    # the replaced rows are the first n_track dead ones in index order
    dead0 = torch.where(inp["fired"][0] == 0)[0]
    assert torch.equal(good["W"][0, dead0[5]], inp["new_rows"][0, 5] * inp["enc_scale"][0])
    assert int(good["counts"][0]) == min(dead0.numel(), 700)


def _close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= tol * (b.abs() + b.abs().mean())).all())


def _thresh_case(Mt=2, Bt=33, d=20, n=36, seed=5):
    inp = R.gemm_inputs(Mt, Bt, d, n, seed)
    gen = inp["gen"]
    scale = 0.5 + torch.rand(Mt, n, generator=gen)
    scale[:, 1] = 5e-5  # a^2 < 1e-8: the clamp is active
    u = 0.95 + 0.12 * torch.randn(Mt, Bt, n, generator=gen)
    c = R.gate_g(u) * scale[:, None, :] ** 2
    return inp["xm"], inp["W"], c, u, scale, torch.tensor([1e-3, 1e-2])


def test_gc_thresh_reference_matches_autograd():
    r, W, c, u, scale, l1 = _thresh_case()
    ref = R.gc_thresh(r, W, c, u, scale, l1)
    gpre, g_gain, g_scale = R.gc_thresh_autograd(ref["gv"], u, scale)
    assert ((u > 0.9) & (u < 1.0)).any() and (u > 1.0).any() and (u < 0.9).any()
    assert _close(ref["gpre"], gpre)
    assert _close(ref["gpre"].sum(dim=1), g_gain)
    assert _close(ref["t_scale"].sum(dim=1), g_scale)
    assert g_scale[:, 1].abs().max() > 0  # the clamped column still gets the g(u) 2a term
    # and an fp32 run of the same autograd is inside the bounds
    with R.stand_in_precision():
        gpre32, g_gain32, g_scale32 = R.gc_thresh_autograd(ref["gv"], u, scale)
    R.check("gpre", gpre32, ref["gpre"], ref["e_gpre"], ref["undecided"])
    R.sum_check("g_gain", g_gain32, torch.zeros(2, 36), ref["gpre"], ref["e_gpre"], R.col_sum_depth(33), 1,
                slack=ref["flip_gain"].sum(dim=1))
    R.sum_check("g_scale", g_scale32, torch.zeros(2, 36), ref["t_scale"], ref["e_t"], R.col_sum_depth(33), 1,
                slack=ref["flip_scale"].sum(dim=1))


def _lista_case(Ml=2, Bl=9, n=12, seed=6, carry=True):
    gen = torch.Generator().manual_seed(seed)
    r = torch.randint(-8, 9, (Ml, Bl, n), generator=gen).float() / 4
    theta = torch.full((Ml, n), 0.5)
    x = torch.sign(r) * torch.clamp(r.abs() - 0.5, min=0.0)
    t = lambda: torch.randn(Ml, Bl, n, generator=gen)
    return dict(g_y=t(), carry_in=t() if carry else None, r=r, theta=theta, x=x, x_prev=t(),
                mom=torch.tensor([0.1, 0.6]))


@pytest.mark.parametrize("carry", [True, False])
def test_lista_bwd_reference_matches_autograd(carry):
    k = _lista_case(carry=carry)
    assert (k["r"].abs() == 0.5).any() and (k["r"] == 0).any()
    ref = R.lista_bwd(**k)
    g_r, carry_out, g_theta, g_rho = R.lista_bwd_autograd(
        k["g_y"], k["carry_in"], k["r"], k["theta"], k["x_prev"], k["mom"])
    assert _close(ref["g_r"], g_r)
    assert _close(ref["carry"], carry_out)
    assert _close(ref["t_theta"].sum(dim=1), g_theta)
    assert _close(ref["t_rho"].sum(dim=(1, 2)), g_rho)
    assert (ref["g_r"][k["r"].abs() == 0.5] == 0).all()  # the mask is strict


def _adam_case(Ma=3, n=10, d=20, seed=7):
    gen = torch.Generator().manual_seed(seed)
    t = lambda *s: torch.randn(*s, generator=gen)
    W = t(Ma, n, d)
    W[0, 0] = 1e-10 * t(d)  # norm <= eps_norm
    return dict(W=W, gw=t(Ma, n, d), mu=0.1 * t(Ma, n, d), nu=0.01 * t(Ma, n, d).abs() + 1e-4,
                step=torch.tensor([1.0, 7.0, 1000.0]),
                lr_mult=(torch.rand(Ma, n, 1, generator=gen) > 0.3).float()
                * torch.rand(Ma, n, 1, generator=gen))


HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


@pytest.mark.parametrize("project,clamp", [(True, False), (False, False), (True, True)])
def test_project_adam_reference_matches_autograd(project, clamp):
    k = _adam_case()
    w_used = torch.clamp(k["W"], min=0.0) if clamp else None
    g, e_g = R.project_grad(k["W"], k["gw"], project, w_used, clamp)
    g_auto = R.project_grad_autograd(k["W"], k["gw"], project, clamp)
    assert _close(g, g_auto)
    ref = R.adam_chain(k["W"], g, e_g, k["mu"], k["nu"], k["step"], lr_mult=k["lr_mult"], **HYP)
    p, mu, nu = R.adam_autograd(k["W"], g_auto, k["mu"], k["nu"], k["step"], lr_mult=k["lr_mult"], **HYP)
    assert _close(ref["p"], p) and _close(ref["mu"], mu) and _close(ref["nu"], nu)
    # fp32 through the same signature code stays inside the bounds
    with R.stand_in_precision():
        g32 = R.project_grad_autograd(k["W"], k["gw"], project, clamp)
        p32, mu32, nu32 = R.adam_autograd(k["W"], g32, k["mu"], k["nu"], k["step"],
                                          lr_mult=k["lr_mult"], **HYP)
    assert p32.dtype == torch.float32
    R.check("W", p32, p, ref["e_p"])
    R.check("mu", mu32, mu, ref["e_mu"])
    R.check("nu", nu32, nu, ref["e_nu"])
    # and a wrong bias correction (step t-1 for t) does not
    wrong = R.adam_autograd(k["W"], g_auto, k["mu"], k["nu"], k["step"] + 1.0, lr_mult=k["lr_mult"], **HYP)[0]
    with pytest.raises(R.Mismatch):
        R.check("W", wrong, p, ref["e_p"])


@pytest.mark.parametrize("decay", [False, True])
def test_bias_adam_reference_matches_autograd(decay):
    gen = torch.Generator().manual_seed(8)
    Ma, n = 3, 50
    bias = torch.randn(Ma, n, generator=gen)
    bias[2] = 0.0  # decay gradient at 0 is 0
    gb = torch.randn(Ma, n, generator=gen)
    mu, nu = 0.1 * torch.randn(Ma, n, generator=gen), 0.01 * torch.rand(Ma, n, generator=gen) + 1e-4
    bd = torch.tensor([0.01, 0.1, 0.05]) if decay else torch.zeros(Ma)
    step = torch.tensor([1.0, 7.0, 1000.0])
    g, e_g = R.bias_grad(bias, gb, bd)
    g_auto = R.bias_grad_autograd(bias, gb, bd)
    assert _close(g, g_auto)
    assert torch.equal(g_auto[2], gb[2].double())
    ref = R.adam_chain(bias, g, e_g, mu, nu, step, **HYP)
    p, m1, v1 = R.adam_autograd(bias, g_auto, mu, nu, step, **HYP)
    assert _close(ref["p"], p) and _close(ref["mu"], m1) and _close(ref["nu"], v1)
    with R.stand_in_precision():
        p32, m32, v32 = R.adam_autograd(bias, R.bias_grad_autograd(bias, gb, bd), mu, nu, step, **HYP)
    R.check("bias", p32, p, ref["e_p"])
    R.check("mu", m32, m1, ref["e_mu"])
    R.check("nu", v32, v1, ref["e_nu"])


def test_forward_references_accept_fp32_signature_code():
    """gate / LISTA layer / reverse code / decoder: the signature code run in
    fp32 on the CPU is inside the bounds derived for the kernels."""
    inp = R.gemm_inputs(M, 33, 20, 36, seed=9)
    gen = inp["gen"]
    x, W = inp["x"], inp["W"]
    scale = 0.5 + torch.rand(M, 36, generator=gen)
    scale[:, 1] = 5e-5
    gain = scale ** 2 * (0.95 + 0.1 * torch.randn(M, 36, generator=gen))
    ref = R.enc_gate(x, W, scale, gain)
    with R.stand_in_precision():
        got = R.enc_gate(x, W, scale, gain)
    assert got["c"].dtype == torch.float32
    R.check("gate code", got["c"], ref["c"], ref["e"])
    R.check("gate u", got["u"], ref["u"], ref["e_u"])
    assert (ref["u"] > 1.0).any() and ((ref["u"] > 0.9) & (ref["u"] < 1.0)).any() and (ref["u"] < 0.9).any()

    y, xp = inp["xm"][..., :1] * torch.randn(M, 33, 36, generator=gen), torch.randn(M, 33, 36, generator=gen)
    theta, mom = 0.02 * torch.randn(M, 36, generator=gen), torch.tensor([0.1, 0.6])
    ref = R.enc_lista(inp["xm"], W, y, xp, theta, mom)
    with R.stand_in_precision():
        got = R.enc_lista(inp["xm"], W, y, xp, theta, mom)
    for k, e in (("r", "e_r"), ("x", "e_x"), ("y", "e_y")):
        R.check("lista " + k, got[k], ref[k], ref[e])

    ref = R.enc_reverse(x, W, inp["bias"])
    with R.stand_in_precision():
        got = R.enc_reverse(x, W, inp["bias"])
    assert (ref["c"] < 0).any()
    R.check("reverse", got["c"], ref["c"], ref["e"], ref["undecided"])

    c = torch.clamp(inp["xm"][..., :1] * torch.randn(M, 33, 36, generator=gen), min=0.0)
    ref = R.dec(c, W, x)
    with R.stand_in_precision():
        got = R.dec(c, W, x)
    R.check("dec", got["r"], ref["r"], ref["e"])


def test_row_norms_reference_accepts_fp32_and_clamps():
    gen = torch.Generator().manual_seed(10)
    W = torch.randn(15, 256, generator=gen)
    W[3] = 0.0
    W[7] = 2.0 ** -70
    ref = R.row_norms(W, 1e-8)
    R.check("norms", W.norm(dim=-1), ref["norms"], ref["e_norms"])
    R.check("inv", 1.0 / torch.clamp(W.norm(dim=-1), min=1e-8), ref["inv"], ref["e_inv"])
    assert ref["inv"][3] == 1e8 and ref["inv"][7] == 1e8 and not ref["undecided"].any()
    with pytest.raises(R.Mismatch):  # an unclamped inverse
        R.check("inv", 1.0 / W.norm(dim=-1), ref["inv"], ref["e_inv"])


@pytest.mark.parametrize("shape", [(192, 96, 160), (130, 68, 132), (33, 20, 36)])
def test_undecided_share_of_the_references(shape):
    """The references alone leave far fewer than 0.5 % of the elements
    undecided with these inputs."""
    Bs, d, n = shape
    inp = R.gemm_inputs(M, Bs, d, n, seed=11)
    gen = inp["gen"]
    scale = 0.5 + torch.rand(M, n, generator=gen)
    gain = scale ** 2 * (0.95 + 0.1 * torch.randn(M, n, generator=gen))
    shares = {
        "relu": R.enc_relu(inp["x"], inp["W"], inp["bias"], True)["undecided"],
        "reverse": R.enc_reverse(inp["x"], inp["W"], inp["bias"])["undecided"],
        "gate": R.enc_gate(inp["x"], inp["W"], scale, gain)["undecided"],
    }
    for k, und in shares.items():
        share = und.double().mean().item()
        print(f"undecided {k} (B,d,n)={shape}: {share:.2e}")
        assert share <= R.MAX_UNDECIDED / 5, (k, share)


@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
def test_pre_staging_resolves_to_t_for_a_ragged_batch(tied):
    """The fix that goes with the ragged full-step GPU test, seen through the
    launch recorder: under staging="pre" a batch size that is no multiple of 4
    gets the transpose-in-staging chain and workspaces (the pre-transposed
    operands have leading dimension B and are staged as float4), decided once
    per allocation; a later batch of a good size goes back to "pre"."""
    from sparse_coding_amd.engine import hip_step as hs
    from sparse_coding_amd.models import sae_signatures as sigs
    from sparse_coding_amd.ops.kconfig import DEFAULTS, kernel_config, set_kernel_config
    from tests.test_hip_step_trace import RecordingExt, _ensemble

    sig = sigs.FunctionalTiedSAE if tied else sigs.FunctionalSAE

    def launches(staging, batches):
        old = kernel_config()
        set_kernel_config(**dict(DEFAULTS, staging=staging))
        try:
            torch.manual_seed(0)
            ext = RecordingExt()
            step = hs.HipSAEStep(_ensemble(sig, [sig.init(32, 64, l1) for l1 in (1e-3, 3e-3)]), ext, tied=tied)
            ext.step = step
            out = []
            for Bq in batches:
                ext.x = x = torch.randn(Bq, 32)
                del ext.calls[:]
                step.update_phase(step.grads_phase(x))
                out.append((step.kc["staging"], [fn for fn, _ in ext.calls], hasattr(step, "xT")))
            return out
        finally:
            set_kernel_config(**old)

    (s90, pre90, _), (s92, pre92, has_xT) = launches("pre", [90, 92])
    (_, t90, t_has_xT), = launches("t", [90])
    assert s90 == "t" and pre90 == t90 and "enc_fwd2" not in pre90 and not t_has_xT
    assert s92 == "pre" and has_xT and "enc_fwd2" in pre92 and "gc2" in pre92

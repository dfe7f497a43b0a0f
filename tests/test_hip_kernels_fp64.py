"""Every launcher of ops/hip/sae_ops.hip against an fp64 CPU reference with
derived componentwise bounds (tests/hip_reference.py), at shapes with tails on
every axis, with power-of-two row scales 2^-10..2^10 on the inputs, and with
every accumulated output started from a nonzero value.

Branch -> test
  enc_fwd  mode 0, dict_sizes, shared / per-model x   test_enc_fwd_relu
           mode 1 (side outputs untouched)            test_enc_fwd_raw
           mode 2 gate, clamped a^2 column            test_enc_fwd_gate
           mode 3 reverse                             test_enc_fwd_reverse
           mode 4 LISTA layer, inv_norms absent       test_enc_fwd_lista
           mode 5 y_in - acc                          test_enc_fwd_sub
  dec_fwd  shared / per-model x                       test_dec_fwd
  gc       gc_mode 0, accumulate on / off             test_gc[0-*]
           gc_mode 1 (g_bias untouched)               test_gc[1-*]
  gc_thresh                                           test_gc_thresh
  grad_w   alpha/beta, shared / per-model Q           test_grad_w
  colsum   plain / absval, split and unsplit batch    test_colsum
  transpose_scale  3-D + scale, 2-D no scale          test_transpose_scale
  enc_fwd2 mode 0 + dict_sizes, mode 1; gc2 mode 0/1  test_enc_fwd2_gc2
  row_norms  float4 path (d % 256 == 0) and scalar    test_row_norms
  topk_select  distinct, specials, k = 0, ties        test_topk_select_*
  resample  none/mixed/all dead, early break,
            with and without dec / bias               test_resample
  lista_bwd_elem  carry_in absent / present           test_lista_bwd_elem
  project_adam  project on / off, norm <= eps_norm,
            w_used + clamp_mask, lr_mult absent /
            with zeros, per-model step t > 1          test_project_adam
  bias_adam  decay off / on, zero bias, lr_mult       test_bias_adam
  HipSAEStep ragged batch under staging t / pre       test_ragged_full_step
"""

import functools

import pytest
import torch

from tests import hip_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (bk, prio, bn): the compiled GEMM variants
VARIANTS = [(32, False, 128), (16, True, 128), (16, False, 256)]
VARIANTS_128 = VARIANTS[:2]
_vid = lambda v: f"bk{v[0]}-p{int(v[1])}-bn{v[2]}"
variants = pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
variants_128 = pytest.mark.parametrize("variant", VARIANTS_128, ids=_vid)

# (M, B, d, n): a 2-row row tile, K tail of 4 at both depths, column tails of 4
# at both widths / K smaller than the tile depth / exactly one tile
SHAPES = [(2, 130, 68, 260), (2, 5, 4, 4), (1, 128, 32, 128)]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))


def _ext():
    from sparse_coding_amd import ops

    return ops.get_extension()


def g(t):
    return t.to(DEV).contiguous()


def _report(name, *stats):
    print(f"[fp64] {name}: " + " ".join(
        f"worst={s['worst']:.3f} undecided={s['undecided']:.2e}" for s in stats))


def _randn(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(5 + sum(shape)))


def _per_model(vals, M):
    return torch.tensor(vals[:M], dtype=torch.float32)


def _dict_sizes(M, n):
    return [n, max(n - 3, 1)][:M] if M > 1 else [max(n - 3, 1)]


def _inv_norms(ext, W_dev):
    norms = torch.empty(W_dev.shape[:-1], device=DEV)
    inv = torch.empty_like(norms)
    ext.row_norms(W_dev, norms, inv, R.EPS_NORM)
    return norms, inv


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed=100):
    return R.gemm_inputs(*shape, seed=seed + sum(shape))


def _x(inp, per_model):
    return inp["xm"] if per_model else inp["x"]


# ---------------------------------------------------------------------------
# enc_fwd
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _relu_ref(shape, per_model):
    inp = _inputs(shape)
    ds = _dict_sizes(shape[0], shape[3])
    return ds, R.enc_relu(_x(inp, per_model), inp["W"], inp["bias"], True, ds)


@variants
@shapes
@pytest.mark.parametrize("per_model", [False, True], ids=["xshared", "xpermodel"])
def test_enc_fwd_relu(variant, shape, per_model):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    ds, ref = _relu_ref(shape, per_model)
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    c = torch.full((M, B, n), float("nan"), device=DEV)
    lp0 = torch.tensor([[3.0, 5.0]]).repeat(M, 1)
    fired0 = torch.full((M, n), 2.0)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd(g(_x(inp, per_model)), W, g(inp["bias"]), inv, c, lp, fired, 0, bk, prio, bn,
                dict_sizes=g(torch.tensor(ds, dtype=torch.int32)))
    st = R.check("c", c, ref["c"], ref["e"])
    for m in range(M):  # masked columns exactly zero
        assert (c[m, :, ds[m]:] == 0).all()
    lo, hi = R.fired_range(ref["on"], ref["undecided"], fired0)
    R.check_counts("fired", fired, lo, hi)
    st2 = R.sum_check("l1", lp[:, 1], lp0[:, 1], ref["c"], ref["e"], R.epi_sum_depth(B, n, bn), (1, 2))
    R.check_bits("loss_parts[:,0]", lp[:, 0].cpu(), lp0[:, 0])
    assert ref["undecided"].double().mean().item() <= R.MAX_UNDECIDED
    _report("enc_fwd relu", st, st2)


@variants
@shapes
def test_enc_fwd_raw(variant, shape):
    """mode 1 writes the raw scores and nothing else: bias ignored, loss_parts
    and fired bit for bit what they were."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    ref = R.enc_raw(inp["x"], inp["W"], True)
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    c = torch.full((M, B, n), float("nan"), device=DEV)
    lp0, fired0 = _randn(M, 2), _randn(M, n)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd(g(inp["x"]), W, g(inp["bias"]), inv, c, lp, fired, 1, bk, prio, bn)
    st = R.check("scores", c, ref["c"], ref["e"])
    R.check_bits("loss_parts", lp.cpu(), lp0)
    R.check_bits("fired", fired.cpu(), fired0)
    _report("enc_fwd raw", st)


@functools.lru_cache(maxsize=None)
def _gate_case(shape):
    inp = _inputs(shape)
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(7)
    scale = 0.5 + torch.rand(M, n, generator=gen)
    scale[:, 1] = 5e-5  # a^2 = 2.5e-9 < 1e-8: the clamp of the gate is active
    # the small rows of x (|pre| ~ 1e-3) then have u = 0.95 +- 0.1: both knees
    gain = scale ** 2 * (0.95 + 0.1 * torch.randn(M, n, generator=gen))
    return scale, gain, R.enc_gate(inp["x"], inp["W"], scale, gain)


@variants
@shapes
def test_enc_fwd_gate(variant, shape):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    scale, gain, ref = _gate_case(shape)
    if B > 100:
        u = ref["u"]
        assert (u < 0.9).any() and ((u > 0.9) & (u < 1.0)).any() and (u > 1.0).any()
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    c = torch.full((M, B, n), float("nan"), device=DEV)
    u_out = torch.full((M, B, n), float("nan"), device=DEV)
    lp0, fired0 = torch.tensor([[3.0, 5.0]]).repeat(M, 1), torch.full((M, n), 2.0)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd(g(inp["x"]), W, g(torch.zeros(M, n)), inv, c, lp, fired, 2, bk, prio, bn,
                act_scale=g(scale), act_gain=g(gain), u_out=u_out)
    st_u = R.check("u", u_out, ref["u"], ref["e_u"])
    st_c = R.check("code", c, ref["c"], ref["e"])
    lo, hi = R.fired_range(ref["on"], ref["undecided"], fired0)
    R.check_counts("fired", fired, lo, hi)
    st_l = R.sum_check("l1", lp[:, 1], lp0[:, 1], ref["c"], ref["e"], R.epi_sum_depth(B, n, bn), (1, 2))
    R.check_bits("loss_parts[:,0]", lp[:, 0].cpu(), lp0[:, 0])
    assert ref["undecided"].double().mean().item() <= R.MAX_UNDECIDED
    _report("enc_fwd gate", st_u, st_c, st_l)


@functools.lru_cache(maxsize=None)
def _reverse_ref(shape):
    inp = _inputs(shape)
    return R.enc_reverse(inp["x"], inp["W"], inp["bias"])


@variants
@shapes
def test_enc_fwd_reverse(variant, shape):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    ref = _reverse_ref(shape)
    assert (ref["c"] < 0).any() and (ref["c"] > 0).any()
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    c = torch.full((M, B, n), float("nan"), device=DEV)
    lp0, fired0 = torch.tensor([[3.0, 5.0]]).repeat(M, 1), torch.full((M, n), 2.0)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd(g(inp["x"]), W, g(inp["bias"]), inv, c, lp, fired, 3, bk, prio, bn)
    st = R.check("code", c, ref["c"], ref["e"], ref["undecided"])
    lo, hi = R.fired_range(ref["on"], ref["undecided"], fired0)
    R.check_counts("fired", fired, lo, hi)
    st_l = R.sum_check("l1 = sum|code|", lp[:, 1], lp0[:, 1], ref["c"].abs(), ref["e"],
                       R.epi_sum_depth(B, n, bn), (1, 2), slack=ref["flip"].sum(dim=(1, 2)))
    R.check_bits("loss_parts[:,0]", lp[:, 0].cpu(), lp0[:, 0])
    _report("enc_fwd reverse", st, st_l)


@functools.lru_cache(maxsize=None)
def _lista_case(shape):
    inp = _inputs(shape)
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(8)
    y = R.scaled_randn(gen, M, B, n)
    x_prev = R.scaled_randn(gen, M, B, n)
    theta = 0.05 * torch.rand(M, n, generator=gen)
    theta[:, 0] = 0.0
    mom = _per_model([0.1, 0.6], M)
    return y, x_prev, theta, mom, R.enc_lista(inp["xm"], inp["W"], y, x_prev, theta, mom)


@variants
@shapes
def test_enc_fwd_lista(variant, shape):
    """mode 4: r, x = shrink(r, theta) and y' = x + m (x - x_prev) against
    LISTALayer.forward; per-model momentum, nonzero x_prev, no inv_norms."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    y, x_prev, theta, mom, ref = _lista_case(shape)
    nan = lambda: torch.full((M, B, n), float("nan"), device=DEV)
    c, u_out, x_out = nan(), nan(), nan()
    lp0, fired0 = _randn(M, 2), _randn(M, n)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd(g(inp["xm"]), g(inp["W"]), g(torch.ones(M, n)), None, c, lp, fired, 4, bk, prio, bn,
                act_scale=g(theta), u_out=u_out, y_in=g(y), x_prev=g(x_prev), x_out=x_out, mom=g(mom))
    st = [R.check("r", u_out, ref["r"], ref["e_r"]), R.check("x", x_out, ref["x"], ref["e_x"]),
          R.check("y'", c, ref["y"], ref["e_y"])]
    if B > 100:
        assert (ref["x"] == 0).any() and (ref["x"] > 0).any() and (ref["x"] < 0).any()
    R.check_bits("loss_parts", lp.cpu(), lp0)
    R.check_bits("fired", fired.cpu(), fired0)
    _report("enc_fwd lista", *st)


@variants
@shapes
def test_enc_fwd_sub(variant, shape):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    y = _lista_case(shape)[0]
    ref = R.enc_sub(inp["xm"], inp["W"], y)
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    c = torch.full((M, B, n), float("nan"), device=DEV)
    lp0, fired0 = _randn(M, 2), _randn(M, n)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd(g(inp["xm"]), W, g(torch.ones(M, n)), inv, c, lp, fired, 5, bk, prio, bn, y_in=g(y))
    st = R.check("y - acc", c, ref["c"], ref["e"])
    R.check_bits("loss_parts", lp.cpu(), lp0)
    R.check_bits("fired", fired.cpu(), fired0)
    _report("enc_fwd sub", st)


# ---------------------------------------------------------------------------
# dec_fwd, gc, gc_thresh, grad_w, colsum
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _codes(shape, signed=False):
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(9)
    c = R.scaled_randn(gen, M, B, n)
    c[torch.rand(M, B, n, generator=gen) < 0.3] = 0.0
    return c if signed else torch.clamp(c, min=0.0)


@functools.lru_cache(maxsize=None)
def _dec_ref(shape, per_model):
    inp = _inputs(shape)
    return R.dec(_codes(shape), inp["W"], _x(inp, per_model))


@variants
@shapes
@pytest.mark.parametrize("per_model", [False, True], ids=["xshared", "xpermodel"])
def test_dec_fwd(variant, shape, per_model):
    """K is the dictionary size here (260: K tails at both depths)."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    ref = _dec_ref(shape, per_model)
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    r = torch.full((M, B, d), float("nan"), device=DEV)
    lp0 = torch.tensor([[3.0, 5.0]]).repeat(M, 1)
    lp = g(lp0)
    ext.dec_fwd(g(_codes(shape)), W, inv, g(_x(inp, per_model)), r, lp, bk, prio, bn)
    st = R.check("r", r, ref["r"], ref["e"])
    st_l = R.sum_check("mse", lp[:, 0], lp0[:, 0], ref["sq"], ref["e_sq"], R.epi_sum_depth(B, d, bn), (1, 2))
    R.check_bits("loss_parts[:,1]", lp[:, 1].cpu(), lp0[:, 1])
    _report("dec_fwd", st, st_l)


L1 = [1e-3, 1e-2]


@functools.lru_cache(maxsize=None)
def _gc_ref(shape, gc_mode):
    inp = _inputs(shape)
    return R.gc(inp["xm"], inp["W"], _codes(shape, signed=gc_mode == 1), _per_model(L1, shape[0]), gc_mode)


@variants
@shapes
@pytest.mark.parametrize("gc_mode", [0, 1])
def test_gc(variant, shape, gc_mode):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    ref = _gc_ref(shape, gc_mode)
    c = _codes(shape, signed=gc_mode == 1)
    if gc_mode == 1 and B > 100:
        assert (c < 0).any() and (c > 0).any() and (c == 0).any()
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    l1 = g(_per_model(L1, M))
    gb0 = _randn(M, n)
    for accumulate in (True, False):
        gpre = torch.full((M, B, n), float("nan"), device=DEV)
        gb = g(gb0)
        ext.gc(g(inp["xm"]), W, inv, g(c), l1, gpre, gb, bk, prio, gc_mode=gc_mode, bn=bn,
               accumulate=accumulate)
        st = R.check("gpre", gpre, ref["gpre"], ref["e"])
        if gc_mode == 1:  # the reverse code path gives the bias no gradient
            R.check_bits("g_bias", gb.cpu(), gb0)
            _report("gc reverse", st)
        else:
            start = gb0 if accumulate else torch.zeros(M, n)
            st_b = R.sum_check("g_bias", gb, start, ref["gpre"], ref["e"], R.col_sum_depth(B), 1)
            _report(f"gc accumulate={accumulate}", st, st_b)


@functools.lru_cache(maxsize=None)
def _thresh_case(shape):
    inp = _inputs(shape)
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(10)
    scale = 0.5 + torch.rand(M, n, generator=gen)
    scale[:, 1] = 5e-5
    u = 0.95 + 0.12 * torch.randn(M, B, n, generator=gen)
    u[:, : B // 2] *= R.row_scales(B // 2, gen, 0)[:, None] if B > 2 else 1.0
    c = (R.gate_g(u.double()) * scale[:, None, :].double() ** 2).float()
    l1 = _per_model(L1, M)
    ref = R.gc_thresh(inp["xm"], inp["W"], c, u, scale, l1)
    auto = R.gc_thresh_autograd(ref["gv"], u, scale)
    return scale, u, c, l1, ref, auto


@variants_128
@shapes
def test_gc_thresh(variant, shape):
    """gpre, g_gain, g_scale against fp64 autograd through the gate; the two
    column sums are added onto nonzero starts."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, _ = variant
    inp = _inputs(shape)
    scale, u, c, l1, ref, (gpre_ref, g_gain_ref, g_scale_ref) = _thresh_case(shape)
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    gpre = torch.full((M, B, n), float("nan"), device=DEV)
    gg0, gs0 = _randn(M, n), _randn(n, M).T.contiguous()
    gg, gs = g(gg0), g(gs0)
    ext.gc_thresh(g(inp["xm"]), W, inv, g(c), g(u), g(scale), g(l1), gpre, gg, gs, bk, prio)
    st = R.check("gpre", gpre, gpre_ref, ref["e_gpre"], ref["undecided"])
    depth = R.col_sum_depth(B)
    st_g = R.sum_check("g_gain", gg, gg0, ref["gpre"], ref["e_gpre"], depth, 1,
                       slack=ref["flip_gain"].sum(dim=1), total=g_gain_ref)
    st_s = R.sum_check("g_scale", gs, gs0, ref["t_scale"], ref["e_t"], depth, 1,
                       slack=ref["flip_scale"].sum(dim=1), total=g_scale_ref)
    _report("gc_thresh", st, st_g, st_s)


@variants
@shapes
def test_grad_w(variant, shape):
    """gw = beta gw + alpha P^T Q with K = B (130: K tails at both depths);
    shared and per-model Q.  c = c_dot(B) + 3 (alpha, beta, the add)."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    P = _codes(shape, signed=True)
    gw0 = torch.randn(M, n, d, generator=torch.Generator().manual_seed(11))
    for Q, eq in ((inp["xm"], "mbn,mbd->mnd"), (inp["x"], "mbn,bd->mnd")):
        acc, absdot = R.dot(eq, P, Q)
        gw = g(gw0)
        ext.grad_w(g(P), g(Q), gw, 0.5, -2.0, bk, prio, bn)
        ref = 0.5 * acc - 2.0 * gw0.double()
        st = R.check("gw", gw, ref, (R.c_dot(B) + 3) * R.U * (0.5 * absdot + 2.0 * gw0.double().abs()))
        gw = torch.full((M, n, d), float("nan"), device=DEV)  # beta = 0 never reads gw
        ext.grad_w(g(P), g(Q), gw, 1.0, 0.0, bk, prio, bn)
        st2 = R.check("gw beta=0", gw, acc, (R.c_dot(B) + 1) * R.U * absdot)
        _report("grad_w", st, st2)


@pytest.mark.parametrize("B", [130, 700])
@pytest.mark.parametrize("absval", [False, True])
def test_colsum(B, absval):
    """out = alpha sum_b X (or |X|): the batch is split over B // 256 blocks
    combined with atomics; the output is overwritten, not accumulated.  Depth:
    a slice's rows in one thread, one atomic per slice, the alpha product."""
    ext = _ext()
    M, n = 2, 260
    X = R.scaled_randn(torch.Generator().manual_seed(12), M, B, n)
    out = torch.full((M, n), float("nan"), device=DEV)
    ext.colsum(g(X), out, 0.25, absval)
    terms = 0.25 * (X.double().abs() if absval else X.double())
    nsplit = min(max(B // 256, 1), 16)
    st = R.sum_check("colsum", out, torch.zeros(M, n), terms, torch.zeros_like(terms),
                     R.cdiv(B, nsplit) + nsplit + 2, 1)
    _report("colsum", st)


# ---------------------------------------------------------------------------
# transpose_scale and the pre-transposed GEMMs
# ---------------------------------------------------------------------------

def test_transpose_scale():
    ext = _ext()
    gen = torch.Generator().manual_seed(13)
    src = torch.randn(3, 65, 130, generator=gen)
    scale = torch.randn(3, 65, generator=gen)
    dst = torch.full((3, 130, 65), float("nan"), device=DEV)
    ext.transpose_scale(g(src), dst, g(scale))
    R.check_bits("3-D scaled", dst.cpu(), (src * scale[..., None]).transpose(-1, -2).contiguous())
    src = torch.randn(130, 65, generator=gen)
    dst = torch.full((65, 130), float("nan"), device=DEV)
    ext.transpose_scale(g(src), dst, None)
    R.check_bits("2-D", dst.cpu(), src.transpose(-1, -2).contiguous())


@variants_128
def test_enc_fwd2_gc2(variant):
    """The all-direct-staged pair on the transposes k_transpose_scale makes,
    against the same references as enc_fwd / gc."""
    ext = _ext()
    shape = (2, 132, 68, 132)
    M, B, d, n = shape
    bk, prio, _ = variant
    inp = _inputs(shape)
    ds = _dict_sizes(M, n)
    W = g(inp["W"])
    _, inv = _inv_norms(ext, W)
    xT = torch.empty(d, B, device=DEV)
    WT = torch.empty(M, d, n, device=DEV)
    ext.transpose_scale(g(inp["x"]), xT, None)
    ext.transpose_scale(W, WT, inv)

    ref = R.enc_relu(inp["x"], inp["W"], inp["bias"], True, ds)
    c = torch.full((M, B, n), float("nan"), device=DEV)
    lp0, fired0 = torch.tensor([[3.0, 5.0]]).repeat(M, 1), torch.full((M, n), 2.0)
    lp, fired = g(lp0), g(fired0)
    ext.enc_fwd2(xT, WT, g(inp["bias"]), c, lp, fired, 0, bk, prio,
                 dict_sizes=g(torch.tensor(ds, dtype=torch.int32)))
    st = R.check("c", c, ref["c"], ref["e"])
    assert (c[1, :, ds[1]:] == 0).all()
    lo, hi = R.fired_range(ref["on"], ref["undecided"], fired0)
    R.check_counts("fired", fired, lo, hi)
    st_l = R.sum_check("l1", lp[:, 1], lp0[:, 1], ref["c"], ref["e"], R.epi_sum_depth(B, n), (1, 2))
    R.check_bits("loss_parts[:,0]", lp[:, 0].cpu(), lp0[:, 0])

    raw = R.enc_raw(inp["x"], inp["W"], True)
    s = torch.full((M, B, n), float("nan"), device=DEV)
    ext.enc_fwd2(xT, WT, g(inp["bias"]), s, lp, fired, 1, bk, prio)
    st_r = R.check("scores", s, raw["c"], raw["e"])
    _report("enc_fwd2", st, st_l, st_r)

    rT = torch.empty(M, d, B, device=DEV)
    ext.transpose_scale(g(inp["xm"]), rT, None)
    l1 = g(_per_model(L1, M))
    for gc_mode in (0, 1):
        code = _codes(shape, signed=gc_mode == 1)
        gref = R.gc(inp["xm"], inp["W"], code, _per_model(L1, M), gc_mode)
        gpre = torch.full((M, B, n), float("nan"), device=DEV)
        gb0 = torch.randn(M, n, generator=torch.Generator().manual_seed(14))
        gb = g(gb0)
        ext.gc2(rT, WT, g(code), l1, gpre, gb, bk, prio, gc_mode)
        st = R.check("gpre", gpre, gref["gpre"], gref["e"])
        if gc_mode == 1:
            R.check_bits("g_bias", gb.cpu(), gb0)
            _report("gc2 reverse", st)
        else:
            st_b = R.sum_check("g_bias", gb, gb0, gref["gpre"], gref["e"], R.col_sum_depth(B), 1)
            _report("gc2", st, st_b)


# ---------------------------------------------------------------------------
# row_norms
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", [256, 512, 68, 4])
def test_row_norms(d):
    """float4 path (d % 256 == 0) and scalar path; 15 rows (8 per block); an
    all-zero row and a row whose squares underflow must come out clamped."""
    ext = _ext()
    gen = torch.Generator().manual_seed(15)
    W = torch.randn(3, 5, d, generator=gen) * R.row_scales(5, gen, 0)[:, None]
    W[0, 3] = 0.0
    W[1, 2] = 2.0 ** -70
    ref = R.row_norms(W, R.EPS_NORM)
    assert not ref["undecided"].any()
    norms, inv = _inv_norms(ext, g(W))
    st = R.check("norms", norms, ref["norms"], ref["e_norms"])
    st_i = R.check("inv", inv, ref["inv"], ref["e_inv"])
    clamped = (torch.ones(1) / torch.tensor([R.EPS_NORM], dtype=torch.float32)).item()
    inv = inv.cpu()
    assert torch.isfinite(inv).all()
    assert inv[0, 3].item() == clamped and inv[1, 2].item() == clamped
    _report("row_norms", st, st_i)


# ---------------------------------------------------------------------------
# topk_select
# ---------------------------------------------------------------------------

def _topk_scores(n, seed):
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn(3, 7, n, generator=gen)
    s[:, 1] -= 3.0 if n > 4 else 5.0          # fewer than k positives
    s[:, 2, 0], s[:, 2, 1] = 0.0, -0.0        # both zeros (never at a k boundary)
    if n == 4:
        s[:, 2, 2], s[:, 2, 3] = 1.5, -2.0
    s[:, 3, 0], s[:, 3, 1], s[:, 3, 2] = 1e-40, -1e-40, 3e-42   # denormals
    s[:, 4, 0], s[:, 4, 1] = float("inf"), float("-inf")
    return s


@pytest.mark.parametrize("n", [4, 1000])
@pytest.mark.parametrize("ks", [(1, 7, None), (0, 3, 0)], ids=["k1-7-n+5", "k0"])
def test_topk_select_distinct(n, ks):
    """Distinct scores: c equals torch.topk + scatter + clamp bit for bit (up to
    the sign of a zero), fired is added onto a nonzero start."""
    ext = _ext()
    ks = tuple(n + 5 if k is None else k for k in ks)
    s = _topk_scores(n, 16)
    for b in (0, 1, 3, 4, 5, 6):
        assert all(s[m, b].unique().numel() == n for m in range(3))
    c_ref, inc = R.topk_ref(s, ks)
    c = torch.full((3, 7, n), float("nan"), device=DEV)
    fired0 = torch.full((3, n), 2.0)
    fired = g(fired0)
    ext.topk_select(g(s), c, fired, g(torch.tensor(ks, dtype=torch.int32)))
    R.check_bits("c", R.canon_zero(c), R.canon_zero(c_ref))
    R.check_bits("fired", fired.cpu(), fired0 + inc)
    for m, k in enumerate(ks):
        if k == 0:
            assert (c[m] == 0).all()


@pytest.mark.parametrize("n", [4, 1000])
def test_topk_select_ties(n):
    """Scores on a 1/4 grid, shifted positive so a selected slot shows."""
    ext = _ext()
    ks = (1, 7, n + 5)
    gen = torch.Generator().manual_seed(17)
    s = ((torch.randn(3, 7, n, generator=gen) * 4).round() / 4 + 8.0).clamp_min(0.25)
    s[:, 6] = 3.0  # a row that is one big tie
    c = torch.full((3, 7, n), float("nan"), device=DEV)
    fired0 = torch.full((3, n), 2.0)
    fired = g(fired0)
    ext.topk_select(g(s), c, fired, g(torch.tensor(ks, dtype=torch.int32)))
    R.check_topk_properties("ties", s, c, ks)
    R.check_bits("fired", fired.cpu(), fired0 + (c.cpu() > 0).float().sum(dim=1))


# ---------------------------------------------------------------------------
# resample
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_track", [1, 64, 700])
@pytest.mark.parametrize("dead", ["mixed", "none", "all"])
@pytest.mark.parametrize("extras", [False, True], ids=["enc-only", "dec+bias"])
def test_resample(n_track, dead, extras):
    """The index-order rule of the CPU resampler, bit for bit on every tensor:
    replaced rows, zeroed moments, untouched rest, exact counts.  n_track 1 and
    64 exhaust the budget in the first 256-column segment (the early break),
    700 exceeds the number of features."""
    ext = _ext()
    M, n, d = 2, 600, 12
    gen = torch.Generator().manual_seed(18)
    fired = torch.randint(1, 9, (M, n), generator=gen).float()
    if dead == "mixed":
        fired[torch.rand(M, n, generator=gen) < 0.3] = 0.0
        fired[:, [0, 63, 64, 255, 256, 599]] = 0.0
    elif dead == "all":
        fired.zero_()
    t = lambda *s: torch.randn(*s, generator=gen)
    pool = t(M, n_track, d)
    k = dict(fired=fired, new_rows=pool / pool.norm(dim=-1, keepdim=True),
             enc_scale=torch.tensor([0.2, 0.7]), W=t(M, n, d), mu_w=t(M, n, d), nu_w=t(M, n, d).abs())
    if extras:
        k.update(dec=t(M, n, d), mu_d=t(M, n, d), nu_d=t(M, n, d).abs(),
                 bias=t(M, n), mu_b=t(M, n), nu_b=t(M, n).abs())
    ref = R.resample_ref(**k)
    dev = {name: g(v) for name, v in k.items()}
    counts = torch.full((M,), -1, device=DEV, dtype=torch.int32)
    ext.resample(counts_out=counts, **dev)
    R.check_bits("counts", counts.cpu(), ref["counts"])
    for name in k:
        if name not in ("fired", "new_rows", "enc_scale"):
            R.check_bits(name, dev[name].cpu(), ref[name])
    for name in ("fired", "new_rows", "enc_scale"):
        R.check_bits(name, dev[name].cpu(), k[name])
    if dead == "mixed":
        assert 0 < int(ref["counts"][0]) == min(int((fired[0] == 0).sum()), n_track)


# ---------------------------------------------------------------------------
# lista_bwd_elem
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [False, True], ids=["nocarry", "carry"])
def test_lista_bwd_elem(carry):
    """Two row blocks and two column blocks.  r on a 1/4 grid with theta = 0.5
    makes |r| == theta and r == 0 occur exactly: the mask is strict and exact.
    g_theta and g_rho are added onto nonzero starts."""
    ext = _ext()
    M, B, n = 2, 300, 260
    gen = torch.Generator().manual_seed(19)
    r = torch.randint(-8, 9, (M, B, n), generator=gen).float() / 4
    assert (r.abs() == 0.5).any() and (r == 0).any()
    theta = torch.full((M, n), 0.5)
    x = torch.sign(r) * torch.clamp(r.abs() - 0.5, min=0.0)  # exact in fp32
    k = dict(g_y=R.scaled_randn(gen, M, B, n), carry_in=R.scaled_randn(gen, M, B, n) if carry else None,
             r=r, theta=theta, x=x, x_prev=torch.randn(M, B, n, generator=gen), mom=torch.tensor([0.1, 0.6]))
    ref = R.lista_bwd(**k)
    g_r_ref, carry_ref, g_theta_ref, g_rho_ref = R.lista_bwd_autograd(
        k["g_y"], k["carry_in"], r, theta, k["x_prev"], k["mom"])
    g_r = torch.full((M, B, n), float("nan"), device=DEV)
    carry_out = torch.full((M, B, n), float("nan"), device=DEV)
    gt0, gr0 = torch.randn(M, n, generator=gen), torch.tensor([3.0, -5.0])
    g_theta, g_rho = g(gt0), g(gr0)
    ext.lista_bwd_elem(g(k["g_y"]), g(k["carry_in"]) if carry else None, g(r), g(theta), g(x),
                       g(k["x_prev"]), g(k["mom"]), g_r, carry_out, g_theta, g_rho)
    st = [R.check("g_r", g_r, g_r_ref, ref["e_gr"]),
          R.check("carry_out", carry_out, carry_ref, ref["e_carry"]),
          R.sum_check("g_theta", g_theta, gt0, ref["t_theta"], ref["e_gr"], R.lista_theta_depth(B), 1,
                      total=g_theta_ref),
          R.sum_check("g_rho", g_rho, gr0, ref["t_rho"], ref["e_trho"], R.lista_rho_depth(B, n), (1, 2),
                      total=g_rho_ref)]
    assert (g_r.cpu()[r.abs() <= 0.5] == 0).all()
    _report("lista_bwd_elem", *st)


# ---------------------------------------------------------------------------
# Adam kernels
# ---------------------------------------------------------------------------

HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
STEPS = torch.tensor([1.0, 7.0, 1000.0])


@pytest.mark.parametrize("d", [68, 4])
@pytest.mark.parametrize("mode", ["project", "plain", "clamp"])
@pytest.mark.parametrize("use_lr_mult", [False, True], ids=["lr", "lrmult"])
def test_project_adam(d, mode, use_lr_mult):
    """W, mu, nu each against fp64 autograd through normalize_rows (the
    gradient) and functional.optim.adam (the update), at per-model steps
    1 / 7 / 1000 from nonzero moments; 33 rows (8 per block)."""
    ext = _ext()
    M, n = 3, 11
    gen = torch.Generator().manual_seed(20)
    t = lambda *s: torch.randn(*s, generator=gen)
    W = t(M, n, d)
    W[0, 0] = 1e-10 * t(d)  # norm <= eps_norm: no projection, g = gw / eps
    gw, mu0, nu0 = t(M, n, d), 0.1 * t(M, n, d), 0.01 * t(M, n, d).abs() + 1e-4
    project, clamp = mode != "plain", mode == "clamp"
    w_used = torch.clamp(W, min=0.0) if clamp else None
    if clamp:
        assert (W < 0).any()
    lr_mult = None
    if use_lr_mult:
        lr_mult = torch.rand(M, n, generator=gen)
        lr_mult[:, ::3] = 0.0  # frozen rows
    lrm3 = lr_mult[..., None] if use_lr_mult else None

    g_ref, e_g = R.project_grad(W, gw, project, w_used, clamp)
    g_auto = R.project_grad_autograd(W, gw, project, clamp)
    bnd = R.adam_chain(W, g_ref, e_g, mu0, nu0, STEPS, lr_mult=lrm3, **HYP)
    W_ref, mu_ref, nu_ref = R.adam_autograd(W, g_auto, mu0, nu0, STEPS, lr_mult=lrm3, **HYP)

    Wd, mu, nu = g(W), g(mu0), g(nu0)
    norms, _ = _inv_norms(ext, g(w_used) if clamp else Wd)
    ext.project_adam(Wd, g(gw), norms, mu, nu, g(STEPS), n, HYP["lr"], HYP["b1"], HYP["b2"],
                     HYP["eps"], R.EPS_NORM, project, w_used=g(w_used) if clamp else None,
                     clamp_mask=clamp, lr_mult=g(lr_mult) if use_lr_mult else None)
    st = [R.check("mu", mu, mu_ref, bnd["e_mu"]), R.check("nu", nu, nu_ref, bnd["e_nu"]),
          R.check("W", Wd, W_ref, bnd["e_p"])]
    if use_lr_mult:  # a frozen row keeps its weights bit for bit; its moments move
        R.check_bits("frozen rows", Wd.cpu()[:, ::3], W[:, ::3])
        assert (mu.cpu()[:, ::3] != mu0[:, ::3]).all()
    _report(f"project_adam {mode}", *st)


@pytest.mark.parametrize("decay", [False, True], ids=["nodecay", "decay"])
@pytest.mark.parametrize("use_lr_mult", [False, True], ids=["lr", "lrmult"])
def test_bias_adam(decay, use_lr_mult):
    """n = 1030: three strides of the 512-thread block, the last one partial.
    Model 2's bias is all zero: its decay gradient must be 0, not NaN."""
    ext = _ext()
    M, n = 3, 1030
    gen = torch.Generator().manual_seed(21)
    t = lambda *s: torch.randn(*s, generator=gen)
    bias = t(M, n)
    bias[2] = 0.0
    gb, mu0, nu0 = t(M, n), 0.1 * t(M, n), 0.01 * t(M, n).abs() + 1e-4
    bd = torch.tensor([0.01, 0.1, 0.05]) if decay else torch.zeros(M)
    lr_mult = None
    if use_lr_mult:
        lr_mult = torch.rand(M, n, generator=gen)
        lr_mult[:, ::3] = 0.0
    g_ref, e_g = R.bias_grad(bias, gb, bd)
    g_auto = R.bias_grad_autograd(bias, gb, bd)
    bnd = R.adam_chain(bias, g_ref, e_g, mu0, nu0, STEPS, lr_mult=lr_mult, **HYP)
    b_ref, mu_ref, nu_ref = R.adam_autograd(bias, g_auto, mu0, nu0, STEPS, lr_mult=lr_mult, **HYP)
    b, mu, nu = g(bias), g(mu0), g(nu0)
    ext.bias_adam(b, g(gb), g(bd), mu, nu, g(STEPS), HYP["lr"], HYP["b1"], HYP["b2"], HYP["eps"],
                  lr_mult=g(lr_mult) if use_lr_mult else None)
    st = [R.check("mu", mu, mu_ref, bnd["e_mu"]), R.check("nu", nu, nu_ref, bnd["e_nu"]),
          R.check("bias", b, b_ref, bnd["e_p"])]
    assert torch.isfinite(b).all()
    if use_lr_mult:
        R.check_bits("frozen entries", b.cpu()[:, ::3], bias[:, ::3])
        assert (mu.cpu()[:, ::3] != mu0[:, ::3]).all()
    _report("bias_adam", *st)


# ---------------------------------------------------------------------------
# ragged full steps
# ---------------------------------------------------------------------------

def _rel_err(a, b):
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


@pytest.fixture
def staging(request, monkeypatch):
    from sparse_coding_amd.ops.kconfig import kernel_config, set_kernel_config

    old = kernel_config()
    set_kernel_config(staging=request.param)
    # two eager steps, then the captured one: both paths see the ragged batch
    monkeypatch.delenv("SPARSE_CODING_AMD_NO_GRAPH", raising=False)
    yield request.param
    set_kernel_config(**old)


@pytest.mark.parametrize("staging", ["t", "pre"], indirect=True)
@pytest.mark.parametrize("B", [100, 90])
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
def test_ragged_full_step(staging, B, tied):
    """A batch that is no multiple of the 128-row tile (100) nor of 4 (90: the
    last batch of a chunk) trains under either staging and tracks the torch
    backend; with B % 4 != 0 the step resolves "pre" to "t" for the allocation."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalSAE, FunctionalTiedSAE

    sig = FunctionalTiedSAE if tied else FunctionalSAE
    torch.manual_seed(22)
    d, n = 64, 128
    models = [sig.init(d, n, l1, device=DEV) for l1 in (1e-3, 3e-3)]
    ens_hip = FunctionalEnsemble(models, sig, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    models2 = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
               for p, b in ens_hip.unstack()]
    ens_ref = FunctionalEnsemble(models2, sig, adam, {"lr": 1e-3}, device=DEV, backend="torch")
    assert ens_hip._hip_step is not None
    x = torch.randn(B, d, device=DEV)
    for i in range(3):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        assert _rel_err(aux_hip["c"], aux_ref["c"]) < 1e-3, i
    assert ens_hip._hip_step.kc["staging"] == (staging if B % 4 == 0 else "t")
    for k in ens_ref.params:
        assert _rel_err(ens_hip.params[k], ens_ref.params[k]) < 2e-3, k

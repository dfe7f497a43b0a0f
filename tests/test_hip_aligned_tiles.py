"""The guard-free (ALIGNED) GEMM kernels against the guarded ones.

On a tile-aligned launch (rows % 128 == 0, cols % TBN == 0, K % TBK == 0,
16-byte aligned operands) the launchers of ops/hip/sae_ops.hip take kernel
variants without row / column / K-tail guards; `set_aligned_tiles(False)` sends
the same launch to the guarded kernels.  K-loop, MFMA order and epilogue
arithmetic are shared, so every output that is not built from float atomics must
agree bit for bit between the two; the atomically summed ones (loss_parts,
g_gain, g_scale) are held to the fp64 reference's bound instead, and the
on-path outputs of the aligned run are checked against the fp64 reference once.

Shapes (M, B, d, n):
  (2, 128,  32, 128)  one tile; two K-steps at depth 16, one at depth 32
  (1, 128, 128, 128)
  (2, 256, 128, 256)  2x2 tiles (XCD swizzle), 8 K-steps; d = 128 aligns the
                      columns of grad_w and dec, n = 256 the 256-wide variant
  (2, 256, 128, 260)  not aligned: both settings run the guarded kernels
"""

import functools

import pytest
import torch

from tests import hip_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

VARIANTS = [(32, False, 128), (16, True, 128), (16, False, 256)]
VARIANTS_128 = VARIANTS[:2]
_vid = lambda v: f"bk{v[0]}-p{int(v[1])}-bn{v[2]}"
variants = pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
variants_128 = pytest.mark.parametrize("variant", VARIANTS_128, ids=_vid)

SHAPES = [(2, 128, 32, 128), (1, 128, 128, 128), (2, 256, 128, 256), (2, 256, 128, 260)]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))

L1 = [1e-3, 1e-2]


def _ext():
    from sparse_coding_amd import ops

    return ops.get_extension()


def g(t):
    return t.to(DEV).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _per_model(vals, M):
    return torch.tensor(vals[:M], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.gemm_inputs(*shape, seed=100 + sum(shape))


def _x(inp, per_model):
    return inp["xm"] if per_model else inp["x"]


def _inv_norms(ext, W_dev):
    norms = torch.empty(W_dev.shape[:-1], device=DEV)
    inv = torch.empty_like(norms)
    ext.row_norms(W_dev, norms, inv, R.EPS_NORM)
    return inv


@functools.lru_cache(maxsize=None)
def _codes(shape, signed=False):
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(9)
    c = R.scaled_randn(gen, M, B, n)
    c[torch.rand(M, B, n, generator=gen) < 0.3] = 0.0
    return c if signed else torch.clamp(c, min=0.0)


def _both(run):
    """run() -> {name: tensor} with the aligned kernels on, then off."""
    ext = _ext()
    assert ext.aligned_tiles(), "the switch must default to on"
    try:
        on = run()
        ext.set_aligned_tiles(False)
        assert not ext.aligned_tiles()
        off = run()
    finally:
        ext.set_aligned_tiles(True)
    torch.cuda.synchronize()
    return on, off


def _same(on, off, names):
    """torch.equal, and the same bit patterns (NaN fill of an output a mode
    leaves alone, signed zeros)."""
    for k in names:
        a, b = on[k], off[k]
        assert a.shape == b.shape
        ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        if not torch.equal(ai, bi):
            idx = tuple(int(i) for i in (ai != bi).nonzero()[0])
            raise AssertionError(f"{k}: {int((ai != bi).sum())} of {a.numel()} elements differ between the aligned "
                                 f"and the guarded kernel; first at {idx}: {a[idx].item()!r} vs {b[idx].item()!r}")
        if not torch.isnan(a).any():
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# enc_fwd, modes 0-5
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _enc_aux(shape):
    """Mode-specific operands, from fixed seeds."""
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(7)
    scale = 0.5 + torch.rand(M, n, generator=gen)
    scale[:, 1] = 5e-5
    gain = scale ** 2 * (0.95 + 0.1 * torch.randn(M, n, generator=gen))
    y = R.scaled_randn(gen, M, B, n)
    x_prev = R.scaled_randn(gen, M, B, n)
    theta = 0.05 * torch.rand(M, n, generator=gen)
    mom = _per_model([0.1, 0.6], M)
    ds = [n, max(n - 3, 1)][:M] if M > 1 else [max(n - 3, 1)]
    return dict(scale=scale, gain=gain, y=y, x_prev=x_prev, theta=theta, mom=mom, ds=ds)


LP0 = [3.0, 5.0]


def _run_enc(shape, variant, mode, per_model):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp, aux = _inputs(shape), _enc_aux(shape)
    W = g(inp["W"])
    inv = None if mode == 4 else _inv_norms(ext, W)
    out = dict(c=_nan(M, B, n), u_out=_nan(M, B, n), x_out=_nan(M, B, n),
               lp=g(torch.tensor([LP0]).repeat(M, 1)), fired=g(torch.full((M, n), 2.0)))
    kw = {}
    if mode == 0:
        kw = dict(dict_sizes=g(torch.tensor(aux["ds"], dtype=torch.int32)))
    elif mode == 2:
        kw = dict(act_scale=g(aux["scale"]), act_gain=g(aux["gain"]), u_out=out["u_out"])
    elif mode == 4:
        kw = dict(act_scale=g(aux["theta"]), u_out=out["u_out"], y_in=g(aux["y"]), x_prev=g(aux["x_prev"]),
                  x_out=out["x_out"], mom=g(aux["mom"]))
    elif mode == 5:
        kw = dict(y_in=g(aux["y"]))
    ext.enc_fwd(g(_x(inp, per_model)), W, g(inp["bias"]), inv, out["c"], out["lp"], out["fired"],
                mode, bk, prio, bn, **kw)
    return out


@functools.lru_cache(maxsize=None)
def _enc_ref(shape, mode, per_model):
    inp, aux = _inputs(shape), _enc_aux(shape)
    x = _x(inp, per_model)
    if mode == 0:
        return R.enc_relu(x, inp["W"], inp["bias"], True, aux["ds"])
    if mode == 2:
        return R.enc_gate(x, inp["W"], aux["scale"], aux["gain"])
    if mode == 3:
        return R.enc_reverse(x, inp["W"], inp["bias"])
    return None


@variants
@shapes
@pytest.mark.parametrize("per_model", [False, True], ids=["xshared", "xpermodel"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
def test_enc_fwd(variant, shape, mode, per_model):
    M, B, d, n = shape
    bn = variant[2]
    on, off = _both(lambda: _run_enc(shape, variant, mode, per_model))
    _same(on, off, ["c", "u_out", "x_out", "fired"])
    lp0 = torch.tensor([LP0]).repeat(M, 1)
    ref = _enc_ref(shape, mode, per_model)
    if ref is None:  # modes 1, 4, 5 leave loss_parts alone
        for o in (on, off):
            R.check_bits("loss_parts", o["lp"].cpu(), lp0)
        return
    und = ref["undecided"].double().mean().item()
    print(f"[aligned] enc mode {mode}: undecided share {und:.2e}")
    assert und <= R.MAX_UNDECIDED
    terms = ref["c"].abs() if mode == 3 else ref["c"]
    slack = ref["flip"].sum(dim=(1, 2)) if mode == 3 else None
    for o in (on, off):
        R.sum_check("l1", o["lp"][:, 1], lp0[:, 1], terms, ref["e"], R.epi_sum_depth(B, n, bn), (1, 2),
                    slack=slack)
        R.check_bits("loss_parts[:,0]", o["lp"][:, 0].cpu(), lp0[:, 0])
    if mode == 0:  # the flagship epilogue, against the fp64 reference
        st = R.check("c", on["c"], ref["c"], ref["e"])
        lo, hi = R.fired_range(ref["on"], ref["undecided"], torch.full((M, n), 2.0))
        R.check_counts("fired", on["fired"], lo, hi)
        print(f"[aligned] enc relu vs fp64: worst={st['worst']:.3f}")


# ---------------------------------------------------------------------------
# dec_fwd
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dec_ref(shape, per_model):
    inp = _inputs(shape)
    return R.dec(_codes(shape), inp["W"], _x(inp, per_model))


@variants
@shapes
@pytest.mark.parametrize("per_model", [False, True], ids=["xshared", "xpermodel"])
def test_dec_fwd(variant, shape, per_model):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    lp0 = torch.tensor([LP0]).repeat(M, 1)

    def run():
        W = g(inp["W"])
        out = dict(r=_nan(M, B, d), lp=g(lp0))
        ext.dec_fwd(g(_codes(shape)), W, _inv_norms(ext, W), g(_x(inp, per_model)), out["r"], out["lp"],
                    bk, prio, bn)
        return out

    on, off = _both(run)
    _same(on, off, ["r"])
    ref = _dec_ref(shape, per_model)
    st = R.check("r", on["r"], ref["r"], ref["e"])
    for o in (on, off):
        R.sum_check("mse", o["lp"][:, 0], lp0[:, 0], ref["sq"], ref["e_sq"], R.epi_sum_depth(B, d, bn), (1, 2))
        R.check_bits("loss_parts[:,1]", o["lp"][:, 1].cpu(), lp0[:, 1])
    print(f"[aligned] dec vs fp64: worst={st['worst']:.3f}")


# ---------------------------------------------------------------------------
# gc, gc_thresh
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gc_ref(shape, gc_mode):
    inp = _inputs(shape)
    return R.gc(inp["xm"], inp["W"], _codes(shape, signed=gc_mode == 1), _per_model(L1, shape[0]), gc_mode)


@variants
@shapes
@pytest.mark.parametrize("accumulate", [True, False], ids=["acc", "overwrite"])
@pytest.mark.parametrize("gc_mode", [0, 1])
def test_gc(variant, shape, gc_mode, accumulate):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    c = _codes(shape, signed=gc_mode == 1)
    gb0 = torch.randn(M, n, generator=torch.Generator().manual_seed(14))

    def run():
        W = g(inp["W"])
        out = dict(gpre=_nan(M, B, n), g_bias=g(gb0))
        ext.gc(g(inp["xm"]), W, _inv_norms(ext, W), g(c), g(_per_model(L1, M)), out["gpre"], out["g_bias"],
               bk, prio, gc_mode=gc_mode, bn=bn, accumulate=accumulate)
        return out

    on, off = _both(run)
    _same(on, off, ["gpre", "g_bias"])
    ref = _gc_ref(shape, gc_mode)
    st = R.check("gpre", on["gpre"], ref["gpre"], ref["e"])
    if gc_mode == 1:
        R.check_bits("g_bias", on["g_bias"].cpu(), gb0)
    else:
        start = gb0 if accumulate else torch.zeros(M, n)
        R.sum_check("g_bias", on["g_bias"], start, ref["gpre"], ref["e"], R.col_sum_depth(B), 1)
    print(f"[aligned] gc mode {gc_mode} vs fp64: worst={st['worst']:.3f}")


@functools.lru_cache(maxsize=None)
def _thresh_case(shape):
    inp = _inputs(shape)
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(10)
    scale = 0.5 + torch.rand(M, n, generator=gen)
    scale[:, 1] = 5e-5
    u = 0.95 + 0.12 * torch.randn(M, B, n, generator=gen)
    u[:, : B // 2] *= R.row_scales(B // 2, gen, 0)[:, None]
    c = (R.gate_g(u.double()) * scale[:, None, :].double() ** 2).float()
    l1 = _per_model(L1, M)
    ref = R.gc_thresh(inp["xm"], inp["W"], c, u, scale, l1)
    return scale, u, c, l1, ref, R.gc_thresh_autograd(ref["gv"], u, scale)


@variants_128
@shapes
def test_gc_thresh(variant, shape):
    ext = _ext()
    M, B, d, n = shape
    bk, prio, _ = variant
    inp = _inputs(shape)
    scale, u, c, l1, ref, (gpre_ref, g_gain_ref, g_scale_ref) = _thresh_case(shape)
    gen = torch.Generator().manual_seed(15)
    gg0, gs0 = torch.randn(M, n, generator=gen), torch.randn(M, n, generator=gen)

    def run():
        W = g(inp["W"])
        out = dict(gpre=_nan(M, B, n), g_gain=g(gg0), g_scale=g(gs0))
        ext.gc_thresh(g(inp["xm"]), W, _inv_norms(ext, W), g(c), g(u), g(scale), g(l1), out["gpre"],
                      out["g_gain"], out["g_scale"], bk, prio)
        return out

    on, off = _both(run)
    _same(on, off, ["gpre"])
    und = ref["undecided"].double().mean().item()
    print(f"[aligned] gc_thresh: undecided share {und:.2e}")
    R.check("gpre", on["gpre"], gpre_ref, ref["e_gpre"], ref["undecided"])
    depth = R.col_sum_depth(B)
    for o in (on, off):  # float atomics across the row tiles
        R.sum_check("g_gain", o["g_gain"], gg0, ref["gpre"], ref["e_gpre"], depth, 1,
                    slack=ref["flip_gain"].sum(dim=1), total=g_gain_ref)
        R.sum_check("g_scale", o["g_scale"], gs0, ref["t_scale"], ref["e_t"], depth, 1,
                    slack=ref["flip_scale"].sum(dim=1), total=g_scale_ref)


# ---------------------------------------------------------------------------
# grad_w
# ---------------------------------------------------------------------------

@variants
@shapes
@pytest.mark.parametrize("shared_q", [False, True], ids=["qpermodel", "qshared"])
def test_grad_w(variant, shape, shared_q):
    """beta != 0 on a started gw, and beta = 0 on a NaN-filled one."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    P = _codes(shape, signed=True)
    Q = inp["x"] if shared_q else inp["xm"]
    gw0 = torch.randn(M, n, d, generator=torch.Generator().manual_seed(11))

    def run():
        out = dict(gw=g(gw0), gw_b0=_nan(M, n, d))
        ext.grad_w(g(P), g(Q), out["gw"], 0.5, -2.0, bk, prio, bn)
        ext.grad_w(g(P), g(Q), out["gw_b0"], 1.0, 0.0, bk, prio, bn)
        return out

    on, off = _both(run)
    _same(on, off, ["gw", "gw_b0"])
    acc, absdot = R.dot("mbn,bd->mnd" if shared_q else "mbn,mbd->mnd", P, Q)
    st = R.check("gw", on["gw"], 0.5 * acc - 2.0 * gw0.double(),
                 (R.c_dot(B) + 3) * R.U * (0.5 * absdot + 2.0 * gw0.double().abs()))
    R.check("gw beta=0", on["gw_b0"], acc, (R.c_dot(B) + 1) * R.U * absdot)
    print(f"[aligned] grad_w vs fp64: worst={st['worst']:.3f}")


@variants
@pytest.mark.parametrize("shape", [(3, 128, 128, 128)], ids=["3x128x128x128"])
def test_grad_w_model_slices(variant, shape):
    """The data-parallel step hands grad_w dim-0 slices of P, Q and gw (model
    groups): contiguous views whose base pointer is offset into the storage.
    The slices' results must equal the whole-tensor launch, aligned or not."""
    ext = _ext()
    M, B, d, n = shape
    bk, prio, bn = variant
    inp = _inputs(shape)
    P, Q = g(_codes(shape, signed=True)), g(inp["xm"])
    gw0 = torch.randn(M, n, d, generator=torch.Generator().manual_seed(11))

    def run():
        out = dict(whole=g(gw0), sliced=g(gw0))
        ext.grad_w(P, Q, out["whole"], 0.5, -2.0, bk, prio, bn)
        for sl in (slice(0, 1), slice(1, 3)):
            assert P[sl].is_contiguous() and out["sliced"][sl].is_contiguous()
            ext.grad_w(P[sl], Q[sl], out["sliced"][sl], 0.5, -2.0, bk, prio, bn)
        return out

    on, off = _both(run)
    _same(on, off, ["whole", "sliced"])
    _same(on, {"whole": on["sliced"]}, ["whole"])


# ---------------------------------------------------------------------------
# full step
# ---------------------------------------------------------------------------

def test_full_tied_step_bitwise(monkeypatch):
    """A tied HipSAEStep at (2, 128, 128, 256): two eager steps, then the first
    graph replay, with the aligned kernels on and off.  The parameters (and the
    Adam moments) must come out bit for bit the same."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.sae_signatures import FunctionalTiedSAE

    monkeypatch.delenv("SPARSE_CODING_AMD_NO_GRAPH", raising=False)
    M, B, d, n = 2, 128, 128, 256
    torch.manual_seed(23)
    init = [FunctionalTiedSAE.init(d, n, l1, device=DEV) for l1 in (1e-3, 3e-3)]
    x = torch.randn(B, d, device=DEV)

    def run():
        models = [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
                  for p, b in init]
        ens = FunctionalEnsemble(models, FunctionalTiedSAE, adam, {"lr": 1e-3}, device=DEV, backend="hip")
        assert ens._hip_step is not None
        for _ in range(3):
            losses, _ = ens.step_batch(x)
        torch.cuda.synchronize()
        out = {f"params.{k}": v.detach().clone() for k, v in ens.params.items()}
        flat = []

        def walk(label, obj):
            if torch.is_tensor(obj):
                flat.append((label, obj))
            elif isinstance(obj, dict):
                for k, v in obj.items():
                    walk(f"{label}.{k}", v)
            elif isinstance(obj, (list, tuple)):
                for i, v in enumerate(obj):
                    walk(f"{label}.{i}", v)

        walk("optim", ens.optim_states)
        out.update({k: v.detach().clone().float() for k, v in flat})
        out["loss"] = losses["loss"].detach().clone()
        return out

    on, off = _both(run)
    names = [k for k in on if k != "loss"]
    assert any(k.startswith("params.") for k in names)
    _same(on, off, names)
    assert torch.isfinite(on["loss"]).all()
    # the loss is summed with float atomics: equal to rounding, not to the bit
    assert torch.allclose(on["loss"], off["loss"], rtol=1e-5, atol=0.0)

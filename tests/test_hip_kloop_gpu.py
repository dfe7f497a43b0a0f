"""The GEMM K-loop at its first three trip counts, aligned against guarded.

The main loop of the GEMM kernels is a prologue (tile 0 staged into LDS buffer
0), one loop trip per further K-tile (prefetch tile t+1, MFMA on tile t, write
tile t+1 into the other buffer, barrier, flip) and a last MFMA phase.  A
contraction of exactly one K-tile runs the prologue alone, two K-tiles take one
trip, three make the buffer index flip back to 0.  These tests run exactly 1,
2 and 3 K-tiles through the guard-free (ALIGNED) kernels, whose K-loop schedule
is pinned by hand (sae_kernels.hip, gemm_mainloop), and compare them bit for
bit with the guarded kernels, and each with the fp64 reference.

    grad_w   K = B: 16, 32, 48 at depth 16; 32, 64, 96 at depth 32; n = d = 128
    enc_fwd  (mode 0), gc   K = d: 16, 32, 48 at depth 16; B = n = 128
    dec_fwd  K = n: 32, 64, 96 at depth 32; B = d = 128
"""

import functools

import pytest
import torch

from tests import hip_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M = 2
L1 = torch.tensor([1e-3, 1e-2])
LP0 = [3.0, 5.0]


def _ext():
    from sparse_coding_amd import ops

    return ops.get_extension()


def g(t):
    return t.to(DEV).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@functools.lru_cache(maxsize=None)
def _inputs(B, d, n):
    return R.gemm_inputs(M, B, d, n, seed=300 + B + 2 * d + 3 * n)


@functools.lru_cache(maxsize=None)
def _codes(B, n, signed=False):
    gen = torch.Generator().manual_seed(19)
    c = R.scaled_randn(gen, M, B, n)
    c[torch.rand(M, B, n, generator=gen) < 0.3] = 0.0
    return c if signed else torch.clamp(c, min=0.0)


def _inv_norms(ext, W_dev):
    norms = torch.empty(W_dev.shape[:-1], device=DEV)
    inv = torch.empty_like(norms)
    ext.row_norms(W_dev, norms, inv, R.EPS_NORM)
    return inv


def _both(run):
    """run() -> {name: tensor} with the aligned kernels on, then off."""
    ext = _ext()
    assert ext.aligned_tiles(), "the switch must default to on"
    try:
        on = run()
        ext.set_aligned_tiles(False)
        off = run()
    finally:
        ext.set_aligned_tiles(True)
    torch.cuda.synchronize()
    return on, off


def _same(on, off, names):
    for k in names:
        a, b = on[k].contiguous().view(torch.int32), off[k].contiguous().view(torch.int32)
        if not torch.equal(a, b):
            idx = tuple(int(i) for i in (a != b).nonzero()[0])
            raise AssertionError(f"{k}: {int((a != b).sum())} of {a.numel()} elements differ between the aligned and "
                                 f"the guarded kernel; first at {idx}: {on[k][idx].item()!r} vs {off[k][idx].item()!r}")


def _tiles_aligned(rows, cols, K, bk):
    """What the launcher asks of a shape before it takes the ALIGNED kernel."""
    return rows % 128 == 0 and cols % 128 == 0 and K % bk == 0


GRAD_W_CASES = [(16, B) for B in (16, 32, 48)] + [(32, B) for B in (32, 64, 96)]


@pytest.mark.parametrize("bk,B", GRAD_W_CASES, ids=[f"bk{bk}-B{B}" for bk, B in GRAD_W_CASES])
@pytest.mark.parametrize("shared_q", [False, True], ids=["qpermodel", "qshared"])
@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
def test_grad_w_k_tiles(bk, B, shared_q, beta):
    ext = _ext()
    n = d = 128
    assert _tiles_aligned(n, d, B, bk) and B // bk in (1, 2, 3)
    inp = _inputs(B, d, n)
    P = _codes(B, n, signed=True)
    Q = inp["x"] if shared_q else inp["xm"]
    gw0 = torch.randn(M, n, d, generator=torch.Generator().manual_seed(11))

    def run():
        # beta = 0 must not read gw: NaN-filled
        out = dict(gw=g(gw0) if beta else _nan(M, n, d))
        ext.grad_w(g(P), g(Q), out["gw"], 0.5, beta, bk, bk == 16, 128)
        return out

    on, off = _both(run)
    _same(on, off, ["gw"])
    acc, absdot = R.dot("mbn,bd->mnd" if shared_q else "mbn,mbd->mnd", P, Q)
    st = R.check("gw", on["gw"], 0.5 * acc + beta * gw0.double(),
                 (R.c_dot(B) + 3) * R.U * (0.5 * absdot + beta * gw0.double().abs()))
    print(f"[kloop] grad_w bk{bk} B{B} vs fp64: worst={st['worst']:.3f}")


@pytest.mark.parametrize("d", [16, 32, 48])
def test_enc_fwd_k_tiles(d):
    ext = _ext()
    B = n = 128
    bk = 16
    assert _tiles_aligned(B, n, d, bk) and d // bk in (1, 2, 3)
    inp = _inputs(B, d, n)
    ds = [n, n - 3]
    lp0 = torch.tensor([LP0]).repeat(M, 1)

    def run():
        W = g(inp["W"])
        out = dict(c=_nan(M, B, n), lp=g(lp0), fired=g(torch.full((M, n), 2.0)))
        ext.enc_fwd(g(inp["x"]), W, g(inp["bias"]), _inv_norms(ext, W), out["c"], out["lp"], out["fired"],
                    0, bk, True, 128, dict_sizes=g(torch.tensor(ds, dtype=torch.int32)))
        return out

    on, off = _both(run)
    _same(on, off, ["c", "fired"])
    ref = R.enc_relu(inp["x"], inp["W"], inp["bias"], True, ds)
    assert ref["undecided"].double().mean().item() <= R.MAX_UNDECIDED
    st = R.check("c", on["c"], ref["c"], ref["e"])
    lo, hi = R.fired_range(ref["on"], ref["undecided"], torch.full((M, n), 2.0))
    R.check_counts("fired", on["fired"], lo, hi)
    for o in (on, off):
        R.sum_check("l1", o["lp"][:, 1], lp0[:, 1], ref["c"], ref["e"], R.epi_sum_depth(B, n, 128), (1, 2))
    print(f"[kloop] enc d{d} vs fp64: worst={st['worst']:.3f}")


@pytest.mark.parametrize("d", [16, 32, 48])
def test_gc_k_tiles(d):
    ext = _ext()
    B = n = 128
    bk = 16
    assert _tiles_aligned(B, n, d, bk) and d // bk in (1, 2, 3)
    inp = _inputs(B, d, n)
    c = _codes(B, n)
    gb0 = torch.randn(M, n, generator=torch.Generator().manual_seed(14))

    def run():
        W = g(inp["W"])
        out = dict(gpre=_nan(M, B, n), g_bias=g(gb0))
        ext.gc(g(inp["xm"]), W, _inv_norms(ext, W), g(c), g(L1), out["gpre"], out["g_bias"],
               bk, True, gc_mode=0, bn=128, accumulate=True)
        return out

    on, off = _both(run)
    _same(on, off, ["gpre", "g_bias"])
    ref = R.gc(inp["xm"], inp["W"], c, L1, 0)
    st = R.check("gpre", on["gpre"], ref["gpre"], ref["e"])
    R.sum_check("g_bias", on["g_bias"], gb0, ref["gpre"], ref["e"], R.col_sum_depth(B), 1)
    print(f"[kloop] gc d{d} vs fp64: worst={st['worst']:.3f}")


@pytest.mark.parametrize("n", [32, 64, 96])
def test_dec_fwd_k_tiles(n):
    ext = _ext()
    B = d = 128
    bk = 32
    assert _tiles_aligned(B, d, n, bk) and n // bk in (1, 2, 3)
    inp = _inputs(B, d, n)
    c = _codes(B, n)
    lp0 = torch.tensor([LP0]).repeat(M, 1)

    def run():
        W = g(inp["W"])
        out = dict(r=_nan(M, B, d), lp=g(lp0))
        ext.dec_fwd(g(c), W, _inv_norms(ext, W), g(inp["x"]), out["r"], out["lp"], bk, False, 128)
        return out

    on, off = _both(run)
    _same(on, off, ["r"])
    ref = R.dec(c, inp["W"], inp["x"])
    st = R.check("r", on["r"], ref["r"], ref["e"])
    for o in (on, off):
        R.sum_check("mse", o["lp"][:, 0], lp0[:, 0], ref["sq"], ref["e_sq"], R.epi_sum_depth(B, d, 128), (1, 2))
    print(f"[kloop] dec n{n} vs fp64: worst={st['worst']:.3f}")

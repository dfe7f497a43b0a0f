"""The sparse TopK chain (topk_chain="sparse"): k_sparse_dec_gc + k_sparse_grad_w.

1. The TopK and BatchTopK steps under the sparse chain against fp64 autograd:
   the body and the bounds of test_hip_step_grads_gpu (8 e32 + 16 U scale).
2. The two launchers on constructed codes against dense fp64 formulas, under
   componentwise bounds c U sum|terms| with c counted from the kernel code: at
   every compiled register depth, full and entered from below; at exact hit
   counts on both sides of the light/heavy switch; with a per-model x.
3. r's first 64 columns are the same bits at every depth.
4. Two runs into fresh outputs are equal bit for bit.

Worst err / bound of 1 per case over its shapes (MI355X, ``[step64]`` lines):

    case            worst err/bound     at 36x772x132 alone
    topk            0.156               0.233
    batch_topk      0.099               0.233

and per output of the launchers (``[sparse64]`` lines):

    cases                                   r       gw      gpre    loss
    d = 64, 68, 2044, 2048                  0.415   0.020   0.064   0.021
    the depth grid (d = 3 .. 1028)          0.467   0.021   0.069   0.028
    constructed hit counts                  0.222   0.054   0.040   0.017
    per-model x                             0.399   0.015   0.027   0.013
"""

import pytest
import torch

from tests import hip_reference as H
from tests import step_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = R.U


@pytest.fixture
def sparse_chain():
    from sparse_coding_amd.ops.kconfig import kernel_config, set_kernel_config

    old = kernel_config()
    set_kernel_config(topk_chain="sparse")
    yield
    set_kernel_config(**old)


@pytest.mark.parametrize("shape", [R.ALIGNED, R.RAGGED, R.DEEP_D], ids=lambda s: "x".join(map(str, s[1:])))
@pytest.mark.parametrize("name", ["topk", "batch_topk"])
def test_sparse_step_gradients_match_fp64_autograd(name, shape, sparse_chain):
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam

    M, B, d, n = shape
    c = R.case(name)
    entry = (name, shape, None)
    assert R.decisions(name, shape)["near"] == 0  # before touching the GPU
    ref = R.reference(name, shape)
    models, x = R.build(name, shape)
    to_dev = lambda tree: R.tree_apply(lambda t: t.to(DEV), tree)  # noqa: E731
    ens = FunctionalEnsemble([(to_dev(p), to_dev(b)) for p, b in models], c.sig, adam, {"lr": 0.0},
                             device=DEV, backend="hip")
    hs = ens._hip_step
    assert type(hs).__name__ == c.step_class
    params0 = R.tree_apply(lambda t: t.detach().cpu().clone(), ens.params)
    xg = x.to(DEV)

    losses, aux = ens.step_batch(xg)
    torch.cuda.synchronize()
    assert hs.kc["topk_chain"] == "sparse" and not hasattr(hs, "g_bias_scratch")
    worst = {}
    worst["loss"] = R.compare_losses(losses, ref, R.loss_depths(c, B, d, n))
    assert set(worst["loss"]) >= set(ref["loss64"]) - {"threshold"}
    worst["c"] = R.compare_codes(aux["c"], ref, None)
    st = ens.optim_states
    assert (st["step"] == 1).all()
    worst["mu1"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 1, None)
    worst["nu1"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 1, None)

    ens.step_batch(xg)
    assert hs._graph is None
    ens.step_batch(xg)  # the first replay of the captured graph
    torch.cuda.synchronize()
    assert hs._graph is not None and (st["step"] == 3).all()
    worst["mu3"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 3, None)
    worst["nu3"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 3, None)
    for (path, p0), (_, p) in zip(R.tree_items(params0), R.tree_items(ens.params)):
        p = p.detach().cpu()
        assert p.dtype == p0.dtype and torch.equal(p0.view(torch.int32), p.view(torch.int32)), \
            f"{path} moved at lr = 0"

    for what, ratios in worst.items():
        for leaf, ratio in ratios.items():
            print(f"[step64] sparse {R.grid_id(entry)} {what} {leaf} {ratio:.3f}")
    print(f"[step64] sparse {R.grid_id(entry)} worst {max(max(r.values()) for r in worst.values()):.3f}")


def _inputs(M, B, d, n):
    """c: about 6% positives; column 1 positive on every row and row 0 in every
    column, except that row B-1 and column n-1 are all zero."""
    gen = torch.Generator().manual_seed(B * n + d)
    c = torch.where(torch.rand(M, B, n, generator=gen) < 0.06,
                    torch.randn(M, B, n, generator=gen).abs() + 0.1, torch.zeros(()))
    full = torch.rand(M, B, n, generator=gen) + 0.1
    c[:, :, 1], c[:, 0, :] = full[:, :, 1], full[:, 0, :]
    c[:, B - 1, :] = 0.0
    c[:, :, n - 1] = 0.0
    W = torch.randn(M, n, d, generator=gen)
    return c, W, 1.0 / W.norm(dim=-1), torch.randn(B, d, generator=gen)


def _per_model_x(M, B, d):
    """x as [M, B, d], different data per model."""
    return torch.randn(M, B, d, generator=torch.Generator().manual_seed(M * B + d))


# k_sparse_grad_w sums a feature's hits in one wave up to SGW_LIGHT = 32 of them
# and in 8 slices of ceil(K / 8) above: 33 hits leave the last slice empty
# (slices of 5), 40 fill all 8, B - 1 is every row but the all-zero one.  0 to 3
# hits: sgw_accum's pair loop not at all, its odd tail alone, one pair, both.
HIT_COUNTS = (0, 1, 2, 3, 32, 33, 40, -1)  # -1: B - 1


def _counted_inputs(M, B, d, n):
    """_inputs with columns rewritten to hold an exact number of hits: model 0
    has HIT_COUNTS in columns 2.., model 1 the same counts reversed, and both
    3, 33 and 32 hits in the last (partial) strip of 64 features.  The k hit
    rows are spread evenly over rows 0 .. B-2, so the lists of the larger counts
    are put together from all eight row slices of phase 1.  Returns the inputs
    and want [M, n]: the constructed count, -1 where the column is _inputs'."""
    c, W, inv, x = _inputs(M, B, d, n)
    gen = torch.Generator().manual_seed(7 * B + d)
    last = 64 * ((n - 1) // 64)
    assert B - 1 > 40 and 2 + len(HIT_COUNTS) <= last and last + 4 < n - 1
    want = torch.full((M, n), -1)
    for m in range(M):
        counts = HIT_COUNTS if m % 2 == 0 else HIT_COUNTS[::-1]
        cols = list(zip(range(2, 2 + len(counts)), counts)) + [(last + 1, 3), (last + 2, 33), (last + 3, 32)]
        for col, k in cols:
            k = B - 1 if k < 0 else k
            rows = (torch.arange(k) * (B - 1) + (B - 1) // 2) // max(k, 1)
            c[m, :, col] = 0.0
            c[m, rows, col] = torch.rand(k, generator=gen) + 0.1
            want[m, col] = k
    assert ((c > 0).sum(1)[want >= 0] == want[want >= 0]).all()  # the rows are distinct
    return c, W, inv, x, want


def _launch(ext, c, W, inv, x):
    M, B, n = c.shape
    d = W.shape[-1]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    r, gpre, gw, lp = nan(M, B, d), nan(M, B, n), nan(M, n, d), torch.zeros(M, 2, device=DEV)
    hits = torch.empty(ext.sparse_hits_size(M, B, n), device=DEV, dtype=torch.int32)
    counts = torch.empty(M, n, device=DEV, dtype=torch.int32)
    ext.sparse_dec_gc(c, W, inv, x, r, gpre, lp)
    ext.sparse_grad_w(c, gpre, r, x, gw, hits, counts)
    torch.cuda.synchronize()
    return r.cpu(), gpre.cpu(), gw.cpu(), lp.cpu(), counts.cpu()


# The depths SPARSE_DISPATCH_DL compiles (test_sparse_depth_grid_cpu holds this
# tuple against the macro); a launcher takes the smallest one >= ceil(d / 64).
DEPTHS = (1, 2, 4, 8, 12, 16, 32)

# the last: a feature above 32 hits at the deepest instantiation, whose slice
# partials go through LDS in two rounds
SHAPES = [(2, 128, 64, 128), (2, 70, 68, 132), (1, 6, 2048, 70), (1, 5, 2044, 66), (1, 40, 2044, 66)]
# Every compiled depth once full (d = 64 DL) and once entered from below, where
# whole registers lie past d: they must stay exact zeros from the first pass to
# the stores.  B >= 34 gives column 1 more than 32 hits, so k_sparse_grad_w's
# LDS combine runs at its width of 768 (DL = 12, the one that is no power of
# two), at 1024 in one round (DL = 16) and in a second round of 4 columns
# (d = 1028).  n = 520: three float4 steps of 256 columns; n = 522 adds the
# 2-column tail behind them and puts every other row off 16 bytes.
SHAPES += [(2, 5, 3, 66),
           (2, 48, 256, 132), (1, 44, 130, 70), (1, 6, 130, 522),
           (2, 40, 512, 140), (2, 34, 260, 520),
           (2, 37, 768, 66), (1, 48, 516, 134),
           (2, 36, 1024, 70), (1, 45, 772, 98),
           (1, 44, 1028, 66)]


def _check_against_fp64(tag, c, W, inv, x):
    """Launch both kernels on CPU fp32 inputs (x [B, d] or [M, B, d]) and hold
    r, gpre, gw, the loss and the hit counts against dense fp64 formulas."""
    from sparse_coding_amd import ops

    (M, B, n), d = c.shape, W.shape[-1]
    r, gpre, gw, lp, counts = _launch(ops.get_extension(), *(t.to(DEV) for t in (c, W, inv, x)))

    c64, W64, inv64, x64 = (t.double() for t in (c, W, inv, x))
    hit = c64 > 0
    # DL is ceil(d / 64) also where the compiled depth is larger: the registers
    # past d hold exact zeros, so their fmas and tree terms add 0 and round nothing
    What, gs, DL = W64 * inv64[..., None], 2.0 / (B * d), H.cdiv(d, 64)
    # r: per hit of the row one product c*inv and one fma, then the subtraction
    r64 = c64 @ What - x64
    e_r = (hit.sum(-1, keepdim=True) + 2) * U * (c64 @ What.abs() + x64.abs())
    # gpre: r's error through the dot, then DL fmas in the lane, 6 tree levels,
    # gscale (one division), gscale*inv and the product with the dot
    g64 = gs * (r64 @ What.mT)
    e_g = gs * (e_r @ What.abs().mT) + (DL + 9) * U * gs * (r64.abs() @ What.abs().mT)
    # gw: per hit gscale*c (after gscale's division) and two fmas; a feature's
    # list of K hits is summed serially up to 32, else in 8 slices of
    # ceil(K / 8) plus 7 combine adds
    K = hit.sum(1)[..., None]  # [M, n, 1]
    c_w = torch.where(K <= 32, 2 * K, 2 * ((K + 7) // 8) + 7) + 2
    gm, cm = g64 * hit, gs * c64
    gw64 = cm.mT @ r64 + gm.mT @ x64
    terms = cm.mT @ r64.abs() + gm.abs().mT @ x64.abs()
    e_w = cm.mT @ e_r + (e_g * hit).mT @ x64.abs() + c_w * U * terms
    # loss: r's error, then DL fmas, 6 tree levels, 2 adds over the block's
    # waves and one atomic add per block of 4 rows
    l64 = (r64 ** 2).sum((1, 2))
    e_l = ((2 * r64.abs() + e_r) * e_r).sum((1, 2)) + (DL + 8 + H.cdiv(B, 4)) * U * l64

    out = {"r": H.check("r", r, r64, e_r), "gw": H.check("gw", gw, gw64, e_w),
           "gpre": H.check("gpre", torch.where(hit, gpre.double(), 0.0), gm, e_g),
           "loss": H.check("loss", lp[:, 0], l64, e_l)}
    for k, v in out.items():
        print(f"[sparse64] {tag} {k} {v['worst']:.3f}")
    assert torch.equal(r[:, B - 1], -x.expand(M, B, d)[:, B - 1])  # the all-zero row
    zero_row = gw[:, n - 1]
    assert (zero_row == 0).all() and not torch.signbit(zero_row).any()  # exact +0 over the NaN fill
    assert gpre[~hit].isnan().all()  # written at the hits only
    assert torch.equal(counts.long(), hit.sum(1))
    return r, counts


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sparse_kernels_match_fp64(shape):
    _check_against_fp64("x".join(map(str, shape)), *_inputs(*shape))


@pytest.mark.parametrize("d", [68, 768, 1028])
def test_sparse_kernels_at_constructed_hit_counts(d):
    """Exactly 0, 1, 2, 3, 32, 33, 40 and B - 1 hits in chosen columns: both
    sides of the light/heavy switch and every way through sgw_accum's loop.
    d = 768 combines the heavy ones 768 columns wide, d = 1028 in a second
    round that stores 4 columns."""
    M, B, n = 2, 44, 70
    c, W, inv, x, want = _counted_inputs(M, B, d, n)
    assert {int(k) for k in want[want >= 0]} == {0, 1, 2, 3, 32, 33, 40, B - 1}
    _, counts = _check_against_fp64(f"counted-{M}x{B}x{d}x{n}", c, W, inv, x)
    assert torch.equal(counts.long()[want >= 0], want[want >= 0])


def test_sparse_kernels_take_per_model_x():
    M, B, d, n = 2, 44, 516, 70
    c, W, inv, _ = _inputs(M, B, d, n)
    _check_against_fp64(f"xm-{M}x{B}x{d}x{n}", c, W, inv, _per_model_x(M, B, d))


@pytest.mark.parametrize("d", [130, 512, 768, 772, 1028])
def test_r_is_bit_identical_across_depths(d):
    """r[b, col] is the same fmaf(c inv, W[j, col], acc) over the row's hits in
    ascending j, then the same subtraction, whatever DL the row is held at (and
    gscale, which d enters, is no part of it): the first 64 columns out of
    depth 4, 8, 12, 16 or 32 equal, bit for bit, those of the same problem cut
    to d = 64, which runs depth 1."""
    from sparse_coding_amd import ops

    assert DEPTHS[[H.cdiv(d, 64) <= D for D in DEPTHS].index(True)] in (4, 8, 12, 16, 32)
    c, W, inv, x = _inputs(2, 9, d, 70)
    ext = ops.get_extension()
    deep = _launch(ext, *(t.to(DEV) for t in (c, W, inv, x)))[0]
    shallow = _launch(ext, *(t.to(DEV) for t in (c, W[..., :64].contiguous(), inv, x[..., :64].contiguous())))[0]
    assert shallow.shape[-1] == 64 and not shallow.isnan().any()
    assert torch.equal(deep[..., :64], shallow)


def test_sparse_kernels_are_reproducible():
    from sparse_coding_amd import ops

    c, W, inv, x = (t.to(DEV) for t in _inputs(2, 70, 68, 132))
    a, b = (_launch(ops.get_extension(), c, W, inv, x) for _ in range(2))
    hit = c.cpu() > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[1][hit], b[1][hit])

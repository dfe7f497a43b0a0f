"""The wide sparse chain, 2048 < d <= 8192: k_wsparse_dec_gc, k_sparse_hit_lists
and k_wsparse_grad_w behind the four sparse launchers and the three step classes.

1. The plain and the Matryoshka launchers on constructed codes against dense
   fp64 formulas under componentwise bounds c U sum|terms|: r / S and gw under
   the narrow kernels' bounds (the same chains), gpre and the loss with c counted
   from the eight-wave reductions.  With them the exact outputs, the identities
   between the two launcher pairs and two runs bit for bit.
2. Columns against the narrow kernels, bit for bit.
3. The TopK, BatchTopK and Matryoshka steps against fp64 autograd: the bodies
   and bounds of test_topk_sparse_chain_gpu and test_matryoshka_gpu.
4. d = 8193 is refused.

Worst err / bound of 1 per output (MI355X, ``[wsparse64]`` lines):

    cases                                   S       gw      gpre    loss
    plain launchers, the six shapes         0.465   0.046   0.006   0.019
    Matryoshka launchers, G = 3, 8, 1       0.477   0.015   0.011   0.056
    constructed hit counts                  0.252   0.052   0.009   0.015
    per-model x                             0.415   0.013   0.011   0.010

and of the steps (``[step64]`` lines), at 36x2052x132 and 12x4100x68: topk 0.488
and 0.637, batch_topk 0.488 and 0.516, matryoshka 0.488 and 0.516.
"""

import pytest
import torch

from tests import hip_reference as H
from tests import step_reference as R
from tests import test_matryoshka_gpu as mat
from tests import test_topk_sparse_chain_gpu as plain
from tests.test_topk_sparse_chain_gpu import _counted_inputs, _inputs, _launch, _per_model_x, sparse_chain  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
CAP = 2048  # WSP_CAP (sae_wsparse.hip): the entries of a row's hit list in LDS


def _check(tag, inputs, ends=None):
    """Both kernels through the plain launchers (ends None: one level, S = r) or
    the Matryoshka ones, twice, against dense fp64 formulas."""
    from sparse_coding_amd import ops
    ext, (c, W, inv, x) = ops.get_extension(), inputs
    (M, B, n), d = c.shape, W.shape[-1]
    dev = [t.to(DEV) for t in inputs]
    first = _launch(ext, *dev)
    r, gpre0, gw0 = first[:3]
    if ends is None:
        ends = ((n,),) * M
        lift = lambda o: (o[0][:, None], o[1], o[2], o[3][:, :1], o[4])  # noqa: E731  r as S [M, 1, B, d]
        runs = [lift(first), lift(_launch(ext, *dev))]
    else:
        dev.append(torch.tensor(ends, dtype=torch.int32, device=DEV))
        runs = [mat._launch(ext, *dev) for _ in range(2)]
    (S, gpre, gw, parts, counts), again, G = runs[0], runs[1], len(ends[0])

    c64, W64, inv64, x64 = (t.double() for t in inputs)
    hit = c64 > 0
    # DLW = ceil(d / 512) also under the deeper instantiation: registers past d hold exact zeros
    What, gs, DLW = W64 * inv64[..., None], 2.0 / (B * d), H.cdiv(d, 512)
    e = torch.tensor(ends)                                                        # [M, G]
    prefix = (torch.arange(n) < e[..., None])[:, :, None, :]                      # [M, G, 1, n]
    level = (torch.arange(n) >= e[:, :-1, None]).sum(1)                           # [M, n]
    own = (level[:, None, :] == torch.arange(G)[None, :, None])[:, :, None, :]    # [M, G, 1, n]
    # r_g: per hit of the prefix one product c*inv and one fma, then the subtraction (the narrow chain)
    cp = c64[:, None] * prefix
    xl = x64 if x64.dim() == 2 else x64[:, None]
    r64 = cp @ What[:, None] - xl
    e_r = ((hit[:, None] & prefix).sum(-1, keepdim=True) + 2) * U * (cp @ What.abs()[:, None] + xl.abs())
    # S_g = r_g + S_{g+1}: r's errors, and one rounding per level above g
    tail = lambda t: t.flip(1).cumsum(1).flip(1)  # noqa: E731
    S64, adds = tail(r64), torch.arange(G - 1, -1, -1).view(1, G, 1, 1)
    e_S = tail(e_r) + adds * U * (tail(r64.abs()) + tail(e_r))
    # gpre: S's error through the dot; then DLW fmas in the thread, 7 adds over the waves' partials,
    # 6 tree levels, gscale's division, gscale*inv and the product with the dot: DLW + 16
    pick = lambda t: (t * own).sum(1)  # noqa: E731
    g64 = gs * pick(S64 @ What.mT[:, None])
    e_g = gs * pick(e_S @ What.abs().mT[:, None]) + (DLW + 16) * U * gs * pick(S64.abs() @ What.abs().mT[:, None])
    # gw: k_sparse_grad_w's bound (serial up to 32 hits, else 8 slices + 7 adds), on the feature's level of S
    K = hit.sum(1)[..., None]
    c_w = torch.where(K <= 32, 2 * K, 2 * ((K + 7) // 8) + 7) + 2
    gm, cm = g64 * hit, (gs * c64)[:, None] * own
    gw64 = (cm.mT @ S64).sum(1) + gm.mT @ x64
    terms = (cm.mT @ S64.abs()).sum(1) + gm.abs().mT @ x64.abs()
    e_w = (cm.mT @ e_S).sum(1) + (e_g * hit).mT @ x64.abs() + c_w * U * terms
    # loss: r_g's error; then DLW fmas, 6 tree levels, 7 adds over the waves and one atomic add per
    # workgroup, which is one per row: DLW + 13 + B
    l64 = (r64 ** 2).sum((2, 3))
    e_l = ((2 * r64.abs() + e_r) * e_r).sum((2, 3)) + (DLW + 13 + B) * U * l64
    out = {"S": H.check("S", S, S64, e_S), "gw": H.check("gw", gw, gw64, e_w),
           "gpre": H.check("gpre", torch.where(hit, gpre.double(), 0.0), gm, e_g),
           "loss": H.check("loss", parts, l64, e_l)}
    print(f"[wsparse64] {tag} G={G}", {k: round(v["worst"], 3) for k, v in out.items()})
    assert torch.equal(S[:, G - 1, B - 1], -x.expand(M, B, d)[:, B - 1])  # the all-zero row
    assert (gw[:, n - 1] == 0).all() and not torch.signbit(gw[:, n - 1]).any()  # exact +0 over the NaN fill
    assert gpre[~hit].isnan().all() and torch.equal(counts.long(), hit.sum(1))
    assert torch.equal(S[:, G - 1], r)  # the plain launcher's r, at every G
    if G == 1:
        assert torch.equal(gpre[hit], gpre0[hit]) and torch.equal(gw, gw0)
    assert torch.equal(S, again[0]) and torch.equal(gw, again[2]) and torch.equal(gpre[hit], again[1][hit])
    return counts


# first wide d, most registers past d; DLW = 8 full; DLW = 16 entered from below with a heavy feature and
# a fifth window of 4 columns; full and nearly full; a row of CAP + 69 hits (row 0 hits every column but
# the last), which refills the list and sends pass 1 through the rescan, on rows off 16 bytes (n % 4 = 2)
SHAPES = [(1, 5, 2052, 66), (2, 6, 4096, 70), (1, 40, 4100, 66), (1, 5, 8192, 66), (1, 6, 8188, 70),
          (1, 5, 2052, CAP + 70)]
MAT_CASES = [((2, 36, 2052, 132), ((64, 128, 132), (37, 101, 132))),
             ((1, 40, 4100, 66), ((3, 8, 13, 21, 30, 41, 64, 66),)), ((2, 36, 2052, 70), ((70,), (70,)))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_kernels_match_fp64(shape):
    _check("x".join(map(str, shape)), _inputs(*shape))


@pytest.mark.parametrize("case", MAT_CASES, ids=mat.case_id)
def test_wide_matryoshka_kernels_match_fp64_and_the_plain_launchers(case):
    _check(mat.case_id(case), _inputs(*case[0]), case[1])


def test_wide_kernels_at_constructed_hit_counts():
    """Both sides of the light/heavy switch in each of the three windows of d = 2116."""
    c, W, inv, x, want = _counted_inputs(2, 44, 2116, 70)
    counts = _check("counted-2x44x2116x70", (c, W, inv, x))
    assert torch.equal(counts.long()[want >= 0], want[want >= 0])


def test_wide_kernels_take_per_model_x():
    c, W, inv, _ = _inputs(2, 36, 2052, 70)
    _check("xm-2x36x2052x70", (c, W, inv, _per_model_x(2, 36, 2052)))


def test_columns_equal_the_narrow_kernels_bit_for_bit():
    """A column of r or gw is the narrow kernels' chain on that column.  r: the
    narrow decode on the first 2048 columns.  gw: gscale = 2 / (B d) enters its
    terms, so the narrow launch has to see the same B d: the two halves of 1026
    columns (they cut the windows at 1024 and 2048 off their edges) at twice the
    batch, the added rows without a hit, fed the wide run's gpre."""
    from sparse_coding_amd import ops
    ext, (M, B, d, n) = ops.get_extension(), (2, 36, 2052, 70)
    c, W, inv, x = (t.to(DEV) for t in _inputs(M, B, d, n))
    r, gpre, gw, _, _ = _launch(ext, c, W, inv, x)
    assert torch.equal(r[..., :2048], _launch(ext, c, W[..., :2048].contiguous(), inv, x[..., :2048].contiguous())[0])
    pad = lambda t: torch.cat([t, torch.zeros_like(t)], -2).contiguous()  # noqa: E731
    for lo in (0, 1026):
        gw_n = torch.full((M, n, 1026), float("nan"), device=DEV)
        hits = torch.empty(ext.sparse_hits_size(M, 2 * B, n), device=DEV, dtype=torch.int32)
        ext.sparse_grad_w(pad(c), pad(gpre.to(DEV)), pad(r.to(DEV)[..., lo:lo + 1026]), pad(x[..., lo:lo + 1026]),
                          gw_n, hits, torch.empty(M, n, device=DEV, dtype=torch.int32))
        assert torch.equal(gw[..., lo:lo + 1026], gw_n.cpu())


# n = 68, not the kernel tests' 70: the encoder GEMM ahead of every chain takes d and n in multiples of 4 only
STEP_ENDS = {(2, 36, 2052, 132): ((64, 96, 132), (37, 101, 132)), (2, 12, 4100, 68): ((16, 40, 68), (37, 53, 68))}


@pytest.mark.parametrize("shape", list(STEP_ENDS), ids=lambda s: "x".join(map(str, s[1:])))
@pytest.mark.parametrize("name", ["topk", "batch_topk", "matryoshka"])
def test_wide_steps_match_fp64_autograd(name, shape, sparse_chain, monkeypatch):  # noqa: F811
    """The eager step and the first graph replay, lr = 0; both bodies assert
    decisions(...)["near"] == 0 before they touch the GPU."""
    if name == "matryoshka":
        monkeypatch.setitem(mat.STEP_ENDS, shape, STEP_ENDS[shape])
        mat.test_step_gradients_match_fp64_autograd(shape)
    else:
        plain.test_sparse_step_gradients_match_fp64_autograd(name, shape, None)


def test_d_above_8192_is_refused():
    from sparse_coding_amd import ops
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.matryoshka import MatryoshkaBatchTopKEncoder as Mat
    with pytest.raises(RuntimeError, match="8192"):
        _launch(ops.get_extension(), *(t.to(DEV) for t in _inputs(1, 2, 8193, 4)))
    models, x = R.build("batch_topk", (2, 4, 8193, 66))
    models = [tuple(R.tree_apply(lambda t: t.to(DEV), tree) for tree in (p, dict(b, group_ends=torch.tensor((33, 66)))))
              for p, b in models]
    ens = FunctionalEnsemble(models, Mat, adam, {"lr": 0.0}, device=DEV, backend="hip")
    with pytest.raises(RuntimeError, match="8192"):
        ens.step_batch(x.to(DEV))

"""The Matryoshka BatchTopK step: k_sparse_dec_gc + k_sparse_grad_w with LEVELS.

1. HipMatryoshkaStep against fp64 autograd of the signature's own loss, under
   8 e32 + 16 U scale.  Its only nonsmooth decision is BatchTopK's selection
   on the same scores, so batch_topk's clean seeds are the guard.
   Worst err / bound of 1 on an MI355X: 0.128 over 128x64x128 and 130x68x260,
   0.233 at 36x772x132 (the codes; 0.092 for the moments).
2. The launchers on constructed codes against fp64 formulas under bounds
   c U sum|terms|, c counted from the kernel code, at every compiled register
   depth; bit identities with the plain sparse kernels; reproducibility.  The
   last level's squared-error sum meets the plain kernel's in float atomicAdds
   of hardware-picked order: bit for bit up to two blocks, one rounding per
   block beyond (seen both ways).
   Worst err / bound of 1 per output (MI355X, ``[msparse64]`` lines):

    cases                                   S       gw      gpre    mse
    d = 68, 2044, 2048                      0.427   0.021   0.055   0.041
    d = 3 .. 1028 (depths 1, 4 .. 32)       0.524   0.026   0.089   0.046
    per-model x                             0.365   0.019   0.027   0.014
"""

import pytest
import torch

from tests import hip_reference as H
from tests import step_reference as R
from tests.test_topk_sparse_chain_gpu import _inputs, _per_model_x
from tests.test_topk_sparse_chain_gpu import _launch as _launch_plain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
# per model: a boundary on a multiple of 64; ends off 4 and 64 (unaligned segment base, straddled strip)
STEP_ENDS = {R.ALIGNED: ((64, 96, 128), (37, 101, 128)), R.RAGGED: ((64, 128, 260), (37, 101, 260)),
             R.DEEP_D: ((64, 96, 132), (37, 101, 132))}


@pytest.mark.parametrize("shape", [R.ALIGNED, R.RAGGED, R.DEEP_D], ids=lambda s: "x".join(map(str, s[1:])))
def test_step_gradients_match_fp64_autograd(shape):
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.matryoshka import MatryoshkaBatchTopKEncoder as Mat

    M, B, d, n = shape
    assert R.decisions("batch_topk", shape)["near"] == 0  # before touching the GPU
    models, x = R.build("batch_topk", shape)
    models = [(p, dict(b, group_ends=torch.tensor(e))) for (p, b), e in zip(models, STEP_ENDS[shape])]
    ref = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        ref["g" + tag], ref["loss" + tag], ref["c" + tag] = R._grads(Mat.loss, models, x, dtype)
    depths = R.loss_depths(R.case("batch_topk"), B, d, n)
    depths["mse_levels"] = depths["loss"]
    on_dev = [tuple(R.tree_apply(lambda t: t.to(DEV), tree) for tree in m) for m in models]
    ens = FunctionalEnsemble(on_dev, Mat, adam, {"lr": 0.0}, device=DEV, backend="hip")
    hs, st, xg = ens._hip_step, ens.optim_states, x.to(DEV)
    assert type(hs).__name__ == "HipMatryoshkaStep"
    params0 = R.tree_apply(lambda t: t.detach().cpu().clone(), ens.params)
    losses, aux = ens.step_batch(xg)
    torch.cuda.synchronize()
    worst = {"loss": R.compare_losses(losses, ref, depths), "c": R.compare_codes(aux["c"], ref, None)}
    assert set(worst["loss"]) == {"loss", "mse_levels"} and "threshold" in losses and (st["step"] == 1).all()
    worst["mu1"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 1, None)
    worst["nu1"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 1, None)
    ens.step_batch(xg)
    assert hs._graph is None
    losses, _ = ens.step_batch(xg)  # the first replay of the captured graph
    torch.cuda.synchronize()
    assert hs._graph is not None and (st["step"] == 3).all()
    worst["loss3"] = R.compare_losses(losses, ref, depths)
    worst["mu3"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 3, None)
    worst["nu3"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 3, None)
    for (path, p0), (_, p) in zip(R.tree_items(params0), R.tree_items(ens.params)):
        assert torch.equal(p0.view(torch.int32), p.detach().cpu().view(torch.int32)), f"{path} moved at lr = 0"
    print(f"[step64] matryoshka {shape} {worst} worst {max(max(r.values()) for r in worst.values()):.3f}")


def _launch(ext, c, W, inv, x, ends):
    M, B, n = c.shape
    d, G = W.shape[-1], ends.shape[1]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    Rw, gpre, gw, parts = nan(M, G, B, d), nan(M, B, n), nan(M, n, d), torch.zeros(M, G, device=DEV)
    hits = torch.empty(ext.sparse_hits_size(M, B, n), device=DEV, dtype=torch.int32)
    counts = torch.empty(M, n, device=DEV, dtype=torch.int32)
    ext.msparse_dec_gc(c, W, inv, x, ends, Rw, gpre, parts)
    ext.msparse_grad_w(c, gpre, Rw, x, ends, gw, hits, counts)
    torch.cuda.synchronize()
    return Rw.cpu(), gpre.cpu(), gw.cpu(), parts.cpu(), counts.cpu()


# (M, B, d, n), per-model ends.  Third: heavy feature, deepest DL, two-round LDS combine, largest G
CASES = [((2, 70, 68, 132), ((64, 128, 132), (37, 101, 132))), ((1, 6, 2048, 70), ((33, 70),)),
         ((1, 40, 2044, 66), ((3, 8, 13, 21, 30, 41, 64, 66),)), ((2, 70, 68, 132), ((132,), (132,)))]
# The depths between (DL = 4, 8, 12, 16) and DL = 32 entered from below, ends off
# multiples of 4 and 64; B >= 34 makes column 1 a heavy feature.  d = 1024 is
# k_sparse_dec_gc<16, 4, LEVELS>, the 4-waves-per-SIMD instantiation, at G = 8 with the most
# levels live around its 16 registers; G = 1 at d = 768 meets the plain kernels
# bit for bit where the LDS combine is 768 wide.
CASES += [((2, 38, 256, 132), ((64, 128, 132), (37, 101, 132))), ((1, 40, 260, 70), ((33, 70),)),
          ((2, 36, 516, 98), ((37, 66, 98), (5, 41, 98))), ((1, 44, 768, 70), ((21, 50, 70),)),
          ((2, 37, 768, 66), ((66,), (66,))), ((1, 35, 772, 66), ((13, 66),)),
          ((2, 34, 1024, 70), ((37, 70), (10, 70))), ((1, 40, 1024, 66), ((3, 8, 13, 21, 30, 41, 64, 66),)),
          ((1, 44, 1028, 66), ((33, 53, 66),))]
# depth 1, full and with lanes past d in its only register, and depth 4 from below
CASES += [((2, 9, 64, 70), ((33, 70), (64, 70))), ((1, 5, 3, 66), ((13, 66),)), ((1, 36, 130, 66), ((37, 66),))]


def case_id(case):
    (M, B, d, n), ends = case
    return f"{B}x{d}x{n}-G{len(ends[0])}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernels_match_fp64_and_the_plain_kernels(case):
    _check(*case, _inputs(*case[0]))


def test_kernels_take_per_model_x():
    shape, ends = (2, 36, 516, 98), ((37, 66, 98), (5, 41, 98))
    c, W, inv, _ = _inputs(*shape)
    _check(shape, ends, (c, W, inv, _per_model_x(2, 36, 516)))


def _check(shape, ends, inputs):
    from sparse_coding_amd import ops
    (M, B, d, n), G, ext = shape, len(ends[0]), ops.get_extension()
    c, W, inv, x = inputs
    dev = [t.to(DEV) for t in (c, W, inv, x)] + [torch.tensor(ends, dtype=torch.int32, device=DEV)]
    (S, gpre, gw, parts, counts), again = (_launch(ext, *dev) for _ in range(2))
    c64, W64, inv64, x64 = (t.double() for t in (c, W, inv, x))
    hit = c64 > 0
    # DL = ceil(d / 64) also under a larger compiled depth: registers past d hold exact zeros
    What, gs, DL = W64 * inv64[..., None], 2.0 / (B * d), H.cdiv(d, 64)
    e = torch.tensor(ends)                                                        # [M, G]
    prefix = (torch.arange(n) < e[..., None])[:, :, None, :]                      # [M, G, 1, n]
    level = (torch.arange(n) >= e[:, :-1, None]).sum(1)                           # [M, n]
    own = (level[:, None, :] == torch.arange(G)[None, :, None])[:, :, None, :]    # [M, G, 1, n]
    # r_g: per hit of the prefix one product c*inv and one fma, then the subtraction
    cp = c64[:, None] * prefix
    xl = x64 if x64.dim() == 2 else x64[:, None]  # against [M, G, B, d]: a per-model x gets the level axis
    r64 = cp @ What[:, None] - xl
    e_r = ((hit[:, None] & prefix).sum(-1, keepdim=True) + 2) * U * (cp @ What.abs()[:, None] + xl.abs())
    # S_g = r_g + S_{g+1}: r's errors, and one rounding per level above g
    tail = lambda t: t.flip(1).cumsum(1).flip(1)  # noqa: E731
    S64, adds = tail(r64), torch.arange(G - 1, -1, -1).view(1, G, 1, 1)
    e_S = tail(e_r) + adds * U * (tail(r64.abs()) + tail(e_r))
    # gpre: S's error through the dot, DL fmas, 6 tree levels, gscale's division, gscale*inv, the product
    pick = lambda t: (t * own).sum(1)  # noqa: E731  [M, G, B, n] -> a feature's own level
    g64 = gs * pick(S64 @ What.mT[:, None])
    e_g = gs * pick(e_S @ What.abs().mT[:, None]) + (DL + 9) * U * gs * pick(S64.abs() @ What.abs().mT[:, None])
    # gw: as k_sparse_grad_w (serial up to 32 hits, else 8 slices + 7 adds), on the feature's level of S
    K = hit.sum(1)[..., None]  # [M, n, 1]
    c_w = torch.where(K <= 32, 2 * K, 2 * ((K + 7) // 8) + 7) + 2
    gm, cm = g64 * hit, (gs * c64)[:, None] * own                                 # cm: [M, G, B, n]
    gw64 = (cm.mT @ S64).sum(1) + gm.mT @ x64
    terms = (cm.mT @ S64.abs()).sum(1) + gm.abs().mT @ x64.abs()
    e_w = (cm.mT @ e_S).sum(1) + (e_g * hit).mT @ x64.abs() + c_w * U * terms
    # mse_parts: r_g's error, DL fmas, 6 tree levels, 2 adds over the waves, one atomic add per block
    l64, nblocks = (r64 ** 2).sum((2, 3)), H.cdiv(B, 4)
    e_l = ((2 * r64.abs() + e_r) * e_r).sum((2, 3)) + (DL + 8 + nblocks) * U * l64
    out = {"S": H.check("S", S, S64, e_S), "gw": H.check("gw", gw, gw64, e_w),
           "gpre": H.check("gpre", torch.where(hit, gpre.double(), 0.0), gm, e_g),
           "mse": H.check("mse_parts", parts, l64, e_l)}
    assert torch.equal(S[:, G - 1, B - 1], -x.expand(M, B, d)[:, B - 1])  # the all-zero row
    assert (gw[:, n - 1] == 0).all() and not torch.signbit(gw[:, n - 1]).any()  # exact +0 over the NaN fill
    # against the plain kernels: a hit missed or counted twice at a boundary breaks the first
    assert gpre[~hit].isnan().all() and torch.equal(counts.long(), hit.sum(1))
    r, gpre0, gw0, lp, _ = _launch_plain(ext, *dev[:4])
    assert torch.equal(S[:, G - 1], r)
    same = torch.equal(parts[:, G - 1], lp[:, 0])
    assert same if nblocks <= 2 else ((parts[:, G - 1] - lp[:, 0]).abs() <= nblocks * U * lp[:, 0]).all()
    if G == 1:
        assert torch.equal(gpre[hit], gpre0[hit]) and torch.equal(gw, gw0)
    assert torch.equal(S, again[0]) and torch.equal(gw, again[2]) and torch.equal(gpre[hit], again[1][hit])
    print(f"[msparse64] {shape} G={G}", {k: round(v["worst"], 3) for k, v in out.items()}, "mse bits equal:", same)

"""The AuxK chain (ops/hip/sae_auxk.hip) and HipTopKAuxStep on the GPU: the
selection bit for bit, the kernels and the step against fp64, graph replay."""

import pytest
import torch

from sparse_coding_amd import ops
from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models.topk import TopKEncoder
from sparse_coding_amd.models.topk_auxk import TopKAuxEncoder
from sparse_coding_amd.ops.kconfig import kernel_config, set_kernel_config
from tests import hip_reference as H
from tests import step_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = H.U
DEAD_AFTER = 3


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _select(scores, ages, k_aux, KA):
    ext, (M, B, n) = ops.get_extension(), scores.shape
    da, ka, nd = _i32([DEAD_AFTER] * M), _i32(k_aux), _i32([-1] * M)
    idx = torch.full((M, B, KA), -1, dtype=torch.int32, device=DEV)
    val, cnt = torch.full((M, B, KA), float("nan"), device=DEV), _i32([[-1] * B] * M)
    ext.auxk_age(_i32(ages), None, da, nd)
    ext.auxk_select(scores.to(DEV), _i32(ages), da, ka, nd, idx, val, cnt)
    torch.cuda.synchronize()
    return idx.cpu().long(), val.cpu(), cnt.cpu().long(), nd.cpu()


@pytest.mark.parametrize("k_aux", [1, 7, "n"])
@pytest.mark.parametrize("n", [520, 522])
def test_select_matches_topk_over_the_dead_columns(n, k_aux):
    M, B = 3, 5  # model 0 all dead, model 1 none, model 2 mixed
    k_aux = n if k_aux == "n" else k_aux
    gen = torch.Generator().manual_seed(n + k_aux)
    scores = torch.randn(M, B, n, generator=gen)
    ages = torch.zeros(M, n, dtype=torch.int32)
    ages[0] = DEAD_AFTER
    ages[2] = torch.where(torch.rand(n, generator=gen) < 0.5, DEAD_AFTER + 1, DEAD_AFTER - 1)
    idx, val, cnt, nd = _select(scores, ages, [k_aux] * M, k_aux)
    dead = ages >= DEAD_AFTER
    assert torch.equal(nd.long(), dead.sum(1)) and (cnt[1] == 0).all()
    for m in (0, 2):
        top = torch.where(dead[m], scores[m], -torch.inf).topk(min(k_aux, int(dead[m].sum())))
        for b in range(B):
            want = top.indices[b][top.values[b] > 0].sort().values
            got = idx[m, b, :cnt[m, b]]
            assert torch.equal(got, want)  # the set, ascending
            H.check_bits("aux_val", val[m, b, :cnt[m, b]], scores[m, b, want])


def test_select_takes_the_lowest_columns_of_a_tie():
    n = 520
    scores = torch.rand(1, 2, n) - 2.0
    scores[0, :, [10, 70, 300, 500]] = 2.0  # four equal scores over two rounds, room for three
    scores[0, :, 5] = 3.0
    scores[0, 1, 10] = -1.0
    idx, val, cnt, _ = _select(scores, torch.full((1, n), DEAD_AFTER), [4], 4)
    assert cnt.tolist() == [[4, 4]]
    assert idx[0].tolist() == [[5, 10, 70, 300], [5, 70, 300, 500]]
    assert val[0].tolist() == [[3.0, 2.0, 2.0, 2.0]] * 2


@pytest.mark.parametrize("d,B", [(3, 37), (130, 37), (772, 37), (2048, 37), (130, 300)])
def test_aux_kernels_match_fp64(d, B):
    """Dead columns: 1 is hit on every row, 7 once, 9 never, 100 is also a main
    hit on the rows it is an aux hit, and the last strip's 515.. are random.
    B = 300 takes k_auxk_grad_w through a second window of rows."""
    ext, M, n, KA, alpha = ops.get_extension(), 2, 522, 16, 0.25
    gen = torch.Generator().manual_seed(d + B)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    W, x = rnd(M, n, d), rnd(B, d)
    inv = 1.0 / W.norm(dim=-1)
    c = torch.where(torch.rand(M, B, n, generator=gen) < 0.04, rnd(M, B, n).abs() + 0.1, torch.zeros(()))
    ages = torch.zeros(M, n, dtype=torch.int32)
    ages[:, [1, 7, 9, 100] + list(range(515, n))] = DEAD_AFTER
    z = torch.where((torch.rand(M, B, n, generator=gen) < 0.5) & (ages >= DEAD_AFTER)[:, None],
                    rnd(M, B, n).abs() + 0.1, torch.zeros(()))
    z[:, :, 1], z[:, :, 7], z[:, :, 9] = torch.rand(M, B, generator=gen) + 0.1, 0.0, 0.0
    z[:, B // 2, 7] = 0.7
    c[:, :, 100] = z[:, :, 100]
    hit = z > 0
    cnt = hit.sum(-1)
    assert cnt.max() <= KA and (hit[:, :, 1].all() and B > 32) and (c[hit] > 0).any()
    # the compact lists: a stable sort brings a row's hit columns forward, ascending
    order = (~hit).int().sort(dim=-1, stable=True).indices[..., :KA]
    idx, val = order.int(), z.gather(-1, order)

    to = lambda *ts: [t.to(DEV) for t in ts]  # noqa: E731
    cg, Wg, ig, xg, idx_g, val_g, cnt_g = to(c, W, inv, x, idx, val, cnt.int())
    da, ka, nd, al = _i32([DEAD_AFTER] * M), _i32([KA] * M), _i32([-1] * M), torch.full((M,), alpha, device=DEV)
    r, gpre, gw0 = (torch.empty(s, device=DEV) for s in ((M, B, d), (M, B, n), (M, n, d)))
    hits = torch.empty(ext.sparse_hits_size(M, B, n), device=DEV, dtype=torch.int32)
    lp = torch.zeros(M, 2, device=DEV)
    ext.auxk_age(_i32(ages), None, da, nd)
    ext.sparse_dec_gc(cg, Wg, ig, xg, r, gpre, lp)
    ext.sparse_grad_w(cg, gpre, r, xg, gw0, hits, torch.empty(M, n, device=DEV, dtype=torch.int32))
    runs = []
    for _ in range(2):
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        ra, ga, gw, lp1 = nan(M, B, d), nan(M, B, KA), gw0.clone(), lp.clone()
        ext.auxk_dec_gc(idx_g, val_g, cnt_g, Wg, ig, r, al, ka, nd, ra, ga, lp1)
        ext.auxk_grad_w(idx_g, val_g, cnt_g, ga, ra, xg, _i32(ages), da, ka, nd, al, gw)
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in (ra, ga, gw, lp1)])
    (ra, ga, gw, lp1), entry = runs[0], torch.arange(KA) < cnt[..., None]
    assert all(torch.equal(p[0], p[1]) for p in zip(runs[0][::2], runs[1][::2]))  # r_aux and gw, bit for bit
    assert torch.equal(ga[entry], runs[1][1][entry]) and ga[~entry].isnan().all()

    z64, W64, x64, r64 = z.double(), W.double() * inv.double()[..., None], x.double(), r.cpu().double()
    gs, DL, K = alpha * 2.0 / (B * d), H.cdiv(d, 64), hit.sum(1)[..., None]
    # r_aux: per entry one product val*inv and one fma, then the addition of r
    ra64 = z64 @ W64 + r64
    e_r = (cnt[..., None] + 2) * U * (z64 @ W64.abs() + r64.abs())
    # gpre_aux: k_sparse_dec_gc's count, and alpha's product in gs
    g64 = gs * (ra64 @ W64.mT) * hit
    e_g = gs * (e_r @ W64.abs().mT) + (DL + 10) * U * gs * (ra64.abs() @ W64.abs().mT)
    # gw: per hit gs*val (gs: a division and a product) and two fmas, serially;
    # then one load-add-store per window of 256 rows
    terms = (gs * z64).mT @ ra64.abs() + g64.abs().mT @ x64.abs()
    e_w = (gs * z64).mT @ e_r + (e_g * hit).mT @ x64.abs() + (2 * K + 3) * U * terms \
        + H.cdiv(B, 256) * U * (gw0.cpu().double().abs() + terms)
    # loss: as k_sparse_dec_gc's
    l64 = (ra64 ** 2).sum((1, 2))
    e_l = ((2 * ra64.abs() + e_r) * e_r).sum((1, 2)) + (DL + 8 + H.cdiv(B, 4)) * U * l64
    got_g = torch.zeros(M, B, n, dtype=torch.float64).scatter(-1, order, torch.where(entry, ga.double(), 0.0))
    out = {"r_aux": H.check("r_aux", ra, ra64, e_r), "gpre_aux": H.check("gpre_aux", got_g, g64, e_g),
           "gw": H.check("gw", gw.double() - gw0.cpu().double(), (gs * z64).mT @ ra64 + g64.mT @ x64, e_w),
           "l_aux": H.check("l_aux", lp1[:, 1], l64, e_l)}
    print(f"[auxk64] {d}x{B} " + " ".join(f"{k} {v['worst']:.3f}" for k, v in out.items()))
    assert torch.equal(lp1[:, 0], lp.cpu()[:, 0])
    assert torch.equal(gw[:, 9], gw0.cpu()[:, 9]) and torch.equal(gw[:, :1], gw0.cpu()[:, :1])  # no aux hit


def _ensemble(shape, sig_kw, lr, seed=0):
    M, B, d, n = shape
    torch.manual_seed(seed)
    models = [TopKAuxEncoder.init(d, n, 4, auxk=8, auxk_alpha=0.25, dead_after=DEAD_AFTER) for _ in range(M)]
    for (p, b), kw in zip(models, sig_kw):
        b.update(kw)
    to_dev = lambda tree: R.tree_apply(lambda t: t.to(DEV), tree)  # noqa: E731
    ens = FunctionalEnsemble([(to_dev(p), to_dev(b)) for p, b in models], TopKAuxEncoder, adam, {"lr": lr},
                             device=DEV, backend="hip")
    assert type(ens._hip_step).__name__ == "HipTopKAuxStep"
    return ens, torch.randn(B, d).to(DEV)


def _reference(W, x, c, z, alpha, dtype):
    """Per model: loss parts and the gradients with respect to What (the step's
    gw) and to W, on the given selections c > 0 and z (masks, [M, B, n])."""
    out = []
    for m in range(W.shape[0]):
        Wm = W[m].to(dtype).requires_grad_()
        What = (Wm / Wm.norm(dim=-1, keepdim=True)).detach().requires_grad_()
        xd = x.to(dtype)
        for Wh in (What, Wm / Wm.norm(dim=-1, keepdim=True)):
            S = xd @ Wh.T
            x_hat = (S * c[m]) @ Wh
            l_rec = ((x_hat - xd) ** 2).mean()
            l_aux = (((S * z[m]) @ Wh - (xd - x_hat).detach()) ** 2).mean() * bool(z[m].any())
            loss = l_rec + alpha * l_aux
            loss.backward()
        out.append({"loss": loss.detach(), "l_reconstruction": l_rec.detach(), "l_aux": l_aux.detach(),
                    "gw": What.grad, "dict": Wm.grad})
    return R.tree_stack(out)


@pytest.mark.parametrize("shape", [(2, 36, 132, 68), (2, 37, 772, 132)], ids=lambda s: "x".join(map(str, s)))
def test_step_matches_fp64_autograd(shape):
    M, B, d, n = shape
    half = torch.zeros(n, dtype=torch.int32)
    half[::2] = DEAD_AFTER  # model 0 has no dead feature, model 1 about half
    ens, xg = _ensemble(shape, [{}, {"steps_since_fired": half}], lr=0.0)
    hs, W, x = ens._hip_step, ens.params["dict"].detach().cpu().clone(), xg.cpu()
    depths = R.loss_depths(R.case("topk"), B, d, n)
    depths["l_aux"] = depths["l_reconstruction"]  # the same sum, by the same kernel structure
    ages = ens.buffers["steps_since_fired"].cpu().clone()
    for call in (1, 2):
        losses, aux = ens.step_batch(xg)
        torch.cuda.synchronize()
        c = aux["c"].cpu() > 0
        entry = torch.arange(hs.KA) < hs.aux_cnt.cpu()[..., None]
        z = torch.zeros(M, B, n).scatter_add(-1, hs.aux_idx.cpu().long() * entry, entry.float()) > 0
        n_dead = (ages >= DEAD_AFTER).sum(1)
        assert losses["n_dead"].tolist() == n_dead.tolist() and n_dead[0] == 0 and n_dead[1] > 0
        assert z[1].any() and not z[0].any() and losses["l_aux"][0] == 0 and not (z & ~(ages >= DEAD_AFTER)[:, None]).any()
        r64, r32 = (_reference(W, x, c, z, 0.25, t) for t in (torch.float64, torch.float32))
        ref = {"loss64": r64, "loss32": r32}
        worst = R.compare_losses({k: v for k, v in losses.items() if k != "n_dead"}, ref, depths)
        worst.update(R.compare({"gw": hs.gw}, {"gw": r64["gw"]}, {"gw": r32["gw"]}))
        if call == 1:
            for what in ("mu", "nu"):
                worst[what] = R.compare(ens.optim_states[what], {"dict": r64["dict"]}, {"dict": r32["dict"]},
                                        what, 1)["dict"]
            gw_aux = hs.gw.cpu().clone()
        H.check_bits("dict at lr = 0", ens.params["dict"].cpu(), W)
        ages = torch.where(c.any(1), 0, ages + 1).int()
        assert torch.equal(ens.buffers["steps_since_fired"].cpu(), ages)
        print(f"[auxk-step] {'x'.join(map(str, shape))} call {call} " +
              " ".join(f"{k} {v:.3f}" for k, v in worst.items()))

    old = kernel_config()
    set_kernel_config(topk_chain="sparse")
    try:
        plain = FunctionalEnsemble([({"dict": W[m].to(DEV)}, {"sparsity": torch.tensor(4)}) for m in range(M)],
                                   TopKEncoder, adam, {"lr": 0.0}, device=DEV, backend="hip")
        plain.step_batch(xg)
        torch.cuda.synchronize()
    finally:
        set_kernel_config(**old)
    H.check_bits("gw of the model with no dead feature", gw_aux[0], plain._hip_step.gw.cpu()[0])


def test_replayed_graph_follows_a_dying_feature():
    shape = (2, 37, 132, 132)
    (ens, x), (twin, _) = (_ensemble(shape, [{}, {}], lr=1e-3) for _ in range(2))
    twin._hip_step.use_graph = False
    for call in range(4):  # ages start at 0: what never fires is dead at the fourth call
        got, want = ens.step_batch(x), twin.step_batch(x)
        torch.cuda.synchronize()
        assert (ens._hip_step._graph is not None) == (call >= 2) and twin._hip_step._graph is None
        assert got[0]["n_dead"].tolist() == want[0]["n_dead"].tolist()
        assert (got[0]["n_dead"] > 0).all() == (call == 3)
        for a, b in ((ens.params["dict"], twin.params["dict"]),
                     (ens.buffers["steps_since_fired"], twin.buffers["steps_since_fired"])):
            H.check_bits(f"call {call}", a, b)
    assert (got[0]["l_aux"] > 0).all()


def test_d_above_the_limit_is_refused():
    ens, x = _ensemble((1, 4, 2049, 8), [{}], lr=0.0)
    with pytest.raises(RuntimeError, match="d <= 2048"):
        ens.step_batch(x)

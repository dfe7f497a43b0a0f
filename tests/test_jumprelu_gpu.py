"""ops/hip/sae_jumprelu.hip and HipJumpReLUStep on the GPU.  Two models with their
own theta, eps and lambda; eps is wide: the band has entries on both sides of theta."""

import pytest
import torch

from sparse_coding_amd import ops
from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models.jumprelu import JumpReLUEncoder
from tests import hip_reference as H
from tests import step_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = H.U
EPS, LAM = (0.5, 0.4), (0.3, 0.1)


@pytest.mark.parametrize("d,B,n", [(3, 37, 70), (130, 37, 132), (772, 37, 522), (2048, 300, 132), (2052, 37, 132)])
def test_kernels_match_the_fp32_rule_and_fp64(d, B, n):
    """Row 4 has no hit, feature 1 is in the band on every row (below theta on row
    4), model 1 has theta < 0 at column 3 and model 0 theta = 0 at column 5."""
    ext, M, NW = ops.get_extension(), 2, H.cdiv(n, 64)
    gen = torch.Generator().manual_seed(d + B + n)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    S, W, r, theta = rnd(M, B, n), rnd(M, n, d), rnd(M, B, d), 0.6 * torch.rand(M, n, generator=gen)
    theta[1, 3], theta[0, 5] = -0.2, 0.0
    eps, lam, inv = torch.tensor(EPS), torch.tensor(LAM), 1.0 / W.norm(dim=-1)
    S[:, 4] = -1.0 - S[:, 4].abs()
    S[:, :, 1] = theta[:, None, 1] + 0.3 * eps[:, None] * (torch.rand(M, B, generator=gen) - 0.5)
    S[:, 4, 1] = theta[:, 1] - 0.1
    th = theta[:, None]
    hit, band = (S > th) & (S > 0), (S - th).abs() < (0.5 * eps)[:, None, None]
    assert not hit[:, 4].any() and band[:, :, 1].all() and (band & ~hit).any() and (band & hit).any()
    assert hit[1, :, 3].any() and (S[1, :, 3] < 0).any()

    to = lambda *ts: [t.to(DEV) for t in ts]  # noqa: E731
    Sg, Wg, rg, tg, eg, lg, ig = to(S, W, r, theta, eps, lam, inv)
    c, fired = torch.full((M, B, n), float("nan"), device=DEV), torch.full((M, n), 3.0, device=DEV)
    bits = torch.full((M, B, NW), -1, dtype=torch.int64, device=DEV)
    l0 = torch.full((M,), 2, dtype=torch.int32, device=DEV)
    ext.jump_select(Sg, tg, eg, c, fired, bits, l0)
    H.check_bits("c", c.cpu(), torch.where(hit, S, torch.zeros(())))
    H.check_bits("fired", fired.cpu(), 3.0 + hit.sum(1).float())
    assert l0.cpu().tolist() == (2 + hit.sum((1, 2))).tolist()
    padded = torch.zeros(M, B, NW * 64, dtype=torch.int64)
    padded[..., :n] = band
    want_bits = (padded.view(M, B, NW, 64) << torch.arange(64)).sum(-1)  # bit 63 wraps into the sign
    assert torch.equal(bits.cpu(), want_bits)

    runs = []
    for _ in range(2):
        g = torch.full((M, n), float("nan"), device=DEV)
        ext.jump_grad_theta(bits, Wg, ig, rg, tg, eg, lg, g)
        runs.append(g.cpu())
    H.check_bits("g_theta, second launch", runs[1], runs[0])
    W64, th64, eps64, lam64 = W.double() * inv.double()[..., None], theta.double(), eps.double()[:, None], lam.double()[:, None]
    gs, K = 2.0 / (B * d), band.sum(1)
    dots, dots_abs = H.dot("mbd,mnd->mbn", r, W64)
    ref = -(th64 * (gs * dots * band).sum(1) + lam64 * K / B) / eps64
    # per entry a length-d dot, its scale, and a place in a sum of K; then the closing products and the division
    mag = (th64.abs() * (gs * dots_abs * band).sum(1) + lam64 * K / B) / eps64
    out = H.check("g_theta", runs[0], ref, (H.c_dot(d) + K + 8) * U * mag)
    print(f"[jump64] {d}x{B}x{n} g_theta {out['worst']:.3f}")
    assert (K[:, 1] == B).all() and torch.equal(runs[0][K == 0], torch.zeros(int((K == 0).sum())))


def _models(shape, seed=0):
    M, B, d, n = shape
    gen = torch.Generator().manual_seed(seed)
    models = []
    for eps, lam in zip(EPS, LAM):
        p, b = JumpReLUEncoder.init(d, n, lam, bandwidth=eps)
        p["dict"], p["threshold"] = torch.randn(n, d, generator=gen), -0.1 + 0.7 * torch.rand(n, generator=gen)
        models.append((p, b))
    return models, torch.randn(B, d, generator=gen)


def _ensemble(models, dev=DEV, dtype=torch.float32):
    cast = lambda tree: R.tree_apply(lambda t: t.to(dev, dtype), tree)  # noqa: E731
    return FunctionalEnsemble([(cast(p), cast(b)) for p, b in models], JumpReLUEncoder, adam, {"lr": 1e-3},
                              device=dev, backend="hip" if dev == DEV else "torch")


@pytest.mark.parametrize("shape", [(2, 36, 132, 68), (2, 37, 2112, 132)], ids=lambda s: "x".join(map(str, s)))
def test_step_matches_fp64_autograd(shape):
    """Against the torch backend in fp64, its fp32 run the yardstick: gw (projected)
    and g_theta as Adam's moments, the losses, the updated parameters."""
    M, B, d, n = shape
    models, x = _models(shape)
    ens, e64, e32 = _ensemble(models), _ensemble(models, "cpu", torch.float64), _ensemble(models, "cpu")
    assert type(ens._hip_step).__name__ == "HipJumpReLUStep"
    What = e64.params["dict"] / e64.params["dict"].norm(dim=-1, keepdim=True)
    pre, th = x.double() @ What.mT, e64.params["threshold"][:, None]
    knees = torch.stack([pre - th, pre, (pre - th).abs() - 0.5 * e64.buffers["bandwidth"][:, None, None]])
    assert knees.abs().min() > 64 * U * pre.abs().max()
    got = ens.step_batch(x.to(DEV))
    (g64, (l64, aux64)), (g32, (l32, _)) = e64.compute_grads(x.double()), e32.compute_grads(x)
    e64.apply_grads(g64), e32.apply_grads(g32)
    torch.cuda.synchronize()
    assert torch.equal(got[1]["c"].cpu() > 0, aux64["c"] > 0) and (ens._hip_step.g_theta != 0).any()
    depths = R.loss_depths(R.case("topk"), B, d, n)
    depths["l0"] = depths["l_reconstruction"]
    worst = R.compare_losses(got[0], {"loss64": l64, "loss32": l32}, depths)
    for what in ("mu", "nu"):
        worst[what] = R.compare(ens.optim_states[what], g64, g32, what, 1)
    worst["params"] = R.compare(ens.params, e64.params, e32.params)
    print(f"[jump-step] {'x'.join(map(str, shape))} {worst}")


def test_replayed_graph_matches_eager_steps():
    # B = 7: two blocks of k_sparse_dec_gc add into a model's loss partial, and a sum of two has one order
    models, x = _models((2, 7, 132, 132))
    ens, twin, x = _ensemble(models), _ensemble(models), x.to(DEV)
    twin._hip_step.use_graph = False
    for call in range(3):
        got, want = ens.step_batch(x), twin.step_batch(x)
        torch.cuda.synchronize()
        assert (ens._hip_step._graph is not None) == (call == 2) and twin._hip_step._graph is None
        for k in ("dict", "threshold"):
            H.check_bits(f"{k}, call {call}", ens.params[k], twin.params[k])
        for k in ("loss", "l_reconstruction", "l0"):
            H.check_bits(f"{k}, call {call}", got[0][k], want[0][k])


def test_d_above_the_limit_is_refused():
    d = ops.get_extension().sparse_max_d() + 4
    models, x = _models((1, 4, d, 8))
    with pytest.raises(RuntimeError, match=f"d <= {d - 4}, got d = {d}"):
        _ensemble(models[:1]).step_batch(x.to(DEV))

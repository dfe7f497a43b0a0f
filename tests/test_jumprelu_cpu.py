"""JumpReLUEncoder on the CPU: gradients against the formula, the band's edges, stacking."""

import inspect

import torch

from sparse_coding_amd.engine import hip_step
from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models.jumprelu import JumpReLUEncoder

B, N, D, EPS, LAM = 5, 7, 3, 1.0, 0.3


def _model(dtype=torch.float64, eps=EPS, lam=LAM, seed=0):
    torch.manual_seed(seed)
    p, b = JumpReLUEncoder.init(D, N, lam, bandwidth=eps, dtype=dtype)
    p["threshold"] = torch.tensor([0.2, -0.1, 0.5, 0.0, 0.3, 0.1, 0.4], dtype=dtype)
    return p, b, torch.randn(B, D, dtype=dtype)


def _grads(p, b, x):
    return torch.func.grad(JumpReLUEncoder.loss, has_aux=True)(p, b, x)[0]


def _forward(p, x):
    W = p["dict"] / p["dict"].norm(dim=-1, keepdim=True)
    pre = x @ W.T
    return W, pre, (pre > p["threshold"]) & (pre > 0)


def test_autograd_equals_the_formula_and_the_frozen_mask():
    p, b, x = _model()
    g = _grads(p, b, x)
    W, pre, h = _forward(p, x)
    th, r = p["threshold"], (pre * h) @ W - x
    in_band = (pre - th).abs() < EPS / 2
    assert (in_band & h).any() and (in_band & ~h).any() and (~in_band).any()
    want = torch.zeros(N, dtype=torch.float64)
    for j in range(N):
        for i in range(B):
            if abs(pre[i, j] - th[j]) < EPS / 2:
                want[j] -= (th[j] * (2 / (B * D)) * (r[i] @ W[j]) + LAM / B) / EPS
    torch.testing.assert_close(g["threshold"], want, rtol=1e-12, atol=1e-15)

    def frozen(Wraw):
        Wn = Wraw / Wraw.norm(dim=-1, keepdim=True)
        return ((((x @ Wn.T) * h) @ Wn - x) ** 2).mean()
    torch.testing.assert_close(g["dict"], torch.func.grad(frozen)(p["dict"]), rtol=1e-12, atol=1e-15)


def test_empty_band_and_band_below_the_threshold():
    p, b, x = _model(eps=1e-9)
    assert torch.equal(_grads(p, b, x)["threshold"], torch.zeros(N, dtype=torch.float64))
    p, b, x = _model()
    pre = _forward(p, x)[1]
    p["threshold"][2] = pre[:, 2].max() + 0.1  # feature 2 never hits; its best row is 0.1 below
    loss, (data, aux) = JumpReLUEncoder.loss(p, b, x)
    g = _grads(p, b, x)["threshold"][2]
    assert (aux["c"][:, 2] == 0).all() and g < 0
    learned = JumpReLUEncoder.to_learned_dict(p, b)
    assert torch.equal(learned.encode(x), aux["c"]) and data["l0"] * B == (aux["c"] > 0).sum()


def test_ensemble_stacks_the_buffers_and_dispatch_names_the_step():
    models = [_model(torch.float32, eps, lam, seed)[:2] for eps, lam, seed in ((0.5, 0.3, 0), (0.25, 0.1, 1))]
    x = _model(torch.float32)[2]
    ens = FunctionalEnsemble(models, JumpReLUEncoder, adam, {"lr": 1e-3}, device="cpu", backend="torch")
    assert ens.buffers["bandwidth"].tolist() == [0.5, 0.25] and ens.buffers["l0_alpha"].shape == (2,)
    before = ens.params["threshold"].clone()
    data, aux = ens.step_batch(x)
    for m, (p, b) in enumerate(models):
        torch.testing.assert_close(data["loss"][m], JumpReLUEncoder.loss(p, b, x)[0])
    assert not torch.equal(ens.params["threshold"], before)
    assert "JumpReLUEncoder: HipJumpReLUStep" in inspect.getsource(hip_step.maybe_make_step)

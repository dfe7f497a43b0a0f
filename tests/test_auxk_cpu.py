"""TopKAuxEncoder on the CPU (torch backend): the AuxK loss against an explicit
formula, the age rule, and the ensemble keeping the ages."""

import pytest
import torch

from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models.topk_auxk import TopKAuxEncoder

D, N, K, B, DEAD_AFTER = 8, 16, 2, 12, 3


def _model(k_aux, ages=None, dtype=torch.float64, seed=0):
    torch.manual_seed(seed)
    p, b = TopKAuxEncoder.init(D, N, K, auxk=k_aux, auxk_alpha=0.25, dead_after=DEAD_AFTER, dtype=dtype)
    if ages is not None:
        b["steps_since_fired"] = torch.tensor(ages, dtype=torch.int32)
    return p, b, torch.randn(B, D, dtype=dtype)


def test_no_dead_feature_gives_exact_zero():
    p, b, x = _model(4, ages=[DEAD_AFTER - 1] * N)
    loss, (data, aux) = TopKAuxEncoder.loss(p, b, x)
    assert data["l_aux"] == 0 and data["n_dead"] == 0 and torch.equal(loss, data["l_reconstruction"])
    assert TopKAuxEncoder.to_learned_dict(p, b).sparsity == K


@pytest.mark.parametrize("k_aux", [0, 1, 3, N])
def test_loss_equals_the_explicit_formula(k_aux):
    ages = [DEAD_AFTER + (j % 2) if j % 3 else 0 for j in range(N)]
    p, b, x = _model(k_aux, ages)
    loss, (data, aux) = TopKAuxEncoder.loss(p, b, x)

    W = p["dict"] / p["dict"].norm(dim=-1, keepdim=True)
    S = x @ W.T
    dead = torch.tensor(ages) >= DEAD_AFTER
    e = x - torch.zeros_like(S).scatter(-1, S.topk(K).indices, S.topk(K).values).clamp(min=0) @ W
    Sd = torch.where(dead, S, torch.zeros(())).clamp(min=0)
    top = Sd.topk(min(k_aux, int(dead.sum()))).indices
    l_aux = ((torch.zeros_like(S).scatter(-1, top, Sd.gather(-1, top)) @ W - e) ** 2).mean()
    l_aux = l_aux * (k_aux > 0)  # auxk == 0 switches the term off: no mean(e^2) is left behind

    assert data["n_dead"] == dead.sum() and (k_aux == 0) == (data["l_aux"] == 0)
    torch.testing.assert_close(data["l_aux"], l_aux, rtol=1e-13, atol=0)
    torch.testing.assert_close(loss, (e ** 2).mean() + 0.25 * l_aux, rtol=1e-13, atol=0)


def test_update_buffers_resets_and_increments():
    buffers = {"steps_since_fired": torch.tensor([[0, 5, 2], [7, 0, 1]], dtype=torch.int32)}
    c = torch.zeros(2, 4, 3)
    c[0, 2, 1], c[1, 0, 2], c[1, 3, 2] = 0.5, 1.0, 2.0
    TopKAuxEncoder.update_buffers(buffers, {"c": c})
    assert buffers["steps_since_fired"].tolist() == [[1, 0, 3], [8, 1, 0]]
    assert buffers["steps_since_fired"].dtype == torch.int32


def test_ensemble_keeps_the_ages():
    models = [_model(4, dtype=torch.float32, seed=s)[:2] for s in (0, 1)]
    x = _model(4, dtype=torch.float32)[2]
    ens = FunctionalEnsemble(models, TopKAuxEncoder, adam, {"lr": 1e-3}, device="cpu", backend="torch",
                             no_stacking=True)
    want = torch.zeros(2, N, dtype=torch.int32)
    for _ in range(2):
        data, aux = ens.step_batch(x)
        want = torch.where((aux["c"] > 0).any(1), 0, want + 1).int()
        assert torch.equal(ens.buffers["steps_since_fired"], want)
        assert data["n_dead"].tolist() == [0, 0] and (data["l_aux"] == 0).all()

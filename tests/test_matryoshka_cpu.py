"""Matryoshka BatchTopK on the CPU: signature, eval dictionaries, eager step."""

import pytest
import torch

from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models import MatryoshkaBatchTopKEncoder as Mat
from sparse_coding_amd.models.batch_topk import BatchTopKEncoder, BatchTopKLearnedDict

B, D, N, K = 48, 16, 40, 3


def _model(ends, dtype=torch.float32):
    torch.manual_seed(0)
    p, b = Mat.init(D, ends[-1], K, ends, dtype=dtype)
    return p, b, torch.randn(B, D, dtype=dtype)


@pytest.mark.parametrize("ends", [(N,), (64,)], ids=str)
def test_one_level_is_batch_topk(ends):
    p, b, x = _model(ends, torch.float64)
    with torch.enable_grad():
        g, (ld, aux) = torch.func.grad(Mat.loss, has_aux=True)(p, b, x)
        g0, (ld0, aux0) = torch.func.grad(BatchTopKEncoder.loss, has_aux=True)(p, b, x)
    assert torch.equal(ld["loss"], ld0["loss"]) and torch.equal(ld["mse_levels"], ld0["loss"][None])
    assert all(torch.equal(aux[k], aux0[k]) for k in ("c", "threshold"))
    assert torch.equal(g["dict"], g0["dict"]) and g["dict"].abs().max() > 0


def test_loss_is_the_sum_of_masked_decodes():
    p, b, x = _model(ends := (7, 22, N), torch.float64)
    loss, (ld, aux) = Mat.loss(p, b, x)
    What = p["dict"] / p["dict"].norm(dim=-1, keepdim=True)
    c = BatchTopKEncoder.encode_train(x, K, What)[0]
    want = torch.stack([(((c * (torch.arange(N) < e)) @ What - x) ** 2).mean() for e in ends])
    assert torch.equal(aux["c"], c) and (c > 0).sum() == K * B
    torch.testing.assert_close(ld["mse_levels"], want, rtol=1e-13, atol=0)
    torch.testing.assert_close(loss, want.sum(), rtol=1e-13, atol=0)
    assert loss is ld["loss"] and set(ld) == {"loss", "mse_levels"} and set(aux) == {"c", "threshold"}


def test_prefix_dicts_are_nested():
    p, b, x = _model(ends := (7, 22, N))
    b["threshold"].fill_(0.4)
    ld = Mat.to_learned_dict(p, b)
    full = ld.encode(x)
    assert ld.group_ends == list(ends) and 0 < (full != 0).sum() < full.numel()
    for g, e in enumerate(ends):
        sub = ld.prefix(g)
        assert type(sub) is BatchTopKLearnedDict and sub.threshold == ld.threshold and sub.n_feats == e
        torch.testing.assert_close(sub.encode(x), full[:, :e], rtol=1e-6, atol=0)


@pytest.mark.parametrize("ends", [(), (0, N), (8, 8, N), (20, 10, N), (8, N - 1), (8, N + 1),
                                  tuple(range(1, 9)) + (N,)])
def test_invalid_group_ends_raise(ends):
    with pytest.raises(ValueError):
        Mat.init(D, N, K, ends)


def test_eager_ensemble_steps():
    torch.manual_seed(1)
    models = [Mat.init(D, N, k, ends) for k, ends in ((2, (8, 20, N)), (4, (5, 33, N)))]
    ens = FunctionalEnsemble(models, Mat, adam, {"lr": 1e-3}, device="cpu", backend="torch", no_stacking=True)
    w0 = ens.params["dict"].clone()
    losses, aux = ens.step_batch(torch.randn(B, D))
    assert losses["mse_levels"].shape == (2, 3) and torch.allclose(losses["loss"], losses["mse_levels"].sum(1))
    assert ens.buffers["threshold_n"].tolist() == [1, 1] and ens.buffers["group_ends"].shape == (2, 3)
    assert torch.equal(ens.buffers["threshold"], torch.clamp(aux["threshold"], min=0.0))
    assert not torch.equal(ens.params["dict"], w0)  # and it trained

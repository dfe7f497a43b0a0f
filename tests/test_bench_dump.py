"""bench.py --dump-outputs writer: names, dtypes, size budget, fixed sample."""

import os

import numpy as np
import torch

import bench


def _step_outputs():
    g = torch.Generator().manual_seed(0)
    losses = {"loss": torch.rand(3, generator=g), "l_l1": torch.rand(3, generator=g).double()}
    aux = {"c": torch.rand(3, 40, 50, generator=g), "idx": torch.arange(7)}
    return losses, aux


def test_dump_outputs_whole_arrays(tmp_path):
    losses, aux = _step_outputs()
    bench.dump_outputs(str(tmp_path), losses, aux)
    assert sorted(os.listdir(tmp_path)) == ["aux_c.npy", "aux_idx.npy", "losses_l_l1.npy", "losses_loss.npy"]
    c = np.load(tmp_path / "aux_c.npy")
    assert c.dtype == np.float32 and c.shape == (3, 40, 50)
    assert np.array_equal(c, aux["c"].numpy())
    assert np.load(tmp_path / "losses_l_l1.npy").dtype == np.float64
    assert np.load(tmp_path / "aux_idx.npy").dtype == np.float32


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    losses, aux = _step_outputs()
    bench.dump_outputs(str(tmp_path / "a"), losses, aux)
    bench.dump_outputs(str(tmp_path / "b"), losses, aux)
    files = sorted(os.listdir(tmp_path / "a"))
    arrays = {f: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in arrays.values()) <= 4096
    # small arrays stay whole; the large one becomes a 1-D sample of its own elements
    assert np.array_equal(arrays["losses_loss.npy"], losses["loss"].numpy())
    c = arrays["aux_c.npy"]
    assert c.ndim == 1 and 0 < c.size < aux["c"].numel()
    flat = aux["c"].numpy().ravel()
    idx = np.arange(c.size, dtype=np.int64) * flat.size // c.size  # evenly spaced, distinct
    assert len(np.unique(idx)) == c.size
    assert np.array_equal(c, flat[idx])
    for f in files:
        assert np.array_equal(arrays[f], np.load(tmp_path / "b" / f))

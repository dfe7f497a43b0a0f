"""The fused Matryoshka BatchTopK step.  It lives beside engine/hip_step.py, whose
step classes are the grid of tests/step_reference.py; maybe_make_step
registers it with the others."""

from __future__ import annotations

import torch

from sparse_coding_amd.engine.hip_step import HipBatchTopKStep, _announce
from sparse_coding_amd.models.matryoshka import check_group_ends


class HipMatryoshkaStep(HipBatchTopKStep):
    """Fused Matryoshka BatchTopK training step (models/matryoshka.py): the
    BatchTopK step whose loss is the sum of the reconstruction errors of the
    G nested prefixes ``[:group_ends[g]]`` of the dictionary.

    Row norms, the encoder GEMM, the batch-level selection, the threshold
    state, Adam and graph capture are HipBatchTopKStep's.  Behind the selection
    it always runs k_sparse_dec_gc and k_sparse_grad_w (LEVELS), whatever
    ``topk_chain`` says: the nested losses come out of the sparse decode's
    running accumulator at the level boundaries, and a dense chain would pay
    one decode GEMM and its backward per level.  So it serves
    d <= ext.sparse_max_d() (8192) and raises at allocation beyond that; above
    d = 2048 the same two launchers run k_wsparse_dec_gc, k_sparse_hit_lists
    and k_wsparse_grad_w, which split a row over a workgroup's waves.

    ``R`` [M, G, B, d] holds, after a step, the suffix sums S_g of the prefix
    residuals (what feature j's gradient sees where the plain chain has r);
    ``r`` is the view R[:, G-1], the full-dictionary residual, and
    ``mse_parts`` [M, G] the levels' squared-error sums.
    """

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext)
        ends = ensemble.buffers["group_ends"].reshape(self.n_models, -1)
        for row in ends.tolist():
            check_group_ends(row, self.n_dict)
        self.n_levels = ends.shape[1]
        # allocated here like lr_mult: a captured graph holds its address
        self.ends_i32 = ends.to(self._dev, torch.int32).contiguous()

    def _alloc_workspaces(self, B: int):
        M, d, G = self.n_models, self.d_act, self.n_levels
        if d > self.ext.sparse_max_d():
            raise RuntimeError(f"HipMatryoshkaStep serves d <= {self.ext.sparse_max_d()}, got d = {d}")
        self.kc["topk_chain"] = "sparse"  # the hit lists; there is no dense Matryoshka chain
        super()._alloc_workspaces(B)
        self.R = self._empty(M, G, B, d)
        self.r = self.R[:, G - 1]
        self.mse_parts = self._empty(M, G)

    def _behind_selection(self, x, W, B, on_grads):
        ext = self.ext
        self.mse_parts.zero_()
        ext.msparse_dec_gc(self.c, W, self.inv_norms, x, self.ends_i32, self.R, self.gpre, self.mse_parts)
        ext.msparse_grad_w(self.c, self.gpre, self.R, x, self.ends_i32, self.gw, self.hits, self.hit_counts)
        _announce(on_grads, self.gw)

    def _loss_data(self, B: int):
        scale = B * self.d_act
        return {"loss": self.mse_parts.sum(1) / scale, "mse_levels": self.mse_parts / scale,
                "threshold": self.thr_batch}

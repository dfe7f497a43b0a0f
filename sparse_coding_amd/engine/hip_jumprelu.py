"""The fused JumpReLU step.  It lives beside engine/hip_step.py, whose step
classes are the grid of tests/step_reference.py; maybe_make_step registers it
with the others."""

from __future__ import annotations

import torch

from sparse_coding_amd.engine.hip_step import HipTopKStep, _announce, _HipStep


class HipJumpReLUStep(HipTopKStep):
    """Fused JumpReLU training step (models/jumprelu.py):
    L = L_rec + l0_alpha * mean hits per row, with a learned threshold.

    Row norms, the encoder GEMM, Adam on ``dict`` and graph capture are
    HipTopKStep's.  The selection is a threshold test, and behind it always
    runs the sparse chain, whatever ``topk_chain`` says: a row has any number
    of hits, and that chain asks only for ``c > 0``.  With the kernels of
    ops/hip/sae_jumprelu.hip the order is:

      jump_select      c, fired, l0_count, and the band |S - theta| < eps / 2
                       as ballot words; ahead of sparse_grad_w, which
                       overwrites the bytes of ``scores``
      sparse_dec_gc    r, loss_parts[:, 0], gpre
      jump_grad_theta  g_theta over the band, hits or not
      sparse_grad_w    gw

    Nothing is read on the host, so the whole step is captured like
    HipTopKStep's.  ``bandwidth`` and ``l0_alpha`` are copied at construction.

    It serves d <= ext.sparse_max_d() (8192) and raises at allocation beyond.
    """

    def __init__(self, ensemble, ext):
        # HipTopKStep's constructor minus the per-model k, which this model has not
        _HipStep.__init__(self, ensemble, ext)
        b, M, dev = ensemble.buffers, self.n_models, self._dev
        self.dummy_bias = torch.zeros(M, self.n_dict, device=dev)
        self.lr_mult = torch.ones(M, self.n_dict, device=dev)
        # allocated here like lr_mult: a captured graph holds their addresses
        self.bandwidth = b["bandwidth"].detach().to(dev, torch.float32).reshape(M).contiguous()
        self.l0_alpha = b["l0_alpha"].detach().to(dev, torch.float32).reshape(M).contiguous()

    def _alloc_workspaces(self, B: int):
        M, n, d = self.n_models, self.n_dict, self.d_act
        if d > self.ext.sparse_max_d():
            raise RuntimeError(f"HipJumpReLUStep serves d <= {self.ext.sparse_max_d()}, got d = {d}")
        self.kc["topk_chain"] = "sparse"  # rows have any number of hits
        super()._alloc_workspaces(B)
        self.band_bits = torch.empty(M, B, (n + 63) // 64, device=self._dev, dtype=torch.int64)
        self.l0_count = torch.zeros(M, device=self._dev, dtype=torch.int32)
        self.g_theta = self._empty(M, n)

    def _select(self):
        self.l0_count.zero_()  # jump_select adds into it
        self.ext.jump_select(self.scores, self.ens.params["threshold"], self.bandwidth, self.c, self.fired,
                             self.band_bits, self.l0_count)

    def _behind_selection(self, x, W, B, on_grads):
        ext = self.ext
        ext.sparse_dec_gc(self.c, W, self.inv_norms, x, self.r, self.gpre, self.loss_parts)
        ext.jump_grad_theta(self.band_bits, W, self.inv_norms, self.r, self.ens.params["threshold"],
                            self.bandwidth, self.l0_alpha, self.g_theta)
        ext.sparse_grad_w(self.c, self.gpre, self.r, x, self.gw, self.hits, self.hit_counts)
        _announce(on_grads, self.gw, self.g_theta)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("dict", self.gw, t, project=True, lr_mult=self.lr_mult, eps_norm=self.EPS)
        self._adam_vector("threshold", self.g_theta, t)

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        l0 = self.l0_count / B
        return {"loss": mse + self.l0_alpha * l0, "l_reconstruction": mse, "l0": l0}

    def dp_grad_tensors(self):
        return [self.gw, self.g_theta]

"""The fused TopK step with the AuxK dead-latent loss.  It lives beside
engine/hip_step.py, whose step classes are the grid of tests/step_reference.py;
maybe_make_step registers it with the others."""

from __future__ import annotations

import torch

from sparse_coding_amd.engine.hip_step import HipTopKStep, _announce


class HipTopKAuxStep(HipTopKStep):
    """Fused TopK training step with the auxiliary dead-latent loss
    (models/topk_auxk.py): L = L_rec + auxk_alpha * L_aux.

    Row norms, the encoder GEMM, the per-row selection, Adam and graph capture
    are HipTopKStep's.  Behind the selection it always runs the sparse chain,
    whatever ``topk_chain`` says: that chain's ``hit_counts`` are "did this
    feature fire in this batch", which the ages are updated from.  Around it
    run the kernels of ops/hip/sae_auxk.hip, in this order:

      auxk_age       n_dead per model from the ages, as they are before the step
      auxk_select    per row the min(k_aux, n_dead) best positive scores over
                     the dead columns, as compact ascending lists; ahead of
                     sparse_grad_w, which overwrites the bytes of ``scores``
      sparse_dec_gc  r, loss_parts[:, 0], gpre
      auxk_dec_gc    r_aux = z @ What + r, loss_parts[:, 1], gpre_aux
      sparse_grad_w  gw, hit_counts
      auxk_grad_w    gw += the aux loss's gradient
      auxk_age       the ages' update from hit_counts

    A model with no dead feature (or ``auxk == 0``) costs the launches alone:
    its workgroups leave at once, ``l_aux`` is an exact 0 and ``gw`` holds the
    bits of a plain HipTopKStep under ``topk_chain="sparse"``.  Nothing is read
    on the host, so the whole step is captured like HipTopKStep's.

    The ages (buffer "steps_since_fired", int32 [M, n]) are read from
    ``ens.buffers`` at every launch, not at construction: a resumed sweep
    replaces the whole buffer tree.  A captured graph holds the buffer's
    address, so when it changes the graph is dropped and captured again.
    ``auxk``, ``auxk_alpha`` and ``dead_after`` are copied at construction.
    ``codes`` stays the main ``c``: aux activations are no part of it and do
    not count as firing.

    It serves d <= ext.auxk_max_d() (2048) and raises at allocation beyond.

    Under data parallelism each rank ages its features by its local batch;
    the ages are not synchronised across ranks.
    """

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext)
        b, M, dev = ensemble.buffers, self.n_models, self._dev
        k_aux = [int(k) for k in b["auxk"].reshape(-1).tolist()]
        # allocated here like lr_mult: a captured graph holds their addresses
        self.k_aux_i32 = torch.tensor(k_aux, device=dev, dtype=torch.int32)
        self.alpha = b["auxk_alpha"].detach().to(dev, torch.float32).reshape(M).contiguous()
        self.dead_after_i32 = b["dead_after"].detach().to(dev, torch.int32).reshape(M).contiguous()
        self.n_dead = torch.zeros(M, device=dev, dtype=torch.int32)
        # stride of the row lists: a row takes min(k_aux, n_dead) <= n entries
        self.KA = max(1, min(max(k_aux), self.n_dict))

    def _ages(self):
        return self.ens.buffers["steps_since_fired"]

    def _alloc_workspaces(self, B: int):
        M, d, KA = self.n_models, self.d_act, self.KA
        if d > self.ext.auxk_max_d():
            raise RuntimeError(f"HipTopKAuxStep serves d <= {self.ext.auxk_max_d()}, got d = {d}")
        self.kc["topk_chain"] = "sparse"  # hit_counts exist on that chain only
        super()._alloc_workspaces(B)
        self.aux_idx = torch.empty(M, B, KA, device=self._dev, dtype=torch.int32)
        self.aux_cnt = torch.empty(M, B, device=self._dev, dtype=torch.int32)
        self.aux_val = self._empty(M, B, KA)
        self.gpre_aux = self._empty(M, B, KA)
        self.r_aux = self._empty(M, B, d)

    def _behind_selection(self, x, W, B, on_grads):
        ext, ages = self.ext, self._ages()
        state = (self.k_aux_i32, self.n_dead)
        lists = (self.aux_idx, self.aux_val, self.aux_cnt)
        ext.auxk_age(ages, None, self.dead_after_i32, self.n_dead)
        ext.auxk_select(self.scores, ages, self.dead_after_i32, *state, *lists)
        ext.sparse_dec_gc(self.c, W, self.inv_norms, x, self.r, self.gpre, self.loss_parts)
        ext.auxk_dec_gc(*lists, W, self.inv_norms, self.r, self.alpha, *state, self.r_aux, self.gpre_aux,
                        self.loss_parts)
        ext.sparse_grad_w(self.c, self.gpre, self.r, x, self.gw, self.hits, self.hit_counts)
        ext.auxk_grad_w(*lists, self.gpre_aux, self.r_aux, x, ages, self.dead_after_i32, *state, self.alpha,
                        self.gw)
        ext.auxk_age(ages, self.hit_counts, self.dead_after_i32, self.n_dead)
        _announce(on_grads, self.gw)

    def graph_key(self):
        return super().graph_key() + (self._ages().data_ptr(),)

    def _loss_data(self, B: int):
        parts = self.loss_parts / (B * self.d_act)
        return {"loss": parts[:, 0] + self.alpha * parts[:, 1], "l_reconstruction": parts[:, 0],
                "l_aux": parts[:, 1], "n_dead": self.n_dead}

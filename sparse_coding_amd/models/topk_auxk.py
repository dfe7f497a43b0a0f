"""TopK encoder with the auxiliary dead-latent loss ("AuxK", Gao et al. 2024).

A feature that never makes a row's top-k gets no gradient and stays dead.  AuxK
gives the dead features a loss of their own: they are asked to reconstruct what
the live ones left over.

Semantics, per model (the fused step ``HipTopKAuxStep`` implements exactly
these, in the ``k_auxk_*`` kernels):

* ``W_hat``, ``S = x @ W_hat.T``, ``c = relu(TopK_k(S))``, ``x_hat = c @ W_hat``
  and ``L_rec = mse(x, x_hat)`` are ``TopKEncoder``'s;
* feature j is dead when ``steps_since_fired[j] >= dead_after``, read before
  the step; ``n_dead`` counts them;
* with ``n_dead == 0`` or ``auxk == 0``, ``L_aux = 0`` exactly.  Otherwise ``z``
  keeps, per row, the ``min(auxk, n_dead)`` largest of ``S`` over the dead
  columns, and of those only where ``S > 0``; among equal scores at the cut the
  lowest column wins.  ``e = x - x_hat`` is a constant, and
  ``L_aux = mean((z @ W_hat - e)^2)`` over ``B * d`` elements, as ``L_rec``;
* ``L = L_rec + auxk_alpha * L_aux``; the gradient flows through ``z`` into
  ``W_hat`` in both of its roles, as it does through ``c``.  A dead feature in
  a row's main top-k gets both contributions;
* after the step ``steps_since_fired[j]`` is 0 where any row has ``c[:, j] > 0``
  and one more otherwise.  Aux activations do not count as firing.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from sparse_coding_amd.models.sae_signatures import DictSignature
from sparse_coding_amd.models.topk import TopKEncoder, TopKLearnedDict


def aux_select(scores, dead, k_aux):
    """(idx, keep): per row the min(k_aux, n_dead) best dead columns of scores,
    lowest column first among equals, and which of them are positive."""
    kk = min(int(k_aux), int(dead.sum()))
    masked = torch.where(dead & (scores > 0), scores, torch.full_like(scores, -float("inf")))
    vals, idx = torch.sort(masked, dim=-1, descending=True, stable=True)
    return idx[..., :kk], vals[..., :kk] > 0


class TopKAuxEncoder(DictSignature):
    @staticmethod
    def init(d_activation, n_features, sparsity, auxk=None, auxk_alpha=1.0 / 32, dead_after=1000,
             dtype=torch.float32):
        params = {"dict": torch.randn(n_features, d_activation, dtype=dtype)}
        buffers = {
            "sparsity": torch.tensor(sparsity, dtype=torch.long),
            "auxk": torch.tensor(d_activation // 2 if auxk is None else auxk, dtype=torch.long),
            "auxk_alpha": torch.tensor(auxk_alpha, dtype=torch.float32),
            "dead_after": torch.tensor(dead_after, dtype=torch.long),
            "steps_since_fired": torch.zeros(n_features, dtype=torch.int32),
        }
        return params, buffers

    @staticmethod
    def loss(params, buffers, batch):
        normed = params["dict"] / torch.norm(params["dict"], dim=-1)[:, None]
        scores = batch @ normed.T
        code = TopKEncoder.encode(batch, buffers["sparsity"], normed)
        x_hat = code @ normed
        l_rec = F.mse_loss(batch, x_hat)
        dead = buffers["steps_since_fired"] >= buffers["dead_after"]
        n_dead = dead.sum()
        l_aux = torch.zeros_like(l_rec)
        if int(n_dead) > 0 and int(buffers["auxk"]) > 0:
            idx, keep = aux_select(scores.detach(), dead, buffers["auxk"])
            z = torch.zeros_like(scores).scatter(-1, idx, scores.gather(-1, idx) * keep)
            l_aux = F.mse_loss(z @ normed, (batch - x_hat).detach())
        loss = l_rec + buffers["auxk_alpha"].to(l_rec.dtype) * l_aux
        loss_data = {"loss": loss, "l_reconstruction": l_rec, "l_aux": l_aux, "n_dead": n_dead}
        return loss, (loss_data, {"c": code})

    @staticmethod
    def update_buffers(buffers, aux):
        """Age the stacked features by this step's codes (aux["c"], [M, B, n]),
        in place: 0 where a feature fired on any row, one more otherwise."""
        age = buffers["steps_since_fired"]
        fired = (aux["c"].detach() > 0).any(dim=-2).reshape(age.shape)
        age.copy_(torch.where(fired, torch.zeros_like(age), age + 1))

    @staticmethod
    def to_learned_dict(params, buffers):
        normed = params["dict"] / torch.norm(params["dict"], dim=-1)[:, None]
        return TopKLearnedDict(normed, buffers["sparsity"].item())

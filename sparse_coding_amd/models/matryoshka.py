"""Matryoshka BatchTopK encoder signature + learned dict.

A Matryoshka SAE (Bussmann, Nabeshima, Karvonen & Nanda, 2025) trains nested
dictionaries at once: the features are cut into ``G`` levels by the ascending
``group_ends = (e_0, ..., e_{G-1})``, ``e_{G-1} = n``, and the loss is the sum
of the reconstruction errors of the ``G`` prefixes ``[:e_g]``.  The early
features have to reconstruct on their own, which keeps them general and stops
a large dictionary from splitting or absorbing them.

Semantics, per model (the fused step ``HipMatryoshkaStep`` implements exactly
these, in the ``k_msparse_*`` kernels):

* ``group_ends`` is int64 ``[G]`` with ``1 <= G <= 8``, strictly increasing,
  ``group_ends[0] >= 1`` and ``group_ends[-1] == n_features``; ``init`` raises
  ``ValueError`` otherwise.  The models of one ensemble share ``G`` (the
  buffers stack to ``[M, G]``); their ends may differ;
* scores, selection, the threshold ``t``, the code ``c``, the ``K == 0`` case,
  ``update_buffers`` and the inference threshold are ``BatchTopKEncoder``'s:
  one selection ranks all ``n`` features, whatever their level;
* with ``W_hat`` the row-normalised dictionary (no eps clamp):
  ``xhat_g = c[:, :e_g] @ W_hat[:e_g]`` and ``loss = sum_g mse(x, xhat_g)``.
  ``t`` is a constant and the gradient flows through the kept entries only;
* ``loss_data = {"loss": loss, "mse_levels": [G]}``,
  ``aux = {"c": c, "threshold": t}``;
* ``to_learned_dict`` gives a ``MatryoshkaBatchTopKLearnedDict``, whose
  ``prefix(g)`` is the ``BatchTopKLearnedDict`` over the rows ``[:e_g]`` at the
  same threshold: the nested dictionary one evaluates;
* with ``G == 1`` everything equals ``BatchTopKEncoder``.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from sparse_coding_amd.models.batch_topk import BatchTopKEncoder, BatchTopKLearnedDict, _normed

MAX_LEVELS = 8


def check_group_ends(group_ends, n_features):
    """The validated ends as a list of ints."""
    ends = [int(e) for e in group_ends]
    if not 1 <= len(ends) <= MAX_LEVELS:
        raise ValueError(f"group_ends needs 1..{MAX_LEVELS} levels, got {len(ends)}")
    if ends[0] < 1 or any(a >= b for a, b in zip(ends, ends[1:])):
        raise ValueError(f"group_ends must be strictly increasing from at least 1, got {ends}")
    if ends[-1] != n_features:
        raise ValueError(f"group_ends must end at n_features = {n_features}, got {ends}")
    return ends


class MatryoshkaBatchTopKEncoder(BatchTopKEncoder):
    @staticmethod
    def init(d_activation, n_features, sparsity, group_ends, threshold_lr=0.01, dtype=torch.float32):
        ends = check_group_ends(group_ends, n_features)
        params, buffers = BatchTopKEncoder.init(d_activation, n_features, sparsity, threshold_lr, dtype)
        buffers["group_ends"] = torch.tensor(ends, dtype=torch.long)
        return params, buffers

    @staticmethod
    def loss(params, buffers, batch):
        normed = _normed(params["dict"])
        code, t = BatchTopKEncoder.encode_train(batch, buffers["sparsity"], normed)
        # int(e) as encode_train's int(sparsity): one read per level, which a
        # device tensor allows under torch.func.grad where .tolist() does not
        levels = torch.stack([F.mse_loss(batch, code[:, :int(e)] @ normed[:int(e)])
                              for e in buffers["group_ends"]])
        loss = levels.sum()
        return loss, ({"loss": loss, "mse_levels": levels}, {"c": code, "threshold": t})

    @staticmethod
    def to_learned_dict(params, buffers):
        return MatryoshkaBatchTopKLearnedDict(_normed(params["dict"]), buffers["sparsity"].item(),
                                              buffers["threshold"].item(), buffers["group_ends"].tolist())


class MatryoshkaBatchTopKLearnedDict(BatchTopKLearnedDict):
    """BatchTopKLearnedDict that knows its levels."""

    def __init__(self, dict, sparsity, threshold, group_ends):
        super().__init__(dict, sparsity, threshold)
        self.group_ends = check_group_ends(group_ends, self.n_feats)

    def prefix(self, g):
        """The nested dictionary of level g: rows [:group_ends[g]], same threshold."""
        return BatchTopKLearnedDict(self.dict[:self.group_ends[g]], self.sparsity, self.threshold)

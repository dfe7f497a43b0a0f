"""BatchTopK encoder signature + learned dict.

BatchTopK (Bussmann, Leask & Nanda, 2024) relaxes the TopK encoder's "exactly
k features per activation" to "k features per activation on average": of the
``[B, n]`` scores of a batch, the ``K = min(k * B, B * n)`` largest are kept,
wherever they fall, so an activation gets as many features as it needs.  At
inference there is no batch to rank against, so a global threshold is learned
as a running average of the training batches' selection thresholds.

Semantics, per model (the fused step ``HipBatchTopKStep`` implements exactly
these, selection in the ``k_btk_*`` kernels):

* scores ``S = x @ W_hat.T`` with ``W_hat`` the row-normalised dictionary (no
  eps clamp, no bias: as ``TopKEncoder``);
* ``t`` = the K-th largest element of ``S`` as a multiset over the whole matrix;
  ``c = S`` where ``S >= t`` and ``S > 0``, else 0.  Every exact tie at ``t`` is
  kept, which makes the code deterministic;
* ``K == 0``: ``c`` is zero, ``t`` is reported as ``+inf`` and the threshold
  state is left alone;
* the gradient flows through the kept entries only, ``t`` is a constant, and
  the loss is ``mse(x, c @ W_hat)``: no L1 term;
* once per training step, with ``stat = max(t, 0)``: ``threshold = stat`` on the
  first update, ``threshold += threshold_lr * (stat - threshold)`` after it;
  ``threshold_n`` counts the updates;
* ``BatchTopKLearnedDict.encode`` keeps ``S`` where ``S >= threshold`` and
  ``S > 0``.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from sparse_coding_amd.models.learned_dict import LearnedDict
from sparse_coding_amd.models.sae_signatures import DictSignature


def _normed(dictionary):
    # as TopKEncoder: the raw norm, no eps clamp
    return dictionary / torch.norm(dictionary, dim=-1)[:, None]


def threshold_gate(scores, threshold):
    """scores where (scores >= threshold) & (scores > 0), else +0."""
    keep = (scores >= threshold) & (scores > 0)
    return torch.where(keep, scores, torch.zeros_like(scores))


class BatchTopKEncoder(DictSignature):
    @staticmethod
    def init(d_activation, n_features, sparsity, threshold_lr=0.01, dtype=torch.float32):
        params = {"dict": torch.randn(n_features, d_activation, dtype=dtype)}
        buffers = {
            "sparsity": torch.tensor(sparsity, dtype=torch.long),
            "threshold": torch.tensor(0.0, dtype=torch.float32),
            "threshold_n": torch.tensor(0, dtype=torch.int32),
            "threshold_lr": torch.tensor(threshold_lr, dtype=torch.float32),
        }
        return params, buffers

    @staticmethod
    def encode_train(b, sparsity, normed_dict):
        """(code, t) of one batch: the K = min(k*B, B*n) largest scores of the
        whole [B, n] matrix, ties at t included."""
        scores = b @ normed_dict.T
        K = min(int(sparsity) * scores.shape[0], scores.numel())
        if K <= 0:
            return torch.zeros_like(scores), scores.new_tensor(float("inf"))
        t = torch.topk(scores.detach().flatten(), K).values[-1]
        return threshold_gate(scores, t), t

    @staticmethod
    def loss(params, buffers, batch):
        normed = _normed(params["dict"])
        code, t = BatchTopKEncoder.encode_train(batch, buffers["sparsity"], normed)
        x_hat = code @ normed
        loss = F.mse_loss(batch, x_hat)
        return loss, ({"loss": loss}, {"c": code, "threshold": t})

    @staticmethod
    def update_buffers(buffers, aux):
        """Fold this step's selection thresholds (aux["threshold"], [M]) into
        the stacked inference-threshold state, in place."""
        theta, count = buffers["threshold"], buffers["threshold_n"]
        t = aux["threshold"].detach().to(theta.dtype).reshape(theta.shape)
        valid = buffers["sparsity"].reshape(theta.shape) > 0  # K == 0 leaves the state alone
        stat = torch.clamp(t, min=0.0)
        moved = theta + buffers["threshold_lr"].reshape(theta.shape) * (stat - theta)
        new = torch.where((count == 0) | (stat == theta), stat, moved)
        theta.copy_(torch.where(valid, new, theta))
        count.add_(valid.to(count.dtype))

    @staticmethod
    def to_learned_dict(params, buffers):
        return BatchTopKLearnedDict(_normed(params["dict"]), buffers["sparsity"].item(),
                                    buffers["threshold"].item())


class BatchTopKLearnedDict(LearnedDict):
    """Evaluation-time BatchTopK dictionary: the learned global threshold
    stands in for the batch-level selection."""

    def __init__(self, dict, sparsity, threshold):
        self.dict = dict
        self.sparsity = sparsity
        self.threshold = float(threshold)
        self.n_feats, self.activation_size = self.dict.shape

    def to_device(self, device):
        self.dict = self.dict.to(device)

    def encode(self, x):
        return threshold_gate(x @ self.dict.T, self.threshold)

    def get_learned_dict(self):
        return self.dict

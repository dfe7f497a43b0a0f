"""CPU reference and comparator for the batch-level top-k selection
(``ext.batch_topk_select`` / ``BatchTopKEncoder``).

Per model m, with K = min(ks[m] * B, B * n):

  t       = the K-th largest element of scores[m], a multiset over the whole
            [B, n] matrix (+inf when K == 0)
  c[b,j]  = scores[b,j] if scores[b,j] >= t and scores[b,j] > 0, else +0.0
            (every exact tie at t kept; kept values copied bit for bit)
  fired_j = #{b : c[b,j] > 0}

The same fp32 score tensor goes to the kernel and to this reference, so the
comparison is exact: no tolerances.  t is taken in the total order of the
bit patterns (-0.0 below +0.0), which is the order a radix select sees; for
the selection itself the two zeros do not differ because of the `> 0`.
"""

import torch

from tests.hip_reference import Mismatch, canon_zero, check_bits


def _keys(s: torch.Tensor) -> torch.Tensor:
    """int64 keys ordered as the floats are, with -0.0 < +0.0 (no NaN)."""
    i = s.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF) - 1, i)


def _unkey(k: int) -> torch.Tensor:
    bits = k if k >= 0 else ((-(k + 1)) | 0x80000000)
    if bits >= 1 << 31:
        bits -= 1 << 32
    return torch.tensor(bits, dtype=torch.int32).view(torch.float32)


def batch_topk_ref(scores, ks):
    """(c, fired increment, t) by the semantics above; CPU tensors."""
    s = scores.detach().cpu().float().contiguous()
    assert not torch.isnan(s).any(), "NaN scores are outside the contract"
    M, B, n = s.shape
    c = torch.zeros_like(s)
    t = torch.full((M,), float("inf"))
    for m in range(M):
        K = min(int(ks[m]) * B, B * n)
        if K <= 0:
            continue
        kth = torch.sort(_keys(s[m]).flatten(), descending=True).values[K - 1]
        t[m] = _unkey(int(kth))
        keep = (s[m] >= t[m]) & (s[m] > 0)
        c[m] = torch.where(keep, s[m], torch.zeros_like(s[m]))
    return c, (c > 0).float().sum(dim=1), t


def theta_ref(theta, count, stat, a):
    """One update of the inference threshold, in fp64: (theta', count')."""
    theta, stat, a = float(theta), float(stat), float(a)
    if int(count) == 0:
        return stat, 1
    return theta + a * (stat - theta), int(count) + 1


def check_batch_topk(name, scores, c, fired, t, ks):
    """c (after canon_zero), the fired increment and t of a selection must
    equal the reference bit for bit; raises Mismatch otherwise."""
    c_ref, fired_ref, t_ref = batch_topk_ref(scores, ks)
    c = c.detach().cpu()
    if c.shape != c_ref.shape:
        raise Mismatch(f"{name}: c has shape {tuple(c.shape)}, scores {tuple(c_ref.shape)}")
    check_bits(f"{name}: t", t.detach().cpu().float().reshape(-1), t_ref)
    check_bits(f"{name}: c", canon_zero(c), canon_zero(c_ref))
    fired = fired.detach().cpu().float()
    if fired.shape != fired_ref.shape or not torch.equal(fired, fired_ref):
        bad = (fired != fired_ref).nonzero()
        first = tuple(int(i) for i in bad[0]) if len(bad) else ()
        raise Mismatch(f"{name}: fired differs from #{{b: c > 0}} at {len(bad)} features; first at {first}")

"""fp64 autograd references for the gradients every fused step hands to Adam.

Plain helpers (no fixtures, no hooks, no GPU import) shared by
test_step_reference_cpu.py, which validates them on the CPU, and
test_hip_step_grads_gpu.py, which runs every fused step class of
engine/hip_step.py against them.

The observable is Adam's first moment.  After one ``step()`` from zero
optimizer state ``mu = (1-b1) g`` and ``nu = (1-b2) g^2`` with ``g`` the
gradient Adam consumed: projection through the row normalisation, clamp mask,
bias decay and rho gate included.  With ``lr = 0`` the parameters never move,
every step sees the same ``g`` and after ``t`` steps ``mu = (1-b1^t) g``.
``mu`` has the tree of ``ens.params``, so it is compared leaf for leaf with
``torch.func.grad`` of the signature's own ``loss``: no table of workspaces, no
knowledge of a step's internals.

* ``cases()`` / ``GRID``: the thirteen signatures plus the whitened dispatch,
  each with a perturbation that takes the parameters off their trivial initial
  values, and the (case, shape, staging) combinations the GPU module runs.
* ``reference``: per model on the CPU, the float64 loss dict, codes and
  gradient tree, and the same in float32: the yardstick, the code the torch
  backend runs in production.
* ``decisions``: records the argument of every nonsmooth decision of the
  float64 forward against its knee.  The comparison only means something on
  inputs where no decision is within rounding of its knee; ``SEEDS`` holds, per
  grid entry, the first seed for which that is so, found on the CPU from the
  reference alone.
* ``compare`` / ``compare_losses``: the comparators.
* ``doctored``: fp32 autograd gradients of deliberately wrong problems, which
  the comparator has to reject.
"""

from __future__ import annotations

import contextlib
import functools
import math
from dataclasses import dataclass
from typing import Callable, Optional
from unittest import mock

import torch
from torch.overrides import TorchFunctionMode

from sparse_coding_amd.models import sae_signatures as sigs
from sparse_coding_amd.models.batch_topk import BatchTopKEncoder
from sparse_coding_amd.models.lista import (
    FunctionalLISTADenoisingSAE,
    FunctionalResidualDenoisingSAE,
    LISTALayer,
    shrinkage,
)
from sparse_coding_amd.models.positive import FunctionalPositiveTiedSAE
from sparse_coding_amd.models.semilinear import FFLayer, SemiLinearSAE
from sparse_coding_amd.models.topk import TopKEncoder

U = 2.0 ** -24
NEAR = 2.0 ** -18
L1_ALPHAS = (1e-3, 3e-3)
BIAS_DECAY = 0.01


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32).item())


# the Adam defaults as the fp32 values the kernels receive
BETA1, BETA2 = f32(0.9), f32(0.999)


class Mismatch(AssertionError):
    pass


# ---------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------

def tree_items(tree, prefix=""):
    """[(path, leaf)] of a dict/list tree of tensors, in a fixed order."""
    if torch.is_tensor(tree):
        return [(prefix, tree)]
    if isinstance(tree, dict):
        items = [(k, tree[k]) for k in sorted(tree)]
    else:
        items = list(enumerate(tree))
    out = []
    for k, v in items:
        out += tree_items(v, f"{prefix}.{k}" if prefix else str(k))
    return out


def tree_apply(fn, tree):
    if torch.is_tensor(tree):
        return fn(tree)
    if isinstance(tree, dict):
        return {k: tree_apply(fn, v) for k, v in tree.items()}
    return [tree_apply(fn, v) for v in tree]


def tree_stack(trees):
    first = trees[0]
    if torch.is_tensor(first):
        return torch.stack(trees)
    if isinstance(first, dict):
        return {k: tree_stack([t[k] for t in trees]) for k in first}
    return [tree_stack([t[i] for t in trees]) for i in range(len(first))]


def _cast(tree, dtype):
    return tree_apply(lambda t: t.detach().to("cpu", dtype) if t.is_floating_point() else t.detach().cpu(), tree)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    sig: type
    step_class: str                 # the class maybe_make_step has to choose
    make: Callable                  # (gen, B, d, n) -> [(params, buffers)] * 2, fp32 on the CPU
    flags: tuple = ()               # attributes of the step that must be true
    captures_graph: bool = True
    bias_decay: bool = False        # the loss applies buffers["bias_decay"]
    l1_colsum: bool = False         # the step sums the L1 through k_colsum
    dict_sizes: Optional[Callable] = None  # n -> per-model dict sizes (masked)
    x_scale: float = 1.0


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _dict_sizes(n):
    """Two different sizes, neither a multiple of 4, both below the stack width."""
    return (n // 2 + 3, n - 5)


def _sae(sig, **kw):
    def make(gen, B, d, n):
        models = []
        for l1 in L1_ALPHAS:
            p, b = sig.init(d, n, l1, **kw)
            p["encoder_bias"] = 0.1 * _randn(gen, n)
            models.append((p, b))
        return models
    return make


def _masked(sig):
    def make(gen, B, d, n):
        models = []
        for l1, nd in zip(L1_ALPHAS, _dict_sizes(n)):
            p, b = sig.init(d, nd, n, l1, bias_decay=BIAS_DECAY)
            p["encoder_bias"] = 0.1 * _randn(gen, n)
            models.append((p, b))
        return models
    return make


def _reverse(gen, B, d, n):
    models = _sae(sigs.FunctionalReverseSAE, bias_decay=BIAS_DECAY)(gen, B, d, n)
    for p, _ in models:
        p["encoder_bias"] = 0.2 * _randn(gen, n)
    return models


def _centered(gen, B, d, n):
    models = _sae(sigs.FunctionalTiedCenteredSAE)(gen, B, d, n)
    for p, _ in models:
        p["center"] = 0.3 * _randn(gen, d)
    return models


def _whitened(gen, B, d, n):
    # FunctionalTiedSAE with non-identity affine centering buffers, built as
    # test_whitened_tied_step_matches_oracle builds it
    models = []
    for l1 in L1_ALPHAS:
        q, _ = torch.linalg.qr(_randn(gen, d, d))
        p, b = sigs.FunctionalTiedSAE.init(
            d, n, l1, bias_decay=BIAS_DECAY, rotation=q.contiguous(),
            translation=0.3 * _randn(gen, d), scaling=torch.rand(d, generator=gen) + 0.5)
        p["encoder_bias"] = 0.1 * _randn(gen, n)
        models.append((p, b))
    return models


def _positive(gen, B, d, n):
    models = []
    for l1 in L1_ALPHAS:
        p, b = FunctionalPositiveTiedSAE.init(d, n, l1, bias_decay=BIAS_DECAY)
        # init is |xavier|: shift it so that a fair share of the weights is
        # negative and the clamp mask matters
        p["encoder"] = p["encoder"] - 0.4 * p["encoder"].max()
        p["encoder_bias"] = p["encoder_bias"] + 0.1 * _randn(gen, n)
        models.append((p, b))
    return models


def _thresholding(gen, B, d, n):
    # u = (x.What + gain) / scale^2 with x.What ~ N(0, 1): gain and scale
    # spread it so that it lands below 0.9 (most), between the knees (about
    # 1%) and above 1.0 (about 8%).  The relu6 argument is 60 (u - 0.9), so
    # a wider spread of u puts more of it within 2^-18 max|arg| of a knee.
    models = []
    for l1 in L1_ALPHAS:
        p, b = sigs.FunctionalThresholdingSAE.init(d, n, l1)
        p["activation_gain"] = -0.5 + 0.3 * _randn(gen, n)
        p["activation_scale"] = 1.0 + 0.1 * _randn(gen, n)
        models.append((p, b))
    return models


# per layer; model 0 inside (0, 1), model 1 has two layers outside [0, 1] so
# that the gate matters.  HipLISTAStep gates g_rho with the strict
# 0 < rho < 1 while torch.clamp's backward passes the gradient at rho == 0 and
# rho == 1: a known divergence, so rho stays off the exact boundary here.
LISTA_RHO = ((0.1, 0.3, 0.6), (-0.2, 1.3, 0.4))


def _lista(gen, B, d, n):
    models = []
    for l1, rhos in zip(L1_ALPHAS, LISTA_RHO):
        p, b = FunctionalLISTADenoisingSAE.init(d, n, len(rhos), l1)
        for layer, rho in zip(p["encoder_layers"], rhos):
            layer["theta"] = 0.1 * _randn(gen, n)  # both signs
            layer["rho"] = torch.tensor(rho)
        models.append((p, b))
    return models


def _residual(gen, B, d, n):
    models = []
    for l1 in L1_ALPHAS:
        p, b = FunctionalResidualDenoisingSAE.init(d, n, 2, l1)
        for layer in p["encoder_layers"]:
            layer["theta"] = 0.1 * _randn(gen, n)
        p["encoder_bias"] = 0.1 * _randn(gen, n)
        models.append((p, b))
    return models


def semilinear_hidden(d, n):
    """A hidden width that differs from d and n.  On the ragged shape it is a
    multiple of 4 (the launchers need that) but not of 16; on the tile-aligned
    shape it has to be a multiple of the tile for the launches to stay
    guard-free."""
    return 256 if n % 128 == 0 and d % 32 == 0 else 76


def _semilinear(gen, B, d, n):
    models = []
    for l1 in L1_ALPHAS:
        p, b = SemiLinearSAE.init(d, n, l1, hidden_size=semilinear_hidden(d, n))
        for layer in p["encoder_layers"]:
            layer["bias"] = 0.1 * _randn(gen, layer["bias"].shape[0])
        models.append((p, b))
    return models


def _topk(sig, ks):
    def make(gen, B, d, n):
        return [sig.init(d, n, k) for k in ks]
    return make


def cases():
    S = sigs
    return [
        Case("tied", S.FunctionalTiedSAE, "HipSAEStep", _sae(S.FunctionalTiedSAE, bias_decay=BIAS_DECAY),
             flags=("tied",), bias_decay=True),
        Case("untied", S.FunctionalSAE, "HipSAEStep", _sae(S.FunctionalSAE, bias_decay=BIAS_DECAY),
             bias_decay=True),
        Case("masked_tied", S.FunctionalMaskedTiedSAE, "HipSAEStep", _masked(S.FunctionalMaskedTiedSAE),
             flags=("tied", "masked"), dict_sizes=_dict_sizes),
        Case("masked_untied", S.FunctionalMaskedSAE, "HipSAEStep", _masked(S.FunctionalMaskedSAE),
             flags=("masked",), dict_sizes=_dict_sizes),
        Case("reverse", S.FunctionalReverseSAE, "HipSAEStep", _reverse, flags=("tied", "reverse"),
             bias_decay=True),
        Case("centered", S.FunctionalTiedCenteredSAE, "HipCenteredStep", _centered),
        Case("whitened", S.FunctionalTiedSAE, "HipWhitenedStep", _whitened, bias_decay=True),
        Case("positive", FunctionalPositiveTiedSAE, "HipPositiveStep", _positive, bias_decay=True),
        Case("thresholding", S.FunctionalThresholdingSAE, "HipThresholdStep", _thresholding),
        Case("lista", FunctionalLISTADenoisingSAE, "HipLISTAStep", _lista, l1_colsum=True),
        Case("residual", FunctionalResidualDenoisingSAE, "HipResidualDenoisingStep", _residual,
             captures_graph=False, l1_colsum=True),
        Case("semilinear", SemiLinearSAE, "HipSemilinearStep", _semilinear,
             captures_graph=False, l1_colsum=True),
        Case("topk", TopKEncoder, "HipTopKStep", _topk(TopKEncoder, (4, 16))),
        Case("batch_topk", BatchTopKEncoder, "HipBatchTopKStep", _topk(BatchTopKEncoder, (3, 9))),
    ]


def case(name) -> Case:
    return {c.name: c for c in cases()}[name]


# (M, B, d, n).  ALIGNED takes the guard-free kernels.  RAGGED has two row
# tiles, column tails at both widths and K tails at both depths in every GEMM
# of a shallow chain.  The deep chains flip masks too easily there (LISTA has
# 4-8 near-knee arguments per seed), so they get RAGGED_DEEP: a row tail, two
# column tiles, a K tail of 4 at depth 16, K = 20 < 32, K = 132 for dec_fwd and
# K = 36 for grad_w.  PRE runs the pre-transposed pipeline.
ALIGNED = (2, 128, 64, 128)
RAGGED = (2, 130, 68, 260)
RAGGED_DEEP = (2, 36, 20, 132)
PRE = (2, 132, 68, 132)
DEEP = ("lista", "residual", "semilinear")


def _grid():
    g = []
    for c in cases():
        g.append((c.name, ALIGNED, None))
        g.append((c.name, RAGGED_DEEP if c.name in DEEP else RAGGED, None))
    for name in ("tied", "untied", "masked_tied"):
        g.append((name, PRE, "pre"))
    return g


GRID = _grid()


def grid_id(entry):
    name, shape, staging = entry
    return f"{name}-{'x'.join(map(str, shape[1:]))}" + (f"-{staging}" if staging else "")


# The first seed of 0, 1, 2, ... at which decisions() reports no near-knee
# argument, per (case, shape); found on the CPU from the float64 reference
# alone (test_step_reference_cpu.test_seeds_are_the_first_clean_ones).
SEEDS: dict = {
    ('tied', (2, 128, 64, 128)): 0,
    ('tied', (2, 130, 68, 260)): 3,
    ('untied', (2, 128, 64, 128)): 1,
    ('untied', (2, 130, 68, 260)): 0,
    ('masked_tied', (2, 128, 64, 128)): 0,
    ('masked_tied', (2, 130, 68, 260)): 3,
    ('masked_untied', (2, 128, 64, 128)): 1,
    ('masked_untied', (2, 130, 68, 260)): 0,
    ('reverse', (2, 128, 64, 128)): 1,
    ('reverse', (2, 130, 68, 260)): 15,
    ('centered', (2, 128, 64, 128)): 0,
    ('centered', (2, 130, 68, 260)): 0,
    ('whitened', (2, 128, 64, 128)): 0,
    ('whitened', (2, 130, 68, 260)): 3,
    ('positive', (2, 128, 64, 128)): 0,
    ('positive', (2, 130, 68, 260)): 2,
    ('thresholding', (2, 128, 64, 128)): 0,
    ('thresholding', (2, 130, 68, 260)): 5,
    ('lista', (2, 128, 64, 128)): 19,
    ('lista', (2, 36, 20, 132)): 7,
    ('residual', (2, 128, 64, 128)): 6,
    ('residual', (2, 36, 20, 132)): 0,
    ('semilinear', (2, 128, 64, 128)): 0,
    ('semilinear', (2, 36, 20, 132)): 0,
    ('topk', (2, 128, 64, 128)): 0,
    ('topk', (2, 130, 68, 260)): 0,
    ('batch_topk', (2, 128, 64, 128)): 1,
    ('batch_topk', (2, 130, 68, 260)): 0,
    ('tied', (2, 132, 68, 132)): 1,
    ('untied', (2, 132, 68, 132)): 0,
    ('masked_tied', (2, 132, 68, 132)): 1,
}


def seed_of(name, shape):
    return SEEDS.get((name, tuple(shape)), 0)


def build(name, shape, seed=None):
    """(models, x): two fp32 CPU (params, buffers) models and the batch."""
    c = case(name)
    M, B, d, n = shape
    assert M == 2
    seed = seed_of(name, shape) if seed is None else seed
    gen = torch.Generator().manual_seed(1000 + seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(2000 + seed)  # the signatures' init draws from the global generator
        models = c.make(gen, B, d, n)
    x = c.x_scale * _randn(gen, B, d)
    return models, x


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------

def _grads(loss_fn, models, x, dtype):
    gs, ls, cs = [], [], []
    for p, b in models:
        p, b = _cast(p, dtype), _cast(b, dtype)
        with torch.enable_grad():
            g, (loss_data, aux) = torch.func.grad(loss_fn, has_aux=True)(p, b, x.to(dtype))
        gs.append(tree_apply(lambda t: t.detach(), g))
        ls.append({k: v.detach() for k, v in loss_data.items()})
        cs.append(aux["c"].detach())
    return tree_stack(gs), tree_stack(ls), torch.stack(cs)


@functools.lru_cache(maxsize=None)
def reference(name, shape, seed=None):
    """Per model on the CPU: float64 gradient tree, loss dict and codes (g64,
    loss64, c64) and the float32 yardstick (g32, loss32, c32); leaves stacked
    [M, ...].  Computed once per (case, shape) and shared: do not modify."""
    c = case(name)
    models, x = build(name, shape, seed)
    g64, l64, c64 = _grads(c.sig.loss, models, x, torch.float64)
    g32, l32, c32 = _grads(c.sig.loss, models, x, torch.float32)
    return {"g64": g64, "loss64": l64, "c64": c64, "g32": g32, "loss32": l32, "c32": c32}


# ---------------------------------------------------------------------------
# nonsmooth decisions
# ---------------------------------------------------------------------------

# Every torch function a signature's forward may call is either a decision
# handled below or listed here as smooth (or as a selection by a mask that a
# handled comparison produced).  Anything else raises: a new comparison op must
# not pass unrecorded.
SMOOTH = frozenset({
    "__get__", "__getitem__", "matmul", "__matmul__", "__rmatmul__", "linear", "add", "__add__", "__radd__",
    "sub", "__sub__", "__rsub__", "mul", "__mul__", "__rmul__", "div", "__truediv__", "__rtruediv__",
    "true_divide", "pow", "__pow__", "mean", "sum", "mse_loss", "where", "masked_fill", "zeros_like",
    "scatter_", "gather", "detach", "flatten", "new_tensor", "__and__", "numel", "dim", "size",
    "__int__", "__index__", "item", "__len__", "to", "reshape", "unsqueeze", "transpose", "__neg__", "neg",
    "__bool__", "__format__", "__repr__",
})
COMPARISONS = frozenset({"gt", "ge", "lt", "le", "__gt__", "__ge__", "__lt__", "__le__"})


def _near(arg, knee):
    """(count of 0 < |arg - knee| < 2^-18 max|arg|, smallest such nonzero
    distance over max|arg|).  Arguments exactly on a knee are not near: fp32
    reproduces them (zeros out of a ReLU feeding sign, clamped weights)."""
    a = arg.detach().double()
    if a.numel() == 0:
        return 0, math.inf
    top = a.abs().max().item()
    dist = (a - (knee.detach().double() if torch.is_tensor(knee) else float(knee))).abs()
    pos = dist[dist > 0]
    if pos.numel() == 0 or top == 0.0:
        return 0, math.inf
    return int((pos < NEAR * top).sum()), pos.min().item() / top


class DecisionRecorder(TorchFunctionMode):
    """Notes the argument of every ReLU-like decision against its knee(s)."""

    def __init__(self):
        super().__init__()
        self.records = []

    def note(self, op, arg, knee):
        near, margin = _near(arg, knee)
        self.records.append({"op": op, "knee": knee if not torch.is_tensor(knee) else "tensor",
                             "near": near, "margin": margin, "numel": arg.numel()})

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", str(func))
        if name == "relu":
            self.note(name, args[0], 0.0)
        elif name == "relu6":
            self.note(name, args[0], 0.0)
            self.note(name, args[0], 6.0)
        elif name in ("clamp", "clip", "clamp_min", "clamp_max"):
            bounds = list(args[1:]) + [kwargs.get("min"), kwargs.get("max")]
            bounds = [b for b in bounds if b is not None]
            if not bounds:
                raise RuntimeError(f"DecisionRecorder: {name} without a bound")
            for b in bounds:
                self.note(name, args[0], b)
        elif name in ("sign", "abs"):
            self.note(name, args[0], 0.0)
        elif name == "norm":
            p = args[1] if len(args) > 1 else kwargs.get("p", 2)
            if p == 1:  # sum |.|: abs decides at 0
                self.note("norm1", args[0], 0.0)
            elif p not in (2, None, "fro"):
                raise RuntimeError(f"DecisionRecorder: norm with p={p!r} is not known")
        elif name in COMPARISONS:
            a, b = args[0], args[1]
            if not torch.is_tensor(a):
                a, b = b, a
            self.note(name, a, b)
        elif name == "topk":
            scores = args[0].detach().double()
            k = int(args[1] if len(args) > 1 else kwargs["k"])
            dim = args[2] if len(args) > 2 else kwargs.get("dim", -1)
            s = torch.sort(scores, dim=dim, descending=True).values
            top = scores.abs().max().item()
            if k > 0:
                kept = s.narrow(dim, k - 1, 1)
                gaps = [kept.abs()]  # the last kept score against 0 (the relu after the scatter)
                if k < s.shape[dim]:
                    gaps.append(kept - s.narrow(dim, k, 1))  # against the first dropped score
                for what, gap in zip(("topk-zero", "topk-gap"), gaps):
                    pos = gap[gap > 0]
                    self.records.append({
                        "op": what, "knee": k, "numel": gap.numel(),
                        "near": int((pos < NEAR * top).sum()) if top > 0 else 0,
                        "margin": (pos.min().item() / top) if pos.numel() and top > 0 else math.inf})
        elif name not in SMOOTH:
            raise RuntimeError(
                f"DecisionRecorder: the forward calls {name!r}, which is neither a known decision nor listed "
                "as smooth; add it to one of the two")
        return func(*args, **kwargs)


def record(fn):
    """Run fn() under the recorder; returns its records."""
    rec = DecisionRecorder()
    with torch.no_grad(), rec:
        fn()
    return rec.records


@functools.lru_cache(maxsize=None)
def decisions(name, shape, seed=None):
    """{"near": total count of near-knee arguments of the float64 forward over
    both models, "margin": the smallest nonzero relative distance from a knee,
    "records": one entry per decision op and model}."""
    c = case(name)
    models, x = build(name, shape, seed)
    records, x64 = [], x.double()
    for m, (p, b) in enumerate(models):
        p, b = _cast(p, torch.float64), _cast(b, torch.float64)
        for r in record(functools.partial(c.sig.loss, p, b, x64)):
            records.append(dict(r, model=m))
    if not records:
        raise RuntimeError(f"{name}: the recorder saw no decision at all")
    return {"near": sum(r["near"] for r in records), "margin": min(r["margin"] for r in records),
            "records": records}


def first_clean_seed(name, shape, limit=64):
    for seed in range(limit):
        if decisions(name, tuple(shape), seed)["near"] == 0:
            return seed
    raise RuntimeError(f"{name} {shape}: no clean seed below {limit}")


# ---------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------

def _d(t):
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def leaf_bound(g64, g32):
    """e = 8 e32 + 16 U scale in the max norm.  The step and the yardstick are
    both fp32 evaluations of the same sums in different orders: a factor 8
    covers one order-dependent draw against another; the floor covers leaves
    where the yardstick happens to be exact and the roundings in mu = 0.1f g."""
    g64, g32 = _d(g64), _d(g32)
    e32 = (g32 - g64).abs().max().item() if g64.numel() else 0.0
    scale = g64.abs().max().item() if g64.numel() else 0.0
    return 8.0 * e32 + 16.0 * U * scale


def _fail(failures):
    if failures:
        raise Mismatch("; ".join(failures))


def compare(got_tree, ref, yardstick, what="grad", t=1, masked=None):
    """Per leaf and per model, in the max norm: max|got - g64| <= 8 e32 + 16 U
    max|g64| (NaN never passes).  Returns {leaf: worst err/bound over the
    models}; raises Mismatch naming every leaf and model outside its bound.

    got_tree is a tree of [M, ...] leaves with the tree of ref (float64) and
    yardstick (float32):
      what="grad": the gradient itself (also used for the codes);
      what="mu":   Adam's first moment after t steps at lr = 0 from zero state,
                   compared as mu / (1 - b1^t);
      what="nu":   the second moment, nu / (1 - b2^t) against g64^2 under the
                   propagated bound 2 |g64| e + e^2.
    masked = (n, dict_sizes) for the masked signatures: rows from
    dict_sizes[m] on of every leaf with n rows must be exactly zero."""
    got, ref, yard = tree_items(got_tree), tree_items(ref), tree_items(yardstick)
    if [p for p, _ in got] != [p for p, _ in ref]:
        raise Mismatch(f"trees differ: {[p for p, _ in got]} vs {[p for p, _ in ref]}")
    ratios, failures = {}, []
    for (path, g), (_, r64), (_, r32) in zip(got, ref, yard):
        g = _d(g)
        if what == "mu":
            g = g / (1.0 - BETA1 ** t)
        elif what == "nu":
            g = g / (1.0 - BETA2 ** t)
        r64 = _d(r64)
        if g.shape != r64.shape:
            raise Mismatch(f"{path}: shape {tuple(g.shape)} vs reference {tuple(r64.shape)}")
        worst = 0.0
        for m in range(r64.shape[0]):
            e = leaf_bound(r64[m], r32[m])
            if what == "nu":
                target = r64[m] * r64[m]
                bound = 2.0 * r64[m].abs() * e + e * e
            else:
                target, bound = r64[m], torch.full_like(r64[m], e)
            err = (g[m] - target).abs()
            bad = ~(err <= bound)
            if bad.any():
                i = int(torch.argmax(torch.where(err.isnan(), torch.full_like(err, math.inf), err - bound)))
                failures.append(
                    f"{what} {path}[model {m}]: {int(bad.sum())} of {bad.numel()} outside the bound, worst "
                    f"err {err.reshape(-1)[i].item():.3e} > {bound.reshape(-1)[i].item():.3e} "
                    f"(e32 {(_d(r32[m]) - r64[m]).abs().max().item():.3e}, scale {r64[m].abs().max().item():.3e})")
            ok = bound > 0
            if ok.any():
                ratio = (err[ok] / bound[ok]).max().item()
                worst = max(worst, ratio if ratio == ratio else math.inf)
            if masked is not None and g[m].dim() and g[m].shape[0] == masked[0]:
                tail = g[m][int(masked[1][m]):]
                if not (tail == 0).all():
                    failures.append(f"{what} {path}[model {m}]: {int((tail != 0).sum())} masked entries "
                                    "are not exactly zero")
        ratios[path] = worst
    _fail(failures)
    return ratios


def compare_codes(got, ref, dict_sizes=None):
    """The codes under the same rule as a gradient leaf; masked columns == 0."""
    tree = lambda t: {"c": t}  # noqa: E731
    failures = []
    try:
        ratios = compare(tree(got), tree(ref["c64"]), tree(ref["c32"]), what="grad")
    except Mismatch as e:
        raise Mismatch(str(e).replace("grad c", "codes c"))
    if dict_sizes is not None:
        g = _d(got)
        for m, nd in enumerate(dict_sizes):
            if not (g[m][:, int(nd):] == 0).all():
                failures.append(f"codes c[model {m}]: masked columns are not exactly zero")
    _fail(failures)
    return ratios


def cdiv(a, b):
    return (a + b - 1) // b


def epi_sum_depth(B, ncols, bn):
    """hip_reference.epi_sum_depth: additions on the path of one term of a
    GEMM-epilogue scalar sum."""
    return 16 * (bn // 64) + 6 + 8 * cdiv(B, 128) * cdiv(ncols, bn) + 1


def loss_depths(c: Case, B, d, n):
    """D per loss key: the additions (roundings) on the path of one term.

    l_reconstruction: the dec_fwd epilogue sum, epi_sum_depth(B, d, bn), at the
      wider of the two tile widths the kernels are compiled in.
    l_l1: the enc_fwd epilogue sum, epi_sum_depth(B, n, bn); or, where the step
      sums the codes through k_colsum, test_colsum's depth (a slice's rows in
      one thread, one atomic per slice, the alpha product) plus the n - 1
      additions of the row sum that follows, in whatever order.
    l_bias_decay: ||b||_2: n U on the sum of squares in any order, halved by
      the root, the root, the product: n/2 + 2.
    + 8 each for the scalings and final adds; "loss" sums nonnegative parts, so
    the largest depth of a part covers it."""
    def epi(ncols):
        return max(epi_sum_depth(B, ncols, bn) for bn in (128, 256))

    depths = {"l_reconstruction": epi(d) + 8}
    if c.l1_colsum:
        nsplit = min(max(B // 256, 1), 16)
        depths["l_l1"] = cdiv(B, nsplit) + nsplit + 2 + (n - 1) + 8
    else:
        depths["l_l1"] = epi(n) + 8
    depths["l_bias_decay"] = n // 2 + 2 + 8
    depths["loss"] = max(depths.values())
    return depths


def compare_losses(got, ref, depths):
    """Every key the step returns that the signature also returns (BatchTopK's
    "threshold" is not a loss): |L - L64| <= 8 |L32 - L64| + D U L64 per model.
    All the losses are sums of nonnegative terms.  "loss" must be there."""
    if "loss" not in got:
        raise Mismatch(f"the step returned no 'loss': {sorted(got)}")
    ratios, failures = {}, []
    for k in got:
        if k == "threshold" or k not in ref["loss64"]:
            continue
        g, l64, l32 = _d(got[k]), _d(ref["loss64"][k]), _d(ref["loss32"][k])
        if g.shape != l64.shape:
            raise Mismatch(f"loss {k}: shape {tuple(g.shape)} vs {tuple(l64.shape)}")
        assert (l64 >= 0).all()
        bound = 8.0 * (l32 - l64).abs() + depths[k] * U * l64
        err = (g - l64).abs()
        if (~(err <= bound)).any():
            failures.append(f"loss {k}: got {g.tolist()} ref {l64.tolist()} err {err.tolist()} "
                            f"bound {bound.tolist()}")
        ok = bound > 0
        ratios[k] = (err[ok] / bound[ok]).max().item() if ok.any() else 0.0
    _fail(failures)
    return ratios


def tree_zip(fn, *trees):
    first = trees[0]
    if torch.is_tensor(first):
        return fn(*trees)
    if isinstance(first, dict):
        return {k: tree_zip(fn, *[t[k] for t in trees]) for k in first}
    return [tree_zip(fn, *[t[i] for t in trees]) for i in range(len(first))]


def moments(g_tree, t=1, dtype=torch.float32):
    """(mu, nu) Adam holds after t steps at lr = 0 from zero state on the
    gradient g, run as the recurrence in `dtype`."""
    g_tree = tree_apply(lambda g: g.to(dtype), g_tree)
    mu = tree_apply(torch.zeros_like, g_tree)
    nu = tree_apply(torch.zeros_like, g_tree)
    b1, b2 = torch.tensor(BETA1, dtype=dtype), torch.tensor(BETA2, dtype=dtype)
    for _ in range(t):
        mu = tree_zip(lambda m, g: b1 * m + (1 - b1) * g, mu, g_tree)
        nu = tree_zip(lambda v, g: b2 * v + (1 - b2) * g * g, nu, g_tree)
    return mu, nu


# ---------------------------------------------------------------------------
# doctored problems
# ---------------------------------------------------------------------------

class _DetachRowNorms(TorchFunctionMode):
    """Row norms become constants: the gradient with respect to the normalised
    dictionary is handed on unprojected."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        if getattr(func, "__name__", "") == "norm" and kwargs.get("dim") == -1:
            p = args[1] if len(args) > 1 else kwargs.get("p", 2)
            if p != 1:
                return out.detach()
        return out


def _straight_through(value, onto):
    return onto + (value - onto).detach()


def _lista_forward(ungated=False, no_carry=False):
    def forward(params, y, b, x, A):
        rho = params["rho"]
        m = torch.clamp(rho, min=0.0, max=1.0)
        if ungated:
            m = _straight_through(m, rho)
        r = y + (b - y @ A) @ params["W"].T
        x_ = shrinkage(r, params["theta"])
        y_ = x_ + m * (x_ - (x.detach() if no_carry else x))
        return y_, x_
    return staticmethod(forward)


def _ff_forward_no_hidden_mask():
    calls = [0]

    def forward(params, x):
        pre = x @ params["weight"].T + params["bias"]
        out = torch.clamp(pre, min=0.0)
        calls[0] += 1
        return _straight_through(out, pre) if calls[0] % 2 == 1 else out  # the hidden layer comes first
    return staticmethod(forward)


def _replace_buffer(key, value):
    def wrap(loss):
        return lambda p, b, x: loss(p, dict(b, **{key: torch.full_like(b[key], value)}), x)
    return wrap


def _drop_last_row(loss):
    return lambda p, b, x: loss(p, b, x[:-1])


def _mse_padded(loss):
    def doctored(p, b, x):
        total, (ld, aux) = loss(p, b, x)
        B = x.shape[0]
        rec = ld.get("l_reconstruction", ld["loss"])  # the TopK losses are the MSE alone
        return total - rec * (1.0 - B / (128 * cdiv(B + 1, 128))), (ld, aux)
    return doctored


# name -> (applies(case), loss wrapper or None, context factory or None)
DOCTORINGS = {
    # the K-tail term of grad_w dropped
    "drop_last_row": (lambda c: True, _drop_last_row, None),
    # gscale = 2 / (B d) from a batch padded to the next multiple of 128
    "mse_padded_batch": (lambda c: True, _mse_padded, None),
    "l1_alpha_zero": (lambda c: "topk" not in c.name, _replace_buffer("l1_alpha", 0.0), None),
    "bias_decay_zero": (lambda c: c.bias_decay, _replace_buffer("bias_decay", 0.0), None),
    "unprojected": (lambda c: True, None, _DetachRowNorms),
    "rho_ungated": (lambda c: c.name == "lista", None,
                    lambda: mock.patch.object(LISTALayer, "forward", _lista_forward(ungated=True))),
    # m = 0 in the backward only: no carry onto the previous layer's x
    "lista_no_carry": (lambda c: c.name == "lista", None,
                       lambda: mock.patch.object(LISTALayer, "forward", _lista_forward(no_carry=True))),
    "semilinear_no_hidden_mask": (lambda c: c.name == "semilinear", None,
                                  lambda: mock.patch.object(FFLayer, "forward", _ff_forward_no_hidden_mask())),
}


def doctored(doctoring, name, shape):
    """The fp32 autograd gradient tree of a doctored problem, or None where the
    doctoring does not apply to the case."""
    applies, wrap, context = DOCTORINGS[doctoring]
    c = case(name)
    if not applies(c):
        return None
    models, x = build(name, shape)
    loss = wrap(c.sig.loss) if wrap is not None else c.sig.loss
    with (context() if context is not None else contextlib.nullcontext()):
        g32, _, _ = _grads(loss, models, x, torch.float32)
    return g32

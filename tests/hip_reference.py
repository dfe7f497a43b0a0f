"""fp64 references and derived componentwise error bounds for the HIP kernels.

Plain helpers (no fixtures, no hooks) shared by test_hip_reference_cpu.py,
which validates the comparators and the hand-written references on the CPU,
and test_hip_kernels_fp64.py, which runs every launcher of ops/hip/sae_ops.hip
against them on the GPU.

Conventions
-----------
* Every reference is computed on the CPU in float64 from the kernel's fp32
  inputs.  Gradients come from fp64 autograd through the project's signature
  code (``*_autograd``); the hand-written formulas next to them exist only to
  derive the bounds and are tied to the autograd result to 1e-12 by the CPU
  tests.
* ``U = 2^-24`` is the fp32 unit roundoff.  A bound is ``c * U * (|A| |B|)``
  per element, with ``c`` the number of fp32 roundings on the path; each
  function states its count.  Nothing here is tuned to a run.
* An element whose *decision variable* (the argument of a mask) lies within its
  own bound of the knee is *undecided*: the kernel may legitimately take either
  side.  It is skipped for the outputs that depend on the mask, and every check
  asserts that at most ``MAX_UNDECIDED`` of the elements are undecided.
"""

from __future__ import annotations

import contextlib
import math

import torch

from sparse_coding_amd.functional.optim import adam
from sparse_coding_amd.models.learned_dict import normalize_rows
from sparse_coding_amd.models.lista import LISTALayer
from sparse_coding_amd.models.sae_signatures import (
    FunctionalReverseSAE,
    FunctionalThresholdingSAE,
)

U = 2.0 ** -24
GATE_EPS = 1e-8
EPS_NORM = 1e-8
MAX_UNDECIDED = 0.005


# the dtype the references are computed in; only `stand_in_precision` changes it
_DTYPE = [torch.float64]


def d64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", _DTYPE[0])


@contextlib.contextmanager
def stand_in_precision(dtype=torch.float32):
    """Run the reference code in fp32 instead: a CPU stand-in for a kernel that
    the bounds, taken from the fp64 run, have to accept."""
    _DTYPE[0] = dtype
    try:
        yield
    finally:
        _DTYPE[0] = torch.float64


def _f64(t) -> torch.Tensor:
    """For the comparators: always float64, whatever the reference dtype."""
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ---------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------

class Mismatch(AssertionError):
    pass


def check(name, got, ref, bound, undecided=None, max_undecided=MAX_UNDECIDED):
    """|got - ref| <= bound on every decided element (NaN never passes).

    Returns {"worst": max err/bound, "undecided": share} for reporting."""
    got, ref = _f64(got), _f64(ref)
    if got.shape != ref.shape:
        raise Mismatch(f"{name}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}")
    bound = torch.broadcast_to(_f64(bound), ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    share = 0.0
    if undecided is not None:
        undecided = torch.broadcast_to(undecided.cpu(), ref.shape)
        share = undecided.double().mean().item()
        if share > max_undecided:
            raise Mismatch(f"{name}: {share:.2e} of the elements are undecided (> {max_undecided})")
        bad &= ~undecided
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise Mismatch(
            f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {idx}: "
            f"got {got[idx].item():.9e} ref {ref[idx].item():.9e} "
            f"err {err[idx].item():.3e} bound {bound[idx].item():.3e}")
    ok = bound > 0
    if undecided is not None:
        ok &= ~undecided
    worst = (err[ok] / bound[ok]).max().item() if ok.any() else 0.0
    return {"worst": worst, "undecided": share}


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check_bits(name, got, ref):
    """Bitwise equality (fp32 compared through its int32 view: -0.0 != +0.0)."""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        raise Mismatch(f"{name}: {tuple(got.shape)}/{got.dtype} vs {tuple(ref.shape)}/{ref.dtype}")
    diff = _bits(got) != _bits(ref)
    if diff.any():
        idx = tuple(int(i) for i in diff.nonzero()[0])
        raise Mismatch(f"{name}: {int(diff.sum())} of {diff.numel()} elements differ bitwise; first at {idx}: "
                       f"got {got.detach().cpu()[idx].item()!r} ref {ref.detach().cpu()[idx].item()!r}")


def check_counts(name, got, lo, hi):
    """lo <= got <= hi elementwise, got integral: a count that is exact on the
    decided elements and may include any subset of the undecided ones."""
    got, lo, hi = _f64(got), _f64(lo), _f64(hi)
    bad = ~((got >= lo) & (got <= hi) & (got == got.round()))
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise Mismatch(f"{name}: {int(bad.sum())} counts wrong; first at {idx}: "
                       f"got {got[idx].item()} expected [{lo[idx].item()}, {hi[idx].item()}]")


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def row_scales(B: int, gen: torch.Generator, n_tail: int = 4) -> torch.Tensor:
    """Power-of-two row scales 2^-10 .. 2^10; the last `n_tail` rows (the ones
    a partial tile holds) are among the small ones, rows 0/1 are pinned to the
    two extremes.  A max-norm error measure is blind to the small rows; the
    componentwise bound is not."""
    e = torch.randint(-10, 11, (B,), generator=gen).double()
    if B > 2:
        e[0], e[1] = 10.0, -10.0
    t = min(n_tail, B)
    e[B - t:] = torch.randint(-10, -7, (t,), generator=gen).double()
    return (2.0 ** e).float()


def scaled_randn(gen: torch.Generator, *shape) -> torch.Tensor:
    """randn whose rows (dim -2) carry row_scales."""
    x = torch.randn(*shape, generator=gen)
    return x * row_scales(shape[-2], gen)[:, None]


def gemm_inputs(M: int, B: int, d: int, n: int, seed: int) -> dict:
    """fp32 CPU inputs for the GEMM kernels: x shared [B, d] and xm per model
    [M, B, d] with row scales, a dictionary W with row norms spread over
    0.5..1.5 sqrt(d), a bias of the size of a small row's scores."""
    gen = torch.Generator().manual_seed(seed)
    return {
        "x": scaled_randn(gen, B, d),
        "xm": scaled_randn(gen, M, B, d),
        "W": torch.randn(M, n, d, generator=gen) * (0.5 + torch.rand(M, n, 1, generator=gen)),
        "bias": torch.randn(M, n, generator=gen) * 0.1,
        "gen": gen,
    }


# ---------------------------------------------------------------------------
# dot products
# ---------------------------------------------------------------------------

def dot(eq: str, a: torch.Tensor, b: torch.Tensor):
    """(a.b, |a|.|b|) in fp64."""
    a, b = d64(a), d64(b)
    return torch.einsum(eq, a, b), torch.einsum(eq, a.abs(), b.abs())


def c_dot(K: int) -> int:
    """Roundings of a K-term fp32 dot product: one for each product and one for
    each addition, 2K in all (the MFMA fp32 path is not assumed fused).  2K also
    covers the second-order terms of (1+U)^K - 1 for every K used here."""
    return 2 * K


def c_scale(d: int) -> float:
    """Roundings in a row's inverse-norm scale: a square passes through its own
    rounding and at most d-1 additions, so the sum of squares is off by at most
    d U relatively in any order; the square root halves that and adds one, the
    reciprocal and the multiply onto the operand add two, the fp32 value of the
    eps in the clamp one more: d/2 + 4."""
    return d / 2 + 4


def epi_sum_depth(B: int, ncols: int, bn: int = 128) -> int:
    """Additions any one term of a GEMM-epilogue scalar sum (L1, MSE) passes
    through: 16*(bn/64) in its thread, 6 wave shuffles, one atomic per wave of
    every block of the model (8 per block), plus the starting value.  This
    replaces N = B*ncols of the generic N*U*sum|terms| bound by the longest
    chain a term can really be on."""
    return 16 * (bn // 64) + 6 + 8 * cdiv(B, 128) * cdiv(ncols, bn) + 1


def col_sum_depth(B: int) -> int:
    """Additions on the path of a GEMM-epilogue column sum over the batch: 16 in
    the thread, 1 shuffle, then one add per 32-row group (k_colsum_groups; the
    atomic variants add one per 4 groups) and the starting value."""
    return 16 + 1 + cdiv(B, 32) + 1


def sum_check(name, got, start, terms, e_terms, depth, dims, slack=None, total=None):
    """got == start + sum(terms) within depth*U*(|start| + sum|terms|) + sum(e_terms)
    (+ slack, the largest change undecided elements can make).  `total` replaces
    sum(terms) as the reference value where autograd supplies it."""
    terms, e_terms = _f64(terms), _f64(e_terms)
    start = _f64(start)
    ref = start + (terms.sum(dim=dims) if total is None else _f64(total))
    bound = depth * U * (start.abs() + terms.abs().sum(dim=dims)) + e_terms.sum(dim=dims)
    if slack is not None:
        bound = bound + _f64(slack)
    return check(name, got, ref, bound)


# ---------------------------------------------------------------------------
# encoder epilogues
# ---------------------------------------------------------------------------

def enc_pre(x, W, scaled: bool):
    """pre = x @ What^T (What = normalize_rows(W) when `scaled`), |x|.|What| and
    the rounding count c_dot(d) (+ c_scale(d) when scaled)."""
    W64 = normalize_rows(d64(W), EPS_NORM) if scaled else d64(W)
    eq = "mbd,mnd->mbn" if x.dim() == 3 else "bd,mnd->mbn"
    pre, absdot = dot(eq, x, W64)
    d = W.shape[-1]
    return pre, absdot, c_dot(d) + (c_scale(d) if scaled else 0.0)


def enc_raw(x, W, scaled: bool):
    """mode 1: raw scores.  c = c_dot(d) (+ c_scale(d))."""
    pre, absdot, c = enc_pre(x, W, scaled)
    return {"c": pre, "e": c * U * absdot}


def enc_relu(x, W, bias, scaled: bool, dict_sizes=None):
    """mode 0: relu(pre + b), columns >= dict_sizes[m] exactly 0.
    c = c_dot(d) (+ c_scale(d)) + 1 for the bias add; relu is 1-Lipschitz, so
    the code needs no skipping; `undecided` (|pre + b| <= its bound) only
    matters for the fired counts."""
    pre, absdot, c = enc_pre(x, W, scaled)
    M, B, n = pre.shape
    b = d64(bias)[:, None, :]
    z = pre + b
    e = (c + 1) * U * (absdot + b.abs())
    live = torch.ones(M, 1, n, dtype=torch.bool)
    if dict_sizes is not None:
        live = torch.arange(n)[None, None, :] < torch.as_tensor(dict_sizes).reshape(M, 1, 1)
    live = live.expand(M, B, n)
    code = torch.where(live, torch.clamp(z, min=0.0), torch.zeros_like(z))
    e = torch.where(live, e, torch.zeros_like(e))
    und = live & (z.abs() <= e)
    return {"c": code, "e": e, "undecided": und, "on": (code > 0) & ~und, "live": live}


def fired_range(on, undecided, start):
    """[lo, hi] for a fired counter: exact on decided elements."""
    lo = _f64(start) + on.double().sum(dim=1)
    return lo, lo + undecided.double().sum(dim=1)


def enc_reverse(x, W, bias):
    """mode 3, the reverse SAE's code pre * [pre + b > 0], taken from
    FunctionalReverseSAE.loss in fp64.  The value carries c_dot(d)+c_scale(d)
    roundings, the decision variable one more (the bias add).  The mask is a
    jump, so undecided elements are skipped for the code as well."""
    pre, absdot, c = enc_pre(x, W, True)
    M = pre.shape[0]
    codes = []
    zero = torch.zeros((), dtype=_DTYPE[0])
    for m in range(M):
        params = {"encoder": d64(W[m]), "encoder_bias": d64(bias[m])}
        xm = d64(x[m] if x.dim() == 3 else x)
        _, (_, aux) = FunctionalReverseSAE.loss(params, {"l1_alpha": zero, "bias_decay": zero}, xm)
        codes.append(aux["c"])
    code = torch.stack(codes)
    b = d64(bias)[:, None, :]
    und = (pre + b).abs() <= (c + 1) * U * (absdot + b.abs())
    e = c * U * absdot
    return {"c": code, "e": e, "undecided": und, "on": (code != 0) & ~und,
            "flip": torch.where(und, pre.abs() + e, torch.zeros_like(e))}


def gate_g(u):
    return torch.clamp(60.0 * (u - 0.9), 0.0, 6.0) / 6.0 + torch.clamp(u - 1.0, min=0.0)


def enc_gate(x, W, scale, gain):
    """mode 2: u = (pre + gain) / max(a^2, eps), code = gate(pre, a, gain)
    (FunctionalThresholdingSAE.gate in fp64).

    e_u: c_dot(d)+c_scale(d) roundings on pre, then the add, a*a, the fp32
    eps, the reciprocal and the multiply: 5 more, on |pre| + |gain|.
    e_code: g is 11-Lipschitz in u, times a^2 (the constant 11 a^2 of the
    gate); evaluating g in fp32 costs at most 26 U (|u| + 1 + g): the constant
    0.9f is off by 0.45 U, the subtraction rounds once, the factor 60 and its
    rounding make 2*60 U (|u|+1) + 6 U, the division by 6 brings that to
    21 U (|u|+1) + 2 U, relu(u-1) and the final add round twice; then a*a and
    the product round once each: 2 U |code|.  g and the code are continuous:
    nothing is skipped; `undecided` (|u - 0.9| within e_u) is for fired."""
    pre, absdot, c = enc_pre(x, W, True)
    a = d64(scale)[:, None, :]
    gn = d64(gain)[:, None, :]
    a_sq = a * a
    s = torch.clamp(a_sq, min=GATE_EPS)
    u = (pre + gn) / s
    code = FunctionalThresholdingSAE.gate(pre, a, gn)
    e_u = (c * U * absdot + 5 * U * (pre.abs() + gn.abs())) / s
    g = gate_g(u)
    e_code = a_sq * (11.0 * e_u + 26 * U * (u.abs() + 1.0 + g)) + 2 * U * code.abs()
    und = (u - 0.9).abs() <= e_u + 2 * U
    return {"u": u, "e_u": e_u, "c": code, "e": e_code, "undecided": und,
            "on": (code > 0) & ~und}


def enc_lista(neg_e, W, y, x_prev, theta, mom):
    """mode 4, one LISTA layer: LISTALayer.forward in fp64 with A = 0 and
    b = -neg_e, so that r = y - neg_e @ W^T as the kernel has it.

    e_r = (c_dot(d) + 1) U (|neg_e|.|W| + |y|); the shrink is 1-Lipschitz and
    rounds once: e_x = e_r + U (|r| + |theta|); y' = x + m (x - x_prev) rounds
    three times: e_y = (1 + m) e_x + 3 U (m |x - x_prev| + |x|).  All three
    are continuous: nothing is skipped."""
    acc, absdot = dot("mbd,mnd->mbn", neg_e, W)
    M, n, d = W.shape
    y64, xp = d64(y), d64(x_prev)
    mm = d64(mom).reshape(M, 1, 1)
    th = d64(theta)[:, None, :]
    ys, xs = [], []
    A0 = torch.zeros(n, d, dtype=_DTYPE[0])
    for m in range(M):
        params = {"W": d64(W[m]), "theta": d64(theta[m]), "rho": d64(mom).reshape(M)[m]}
        y_, x_ = LISTALayer.forward(params, y64[m], -d64(neg_e[m]), xp[m], A0)
        ys.append(y_)
        xs.append(x_)
    y_new, x_new = torch.stack(ys), torch.stack(xs)
    r = y64 - acc
    e_r = (c_dot(d) + 1) * U * (absdot + y64.abs())
    e_x = e_r + U * (r.abs() + th.abs())
    e_y = (1.0 + mm) * e_x + 3 * U * (mm * (x_new - xp).abs() + x_new.abs())
    return {"r": r, "e_r": e_r, "x": x_new, "e_x": e_x, "y": y_new, "e_y": e_y}


def enc_sub(x, W, y):
    """mode 5: y - x @ What^T.  c = c_dot(d) + c_scale(d) + 1."""
    pre, absdot, c = enc_pre(x, W, True)
    y64 = d64(y)
    return {"c": y64 - pre, "e": (c + 1) * U * (absdot + y64.abs())}


# ---------------------------------------------------------------------------
# decoder, code gradient
# ---------------------------------------------------------------------------

def dec(c, W, x):
    """r = c @ What - x, K = n.  c = c_dot(n) + c_scale(d) + 1 (the subtraction).
    The squared-error terms r^2 carry 2|r| e + e^2 plus one rounding."""
    What = normalize_rows(d64(W), EPS_NORM)
    acc, absdot = dot("mbn,mnd->mbd", c, What)
    x64 = d64(x)
    if x64.dim() == 2:
        x64 = x64.unsqueeze(0)
    n, d = W.shape[1], W.shape[2]
    r = acc - x64
    e = (c_dot(n) + c_scale(d) + 1) * U * (absdot + x64.abs())
    return {"r": r, "e": e, "sq": r * r, "e_sq": 2 * r.abs() * e + e * e + U * r * r}


def gc_gv(r, W, l1_alpha, sign):
    """gv = gscale * r @ What^T + (l1/B) * sign, gscale = 2/(B d).
    c = c_dot(d) + c_scale(d) + 3 (gscale's division, its product, the add; the
    l1/B division is covered by the same three on its own term)."""
    What = normalize_rows(d64(W), EPS_NORM)
    acc, absdot = dot("mbd,mnd->mbn", r, What)
    M, B, d = r.shape
    gscale = 2.0 / (B * d)
    l1t = (d64(l1_alpha) / B).reshape(M, 1, 1)
    gv = gscale * acc + l1t * sign
    e = (c_dot(d) + c_scale(d) + 3) * U * (gscale * absdot + (l1t * sign).abs())
    return gv, e


def gc(r, W, c, l1_alpha, gc_mode: int):
    """k_gc_t / k_gc2_t: gv masked by the code that is an *input*, so the mask
    is exact and nothing is undecided.  gc_mode 0: [c > 0], l1 sign +1;
    gc_mode 1 (reverse): [c != 0], l1 sign = sign(c)."""
    c64 = d64(c)
    if gc_mode == 1:
        mask, sign = c64 != 0, torch.sign(c64)
    else:
        mask, sign = c64 > 0, torch.ones_like(c64)
    gv, e = gc_gv(r, W, l1_alpha, sign)
    zero = torch.zeros_like(gv)
    return {"gpre": torch.where(mask, gv, zero), "e": torch.where(mask, e, zero)}


def gc_thresh_autograd(gv, u, scale):
    """d/d(pre, gain, scale) of sum(gv * gate(pre, scale, gain)) by fp64
    autograd through FunctionalThresholdingSAE.gate, at the pre that gives the
    kernel's input u (gain = 0, pre = u * max(a^2, eps))."""
    M, B, n = u.shape
    a = d64(scale).reshape(M, 1, n).clone().requires_grad_()
    gn = torch.zeros(M, 1, n, dtype=_DTYPE[0], requires_grad=True)
    pre = (d64(u) * torch.clamp(a.detach() ** 2, min=GATE_EPS)).requires_grad_()
    with torch.enable_grad():
        code = FunctionalThresholdingSAE.gate(pre, a, gn)
        (d64(gv) * code).sum().backward()
    return pre.grad, gn.grad.reshape(M, n), a.grad.reshape(M, n)


def gc_thresh(r, W, c, u, scale, l1_alpha):
    """k_gc_thresh_t by hand (for the bounds; == gc_thresh_autograd to 1e-12).

    gv as in gc_gv with sign = [code > 0] (the code is an input).  gpre =
    gv g'(u) f, f = a^2/max(a^2, eps): e = g' f e_gv + 3 U |gpre|.  The g_scale
    term t = gv 2a (g(u) - [a^2 > eps] g'(u) u f): e_t = 2|a| |inner| e_gv +
    2|a| |gv| (26 U (|u| + 1 + g) + 3 U g' |u| f) + 4 U |t|.  u is an input, so
    an element is undecided only where u sits on a knee to within the fp32
    representation of 0.9 (2 U); `flip` is the most such an element can move a
    column sum."""
    c64, u64 = d64(c), d64(u)
    gv, e_gv = gc_gv(r, W, l1_alpha, (c64 > 0).double())
    a = d64(scale)[:, None, :]
    a_sq = a * a
    s = torch.clamp(a_sq, min=GATE_EPS)
    f = a_sq / s
    act = (a_sq > GATE_EPS).double()
    gp = 10.0 * ((u64 > 0.9) & (u64 < 1.0)).double() + (u64 > 1.0).double()
    g = gate_g(u64)
    gpre = gv * gp * f
    e_gpre = gp * f * e_gv + 3 * U * gpre.abs()
    inner = g - act * gp * u64 * f
    t = gv * 2.0 * a * inner
    e_t = (2 * a.abs() * inner.abs() * e_gv
           + 2 * a.abs() * gv.abs() * (26 * U * (u64.abs() + 1.0 + g) + 3 * U * gp * u64.abs() * f)
           + 4 * U * t.abs())
    und = ((u64 - 0.9).abs() <= 2 * U) | ((u64 - 1.0).abs() <= 2 * U)
    zero = torch.zeros_like(gv)
    flip_gain = torch.where(und, 11.0 * f * (gv.abs() + e_gv), zero)
    flip_scale = torch.where(und, 2 * a.abs() * (gv.abs() + e_gv) * (g + 11.0 * u64.abs() * f), zero)
    return {"gv": gv, "gpre": gpre, "e_gpre": e_gpre, "t_scale": t, "e_t": e_t,
            "undecided": und, "flip_gain": flip_gain, "flip_scale": flip_scale}


# ---------------------------------------------------------------------------
# row norms
# ---------------------------------------------------------------------------

def row_norms(W, eps: float):
    """norm and 1/max(norm, eps).  The sum of d squares is off by at most
    d U relatively whatever the order (all terms positive), the square root
    halves that and rounds once: d/2 + 1; each square may also lose up to 2^-126 to
    underflow (flush-to-zero or gradual), at most sqrt(d) 2^-63 on the norm.
    The reciprocal adds the rounding of the fp32 eps and its own."""
    W64 = d64(W)
    d = W.shape[-1]
    nrm = W64.norm(dim=-1)
    c = d / 2 + 1
    e_n = c * U * nrm + math.sqrt(d) * 2.0 ** -63
    inv = 1.0 / torch.clamp(nrm, min=eps)
    # safely below the clamp the inverse does not depend on the norm at all
    e_inv = torch.where(nrm + e_n < eps, 2 * U * inv, (c + 2) * U * inv + e_n * inv * inv)
    return {"norms": nrm, "e_norms": e_n, "inv": inv, "e_inv": e_inv,
            "undecided": (nrm - eps).abs() <= e_n}


# ---------------------------------------------------------------------------
# LISTA backward elementwise pass
# ---------------------------------------------------------------------------

def lista_bwd_autograd(g_y, carry_in, r, theta, x_prev, mom):
    """g_r, carry_out, g_theta, g_rho as the gradients of
    sum(g_y * y') + sum(carry_in * x') w.r.t. (r, x_prev, theta, rho), by fp64
    autograd through LISTALayer.forward (W = A = 0, so its r is the leaf y)."""
    M, B, n = r.shape
    outs = ([], [], [], [])
    for m in range(M):
        rl = d64(r[m]).requires_grad_()
        xp = d64(x_prev[m]).requires_grad_()
        th = d64(theta[m]).requires_grad_()
        rho = d64(mom).reshape(M)[m].clone().requires_grad_()
        Z = torch.zeros(n, 1, dtype=_DTYPE[0])
        with torch.enable_grad():
            y_, x_ = LISTALayer.forward({"W": Z, "theta": th, "rho": rho}, rl,
                                        torch.zeros(B, 1, dtype=_DTYPE[0]), xp, Z)
            L = (d64(g_y[m]) * y_).sum()
            if carry_in is not None:
                L = L + (d64(carry_in[m]) * x_).sum()
            L.backward()
        for o, v in zip(outs, (rl.grad, xp.grad, th.grad, rho.grad)):
            o.append(v)
    return tuple(torch.stack(o) for o in outs)


def lista_bwd(g_y, carry_in, r, theta, x, x_prev, mom):
    """k_lista_bwd_elem by hand (for the bounds; == lista_bwd_autograd to 1e-12
    when x = shrink(r, theta)).

    g_x = (1+m) g_y + carry_in: 3 roundings on |1+m||g_y| + |carry_in|.
    carry_out = -m g_y: one.  The g_theta terms are -g_r sign(r) (e = e_gr), the
    g_rho terms g_y (x - x_prev) round twice.  r and theta are inputs, so the
    strict |r| > theta mask is exact."""
    M = r.shape[0]
    gy, r64, x64, xp = d64(g_y), d64(r), d64(x), d64(x_prev)
    ci = d64(carry_in) if carry_in is not None else torch.zeros_like(gy)
    mm = d64(mom).reshape(M, 1, 1)
    th = d64(theta)[:, None, :]
    gx = (1.0 + mm) * gy + ci
    e_gx = 3 * U * ((1.0 + mm).abs() * gy.abs() + ci.abs())
    mask = (r64.abs() > th).double()
    g_r = gx * mask
    t_rho = gy * (x64 - xp)
    return {"g_r": g_r, "e_gr": e_gx * mask, "carry": -mm * gy, "e_carry": U * (mm * gy).abs(),
            "t_theta": -g_r * torch.sign(r64), "t_rho": t_rho, "e_trho": 2 * U * t_rho.abs()}


def lista_theta_depth(B: int) -> int:
    """g_theta column sums: up to 256 rows added in one thread, one atomic per
    row block, the start value."""
    return min(B, 256) + cdiv(B, 256) + 1


def lista_rho_depth(B: int, n: int) -> int:
    """Longest addition chain of the g_rho sum: up to 256 rows in a thread, 6
    shuffles, 4 waves, one atomic per block of the model, the start value."""
    return min(B, 256) + 6 + 4 + cdiv(B, 256) * cdiv(n, 256) + 1


# ---------------------------------------------------------------------------
# Adam kernels
# ---------------------------------------------------------------------------

def f32(v: float) -> float:
    """The value a double has once the launcher casts it to float."""
    return float(torch.tensor(v, dtype=torch.float32).item())


def adam_autograd(p, g, mu, nu, step_no, lr, b1, b2, eps, lr_mult=None):
    """One functional.optim.adam update per model in fp64 at step `step_no[m]`,
    with the fp32-rounded hyper-parameters the kernel receives.  The update is
    linear in lr, so a per-row lr multiplier scales it afterwards."""
    opt = adam(lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps))
    ps, mus, nus = [], [], []
    for m in range(p.shape[0]):
        state = {"mu": d64(mu[m]), "nu": d64(nu[m]), "step": d64(step_no).reshape(-1)[m] - 1.0}
        upd, st = opt.update(d64(g[m]), state)
        if lr_mult is not None:
            upd = upd * d64(lr_mult[m])
        ps.append(d64(p[m]) + upd)
        mus.append(st["mu"])
        nus.append(st["nu"])
    return torch.stack(ps), torch.stack(mus), torch.stack(nus)


def adam_chain(p, g, e_g, mu, nu, step_no, lr, b1, b2, eps, lr_mult=None, pow_ulp=4.0):
    """The Adam recurrence by hand with its error, given the gradient g +- e_g.

    m1 = b1 mu + (1-b1) g (1-b1 is exact in fp32): 3 roundings.  v1 likewise
    with g*g: 4.  b^t by powf is allowed `pow_ulp` ulp (2 pow_ulp U relative),
    so 1-b^t is off by 2 pow_ulp U b^t/(1-b^t) + U relatively.  Each division,
    the square root (1/2-Hoelder where v is tiny), the eps add, lr*lr_mult, the
    product and the final subtraction round once."""
    p, g, e_g, mu, nu = d64(p), d64(g), d64(e_g), d64(mu), d64(nu)
    b1, b2, lr, eps = f32(b1), f32(b2), f32(lr), f32(eps)
    t = d64(step_no).reshape([-1] + [1] * (p.dim() - 1))
    p1 = torch.tensor(b1, dtype=_DTYPE[0]) ** t
    p2 = torch.tensor(b2, dtype=_DTYPE[0]) ** t
    bc1, bc2 = 1.0 - p1, 1.0 - p2
    d_bc1 = 2 * pow_ulp * U * p1 / bc1 + U
    d_bc2 = 2 * pow_ulp * U * p2 / bc2 + U
    m1 = b1 * mu + (1.0 - b1) * g
    v1 = b2 * nu + (1.0 - b2) * g * g
    e_m1 = (1.0 - b1) * e_g + 3 * U * ((b1 * mu).abs() + ((1.0 - b1) * g).abs())
    e_v1 = (1.0 - b2) * (2 * g.abs() * e_g + e_g * e_g) + 4 * U * (b2 * nu + (1.0 - b2) * g * g)
    mh, vh = m1 / bc1, v1 / bc2
    e_mh = e_m1 / bc1 + mh.abs() * (d_bc1 + U)
    e_vh = e_v1 / bc2 + vh * (d_bc2 + U)
    s = vh.sqrt()
    e_s = torch.minimum(e_vh / (2 * s).clamp_min(1e-300), e_vh.sqrt()) + U * s
    den = s + eps
    e_den = e_s + U * den
    assert (den - e_den > 0.5 * den).all(), "ill-conditioned Adam test case"
    q = mh / den
    e_q = (e_mh + q.abs() * e_den) / (den - e_den) + U * q.abs()
    lr_eff = lr * (d64(lr_mult) if lr_mult is not None else torch.ones((), dtype=_DTYPE[0]))
    upd = lr_eff * q
    p_new = p - upd
    e_p = lr_eff.abs() * e_q + 2 * U * upd.abs() + U * p_new.abs()
    return {"p": p_new, "e_p": e_p, "mu": m1, "e_mu": e_m1, "nu": v1, "e_nu": e_v1}


def project_grad_autograd(W, gw, project: bool, clamp_mask=False, eps_norm=EPS_NORM):
    """The gradient k_project_adam feeds to Adam, by fp64 autograd through
    normalize_rows: d/dW sum(gw * normalize_rows(W_used)), where W_used is W, or
    clamp(W, 0) when the kernel gets w_used + clamp_mask (positive SAE)."""
    if not project:
        return d64(gw)
    Wl = d64(W).requires_grad_()
    with torch.enable_grad():
        Wu = torch.clamp(Wl, min=0.0) if clamp_mask else Wl
        (normalize_rows(Wu, eps_norm) * d64(gw)).sum().backward()
    return Wl.grad


def project_grad(W, gw, project: bool, w_used=None, clamp_mask=False, eps_norm=EPS_NORM):
    """The same gradient by hand, with its bound.  With the row norm nrm +- dn
    (dn = (d/2 + 1) U as in row_norms, the kernel reads the fp32 norms):
    dot = gw.w carries c_dot(d) roundings; dot/nrm^2 adds 2 dn + 2 U; g =
    (gw - ds w)/max(nrm, eps) rounds the product, the subtraction, the
    reciprocal and its product, and inherits dn once more."""
    gw64 = d64(gw)
    if not project:
        return gw64, torch.zeros_like(gw64)
    w = d64(w_used) if w_used is not None else d64(W)
    d = w.shape[-1]
    nrm = w.norm(dim=-1, keepdim=True)
    dn = (d / 2 + 1) * U
    inv = 1.0 / torch.clamp(nrm, min=eps_norm)
    do_proj = nrm > eps_norm
    dotv = (gw64 * w).sum(-1, keepdim=True)
    absdot = (gw64 * w).abs().sum(-1, keepdim=True)
    nsq = torch.where(do_proj, nrm * nrm, torch.ones_like(nrm))
    ds = torch.where(do_proj, dotv / nsq, torch.zeros_like(dotv))
    e_ds = torch.where(do_proj, (c_dot(d) * U * absdot + dotv.abs() * (2 * dn + 2 * U)) / nsq,
                       torch.zeros_like(dotv))
    g = (gw64 - ds * w) * inv
    e_g = (U * gw64.abs() + w.abs() * e_ds + 2 * U * (ds * w).abs()) * inv + g.abs() * (dn + 3 * U)
    if clamp_mask:
        keep = d64(W) >= 0
        g, e_g = g * keep, e_g * keep
    return g, e_g


def bias_grad_autograd(bias, g_bias, decay):
    """g_bias + d/dbias (decay * ||bias||_2) per model, by fp64 autograd (the
    bias-decay term of the SAE losses; its gradient at bias = 0 is 0)."""
    b = d64(bias).requires_grad_()
    with torch.enable_grad():
        (d64(decay) * torch.norm(b, 2, dim=-1)).sum().backward()
    return d64(g_bias) + b.grad


def bias_grad(bias, g_bias, decay):
    """By hand: g + (decay/||b||) b.  The norm is off by (n/2 + 1) U, the
    division, the product and the add round once each."""
    b, g0, bd = d64(bias), d64(g_bias), d64(decay).reshape(-1, 1)
    n = b.shape[-1]
    nrm = b.norm(dim=-1, keepdim=True)
    ds = torch.where(nrm > 0, bd / nrm.clamp_min(1e-300), torch.zeros_like(nrm))
    g = g0 + ds * b
    e_g = U * g.abs() + (ds * b).abs() * ((n / 2 + 1) * U + 3 * U)
    return g, e_g


# ---------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------

def topk_ref(scores, ks):
    """torch.topk + scatter + clamp, per model: the reference TopK encoder.
    Only meaningful for distinct scores.  Returns (c, fired increment)."""
    s = scores.detach().cpu()
    M, B, n = s.shape
    c = torch.zeros_like(s)
    for m in range(M):
        k = min(int(ks[m]), n)
        if k == 0:
            continue
        vals, idx = torch.topk(s[m], k, dim=-1)
        c[m].scatter_(-1, idx, torch.clamp(vals, min=0.0))
    return c, (c > 0).float().sum(dim=1)


def canon_zero(t):
    """+0.0 for either zero, every other bit pattern unchanged: the reference's
    clamp and the kernel's fmaxf may each return either sign for max(-0, +0)."""
    return t.detach().cpu() + 0.0


def check_topk_properties(name, scores, c, ks):
    """What must hold whatever the tie rule, for scores > 0 (so that a selected
    slot shows as c != 0): exactly min(k, n) slots are selected, each holds its
    score bit for bit, every score above the k-th value is selected and none
    below it."""
    s, c = scores.detach().cpu(), c.detach().cpu()
    M, B, n = s.shape
    assert (s > 0).all(), "tie cases need positive scores"
    for m in range(M):
        k = min(int(ks[m]), n)
        sel = c[m] != 0
        cnt = sel.sum(dim=-1)
        if not (cnt == k).all():
            raise Mismatch(f"{name}: model {m} selects {cnt.tolist()} slots per row, k = {k}")
        if k == 0:
            continue
        if not torch.equal(_bits(c[m][sel]), _bits(s[m][sel])):
            raise Mismatch(f"{name}: model {m}: a selected slot does not hold its score")
        kth = torch.sort(s[m], dim=-1, descending=True).values[:, k - 1:k]
        if ((s[m] > kth) & ~sel).any():
            raise Mismatch(f"{name}: model {m}: a score above the k-th value was not selected")
        if ((s[m] < kth) & sel).any():
            raise Mismatch(f"{name}: model {m}: a score below the k-th value was selected")


# ---------------------------------------------------------------------------
# resample
# ---------------------------------------------------------------------------

def resample_ref(fired, new_rows, enc_scale, W, mu_w, nu_w, dec=None, mu_d=None, nu_d=None,
                 bias=None, mu_b=None, nu_b=None, per_segment=None):
    """The index-order rule of EnsembleResampler._resample_cpu on copies of the
    tensors: per model the first n_track dead features (fired == 0) in index
    order get encoder row pool_unit[rank] * scale (decoder row pool_unit[rank]),
    zero bias and zero Adam moments; nothing else changes.

    `per_segment` = a segment width ranks the dead features within each segment
    of that many columns instead of across them: the fault a block-wide scan
    makes when it loses its running base (used to test the comparator)."""
    out = {k: (v.detach().cpu().clone() if v is not None else None) for k, v in dict(
        W=W, mu_w=mu_w, nu_w=nu_w, dec=dec, mu_d=mu_d, nu_d=nu_d,
        bias=bias, mu_b=mu_b, nu_b=nu_b).items()}
    fired, new_rows, enc_scale = fired.cpu(), new_rows.cpu(), enc_scale.cpu()
    M, n_track = new_rows.shape[0], new_rows.shape[1]
    counts = torch.zeros(M, dtype=torch.int32)
    for m in range(M):
        dead = torch.where(fired[m] == 0)[0]
        if per_segment:
            seg = dead // per_segment
            rank = torch.tensor([int((seg[:i] == seg[i]).sum()) for i in range(dead.numel())],
                                dtype=torch.long)
        else:
            rank = torch.arange(dead.numel())
        keep = rank < n_track
        dead, rank = dead[keep], rank[keep]
        counts[m] = min(int((fired[m] == 0).sum()), n_track)
        if dead.numel() == 0:
            continue
        rows = new_rows[m, rank]
        out["W"][m, dead] = rows * enc_scale[m]
        out["mu_w"][m, dead] = 0.0
        out["nu_w"][m, dead] = 0.0
        if dec is not None:
            out["dec"][m, dead] = rows
            out["mu_d"][m, dead] = 0.0
            out["nu_d"][m, dead] = 0.0
        if bias is not None:
            out["bias"][m, dead] = 0.0
            out["mu_b"][m, dead] = 0.0
            out["nu_b"][m, dead] = 0.0
    out["counts"] = counts
    return out

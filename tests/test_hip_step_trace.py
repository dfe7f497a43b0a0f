"""Launch traces of the fused HIP steps, checked on CPU.

The step classes in ``engine/hip_step.py`` only orchestrate: they hand
workspaces and parameters to the extension's launchers.  Given a stand-in
extension they run on CPU tensors, so "which launches, in which order, on
which operands, with which scalars" is testable without a GPU.

The expected traces (``tests/golden/hip_step_trace.json``) were recorded with
this same recorder from the commit before the step classes were folded onto
one base class; a refactor of the orchestration must reproduce them exactly.
One argument is excluded from the comparison: ``accumulate`` of ``gc`` (the
bias gradient is overwritten instead of memset + accumulated; the GPU oracle
tests check its values).

Re-record (from the repository root) with
``python -m tests.test_hip_step_trace --record tests/golden/hip_step_trace.json``.
"""

import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_step_trace.json")

M, B, D, N = 2, 64, 32, 64
L1S = (1e-3, 3e-3)

_REQ = object()

# argument names and defaults of the bindings (PYBIND11_MODULE in
# ops/hip/sae_ops.hip); calls are normalised to full keyword form with these
BINDINGS = {
    "row_norms": [("W", _REQ), ("norms", _REQ), ("inv_norms", _REQ), ("eps", _REQ)],
    "transpose_scale": [("src", _REQ), ("dst", _REQ), ("scale", _REQ)],
    "enc_fwd2": [("xT", _REQ), ("WT", _REQ), ("bias", _REQ), ("c_out", _REQ), ("loss_parts", _REQ),
                 ("fired", _REQ), ("mode", _REQ), ("bk", 32), ("prio", False), ("dict_sizes", None)],
    "gc2": [("rT", _REQ), ("WT", _REQ), ("c", _REQ), ("l1_alpha", _REQ), ("gpre", _REQ), ("g_bias", _REQ),
            ("bk", 32), ("prio", False), ("gc_mode", 0)],
    "enc_fwd": [("x", _REQ), ("Wenc", _REQ), ("bias", _REQ), ("inv_norms", _REQ), ("c_out", _REQ),
                ("loss_parts", _REQ), ("fired", _REQ), ("mode", _REQ), ("bk", 32), ("prio", False),
                ("bn", 128), ("act_scale", None), ("act_gain", None), ("u_out", None),
                ("dict_sizes", None), ("y_in", None), ("x_prev", None), ("x_out", None), ("mom", None)],
    "topk_select": [("scores", _REQ), ("c_out", _REQ), ("fired", _REQ), ("ks", _REQ)],
    "lista_bwd_elem": [("g_y", _REQ), ("carry_in", _REQ), ("r", _REQ), ("theta", _REQ), ("x", _REQ),
                       ("x_prev", _REQ), ("mom", _REQ), ("g_r", _REQ), ("carry_out", _REQ),
                       ("g_theta", _REQ), ("g_rho", _REQ)],
    "gc_thresh": [("r", _REQ), ("Wdec", _REQ), ("inv_norms", _REQ), ("c", _REQ), ("u", _REQ),
                  ("act_scale", _REQ), ("l1_alpha", _REQ), ("gpre", _REQ), ("g_gain", _REQ),
                  ("g_scale", _REQ), ("bk", 32), ("prio", False)],
    "dec_fwd": [("c", _REQ), ("Wdec", _REQ), ("inv_norms", _REQ), ("x", _REQ), ("r_out", _REQ),
                ("loss_parts", _REQ), ("bk", 32), ("prio", False), ("bn", 128)],
    "gc": [("r", _REQ), ("Wdec", _REQ), ("inv_norms", _REQ), ("c", _REQ), ("l1_alpha", _REQ),
           ("gpre", _REQ), ("g_bias", _REQ), ("bk", 32), ("prio", False), ("gc_mode", 0), ("bn", 128),
           ("accumulate", True)],
    "grad_w": [("P", _REQ), ("Q", _REQ), ("gw", _REQ), ("alpha", _REQ), ("beta", _REQ),
               ("bk", 32), ("prio", False), ("bn", 128)],
    "project_adam": [("W", _REQ), ("gw", _REQ), ("norms", _REQ), ("mu", _REQ), ("nu", _REQ),
                     ("step_no", _REQ), ("n_per_model", _REQ), ("lr", _REQ), ("b1", _REQ), ("b2", _REQ),
                     ("eps_adam", _REQ), ("eps_norm", _REQ), ("project", _REQ), ("w_used", None),
                     ("clamp_mask", False), ("lr_mult", None)],
    "colsum": [("X", _REQ), ("out", _REQ), ("alpha", 1.0), ("absval", False)],
    "bias_adam": [("bias", _REQ), ("g_bias", _REQ), ("decay", _REQ), ("mu", _REQ), ("nu", _REQ),
                  ("step_no", _REQ), ("lr", _REQ), ("b1", _REQ), ("b2", _REQ), ("eps_adam", _REQ),
                  ("lr_mult", None)],
}
# deliberately not compared (module docstring)
DROPPED = {("gc", "accumulate")}


def _storage(t):
    return t.untyped_storage().data_ptr()


class RecordingExt:
    """Stand-in for the extension module: records every launch, runs nothing."""

    def __init__(self):
        self.calls = []
        self.step = None
        self.x = None

    def _owners(self):
        own = {}

        def walk(label, obj):
            if torch.is_tensor(obj):
                own.setdefault(_storage(obj), label)
            elif isinstance(obj, dict):
                for k, v in obj.items():
                    walk(f"{label}.{k}", v)
            elif isinstance(obj, (list, tuple)):
                for i, v in enumerate(obj):
                    walk(f"{label}.{i}", v)

        ens = self.step.ens
        walk("x", self.x)
        walk("params", ens.params)
        for k, v in ens.optim_states.items():
            walk(k, v)
        walk("buffers", ens.buffers)
        for name in sorted(vars(self.step)):
            v = getattr(self.step, name)
            if name.startswith("_"):
                continue
            if torch.is_tensor(v):
                own.setdefault(_storage(v), name)
            elif isinstance(v, list):
                for i, t in enumerate(v):
                    if torch.is_tensor(t):
                        own.setdefault(_storage(t), f"{name}[{i}]")
        return own

    def _value(self, v, owners):
        if torch.is_tensor(v):
            return [owners.get(_storage(v), "<unowned>"), v.storage_offset(), list(v.shape)]
        assert v is None or isinstance(v, (bool, int, float)), type(v)
        return v

    def __getattr__(self, fn):
        if fn not in BINDINGS:
            raise AttributeError(fn)
        spec = BINDINGS[fn]

        def launch(*args, **kwargs):
            assert len(args) <= len(spec), f"{fn}: too many positional arguments"
            bound = {name: a for (name, _), a in zip(spec, args)}
            for k, v in kwargs.items():
                assert k in dict(spec) and k not in bound, f"{fn}: bad keyword {k}"
                bound[k] = v
            owners = self._owners()
            full = {}
            for name, default in spec:
                v = bound.get(name, default)
                assert v is not _REQ, f"{fn}: missing argument {name}"
                if (fn, name) not in DROPPED:
                    full[name] = self._value(v, owners)
            self.calls.append([fn, full])

        return launch


def _ensemble(sig, models):
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam

    return FunctionalEnsemble(models, sig, adam, {"lr": 1e-3}, device="cpu", backend="torch")


def _targets():
    """name -> (signature, models factory, step factory(ens, ext))"""
    from sparse_coding_amd.engine import hip_step as hs
    from sparse_coding_amd.models import sae_signatures as sigs
    from sparse_coding_amd.models.lista import (
        FunctionalLISTADenoisingSAE,
        FunctionalResidualDenoisingSAE,
    )
    from sparse_coding_amd.models.positive import FunctionalPositiveTiedSAE
    from sparse_coding_amd.models.semilinear import SemiLinearSAE
    from sparse_coding_amd.models.topk import TopKEncoder

    def whitened():
        out = []
        for l1 in L1S:
            q, _ = torch.linalg.qr(torch.randn(D, D))
            out.append(sigs.FunctionalTiedSAE.init(D, N, l1, translation=torch.randn(D) * 0.3,
                                                   rotation=q, scaling=torch.rand(D) + 0.5))
        return out

    plain = lambda sig, **kw: (lambda: [sig.init(D, N, l1, **kw) for l1 in L1S])
    masked = lambda sig: (lambda: [sig.init(D, nd, N, 1e-3) for nd in (N // 2, N)])
    layered = lambda sig: (lambda: [sig.init(D, N, 2, l1) for l1 in L1S])
    return {
        "tied": (sigs.FunctionalTiedSAE, plain(sigs.FunctionalTiedSAE),
                 lambda e, x: hs.HipSAEStep(e, x, tied=True)),
        "untied": (sigs.FunctionalSAE, plain(sigs.FunctionalSAE),
                   lambda e, x: hs.HipSAEStep(e, x, tied=False)),
        "masked_tied": (sigs.FunctionalMaskedTiedSAE, masked(sigs.FunctionalMaskedTiedSAE),
                        lambda e, x: hs.HipSAEStep(e, x, tied=True, masked=True)),
        "masked_untied": (sigs.FunctionalMaskedSAE, masked(sigs.FunctionalMaskedSAE),
                          lambda e, x: hs.HipSAEStep(e, x, tied=False, masked=True)),
        "reverse": (sigs.FunctionalReverseSAE, plain(sigs.FunctionalReverseSAE, bias_decay=0.01),
                    lambda e, x: hs.HipSAEStep(e, x, tied=True, reverse=True)),
        "centered": (sigs.FunctionalTiedCenteredSAE, plain(sigs.FunctionalTiedCenteredSAE),
                     hs.HipCenteredStep),
        "whitened": (sigs.FunctionalTiedSAE, whitened, hs.HipWhitenedStep),
        "positive": (FunctionalPositiveTiedSAE, plain(FunctionalPositiveTiedSAE, bias_decay=0.01),
                     hs.HipPositiveStep),
        "thresholding": (sigs.FunctionalThresholdingSAE, plain(sigs.FunctionalThresholdingSAE),
                         hs.HipThresholdStep),
        "topk": (TopKEncoder, lambda: [TopKEncoder.init(D, N, k) for k in (4, 8)], hs.HipTopKStep),
        "lista": (FunctionalLISTADenoisingSAE, layered(FunctionalLISTADenoisingSAE), hs.HipLISTAStep),
        "residual_denoising": (FunctionalResidualDenoisingSAE, layered(FunctionalResidualDenoisingSAE),
                               hs.HipResidualDenoisingStep),
        "semilinear": (SemiLinearSAE, plain(SemiLinearSAE), hs.HipSemilinearStep),
    }


# (target, staging): every target under the default config, plus the
# pre-transposed variant of the two classes that have one
CASES = [(t, "t") for t in ("tied", "untied", "masked_tied", "masked_untied", "reverse", "centered",
                            "whitened", "positive", "thresholding", "topk", "lista",
                            "residual_denoising", "semilinear")] + [("tied", "pre"), ("untied", "pre")]


def run_case(target, staging, with_on_grads):
    """One grads_phase + update_phase on a fresh CPU ensemble.  Returns
    (trace, tensors handed to on_grads, dp_grad_tensors())."""
    from sparse_coding_amd.ops.kconfig import DEFAULTS, kernel_config, set_kernel_config

    old = kernel_config()
    set_kernel_config(**dict(DEFAULTS, staging=staging))
    try:
        torch.manual_seed(0)
        sig, models, make = _targets()[target]
        ext = RecordingExt()
        step = make(_ensemble(sig, models()), ext)
        ext.step = step
        ext.x = x = torch.randn(B, D)
        seen = []
        if with_on_grads:
            n = step.grads_phase(x, on_grads=seen.extend)
        else:
            n = step.grads_phase(x)
        step.update_phase(n)
        return ext.calls, seen, step.dp_grad_tensors()
    finally:
        set_kernel_config(**old)


def _key(target, staging, with_on_grads):
    return f"{target}/{staging}/{'on_grads' if with_on_grads else 'plain'}"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("with_on_grads", [False, True], ids=["plain", "on_grads"])
@pytest.mark.parametrize("target,staging", CASES, ids=[f"{t}-{s}" for t, s in CASES])
def test_launch_trace_matches_recorded(golden, target, staging, with_on_grads):
    key = _key(target, staging, with_on_grads)
    if key in golden:
        want = golden[key]
    else:
        # recorded before HipTopKStep.grads_phase took on_grads: announcing
        # the gradient must not change a launch
        assert key == "topk/t/on_grads", f"no recorded trace for {key}"
        want = golden[_key(target, staging, False)]
    got, _, _ = run_case(target, staging, with_on_grads)
    got = json.loads(json.dumps(got))
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} of {key} differs:\n got  {g}\n want {w}"


@pytest.mark.parametrize("target,staging", CASES, ids=[f"{t}-{s}" for t, s in CASES])
def test_on_grads_covers_dp_grad_tensors_once(target, staging):
    """During one grads_phase the tensors handed to on_grads cover each
    tensor of dp_grad_tensors() exactly once, whole or as disjoint slices
    along dim 0 (what the data-parallel trainer all-reduces)."""
    _, seen, dp = run_case(target, staging, True)
    assert dp, "no data-parallel gradient tensors"
    rows = {id(t): [] for t in dp}
    for s in seen:
        assert s.is_contiguous()
        for t in dp:
            row = t.numel() // t.shape[0]
            rel = s.storage_offset() - t.storage_offset()
            if _storage(s) == _storage(t) and 0 <= rel < t.numel():
                assert s.shape[1:] == t.shape[1:] and rel % row == 0, (s.shape, t.shape, rel)
                rows[id(t)].append((rel // row, rel // row + s.shape[0]))
                break
        else:
            raise AssertionError(f"on_grads got a tensor {tuple(s.shape)} that is no data-parallel gradient")
    for t in dp:
        end = 0
        for lo, hi in sorted(rows[id(t)]):
            assert lo == end, f"gradient {tuple(t.shape)}: rows {end}:{lo} announced {'twice' if lo < end else 'never'}"
            end = hi
        assert end == t.shape[0], f"gradient {tuple(t.shape)}: rows {end}: never announced"


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    out = {}
    for target, staging in CASES:
        for with_on_grads in (False, True):
            try:
                out[_key(target, staging, with_on_grads)] = run_case(target, staging, with_on_grads)[0]
            except TypeError as e:  # a grads_phase without on_grads: nothing to record
                print(f"skipped {_key(target, staging, with_on_grads)}: {e}")
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        f.write("{\n")
        for ki, (key, calls) in enumerate(out.items()):
            f.write(f" {json.dumps(key)}: [\n")
            f.write(",\n".join("  " + json.dumps(c) for c in calls))
            f.write("\n ]" + ("," if ki + 1 < len(out) else "") + "\n")
        f.write("}\n")
    print(f"recorded {len(out)} traces to {sys.argv[2]}")

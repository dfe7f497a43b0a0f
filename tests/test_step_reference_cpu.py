"""The step-gradient reference validated on the CPU (tests/step_reference.py).

What test_hip_step_grads_gpu.py relies on is checked here without a GPU:
the seeds give inputs on which no nonsmooth decision is near its knee, the
comparator accepts the fp32 yardstick and rejects the fp32 gradients of
deliberately wrong problems, the recorder flags a planted near-knee argument,
ignores an exact-knee one and refuses an op it does not know, and every case's
perturbation does what it is there for.
"""

import pytest
import torch
import torch.nn.functional as F

from tests import step_reference as R

GRID_IDS = [R.grid_id(e) for e in R.GRID]
RAGGED_OF = {name: shape for name, shape, staging in R.GRID if staging is None and shape != R.ALIGNED}


# ---------------------------------------------------------------------------
# cases and seeds
# ---------------------------------------------------------------------------

def test_grid_covers_every_fused_step():
    from sparse_coding_amd.engine import hip_step

    steps = {c.step_class for c in R.cases()}
    fused = {n for n, v in vars(hip_step).items()
             if isinstance(v, type) and issubclass(v, hip_step._HipStep) and v is not hip_step._HipStep}
    assert steps == fused
    assert len(R.cases()) == 14
    for c in R.cases():
        shapes = {s for n, s, st in R.GRID if n == c.name and st is None}
        assert shapes == {R.ALIGNED, R.RAGGED_DEEP if c.name in R.DEEP else R.RAGGED}, c.name
    assert [(n, s) for n, s, st in R.GRID if st == "pre"] == [(n, R.PRE) for n in ("tied", "untied", "masked_tied")]


@pytest.mark.parametrize("entry", R.GRID, ids=GRID_IDS)
def test_seed_is_clean(entry):
    """Zero near-knee arguments for every (case, shape) the GPU module runs."""
    name, shape, _ = entry
    dec = R.decisions(name, shape)
    ops = sorted({r["op"] for r in dec["records"]})
    print(f"[step64] {R.grid_id(entry)} seed={R.seed_of(name, shape)} near={dec['near']} "
          f"margin={dec['margin']:.2e} ops={','.join(ops)}")
    assert dec["near"] == 0
    assert (name, shape) in R.SEEDS


def test_seeds_are_the_first_clean_ones():
    """The table is what the search over 0, 1, 2, ... gives on the float64
    reference: nothing about a seed is a choice."""
    for name, shape, _ in R.GRID:
        assert R.first_clean_seed(name, shape) == R.SEEDS[(name, shape)], (name, shape)


def _stacked(name, shape):
    models, x = R.build(name, shape)
    return R.tree_stack([p for p, _ in models]), R.tree_stack([b for _, b in models]), x


@pytest.mark.parametrize("shape", [R.ALIGNED, R.RAGGED], ids=["aligned", "ragged"])
def test_perturbations_take_the_backward_off_zero(shape):
    """Each case's perturbation, and no gradient leaf identically zero."""
    for c in R.cases():
        shp = shape if shape == R.ALIGNED else RAGGED_OF[c.name]
        p, b, x = _stacked(c.name, shp)
        n = shp[3]
        if "l1_alpha" in b:
            assert b["l1_alpha"][0] != b["l1_alpha"][1]
        if "encoder_bias" in p:
            assert (p["encoder_bias"] != 0).all()
        if "bias_decay" in b:
            assert (b["bias_decay"] == R.f32(R.BIAS_DECAY)).all()
        if c.name == "centered":
            assert (p["center"] != 0).all()
        if c.name == "whitened":
            eye = torch.eye(shp[2]).expand_as(b["center_rot"])
            assert not torch.allclose(b["center_rot"], eye) and (b["center_trans"] != 0).all()
        if c.name == "positive":
            share = (p["encoder"] < 0).float().mean().item()
            assert 0.2 < share < 0.6, share
        if c.name == "thresholding":
            What = p["encoder"] / p["encoder"].norm(dim=-1, keepdim=True)
            a_sq = p["activation_scale"].pow(2)[:, None, :]
            u = (torch.einsum("bd,mnd->mbn", x, What) + p["activation_gain"][:, None, :]) / a_sq
            for lo, hi in ((-1e9, 0.9), (0.9, 1.0), (1.0, 1e9)):
                assert ((u > lo) & (u < hi)).float().mean(dim=(1, 2)).min() > 0.005, (lo, hi)
        if c.name == "lista":
            rho = torch.stack([layer["rho"] for layer in p["encoder_layers"]], dim=1)  # [M, L]
            assert ((rho[0] > 0) & (rho[0] < 1)).all()
            assert (rho[1] < 0).any() and (rho[1] > 1).any()
            assert not ((rho == 0) | (rho == 1)).any()  # the step's gate is strict, clamp's backward is not
            for layer in p["encoder_layers"]:
                assert (layer["theta"] > 0).any() and (layer["theta"] < 0).any()
        if c.name == "residual":
            assert all((layer["theta"] != 0).all() for layer in p["encoder_layers"])
        if c.name == "semilinear":
            h = p["encoder_layers"][0]["weight"].shape[1]
            assert h == R.semilinear_hidden(shp[2], n) and h not in (shp[2], n)
            if shp != R.ALIGNED:
                assert h % 4 == 0 and h % 16 != 0
            assert all((layer["bias"] != 0).all() for layer in p["encoder_layers"])
        if c.dict_sizes is not None:
            ds = b["dict_size"].tolist()
            assert ds == list(c.dict_sizes(n)) and ds[0] != ds[1] and max(ds) < n
        if "topk" in c.name:
            assert b["sparsity"][0] != b["sparsity"][1]
        ref = R.reference(c.name, shp)
        for path, g in R.tree_items(ref["g64"]):
            for m in range(2):
                if c.name == "lista" and path.endswith("rho") and m == 1:
                    continue  # gated: checked below
                assert g[m].abs().max() > 0, (c.name, path, m)
                assert torch.isfinite(g[m]).all(), (c.name, path, m)
        if c.name == "lista":
            # the gate matters: the gated rhos have zero gradient, and would not without the clamp
            g_rho = torch.stack([layer["rho"] for layer in ref["g64"]["encoder_layers"]], dim=1)
            assert (g_rho[1][(rho[1] < 0) | (rho[1] > 1)] == 0).all()
            assert (g_rho[0] != 0).all()


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("entry", R.GRID, ids=GRID_IDS)
def test_comparator_accepts_the_yardstick(entry):
    """The fp32 CPU gradients, run through Adam's recurrence in fp32, pass as
    mu and nu after one and after three steps; so do the fp32 codes/losses."""
    name, shape, _ = entry
    c = R.case(name)
    ref = R.reference(name, shape)
    masked = (shape[3], c.dict_sizes(shape[3])) if c.dict_sizes else None
    for t in (1, 3):
        mu, nu = R.moments(ref["g32"], t)
        r_mu = R.compare(mu, ref["g64"], ref["g32"], "mu", t, masked)
        r_nu = R.compare(nu, ref["g64"], ref["g32"], "nu", t, masked)
        assert max(r_mu.values()) <= 1.0 and max(r_nu.values()) <= 1.0
    R.compare_codes(ref["c32"], ref, masked[1] if masked else None)
    R.compare_losses(ref["loss32"], ref, R.loss_depths(c, *shape[1:]))
    # the yardstick's own error, relative to the leaf's scale: fp32 rounding
    for (path, g64), (_, g32) in zip(R.tree_items(ref["g64"]), R.tree_items(ref["g32"])):
        for m in range(2):
            rel = (g32[m].double() - g64[m]).abs().max() / g64[m].abs().max().clamp_min(1e-300)
            assert rel < 2e-5, (path, m, rel.item())


def test_comparator_details():
    ref = R.reference("masked_untied", R.RAGGED)
    n, sizes = R.RAGGED[3], R.case("masked_untied").dict_sizes(R.RAGGED[3])
    mu, nu = R.moments(ref["g32"], 1)
    # NaN never passes
    bad = R.tree_apply(torch.clone, mu)
    bad["encoder"][1, 3, 5] = float("nan")
    with pytest.raises(R.Mismatch, match=r"mu encoder\[model 1\]"):
        R.compare(bad, ref["g64"], ref["g32"], "mu", 1)
    # masked rows must be exactly zero, however small the entry
    bad = R.tree_apply(torch.clone, mu)
    bad["decoder"][0, sizes[0], 0] = 1e-30
    R.compare(bad, ref["g64"], ref["g32"], "mu", 1)
    with pytest.raises(R.Mismatch, match="masked entries"):
        R.compare(bad, ref["g64"], ref["g32"], "mu", 1, (n, sizes))
    c_bad = ref["c32"].clone()
    c_bad[1, 0, sizes[1]] = 1e-30
    with pytest.raises(R.Mismatch, match="masked columns"):
        R.compare_codes(c_bad, ref, sizes)
    # a wrong step count shows in both moments
    mu3, nu3 = R.moments(ref["g32"], 3)
    for tree, what in ((mu3, "mu"), (nu3, "nu")):
        with pytest.raises(R.Mismatch):
            R.compare(tree, ref["g64"], ref["g32"], what, 2)
    # a sign error is invisible to nu and caught by mu
    neg = R.tree_apply(lambda t: -t, mu)
    with pytest.raises(R.Mismatch):
        R.compare(neg, ref["g64"], ref["g32"], "mu", 1)
    # losses: a missing 'loss', and one off by 1e-4 relative
    depths = R.loss_depths(R.case("masked_untied"), *R.RAGGED[1:])
    with pytest.raises(R.Mismatch, match="no 'loss'"):
        R.compare_losses({"l_l1": ref["loss32"]["l_l1"]}, ref, depths)
    off = dict(ref["loss32"], l_l1=ref["loss32"]["l_l1"] * (1 + 1e-4))
    with pytest.raises(R.Mismatch, match="loss l_l1"):
        R.compare_losses(off, ref, depths)
    assert max(depths.values()) * R.U < 1e-4


DOCTORED = [(doc, c.name) for doc, (applies, _, _) in R.DOCTORINGS.items() for c in R.cases() if applies(c)]


@pytest.mark.parametrize("doctoring,name", DOCTORED, ids=[f"{d}-{n}" for d, n in DOCTORED])
def test_comparator_rejects_doctored_gradients(doctoring, name):
    """The fp32 autograd gradient of a doctored problem, presented as the
    device's mu, is rejected on at least one leaf: a wrong gscale, a dropped
    batch row, a dropped small term, a missing projection, gate or mask."""
    shape = RAGGED_OF[name]
    ref = R.reference(name, shape)
    mu, _ = R.moments(R.doctored(doctoring, name, shape), 1)
    with pytest.raises(R.Mismatch) as exc:
        R.compare(mu, ref["g64"], ref["g32"], "mu", 1)
    leaves = sorted({part.split("[")[0].replace("mu ", "") for part in str(exc.value).split("; ")})
    print(f"[step64] doctored {doctoring} {name}: rejected by {', '.join(leaves)}")


def test_every_doctoring_applies_somewhere():
    assert {d for d, _ in DOCTORED} == set(R.DOCTORINGS)
    assert R.doctored("rho_ungated", "tied", R.RAGGED) is None


# ---------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------

def _near_total(fn):
    return sum(r["near"] for r in R.record(fn))


def test_recorder_flags_near_and_ignores_exact():
    base = torch.tensor([-3.0, 0.0, 0.5, 2.0, 6.0, 8.0], dtype=torch.float64)
    near0 = base.clone()
    near0[2] = 8.0 * 2.0 ** -19          # within 2^-18 max|arg| of the knee at 0
    near6 = base.clone()
    near6[3] = 6.0 - 8.0 * 2.0 ** -19
    just_out = base.clone()
    just_out[2] = 8.0 * 2.0 ** -17
    for fn in (F.relu, torch.relu, lambda t: torch.clamp(t, min=0.0), lambda t: t.clamp(0.0), torch.sign,
               torch.abs, lambda t: t > 0.0, lambda t: torch.norm(t, 1, dim=-1), F.relu6):
        assert _near_total(lambda: fn(base)) == 0       # -3, 0.5, 2, 8 are far; 0 (and 6) exactly on a knee
        assert _near_total(lambda: fn(near0)) == 1
        assert _near_total(lambda: fn(just_out)) == 0
    assert _near_total(lambda: F.relu6(near6)) == 1
    assert _near_total(lambda: F.relu(near6)) == 0
    assert _near_total(lambda: torch.clamp(near6, 0.0, 6.0)) == 1
    assert _near_total(lambda: torch.clamp(near6, min=0.0, max=6.0)) == 1
    # a tensor knee (the reverse SAE's and BatchTopK's comparisons)
    knee = base.clone()
    near_knee = base.clone()
    near_knee[3] += 8.0 * 2.0 ** -19
    assert _near_total(lambda: near_knee >= knee) == 1
    assert _near_total(lambda: base >= knee) == 0
    # zeros out of a ReLU feeding sign: exact, not near
    pre = torch.tensor([-1.0, 2.0, -0.5])
    assert _near_total(lambda: torch.sign(F.relu(pre))) == 0


def test_recorder_topk_gaps():
    s = torch.tensor([[5.0, 4.0, 3.0, 1.0], [5.0, 4.0, 4.0 - 5.0 * 2.0 ** -19, 1.0]], dtype=torch.float64)
    recs = R.record(lambda: torch.topk(s, 2, dim=-1))
    assert {r["op"]: r["near"] for r in recs} == {"topk-zero": 0, "topk-gap": 1}
    s[1, 2] = 3.0
    s[0] = torch.tensor([5.0, 5.0 * 2.0 ** -19, -3.0, -1.0])  # the last kept score next to 0
    recs = R.record(lambda: torch.topk(s, 2, dim=-1))
    assert {r["op"]: r["near"] for r in recs} == {"topk-zero": 1, "topk-gap": 0}
    # the batch selection: one flat top-K
    flat = torch.tensor([9.0, 7.0, 7.0 - 9.0 * 2.0 ** -19, 1.0], dtype=torch.float64)
    recs = R.record(lambda: torch.topk(flat, 2))
    assert {r["op"]: r["near"] for r in recs} == {"topk-zero": 0, "topk-gap": 1}


@pytest.mark.parametrize("fn", [
    lambda t: torch.maximum(t, torch.zeros_like(t)),
    lambda t: t == 0.5,
    lambda t: F.leaky_relu(t),
    lambda t: torch.sort(t),
    lambda t: F.hardtanh(t),
    lambda t: torch.norm(t, 3),
    lambda t: torch.floor(t),
], ids=["maximum", "eq", "leaky_relu", "sort", "hardtanh", "norm3", "floor"])
def test_recorder_refuses_unknown_ops(fn):
    t = torch.tensor([-1.0, 0.5, 2.0], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="DecisionRecorder"):
        R.record(lambda: fn(t))


def test_recorder_sees_every_signatures_decisions():
    """The ops the issue lists, per signature; a forward that records nothing
    raises."""
    expect = {
        "tied": {"clamp", "norm1"},
        "reverse": {"clamp", "gt", "norm1"},
        "thresholding": {"clamp", "relu", "relu6", "norm1"},
        "lista": {"clamp", "relu", "sign", "abs", "norm1"},
        "topk": {"relu", "topk-gap", "topk-zero"},
        "batch_topk": {"ge", "gt", "topk-gap", "topk-zero"},
    }
    for name, ops in expect.items():
        shape = RAGGED_OF[name]
        got = {r["op"].strip("_") for r in R.decisions(name, shape)["records"]}
        assert got == ops, (name, got)

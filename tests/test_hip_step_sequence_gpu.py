"""Every fused step across batch-size changes, each call against fp64 autograd.

A training chunk ends on a short, usually odd-sized batch and the next chunk
starts at the full size again.  For a fused step that one change frees and
reallocates every workspace (out of the caching allocator: ``torch.empty``
hands back the bytes of the previous, differently shaped allocation), resolves
``staging`` and ``topk_chain`` again, drops the captured graph, restarts the
eager count and picks the aligned or the guarded kernels anew.

Here one ensemble per case (``lr = 0``, ``backend="hip"``, capture on) takes
twelve calls on six batches of three sizes against the same two models
(tests/step_reference.py, ``SEQ_GRID``):

    call   1   2   3         4         5   6   7   8         9   10  11        12
    batch  a1  a2  a3        a1        b1  c1  c2  c1        a2  a3  a1        a2
           e   e   captured  replayed  e   e   e   captured  e   e   captured  replayed

(e: eager; calls 5, 6 and 9 reallocate, 6 grows past everything before it; a
class that does not capture runs all twelve eagerly).  The classification is
read off ``hs._graph``.  Adam's state is zeroed in place before every call, so
after it ``mu = (1-b1) g`` and ``nu = (1-b2) g^2`` of that call alone: a
gradient polluted by an earlier batch, by a replay that kept its old input or
by stale workspace bytes shows undiluted.  After every call the losses, the
codes and both moments are held against the float64 reference of that call's
batch under the bounds of test_hip_step_grads_gpu (``8 e32 + 16 U scale``,
``loss_depths`` at that call's B); the fired counts, read and zeroed as
``EnsembleResampler.observe`` does, equal the count of ``c > 0`` in the codes
just returned; BatchTopK's ``threshold_n`` counts the calls; ``staging`` is
"pre", "t" and "pre" again after calls 1, 5 and 9 of the "pre" rows.  After
call 12 every parameter is bit for bit what it was.

Rows: every shallow case at d, n = 68, 260 with B = 132, 37, 260 (132: a
multiple of 4, ragged against the 128-row tile; 37: odd, one partial tile; 260:
larger than anything allocated before); LISTA, residual-denoising and
semilinear at 20, 132 with B = 36, 17, 40; tied, topk and batch_topk also at
64, 128 with B = 128, 37, 256 (guard-free kernels, guarded ones in between);
tied, untied and masked tied under staging="pre" at 68, 132 with B = 132, 37,
136; topk and batch_topk under topk_chain="sparse" and HipMatryoshkaStep at
68, 260, where ``hits`` lives in the bytes of ``scores`` and ``gpre`` is
unspecified off the hits.

Worst ratio err / bound per case over its rows, calls, losses, codes, leaves
and both moments (1.0 is the bound; the module prints them with -s as
``[seq64]`` lines), measured on an MI355X; none of them was known before this
module ran there:

    case            worst err/bound     sparse chain    Matryoshka
    tied            0.163
    untied          0.200
    masked_tied     0.143
    masked_untied   0.184
    reverse         0.123
    centered        0.241
    whitened        0.136
    positive        0.140
    thresholding    0.254
    lista           0.185
    residual        0.161
    semilinear      0.133
    topk            0.149               0.124
    batch_topk      0.158               0.139           0.129

What this module found: k_enc_fwd's reverse epilogue counted a feature as
fired where its code was nonzero, and a reverse code ``pre * [pre + b > 0]`` is
negative where ``-b < pre < 0``.  ``fired`` exceeded the count of ``c > 0``,
which ``EnsembleResampler.observe`` uses on the torch backend and every other
epilogue counts, by exactly the number of negative codes: on every call, in
about half of the 520 columns, by up to 61 in a column, the same figures eager,
captured and replayed.  The two backends disagreed on which reverse features
are dead.  The epilogue now counts ``code > 0``; test_enc_fwd_reverse holds the
kernel to that.
"""

import pytest
import torch

from tests import step_reference as R
from tests.test_hip_step_grads_gpu import staging  # noqa: F401  (fixtures)
from tests.test_topk_sparse_chain_gpu import sparse_chain  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _to_dev(tree):
    return R.tree_apply(lambda t: t.to(DEV), tree)


def _zero_adam_state(st):
    """In place, leaf by leaf: the addresses a captured graph holds stay valid."""
    for tree in (st["mu"], st["nu"], st["step"]):
        for _, leaf in R.tree_items(tree):
            leaf.zero_()


@pytest.mark.parametrize("entry", R.SEQ_GRID, ids=[R.seq_id(e) for e in R.SEQ_GRID])
def test_step_sequence_matches_fp64_autograd(entry, request):
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.engine.resample import EnsembleResampler
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.matryoshka import MatryoshkaBatchTopKEncoder

    name, (d, n), Bs, variant = entry
    c = R.case(name)
    matryoshka = variant == "matryoshka"
    sig, step_class = (MatryoshkaBatchTopKEncoder, "HipMatryoshkaStep") if matryoshka else (c.sig, c.step_class)
    masked = (n, c.dict_sizes(n)) if c.dict_sizes else None
    # before touching the GPU: clean batches, and the references (cached, shared)
    refs, xs = {}, {}
    for key, (which, index) in R.SEQ_BATCHES.items():
        assert R.seq_decisions(name, (d, n), Bs[which], index)["near"] == 0, key
        refs[key] = R.seq_reference(name, (d, n), key, matryoshka)
        xs[key] = R.seq_x(name, (d, n), key)
    models = R.seq_models(name, (d, n), variant)
    if matryoshka:
        from tests.test_matryoshka_gpu import STEP_ENDS
        assert R.SEQ_GROUP_ENDS == STEP_ENDS[R.RAGGED]

    if variant == "pre":
        request.getfixturevalue("staging")("pre")
    elif variant == "sparse":
        request.getfixturevalue("sparse_chain")
    ens = FunctionalEnsemble([(_to_dev(p), _to_dev(b)) for p, b in models], sig, adam, {"lr": 0.0},
                             device=DEV, backend="hip")
    hs, st = ens._hip_step, ens.optim_states
    assert type(hs).__name__ == step_class
    captures = hs.captures_graph
    assert captures == (c.captures_graph or matryoshka)
    try:
        EnsembleResampler(ens)
        resampled = True
    except ValueError:  # no per-feature row to resample: nobody reads this step's fired counts
        resampled = False
    assert resampled == (name not in R.DEEP)
    params0 = R.tree_apply(lambda t: t.detach().cpu().clone(), ens.params)
    xg = {key: x.to(DEV) for key, x in xs.items()}

    worst, graph, fired_off = {}, None, []
    for call, (key, expect) in enumerate(R.SEQ_CALLS, start=1):
        ref, B = refs[key], xs[key].shape[0]
        tag = f"call {call} ({key}, B = {B}, {expect})"
        _zero_adam_state(st)
        losses, aux = ens.step_batch(xg[key])
        torch.cuda.synchronize()

        # ---- eager, captured or replayed -------------------------------------
        if not captures or expect == "eager":
            assert hs._graph is None, tag
        elif expect == "captured":
            assert hs._graph is not None and hs._graph is not graph, tag
        else:
            assert hs._graph is not None and hs._graph is graph, tag
        graph = hs._graph
        assert hs._B == B and aux["c"].shape == (2, B, n), tag
        if variant == "pre" and call in (1, 5, 9):
            assert hs.kc["staging"] == ("t" if B % 4 else "pre"), tag
        if variant == "sparse" or matryoshka:
            assert hs.kc["topk_chain"] == "sparse" and hs.hits.data_ptr() == hs.scores.data_ptr(), tag

        # ---- this call's batch against its own reference ----------------------
        try:
            got = {"loss": R.compare_losses(losses, ref, R.seq_loss_depths(entry, B))}
            assert set(got["loss"]) >= set(ref["loss64"]) - {"threshold"}, tag
            got["c"] = R.compare_codes(aux["c"], ref, masked[1] if masked else None)
            assert (st["step"] == 1).all(), tag
            got["mu"] = R.compare(st["mu"], ref["g64"], ref["g32"], "mu", 1, masked)
            got["nu"] = R.compare(st["nu"], ref["g64"], ref["g32"], "nu", 1, masked)
        except R.Mismatch as e:
            raise R.Mismatch(f"{tag}: {e}") from None
        for what, ratios in got.items():
            for leaf, ratio in ratios.items():
                worst[(what, leaf)] = max(worst.get((what, leaf), (0.0, 0)), (ratio, call))

        # ---- what the resampler reads, as observe() reads it -------------------
        if resampled:
            fired = hs.fired.clone()
            hs.fired.zero_()
            count = (aux["c"] > 0).sum(dim=1).to(fired.dtype)
            if not torch.equal(fired, count):  # asserted below, once the values of all twelve calls are through
                fired_off.append(f"{tag}: {int((fired != count).sum())} of {count.numel()} columns, fired - count "
                                 f"in [{(fired - count).min().item():.0f}, {(fired - count).max().item():.0f}]")
        if "threshold_n" in ens.buffers:
            assert (ens.buffers["threshold_n"] == call).all(), tag

    for (path, p0), (_, p) in zip(R.tree_items(params0), R.tree_items(ens.params)):
        p = p.detach().cpu()
        assert p.dtype == p0.dtype and torch.equal(p0.view(torch.int32), p.view(torch.int32)), \
            f"{path} moved at lr = 0"

    for (what, leaf), (ratio, call) in worst.items():
        print(f"[seq64] {R.seq_id(entry)} {what} {leaf} {ratio:.3f} (call {call})")
    print(f"[seq64] {R.seq_id(entry)} worst {max(r for r, _ in worst.values()):.3f}")
    assert not fired_off, "fired counts differ from the count of c > 0: " + "; ".join(fired_off)

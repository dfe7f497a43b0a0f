"""The batch-level top-k selection kernels and the fused BatchTopK step on
the GPU.  The kernel and the CPU reference get the same fp32 scores, so every
kernel comparison is exact (tests/batch_topk_reference.py): no tolerances."""

import pytest
import torch

from tests import batch_topk_reference as BR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24


def _ext():
    from sparse_coding_amd import ops

    return ops.get_extension()


def _rel_err(a, b):
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


class Select:
    """Device buffers of one launch shape, reused across calls: the same
    workspace is never zeroed by the test, only by the launcher."""

    def __init__(self, M, B, n, state=False, fill=0x5A5A5A5A):
        ext = _ext()
        self.ext, self.shape = ext, (M, B, n)
        self.c = torch.empty(M, B, n, device=DEV)
        self.fired = torch.zeros(M, n, device=DEV)
        self.thr = torch.empty(M, device=DEV)
        # stale garbage: the launcher must reset what it uses
        self.work = torch.full((ext.batch_topk_workspace_size(M),), fill, device=DEV, dtype=torch.int32)
        self.state = None
        if state:
            self.state = (torch.zeros(M, device=DEV), torch.zeros(M, device=DEV, dtype=torch.int32),
                          torch.full((M,), 0.01, device=DEV))

    def __call__(self, scores, ks, scores_dev=None):
        s = scores.to(DEV) if scores_dev is None else scores_dev
        self.c.fill_(float("nan"))
        self.fired.fill_(3.0)
        self.thr.fill_(float("nan"))
        self.ks = torch.tensor(ks, device=DEV, dtype=torch.int32)
        th, thn, thlr = self.state if self.state is not None else (None, None, None)
        self.ext.batch_topk_select(s, self.c, self.fired, self.ks, self.thr, self.work,
                                   threshold=th, threshold_n=thn, threshold_lr=thlr)
        return self.c.cpu(), self.fired.cpu() - 3.0, self.thr.cpu()


def _run(name, scores, ks, **kw):
    sel = Select(*scores.shape, **kw)
    c, fired, t = sel(scores, ks)
    BR.check_batch_topk(name, scores, c, fired, t, ks)
    return c, fired, t


def _distinct(M, B, n, seed):
    """Pairwise distinct scores, both signs, magnitudes over several binades."""
    gen = torch.Generator().manual_seed(seed)
    N = M * B * n
    mag = torch.linspace(0.01, 30.0, N, dtype=torch.float64)[torch.randperm(N, generator=gen)]
    sign = torch.where(torch.rand(N, generator=gen) < 0.5, -1.0, 1.0).double()
    s = (mag * sign).float().view(M, B, n)
    assert torch.unique(s).numel() == N
    return s


# (257, 1030): 264,710 scores per model over 65 blocks of 256 threads, so every
# thread makes three or more trips of its grid-stride loop (a block takes 1024
# scores per trip when it reads float4, 256 when not) and 65 blocks share each
# model: large enough as it is, the grid being one block per 4096 scores; B*n is
# no multiple of 4, so models 0 and 2 read float4 + a scalar tail and model 1,
# whose base is 8 bytes off, reads scalars.  (1, 67) is less than one block.
@pytest.mark.parametrize("B,n", [(1, 67), (5, 67), (64, 300), (257, 1030)])
def test_select_distinct(B, n):
    ks = (1, 5, 40)
    _run(f"distinct {B}x{n}", _distinct(3, B, n, seed=B + n), ks)


def test_select_k_zero_and_k_above_n():
    s = _distinct(3, 33, 70, seed=2)
    c, fired, t = _run("k edges", s, (0, 70, 1000))
    assert (c[0] == 0).all() and t[0] == float("inf") and (fired[0] == 0).all()
    for m in (1, 2):
        assert torch.equal(c[m] != 0, s[m] > 0) and t[m] == s[m].min()


def test_select_ties_across_blocks():
    """Five distinct positive values over 140,000 scores per model (35 blocks):
    thousands tie at t in every block; all are kept, more than K."""
    gen = torch.Generator().manual_seed(3)
    vals = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])
    s = vals[torch.randint(0, 5, (2, 200, 700), generator=gen)]
    ks = (100, 300)
    c, fired, t = _run("ties", s, ks)
    for m, k in enumerate(ks):
        assert (s[m] == t[m]).sum() > 500
        assert (c[m] > 0).sum() > k * 200


def test_select_fewer_positives_than_K():
    s = -_distinct(2, 40, 90, seed=4).abs()
    s[0, ::7, ::5] = s[0, ::7, ::5].abs()  # 6 x 18 = 108 positives, K = 10 * 40
    s[1, 3, 4] = 0.0
    c, fired, t = _run("few positives", s, (10, 10))
    assert t[0] <= 0 and torch.equal(c[0] != 0, s[0] > 0) and (c[0] != 0).sum() == 108
    # all negative (and one zero): nothing kept, t <= 0 so the statistic is 0
    assert (c[1] == 0).all() and t[1] <= 0


def test_select_specials():
    s = _distinct(2, 31, 65, seed=5)
    flat = s.view(2, -1)
    flat[:, 0:3] = float("inf")
    flat[:, 3:6] = float("-inf")
    flat[:, 6:40:2] = 0.0
    flat[:, 7:40:2] = -0.0
    flat[:, 40:50] = torch.tensor([1e-45, 3e-42, 1e-39, -1e-45, -1e-40, 5e-324, 1.1754942e-38, -1.1754942e-38,
                                   1.17549435e-38, 2e-45])
    flat[0, 50:90] = float("inf")
    # model 0, K = 31 of 43 infinities: t = +inf and every one of them is kept.
    # model 1, K just above the number of positives (35 zeros follow them): t
    # is a zero, and every positive, the denormals too, is kept
    n_pos = int((flat[1] > 0).sum())
    c, fired, t = _run("specials", s, (1, n_pos // 31 + 1))
    assert t[0] == float("inf") and (c[0] == float("inf")).sum() == 43 == (c[0] != 0).sum()
    assert (c[1] > 0).sum() == n_pos and t[1] == 0
    assert (c[1] > 0).view(-1)[[40, 41, 42, 49]].all()


def test_select_scale_skew():
    """Rows scaled by 1e-3 .. 1e3: a few rows own almost all of the top K."""
    s = _distinct(2, 96, 200, seed=6)
    scale = torch.logspace(-3, 3, 96)[torch.randperm(96, generator=torch.Generator().manual_seed(6))]
    s = s * scale[None, :, None]
    c, fired, t = _run("skew", s, (3, 20))
    rows = (c[1] > 0).sum(dim=1)
    assert (rows == 0).sum() > 30 and rows.max() > 60


def test_select_misaligned_base_matches_aligned():
    M, B, n = 2, 50, 104  # B*n % 4 == 0: every model reads float4 when aligned
    s = _distinct(M, B, n, seed=7)
    ks = (2, 9)
    want = _run("aligned", s, ks)
    buf = torch.empty(M * B * n + 1, device=DEV)
    view = buf[1:].view(M, B, n)
    view.copy_(s)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    sel = Select(M, B, n)
    got = sel(s, ks, scores_dev=view)
    BR.check_batch_topk("misaligned", s, *got, ks)
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    # misaligned output as well
    cbuf = torch.empty(M * B * n + 1, device=DEV)
    sel.c = cbuf[1:].view(M, B, n)
    BR.check_batch_topk("misaligned out", s, *sel(s, ks), ks)


def test_select_twice_on_one_workspace():
    sel = Select(3, 64, 300)
    ks = (1, 5, 40)
    for seed in (8, 9):
        s = _distinct(3, 64, 300, seed=seed)
        BR.check_batch_topk(f"call seed {seed}", s, *sel(s, ks), ks)
    # and with another k per model on the same buffers
    BR.check_batch_topk("call 3", s, *sel(s, (7, 0, 2)), (7, 0, 2))


def test_select_in_a_replayed_graph():
    M, B, n = 2, 64, 300
    ks = (3, 11)
    sel = Select(M, B, n, state=True)
    static = torch.zeros(M, B, n, device=DEV)
    warm = _distinct(M, B, n, seed=10)
    sel(warm, ks, scores_dev=static.copy_(warm))  # loads the kernels, sets sel.ks
    sel.state[0].zero_()
    sel.state[1].zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sel.ext.batch_topk_select(static, sel.c, sel.fired, sel.ks, sel.thr, sel.work,
                                  threshold=sel.state[0], threshold_n=sel.state[1], threshold_lr=sel.state[2])
    theta, count = 0.0, 0
    for i, seed in enumerate((11, 12, 13)):
        s = _distinct(M, B, n, seed=seed)
        static.copy_(s)
        sel.fired.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        BR.check_batch_topk(f"replay {i}", s, sel.c.cpu(), sel.fired.cpu() - 3.0, sel.thr.cpu(), ks)
        assert sel.state[1].tolist() == [i + 1, i + 1]


def test_threshold_state_update():
    M, B, n = 3, 16, 80
    sel = Select(M, B, n, state=True)
    sel.state[2].copy_(torch.tensor([0.01, 0.3, 0.9]))
    a = sel.state[2].cpu().double().tolist()  # the fp32 rates the kernel sees
    ks = (2, 5, 0)
    theta = [[0.0, 0] for _ in range(M)]
    bound = [0.0] * M
    for call in range(3):
        s = _distinct(M, B, n, seed=20 + call) + (call - 1.0)  # shifts t between calls
        c, fired, t = sel(s, ks)
        BR.check_batch_topk(f"call {call}", s, c, fired, t, ks)
        got, count = sel.state[0].cpu().double(), sel.state[1].cpu()
        for m in range(2):
            stat = max(float(t[m]), 0.0)
            prev = theta[m][0]
            theta[m] = list(BR.theta_ref(*theta[m], stat, a[m]))
            # error carried over shrinks by |1 - a| <= 1; this update adds two roundings
            bound[m] = bound[m] + 2 * U * max(abs(prev), abs(stat))
            assert abs(got[m].item() - theta[m][0]) <= bound[m], (call, m, got[m].item(), theta[m])
            assert count[m].item() == theta[m][1] == call + 1
        assert got[2].item() == 0.0 and count[2].item() == 0  # K == 0: untouched
    # the None branch leaves the state alone
    before = [t_.clone() for t_ in sel.state]
    sel.state, kept = None, sel.state
    sel(s, ks)
    for b, k in zip(before, kept):
        assert torch.equal(b, k)
    with pytest.raises(RuntimeError, match="go together"):
        sel.ext.batch_topk_select(s.to(DEV), sel.c, sel.fired, sel.ks, sel.thr, sel.work, threshold=kept[0])


# ---------------------------------------------------------------------------
# the fused step
# ---------------------------------------------------------------------------

def _clone_models(ens):
    return [({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in b.items()})
            for p, b in ens.unstack()]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "no_graph"])
def test_batch_topk_step_matches_torch(graph, monkeypatch):
    """Fused BatchTopK step vs the no_stacking torch backend, four steps (the
    graph is captured before the third and replayed from then on)."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.batch_topk import BatchTopKEncoder

    if graph:
        monkeypatch.delenv("SPARSE_CODING_AMD_NO_GRAPH", raising=False)
    else:
        monkeypatch.setenv("SPARSE_CODING_AMD_NO_GRAPH", "1")
    torch.manual_seed(11)
    M, B, d, n = 2, 256, 64, 128
    ks = (4, 16)
    models = [BatchTopKEncoder.init(d, n, k) for k in ks]
    ens_hip = FunctionalEnsemble(models, BatchTopKEncoder, adam, {"lr": 1e-3}, device=DEV, backend="hip")
    hs = ens_hip._hip_step
    assert type(hs).__name__ == "HipBatchTopKStep" and hs.use_graph is graph
    ens_ref = FunctionalEnsemble(_clone_models(ens_hip), BatchTopKEncoder, adam, {"lr": 1e-3},
                                 device=DEV, no_stacking=True, backend="torch")
    x = torch.randn(B, d, device=DEV)
    for i in range(4):
        l_hip, aux_hip = ens_hip.step_batch(x)
        l_ref, aux_ref = ens_ref.step_batch(x)
        assert _rel_err(l_hip["loss"], l_ref["loss"]) < 1e-4, i
        if i == 0:
            kept = aux_hip["c"] > 0
            assert kept.sum(dim=(1, 2)).tolist() == [k * B for k in ks]
            for m, k in enumerate(ks):
                assert not (kept[m].sum(dim=-1) == k).all()
            assert _rel_err(l_hip["threshold"], aux_ref["threshold"]) < 1e-5
    assert (hs._graph is not None) is graph
    assert _rel_err(ens_hip.params["dict"], ens_ref.params["dict"]) < 2e-3
    th_hip, th_ref = ens_hip.buffers["threshold"], ens_ref.buffers["threshold"]
    assert ((th_hip - th_ref).abs() <= 1e-4 * th_ref.abs()).all(), (th_hip, th_ref)
    assert ens_hip.buffers["threshold_n"].tolist() == ens_ref.buffers["threshold_n"].tolist() == [4, 4]


def test_step_follows_a_replaced_buffer_tree():
    """big_sweep's resume replaces ens.buffers: the captured graph is dropped,
    the new tensors are updated and the old ones are left alone."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.batch_topk import BatchTopKEncoder

    torch.manual_seed(12)
    ens = FunctionalEnsemble([BatchTopKEncoder.init(32, 64, k) for k in (2, 4)], BatchTopKEncoder, adam,
                             {"lr": 1e-3}, device=DEV, backend="hip")
    x = torch.randn(64, 32, device=DEV)
    for _ in range(3):
        ens.step_batch(x)
    assert ens._hip_step._graph is not None
    old = ens.buffers
    ens.buffers = {k: v.clone() for k, v in old.items()}
    ens.step_batch(x)
    ens.step_batch(x)
    torch.cuda.synchronize()
    assert old["threshold_n"].tolist() == [3, 3]
    assert ens.buffers["threshold_n"].tolist() == [5, 5]
    assert ens._hip_step._graph is not None


def test_batch_topk_resample():
    """EnsembleResampler on a BatchTopK ensemble (the TopK case of
    tests/test_full_stack_gpu.py at a small shape)."""
    from sparse_coding_amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding_amd.engine.resample import EnsembleResampler
    from sparse_coding_amd.functional.optim import adam
    from sparse_coding_amd.models.batch_topk import BatchTopKEncoder

    torch.manual_seed(3)
    d, n, B, M = 64, 1024, 128, 2
    ens = FunctionalEnsemble([BatchTopKEncoder.init(d, n, 4) for _ in range(M)], BatchTopKEncoder, adam,
                             {"lr": 1e-3}, device=DEV, backend="hip")
    rs = EnsembleResampler(ens, n_track=32)
    x = torch.randn(B, d, device=DEV)
    l0, aux = ens.step_batch(x)
    for _ in range(3):
        losses, aux = ens.step_batch(x)
        rs.observe(x, aux)
    assert torch.isfinite(losses["loss"]).all()
    assert (losses["loss"] <= l0["loss"]).all()
    # 3 steps x 512 kept entries over 1024 features leave some unfired
    counts = rs.resample()
    assert (counts > 0).all()

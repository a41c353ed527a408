"""Edge-valued aggregation (gnna_agg_edge_ld_f32, MODE_EDGE of the streaming kernel), edge softmax and the GAT layer built on
them, against fp64."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph, load_extension
from edge_softmax_ref import SOFTMAX_RTOL, _rows_of, _softmax64
from util import assert_close_f64

pytestmark = pytest.mark.gpu
GNNA = load_extension()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _agg64(X, w, rp, ci):
    """fp64 A_w X and its magnitude scale |A_w| |X| (on X's device)."""
    rows, cl = _rows_of(rp.to(X.device)), ci.to(X.device).long()
    Xd, wd = X.double(), w.to(X.device).double()
    ref = torch.zeros(rp.numel() - 1, X.shape[1], dtype=torch.float64, device=X.device)
    scale = torch.zeros_like(ref)
    for c0 in range(0, cl.numel(), 1 << 22):
        sl = slice(c0, c0 + (1 << 22))
        ref.index_add_(0, rows[sl], wd[sl, None] * Xd[cl[sl]])
        scale.index_add_(0, rows[sl], wd[sl, None].abs() * Xd[cl[sl]].abs())
    return ref, scale


def _graph(kind, seed, n=3000, nnz=120000):
    if kind == "powerlaw":
        return graph.powerlaw_graph(n, nnz, 900, seed=seed)
    return graph.uniform_graph(n, nnz, seed=seed)


def _weights(kind, nnz, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.rand(nnz, generator=gen) * 2.0
    if kind == "negative":
        return -torch.rand(nnz, generator=gen) - 0.1
    if kind == "zero":
        w = torch.randn(nnz, generator=gen)
        w[torch.rand(nnz, generator=gen) < 0.5] = 0.0
        return w
    return torch.ones(nnz)


_WKINDS = ("random", "negative", "zero", "ones")


@pytest.mark.parametrize("kind", ["powerlaw", "uniform"])
@pytest.mark.parametrize("partSize", [1, 2, 16, 32, 64])
@pytest.mark.parametrize("dim", [1, 3, 4, 16, 17, 32, 41, 64, 100, 128, 256])
def test_weighted_aggregation_matches_fp64(kind, partSize, dim):
    g = _graph(kind, seed=dim + partSize, n=1500, nnz=40000)
    pp, p2n = [t.cuda() for t in _lib.build_part(partSize, g.row_pointers)]
    ci = g.column_index.cuda()
    X = torch.randn(g.num_nodes, dim, generator=torch.Generator().manual_seed(dim)).cuda()
    wk = _WKINDS[(dim + partSize + (kind == "uniform")) % 4]
    w = _weights(wk, ci.numel(), seed=partSize).cuda()
    Y = GNNA.aggregate_edge(X, ci, w, pp, p2n, partSize)
    ref, scale = _agg64(X, w, g.row_pointers, ci)
    assert_close_f64(Y.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(),
                     what=f"{kind} D={dim} ps={partSize} w={wk}")


@pytest.mark.parametrize("wk", _WKINDS)
@pytest.mark.parametrize("phases", [1, 4])
def test_weight_kinds_and_phases(wk, phases):
    g = _graph("powerlaw", seed=5, n=6000, nnz=400000)
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    ci = g.column_index.cuda()
    X = torch.randn(g.num_nodes, 64, generator=torch.Generator().manual_seed(1)).cuda()
    w = _weights(wk, ci.numel(), seed=3).cuda()
    try:
        _lib.set_tuning(column_phases=phases)
        Y = GNNA.aggregate_edge(X, ci, w, pp, p2n, 32)
    finally:
        _lib.reset_tuning()
    ref, scale = _agg64(X, w, g.row_pointers, ci)
    assert_close_f64(Y.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what=f"w={wk} phases={phases}")


@pytest.mark.parametrize("dim", [16, 41, 64])
def test_leading_dimensions_accumulate_relu(dim):
    """Gapped input ld, a column block of a wider matrix, output into a slice; ACCUMULATE and RELU; the floats around the
    views are never touched."""
    g = _graph("powerlaw", seed=11, n=2500, nnz=150000)
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    ci = g.column_index.cuda()
    n = g.num_nodes
    gen = torch.Generator().manual_seed(dim)
    w = (torch.randn(ci.numel(), generator=gen)).cuda()
    wide = torch.randn(n, 3 * dim + 8, generator=gen).cuda()
    for X in (wide[:, dim:2 * dim],                                           # column block of a wider matrix
              torch.full((n, 128 + dim), 7.5, device="cuda")[:, :dim].copy_(wide[:, :dim])):   # gapped rows
        ref, scale = _agg64(X, w, g.row_pointers, ci)
        obuf = torch.full((n, 2 * dim + 4), -3.25, device="cuda")
        out = obuf[:, dim + 4:]                                               # output into a slice
        GNNA.aggregate_edge(X, ci, w, pp, p2n, 32, out=out)
        assert_close_f64(out.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what="ld")
        assert (obuf[:, :dim + 4] == -3.25).all()
        base = torch.randn(n, dim, generator=gen).cuda()
        out.copy_(base)
        GNNA.aggregate_edge(X, ci, w, pp, p2n, 32, out=out, accumulate=True, relu=True)
        want = torch.clamp(ref + base.double(), min=0)
        assert_close_f64(out.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, scale=(scale + base.double().abs()).cpu().numpy(),
                         what="accumulate + relu")
        Yr = GNNA.aggregate_edge(X, ci, w, pp, p2n, 32, relu=True)
        assert_close_f64(Yr.cpu().numpy(), torch.clamp(ref, min=0).cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(),
                         what="relu")
        assert (obuf[:, :dim + 4] == -3.25).all()


@pytest.mark.parametrize("phases", [1, 2, 8, 32])
@pytest.mark.parametrize("det", [0, 1])
def test_integer_kat_exact(phases, det):
    """Integer features and weights: every partial sum is exact in fp32, so any schedule must give the exact value."""
    g = _graph("powerlaw", seed=17, n=8000, nnz=600000)
    pp, p2n = [t.cuda() for t in _lib.build_part(16, g.row_pointers)]
    ci = g.column_index.cuda()
    gen = torch.Generator().manual_seed(phases)
    X = torch.randint(-8, 9, (g.num_nodes, 64), generator=gen).float().cuda()
    w = torch.randint(-4, 5, (ci.numel(),), generator=gen).float().cuda()
    ref, _ = _agg64(X, w, g.row_pointers, ci)
    try:
        _lib.set_tuning(column_phases=phases, deterministic=det)
        Y1 = GNNA.aggregate_edge(X, ci, w, pp, p2n, 16)
        Y2 = GNNA.aggregate_edge(X, ci, w, pp, p2n, 16)
    finally:
        _lib.reset_tuning()
    assert torch.equal(Y1.double(), ref), f"phases={phases} det={det}: not exact"
    if det:
        assert torch.equal(Y1, Y2)


@pytest.mark.parametrize("dim", [16, 64])
def test_prepared_graph_reads_weights_at_original_positions(dim):
    """w[e] = e % 7 + 1 on a prepared graph with >= 2 phases: a weight read at the packed copy's position instead of the edge's
    original one would be off.  The calls neither synchronise, free nor allocate, and they read the packed ids."""
    g = graph.powerlaw_graph(20000, 2000000, 3000, seed=dim, device="cuda")
    n = g.num_nodes
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers.cpu())]
    ci = g.column_index
    w = (torch.arange(ci.numel(), device="cuda") % 7 + 1).float()
    X = torch.randn(n, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    ref, scale = _agg64(X, w, g.row_pointers, ci)
    try:
        _lib.set_tuning(column_phases=4)
        _lib.prepare_graph(ci, pp, p2n, n, n, 32, [dim])
        torch.cuda.synchronize()
        before = _lib.runtime_counters()
        for _ in range(3):
            Y = GNNA.aggregate_edge(X, ci, w, pp, p2n, 32)
        torch.cuda.synchronize()
        after = _lib.runtime_counters()
    finally:
        _lib.reset_tuning()
        _lib.release_graph(ci)
    for k in ("launch_syncs", "launch_frees", "launch_mallocs"):
        assert after[k] == before[k], k
    assert after["packed_launches"] > before["packed_launches"], "the weighted call must read the packed ids"
    assert_close_f64(Y.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what=f"prepared D={dim}")


def test_weighted_call_in_a_captured_graph():
    g = _graph("powerlaw", seed=23, n=6000, nnz=500000)
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    ci = g.column_index.cuda()
    gen = torch.Generator().manual_seed(4)
    X = torch.randn(g.num_nodes, 64, generator=gen).cuda()
    w = torch.rand(ci.numel(), generator=gen).cuda()
    w2 = torch.randn(ci.numel(), generator=gen).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        GNNA.aggregate_edge(X, ci, w, pp, p2n, 32)        # warm-up (plans, scratch)
    side.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        Y = GNNA.aggregate_edge(X, ci, w, pp, p2n, 32)
    w.copy_(w2)                                            # new weights, same storage
    gr.replay()
    torch.cuda.synchronize()
    ref, scale = _agg64(X, w2, g.row_pointers, ci)
    assert_close_f64(Y.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what="captured replay")


# ---- edge softmax -------------------------------------------------------------------------------------------------------

def _softmax_graph(seed, hub=120000):
    """Empty rows, degree-1 rows, short and medium rows and one hub row of `hub` edges (unsymmetric: not needed here)."""
    gen = np.random.default_rng(seed)
    n = 5000
    deg = gen.integers(0, 40, n)
    deg[gen.random(n) < 0.2] = 0
    deg[gen.random(n) < 0.2] = 1
    deg[::97] = gen.integers(300, 5000, deg[::97].size)
    deg[1234] = hub
    rp = np.r_[0, np.cumsum(deg)].astype(np.int32)
    ci = gen.integers(0, n, rp[-1]).astype(np.int32)
    return torch.from_numpy(rp), torch.from_numpy(ci)


@pytest.mark.parametrize("heads", [1, 4])
def test_edge_softmax_forward_backward(heads):
    rp, _ci = _softmax_graph(heads)
    rpd = rp.cuda()
    nnz = int(rp[-1])
    gen = torch.Generator(device="cuda").manual_seed(heads)
    s = (torch.rand(heads, nnz, device="cuda", generator=gen) * 160.0 - 80.0)     # magnitudes up to 80
    dp = torch.randn(heads, nnz, device="cuda", generator=gen)
    sc = s[0] if heads == 1 else s
    p = GNNA.edge_softmax(sc, rpd)
    p_again = GNNA.edge_softmax(sc, rpd)
    assert torch.equal(p, p_again), "edge softmax must be bit-reproducible"
    ref = _softmax64(s, rpd)
    assert_close_f64(p.view(heads, nnz).cpu().numpy(), ref.cpu().numpy(), rtol=SOFTMAX_RTOL, what=f"softmax heads={heads}")
    dpc = dp[0] if heads == 1 else dp
    ds = GNNA.edge_softmax_backward(p, dpc, rpd)
    assert torch.equal(ds, GNNA.edge_softmax_backward(p, dpc, rpd))
    rows = _rows_of(rpd)
    pd = p.view(heads, nnz).double()
    dot = torch.zeros(heads, rp.numel() - 1, dtype=torch.float64, device="cuda").index_add_(1, rows, pd * dp.double())
    ref_ds = pd * (dp.double() - dot[:, rows])
    adot = torch.zeros_like(dot).index_add_(1, rows, pd * dp.double().abs())
    scale = pd * (dp.double().abs() + adot[:, rows])
    assert_close_f64(ds.view(heads, nnz).cpu().numpy(), ref_ds.cpu().numpy(), rtol=SOFTMAX_RTOL, scale=scale.cpu().numpy(),
                     what=f"softmax backward heads={heads}")


@pytest.mark.parametrize("avg", [2, 20, 300])
def test_edge_softmax_across_segment_widths(avg):
    """The lanes per row follow the average degree (4 .. 64): graphs whose averages pick different widths."""
    gen = np.random.default_rng(avg)
    n = 4000
    deg = gen.poisson(avg, n)
    deg[7] = 70000
    rp = torch.from_numpy(np.r_[0, np.cumsum(deg)].astype(np.int32)).cuda()
    nnz = int(rp[-1])
    s = torch.randn(2, nnz, device="cuda") * 10
    p = GNNA.edge_softmax(s, rp)
    assert_close_f64(p.cpu().numpy(), _softmax64(s, rp).cpu().numpy(), rtol=1e-5, what=f"avg degree {avg}")


# ---- GAT --------------------------------------------------------------------------------------------------------------

class _Info:
    """The slice of decider.inputProperty the edge ops read."""

    def __init__(self, g, partSize=32):
        from gnnadvisor_osdi21_amd.decider import inputProperty
        self.row_pointers, self.column_index = g.row_pointers.cuda(), g.column_index.cuda()
        self.partSize = partSize
        self.partPtr, self.part2Node = [t.cuda() for t in _lib.build_part(partSize, g.row_pointers.cpu())]
        self._edge_arrays = lambda: inputProperty._edge_arrays(self)
        self.reverse_edges = lambda: inputProperty.reverse_edges(self)
        self.edge_rows = lambda: inputProperty.edge_rows(self)


def _gat64(X, W, al, ar, rp, ci, heads, out_dim, concat, slope=0.2):
    """fp64 GAT layer from plain torch ops (autograd gives the reference gradients)."""
    rows, cl = _rows_of(rp), ci.long()
    n = X.shape[0]
    H = (X @ W).view(n, heads, out_dim)
    el, er = (H * al).sum(-1), (H * ar).sum(-1)
    s = torch.nn.functional.leaky_relu(el[rows] + er[cl], slope).t()                      # [heads, nnz]
    m = torch.full((heads, n), -float("inf"), dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(1, rows.expand_as(s), s.detach(), reduce="amax")
    ex = torch.exp(s - m[:, rows])
    den = torch.zeros(heads, n, dtype=s.dtype, device=s.device).index_add(1, rows, ex)
    alpha = ex / den[:, rows]
    Y = torch.zeros(n, heads, out_dim, dtype=s.dtype, device=s.device).index_add(0, rows, alpha.t()[:, :, None] * H[cl])
    return Y.reshape(n, heads * out_dim) if concat or heads == 1 else Y.mean(1)


def _gat_check(g, heads, concat, in_dim, out_dim, seed, sample=None):
    from gnnadvisor_osdi21_amd.ops import GATConv
    info = _Info(g)
    torch.manual_seed(seed)
    conv = GATConv(in_dim, out_dim, heads=heads, concat=concat).cuda()
    X = torch.randn(g.num_nodes, in_dim, device="cuda", requires_grad=True)
    Y = conv(X, info)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    Y64 = _gat64(X64, *P64, info.row_pointers, info.column_index, heads, out_dim, concat)
    (Y64 * wgt.double()).sum().backward()
    idx = slice(None) if sample is None else sample
    what = f"GAT heads={heads} concat={concat}"
    for got, ref, name in ((Y, Y64, "Y"), (X.grad, X64.grad, "dX")):
        r = ref.detach()[idx]
        assert_close_f64(got.detach()[idx].cpu().numpy(), r.cpu().numpy(), rtol=1e-4,
                         scale=np.full(r.shape, float(r.abs().max())), what=f"{what} {name}")
    for got, ref, name in zip((conv.weights.grad, conv.att_l.grad, conv.att_r.grad), P64, ("dW", "da_l", "da_r")):
        r = ref.grad
        assert_close_f64(got.cpu().numpy(), r.cpu().numpy(), rtol=1e-4, scale=np.full(r.shape, float(r.abs().max())),
                         what=f"{what} {name}")


@pytest.mark.parametrize("heads,concat", [(1, True), (4, True), (4, False)])
def test_gatconv_matches_fp64_gat(heads, concat):
    g = graph.powerlaw_graph(2000, 40000, 400, seed=31)
    _gat_check(g, heads, concat, in_dim=48, out_dim=16, seed=heads)


def test_edge_weighted_aggregate_gradients():
    from gnnadvisor_osdi21_amd.ops import EdgeWeightedAggregate
    g = graph.powerlaw_graph(2000, 60000, 500, seed=37)
    info = _Info(g)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for heads, F in ((1, 24), (3, 8), (2, 3)):
        X = torch.randn(g.num_nodes, heads * F, device="cuda", generator=gen, requires_grad=True)
        w = torch.randn(heads, info.column_index.numel(), device="cuda", generator=gen, requires_grad=True)
        Y = EdgeWeightedAggregate.apply(X, w if heads > 1 else w[0], info)
        wgt = torch.randn(Y.shape, device="cuda", generator=gen)
        (Y * wgt).sum().backward()
        X64, w64 = X.detach().double().requires_grad_(), w.detach().double().requires_grad_()
        rows, cl = _rows_of(info.row_pointers), info.column_index.long()
        Y64 = torch.zeros(g.num_nodes, heads, F, dtype=torch.float64, device="cuda").index_add(
            0, rows, w64.t()[:, :, None] * X64.view(-1, heads, F)[cl]).view(g.num_nodes, heads * F)
        (Y64 * wgt.double()).sum().backward()
        for got, ref, name in ((Y.detach(), Y64.detach(), "Y"), (X.grad, X64.grad, "dX"), (w.grad, w64.grad, "dw")):
            assert_close_f64(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4,
                             scale=np.full(ref.shape, float(ref.abs().max())), what=f"heads={heads} F={F} {name}")


# ---- full size -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reddit():
    return graph.make_config_graph("reddit-like", device="cuda")


def test_reddit_like_weighted_aggregation(reddit):
    g = reddit
    n = g.num_nodes
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers.cpu())]
    ci = g.column_index
    gen = torch.Generator(device="cuda").manual_seed(8)
    X = torch.randn(n, 64, device="cuda", generator=gen)
    w = torch.rand(ci.numel(), device="cuda", generator=gen)
    Y = GNNA.aggregate_edge(X, ci, w, pp, p2n, 32)
    sample = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:256]
    rp = g.row_pointers.long()
    for r in sample.tolist():
        b, e = int(rp[r]), int(rp[r + 1])
        ref = (w[b:e].double()[:, None] * X[ci[b:e].long()].double()).sum(0)
        scale = (w[b:e].double()[:, None] * X[ci[b:e].long()].double().abs()).sum(0)
        assert_close_f64(Y[r].cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what=f"row {r}")


def _gat64_chunked(X, W, al, ar, rp, ci, G, slope=0.2, chunk=1 << 22):
    """One-head fp64 GAT layer and the gradients of sum(Y * G), written out by hand and chunked over the edges (the autograd
    form holds [nnz, D] fp64 temporaries: 59 GB at Reddit-like size)."""
    rows, cl = _rows_of(rp), ci.long()
    n, nnz = X.shape[0], cl.numel()
    H = X @ W
    el, er = H @ al, H @ ar
    z = el[rows] + er[cl]
    s = torch.nn.functional.leaky_relu(z, slope)
    m = torch.full((n,), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, rows, s, reduce="amax")
    ex = torch.exp(s - m[rows])
    alpha = ex / torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, rows, ex)[rows]
    Y = torch.zeros_like(H)
    dH = torch.zeros_like(H)
    dalpha = torch.empty_like(alpha)
    for c0 in range(0, nnz, chunk):
        r, c, a = rows[c0:c0 + chunk], cl[c0:c0 + chunk], alpha[c0:c0 + chunk]
        Y.index_add_(0, r, a[:, None] * H[c])
        dH.index_add_(0, c, a[:, None] * G[r])
        dalpha[c0:c0 + chunk] = (G[r] * H[c]).sum(1)
    dot = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, rows, alpha * dalpha)
    dz = alpha * (dalpha - dot[rows]) * torch.where(z > 0, 1.0, slope).to(s.dtype)
    d_el = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, rows, dz)
    d_er = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, cl, dz)
    dH += d_el[:, None] * al[None, :] + d_er[:, None] * ar[None, :]
    # (the parameter gradients are sums over all nodes: their fp32 error scales with the sum of |terms|)
    scales = (X.abs().t() @ dH.abs(), H.abs().t() @ d_el.abs(), H.abs().t() @ d_er.abs())
    return (Y, dH @ W.t(), X.t() @ dH, H.t() @ d_el, H.t() @ d_er), scales


def test_reddit_like_gat_layer(reddit):
    """One GAT layer (D = 64, one head) forward and backward at full size: 256 sampled rows of Y and dX, all of dW, da_l, da_r."""
    from gnnadvisor_osdi21_amd.ops import GATConv
    g = reddit
    info = _Info(g)
    torch.manual_seed(3)
    conv = GATConv(64, 64).cuda()
    X = torch.randn(g.num_nodes, 64, device="cuda", requires_grad=True)
    Y = conv(X, info)
    G = torch.randn(Y.shape, device="cuda")
    (Y * G).sum().backward()
    refs, sums = _gat64_chunked(X.detach().double(), conv.weights.detach().double(), conv.att_l.detach()[0].double(),
                          conv.att_r.detach()[0].double(), info.row_pointers, info.column_index, G.double())
    sample = torch.randperm(g.num_nodes, generator=torch.Generator().manual_seed(2))[:256].cuda()
    gots = (Y.detach()[sample], X.grad[sample], conv.weights.grad, conv.att_l.grad[0], conv.att_r.grad[0])
    refs = (refs[0][sample], refs[1][sample]) + refs[2:]
    for i, (got, ref, name) in enumerate(zip(gots, refs, ("Y", "dX", "dW", "da_l", "da_r"))):
        scale = np.full(ref.shape, float(ref.abs().max())) if i < 2 else sums[i - 2].cpu().numpy()
        assert_close_f64(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=scale, what=f"Reddit-like GAT {name}")


# ---- driver -----------------------------------------------------------------------------------------------------------

def test_driver_gat_trains():
    res = subprocess.run([sys.executable, "-m", "gnnadvisor_osdi21_amd.main", "--model", "gat", "--heads", "2",
                          "--synthetic", "amazon0505-like", "--scale", "0.05", "--num_epoches", "20", "--verbose_mode", "True"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "Time (ms):" in res.stdout
    first = float(re.search(r"# first loss: ([-\d.e+]+)", res.stdout).group(1))
    final = float(re.search(r"# final loss: ([-\d.e+]+)", res.stdout).group(1))
    assert final < first, (first, final)


def test_driver_gat_refuses_hip_graph():
    res = subprocess.run([sys.executable, "-m", "gnnadvisor_osdi21_amd.main", "--model", "gat", "--hip_graph", "True",
                          "--synthetic", "cora-like", "--num_epoches", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "does not support --hip_graph True" in res.stderr

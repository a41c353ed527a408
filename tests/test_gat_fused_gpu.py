"""Fused multi-head GAT attention (gnna_gat_forward_f32 / gnna_gat_backward_f32, ops.GATAttention, GATConv(fused=True),
main.py --fused_attention) against the fp64 formula.  The yardstick is always fp64 torch, never the fused code itself and
never the composed fp32 path (which appears once, as a cross-check and as the thing whose memory the fused path must not need).

Tolerances: rtol 1e-5 of max(1, sum of |terms|) for a single kernel's output, 1e-4 of max|ref| for layer outputs and input
gradients, 1e-4 of the sum-of-|terms| scale for parameter gradients -- the ones of test_edge_attention_gpu.py.  The terms of
d_el / d_er: dz = alpha (dalpha - c) with dalpha = sum_f G H and c = sum_e alpha dalpha, so an edge contributes
alpha (sum_f |G| |H| + sum_e alpha sum_f |G| |H|) to the magnitude sum of the row it feeds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph, load_extension
from test_edge_attention_gpu import _Info, _gat64, _gat64_chunked, _rows_of
from util import assert_close_f64

pytestmark = pytest.mark.gpu
GNNA = load_extension()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _att64(H, el, er, rp, ci, heads, slope):
    """fp64 attention from plain torch ops on (H, el, er) -> (Y [n, heads * dim], lse [n, heads], has_edges [n], sum of |terms|
    of Y).  Differentiable in H, el, er."""
    rows, cl = _rows_of(rp), ci.long()
    n = H.shape[0]
    dim = H.shape[1] // heads
    Hh = H.view(n, heads, dim)
    s = torch.nn.functional.leaky_relu(el[rows] + er[cl], slope)                  # [nnz, heads]
    m = torch.full((n, heads), -float("inf"), dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax")
    ex = torch.exp(s - m[rows])
    den = torch.zeros(n, heads, dtype=s.dtype, device=s.device).index_add(0, rows, ex)
    alpha = ex / den[rows]
    Y = torch.zeros(n, heads, dim, dtype=s.dtype, device=s.device).index_add(0, rows, alpha[:, :, None] * Hh[cl])
    scale = torch.zeros(n, heads, dim, dtype=s.dtype, device=s.device).index_add(
        0, rows, (alpha[:, :, None] * Hh[cl].abs()).detach())
    has = (rp[1:] > rp[:-1])
    lse = torch.where(has[:, None], m + torch.log(den.detach().clamp(min=1e-300)), torch.zeros_like(m))
    return Y.reshape(n, heads * dim), lse, has, scale.reshape(n, heads * dim)


def _graph(kind, seed, n=1500, nnz=40000):
    if kind == "powerlaw":
        return graph.powerlaw_graph(n, nnz, 900, seed=seed)
    return graph.uniform_graph(n, nnz, seed=seed)


def _inputs(n, heads, dim, seed, magnitude=1.0):
    gen = torch.Generator().manual_seed(seed)
    H = torch.randn(n, heads * dim, generator=gen).cuda()
    el = (torch.randn(n, heads, generator=gen) * magnitude).cuda()
    er = (torch.randn(n, heads, generator=gen) * magnitude).cuda()
    return H, el, er


def _check_forward(g, heads, dim, partSize, seed, what, magnitude=1.0, y_rtol=1e-5, slope=0.2):
    rp, ci = g.row_pointers.cuda(), g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(partSize, g.row_pointers.cpu())]
    H, el, er = _inputs(g.num_nodes, heads, dim, seed, magnitude)
    Y, lse = GNNA.gat_forward(H, el, er, rp, ci, pp, p2n, partSize, slope)
    _Y2, lse2 = GNNA.gat_forward(H, el, er, rp, ci, pp, p2n, partSize, slope)
    assert torch.equal(lse, lse2), f"{what}: lse must be bit-reproducible"
    Y64, lse64, has, scale = _att64(H.double(), el.double(), er.double(), rp, ci, heads, slope)
    assert torch.isfinite(Y).all() and torch.isfinite(lse).all(), f"{what}: non-finite output"
    assert_close_f64(Y.cpu().numpy(), Y64.cpu().numpy(), rtol=y_rtol, scale=scale.cpu().numpy(), what=f"{what} Y")
    assert_close_f64(lse[has].cpu().numpy(), lse64[has].cpu().numpy(), rtol=1e-5, what=f"{what} lse")
    assert (Y[~has] == 0).all() and (lse[~has] == 0).all(), f"{what}: rows without edges must give Y = 0, lse = 0"


@pytest.mark.parametrize("kind", ["powerlaw", "uniform"])
@pytest.mark.parametrize("partSize", [1, 16, 32])
@pytest.mark.parametrize("dim", [1, 3, 4, 8, 16, 41, 64])
@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_gat_forward_matches_fp64(kind, partSize, dim, heads):
    g = _graph(kind, seed=dim + partSize + heads)
    _check_forward(g, heads, dim, partSize, seed=dim * 10 + heads, what=f"{kind} heads={heads} dim={dim} ps={partSize}")


@pytest.mark.parametrize("heads,dim", [(1, 64), (4, 16), (8, 3)])
def test_gat_forward_scores_of_magnitude_80(heads, dim):
    """el, er ~ N(0, 1) * 80: the row maximum is subtracted, nothing overflows.  Y at rtol 1e-4: rounding el + er to fp32 near 80
    is 3.8e-6 per score and enters alpha twice (through the score and through lse); the reference starts from the same fp32
    el and er."""
    g = _graph("powerlaw", seed=heads)
    _check_forward(g, heads, dim, 32, seed=heads, what=f"magnitude 80 heads={heads} dim={dim}", magnitude=80.0, y_rtol=1e-4)


def _special_graph(seed, n=3000, nnz=40000, empty=40, loops=200):
    """A symmetric graph with rows without edges (the last `empty` nodes), self loops and a hub (node 0, joined to every
    other node with edges: its row is longer than any long-row threshold of the lse pass, 64 lanes x 4 x 8 = 2048 edges)."""
    g = graph.powerlaw_graph(n, nnz, 400, seed=seed)
    rp, ci = g.row_pointers.long(), g.column_index.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    others = torch.arange(1, n)
    hub = torch.zeros(n - 1, dtype=torch.long)
    loop = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:loops]
    r = torch.cat([rows, hub, others, loop])
    c = torch.cat([ci, others, hub, loop])
    key = torch.unique(r * (n + empty) + c)                      # sorted, duplicates merged
    r, c = key // (n + empty), key % (n + empty)
    counts = torch.bincount(r, minlength=n + empty)
    new_rp = torch.zeros(n + empty + 1, dtype=torch.int32)
    new_rp[1:] = torch.cumsum(counts, 0).int()

    class G:
        pass
    out = G()
    out.row_pointers, out.column_index, out.num_nodes = new_rp, c.int(), n + empty
    assert int(counts[0]) > 2048 and int((counts == 0).sum()) >= empty and int((r == c).sum()) >= loops
    return out


def _backward_case(g, heads, dim, partSize, slope, seed, what):
    rp, ci = g.row_pointers.cuda(), g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(partSize, g.row_pointers.cpu())]
    n = g.num_nodes
    H, el, er = _inputs(n, heads, dim, seed)
    G = torch.randn(n, heads * dim, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    Y, lse = GNNA.gat_forward(H, el, er, rp, ci, pp, p2n, partSize, slope)
    dH, d_el, d_er = GNNA.gat_backward(H, el, er, lse, Y, G, rp, ci, pp, p2n, partSize, slope)
    H64, el64, er64 = [t.double().requires_grad_() for t in (H, el, er)]
    Y64, _lse, _has, _scale = _att64(H64, el64, er64, rp, ci, heads, slope)
    (Y64 * G.double()).sum().backward()
    # magnitude sums (module docstring)
    rows, cl = _rows_of(rp), ci.long()
    with torch.no_grad():
        Hh, Gh = H.double().view(n, heads, dim), G.double().view(n, heads, dim)
        z = el.double()[rows] + er.double()[cl]
        s = torch.nn.functional.leaky_relu(z, slope)
        alpha = torch.exp(s - _lse[rows])
        absdot = (Gh[rows].abs() * Hh[cl].abs()).sum(-1)                             # [nnz, heads]
        crow = torch.zeros(n, heads, dtype=torch.float64, device="cuda").index_add_(0, rows, alpha * absdot)
        term = alpha * (absdot + crow[rows])
        s_el = torch.zeros_like(crow).index_add_(0, rows, term)
        s_er = torch.zeros_like(crow).index_add_(0, cl, term)
        s_dH = torch.zeros(n, heads, dim, dtype=torch.float64, device="cuda").index_add_(
            0, cl, alpha[:, :, None] * Gh[rows].abs()).view(n, heads * dim)
        # the kink of leaky_relu: |z| <= 1e-6 may fall on either side in fp32; the rows such an edge feeds are left out
        kink = (z.abs() <= 1e-6) if slope != 1.0 else torch.zeros_like(z, dtype=torch.bool)
        excluded = int(kink.any(1).sum())
        assert excluded < 1e-3 * max(1, cl.numel()), f"{what}: {excluded} edges at the kink"
        ok_el = torch.ones(n, heads, dtype=torch.bool, device="cuda")
        ok_er = torch.ones(n, heads, dtype=torch.bool, device="cuda")
        if excluded:
            e, h = kink.nonzero(as_tuple=True)
            ok_el[rows[e], h] = False
            ok_er[cl[e], h] = False
    assert torch.isfinite(dH).all() and torch.isfinite(d_el).all() and torch.isfinite(d_er).all(), f"{what}: non-finite gradient"
    assert_close_f64(dH.cpu().numpy(), H64.grad.cpu().numpy(), rtol=1e-5, scale=s_dH.cpu().numpy(), what=f"{what} dH")
    assert_close_f64(d_el[ok_el].cpu().numpy(), el64.grad[ok_el].cpu().numpy(), rtol=1e-5, scale=s_el[ok_el].cpu().numpy(),
                     what=f"{what} d_el")
    assert_close_f64(d_er[ok_er].cpu().numpy(), er64.grad[ok_er].cpu().numpy(), rtol=1e-5, scale=s_er[ok_er].cpu().numpy(),
                     what=f"{what} d_er")
    empty = (rp[1:] == rp[:-1])
    assert (d_el[empty] == 0).all() and (d_er[empty] == 0).all() and (dH[empty] == 0).all()


# every heads and every dim of the forward grid at least once, three partition sizes, both graph kinds
_BWD_GRID = [(1, 64, 32, "powerlaw"), (2, 41, 16, "uniform"), (4, 16, 32, "powerlaw"), (8, 8, 1, "uniform"), (8, 64, 32, "powerlaw"),
             (1, 1, 16, "powerlaw"), (2, 3, 32, "uniform"), (4, 4, 1, "powerlaw"), (3, 8, 32, "uniform"), (16, 4, 16, "powerlaw")]


@pytest.mark.parametrize("heads,dim,partSize,kind", _BWD_GRID)
def test_gat_backward_matches_fp64_autograd(heads, dim, partSize, kind):
    g = _graph(kind, seed=heads * 100 + dim)
    _backward_case(g, heads, dim, partSize, 0.2, seed=heads + dim, what=f"{kind} heads={heads} dim={dim} ps={partSize}")


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
@pytest.mark.parametrize("heads,dim", [(1, 64), (4, 16), (2, 3)])
def test_gat_backward_empty_rows_hub_self_loops_and_slopes(heads, dim, slope):
    g = _special_graph(seed=heads)
    _backward_case(g, heads, dim, 32, slope, seed=7 * heads + dim, what=f"special heads={heads} dim={dim} slope={slope}")
    _check_forward(g, heads, dim, 32, seed=heads, what=f"special forward heads={heads} dim={dim} slope={slope}", slope=slope)


@pytest.mark.parametrize("heads,dim", [(1, 16), (2, 41), (4, 16)])
def test_leading_dimensions(heads, dim):
    """H as a column block of a wider matrix and with gapped rows, out into a slice of a wider buffer, strided Y / dY / dH in the
    backward; the floats around the views keep their fill value."""
    g = _graph("powerlaw", seed=11, n=2500, nnz=150000)
    rp, ci = g.row_pointers.cuda(), g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers.cpu())]
    n, W = g.num_nodes, heads * dim
    gen = torch.Generator().manual_seed(dim)
    wide = torch.randn(n, 3 * W + 8, generator=gen).cuda()
    el, er = torch.randn(n, heads, generator=gen).cuda(), torch.randn(n, heads, generator=gen).cuda()
    for H in (wide[:, W:2 * W], torch.full((n, 128 + W), 7.5, device="cuda")[:, :W].copy_(wide[:, :W])):
        Y64, lse64, has, scale = _att64(H.double().contiguous(), el.double(), er.double(), rp, ci, heads, 0.2)
        obuf = torch.full((n, 2 * W + 4), -3.25, device="cuda")
        out = obuf[:, W + 4:]
        _out, lse = _lib.gat_forward(H, el, er, rp, ci, pp, p2n, 32, 0.2, out=out)
        assert_close_f64(out.cpu().numpy(), Y64.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what="ld Y")
        assert_close_f64(lse[has].cpu().numpy(), lse64[has].cpu().numpy(), rtol=1e-5, what="ld lse")
        assert (obuf[:, :W + 4] == -3.25).all()
        Y2, lse2 = GNNA.gat_forward(H, el, er, rp, ci, pp, p2n, 32, 0.2)                # the module takes the strided H too
        assert torch.equal(lse2, lse)
        assert_close_f64(Y2.cpu().numpy(), Y64.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what="ld Y (module)")
        # backward: dY a column block, dH into a slice
        gwide = torch.randn(n, 2 * W + 3, generator=gen).cuda()
        dY = gwide[:, 3:3 + W]
        dbuf = torch.full((n, W + 9), 1.75, device="cuda")
        dH, d_el, d_er = _lib.gat_backward(H, el, er, lse, out, dY, rp, ci, pp, p2n, 32, 0.2, dH=dbuf[:, 5:5 + W])
        ref = GNNA.gat_backward(H.contiguous(), el, er, lse, out.contiguous(), dY.contiguous(), rp, ci, pp, p2n, 32, 0.2)
        H64, el64, er64 = [t.double().contiguous().requires_grad_() for t in (H, el, er)]
        (_att64(H64, el64, er64, rp, ci, heads, 0.2)[0] * dY.double()).sum().backward()
        big = float(H64.grad.abs().max())
        for got, want, name in ((dH, H64.grad, "dH"), (ref[0], H64.grad, "dH (module)")):
            assert_close_f64(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, scale=np.full(want.shape, big), what=f"ld {name}")
        for got, want, name in ((d_el, el64.grad, "d_el"), (d_er, er64.grad, "d_er"), (ref[1], el64.grad, "d_el (module)")):
            assert_close_f64(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4,
                             scale=np.full(want.shape, float(want.abs().max())), what=f"ld {name}")
        assert (dbuf[:, :5] == 1.75).all() and (dbuf[:, 5 + W:] == 1.75).all()


# ---- layer ------------------------------------------------------------------------------------------------------------

def _layer_check(g, heads, concat, in_dim, out_dim, seed):
    """_gat_check of test_edge_attention_gpu.py with GATConv(fused=True)."""
    from gnnadvisor_osdi21_amd.ops import GATConv
    info = _Info(g)
    torch.manual_seed(seed)
    conv = GATConv(in_dim, out_dim, heads=heads, concat=concat, fused=True).cuda()
    X = torch.randn(g.num_nodes, in_dim, device="cuda", requires_grad=True)
    Y = conv(X, info)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    Y64 = _gat64(X64, *P64, info.row_pointers, info.column_index, heads, out_dim, concat)
    (Y64 * wgt.double()).sum().backward()
    what = f"fused GAT heads={heads} concat={concat}"
    for got, ref, name in ((Y, Y64, "Y"), (X.grad, X64.grad, "dX")):
        r = ref.detach()
        assert_close_f64(got.detach().cpu().numpy(), r.cpu().numpy(), rtol=1e-4,
                         scale=np.full(r.shape, float(r.abs().max())), what=f"{what} {name}")
    for got, ref, name in zip((conv.weights.grad, conv.att_l.grad, conv.att_r.grad), P64, ("dW", "da_l", "da_r")):
        r = ref.grad
        assert_close_f64(got.cpu().numpy(), r.cpu().numpy(), rtol=1e-4, scale=np.full(r.shape, float(r.abs().max())),
                         what=f"{what} {name}")
    assert "rows" not in info._edge_arrays() and "rev" not in info._edge_arrays()
    # cross-check only: the composed path on the same weights (two fp32 paths, each within 1e-4 of fp64)
    comp = GATConv(in_dim, out_dim, heads=heads, concat=concat).cuda()
    comp.load_state_dict(conv.state_dict())
    Xc = X.detach().clone().requires_grad_()
    Yc = comp(Xc, info)
    (Yc * wgt).sum().backward()
    for got, ref, name in ((Y, Yc, "Y"), (X.grad, Xc.grad, "dX"), (conv.weights.grad, comp.weights.grad, "dW")):
        r = ref.detach().double()
        assert_close_f64(got.detach().cpu().numpy(), r.cpu().numpy(), rtol=2e-4, scale=np.full(r.shape, float(r.abs().max())),
                         what=f"{what} {name} against the composed path")


@pytest.mark.parametrize("heads,concat", [(1, True), (4, True), (4, False), (8, True)])
def test_fused_gatconv_matches_fp64_gat(heads, concat):
    g = graph.powerlaw_graph(2000, 40000, 400, seed=31)
    _layer_check(g, heads, concat, in_dim=48, out_dim=16, seed=heads)


def test_no_per_edge_memory():
    """Forward + backward of GATAttention allocates less than ONE [nnz] float array; the composed path on the same inputs holds
    more than heads of them (so the bound discriminates)."""
    from gnnadvisor_osdi21_amd.ops import EdgeSoftmax, EdgeWeightedAggregate, GATAttention
    heads, dim = 2, 8
    g = graph.powerlaw_graph(20000, 12000000, 8000, seed=3)
    info = _Info(g)
    n, nnz = g.num_nodes, info.column_index.numel()
    # every node-sized tensor of the step: H, Y, dY, Y * dY, dH, H.grad; el, er, lse, d_el, d_er, el.grad / er.grad
    node_bytes = 4 * n * (6 * heads * dim + 7 * heads)
    assert nnz * 4 >= 4 * node_bytes
    H, el, er = [t.requires_grad_() for t in _inputs(n, heads, dim, 5)]
    G = torch.randn(n, heads * dim, device="cuda")

    def fused():
        Y = GATAttention.apply(H, el, er, info, 0.2)
        (Y * G).sum().backward()

    def composed():
        rows, ci = info.edge_rows(), info.column_index
        s = torch.nn.functional.leaky_relu(el.index_select(0, rows) + er.index_select(0, ci), 0.2)
        alpha = EdgeSoftmax.apply(s.t().contiguous(), info.row_pointers)
        Y = EdgeWeightedAggregate.apply(H, alpha, info)
        (Y * G).sum().backward()

    def peak(step):
        step()                                                    # warm-up: caches, library scratch, .grad buffers
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    p_fused = peak(fused)
    assert "rows" not in info._edge_arrays() and "rev" not in info._edge_arrays()
    print(f"peak bytes: fused {p_fused}, one [nnz] float array {nnz * 4}")
    assert p_fused < nnz * 4, (p_fused, nnz * 4)
    p_comp = peak(composed)
    print(f"peak bytes: composed {p_comp}, heads * nnz * 4 = {heads * nnz * 4}")
    assert p_comp > heads * nnz * 4, (p_comp, heads * nnz * 4)


def test_asymmetric_structure_is_refused_in_the_backward():
    """A directed CSR: the forward alone works and matches fp64; the backward raises instead of returning a wrong gradient."""
    from gnnadvisor_osdi21_amd.ops import GATAttention
    gen = np.random.default_rng(5)
    n = 400
    deg = gen.integers(0, 12, n)
    rp = torch.from_numpy(np.r_[0, np.cumsum(deg)].astype(np.int32))
    ci = torch.from_numpy(np.concatenate([np.sort(gen.choice(n, d, replace=False)) for d in deg]).astype(np.int32))

    class G:
        pass
    g = G()
    g.row_pointers, g.column_index, g.num_nodes = rp, ci, n
    info = _Info(g)
    heads, dim = 2, 8
    H, el, er = [t.requires_grad_() for t in _inputs(n, heads, dim, 9)]
    Y = GATAttention.apply(H, el, er, info, 0.2)
    Y64, _lse, _has, scale = _att64(H.detach().double(), el.detach().double(), er.detach().double(), info.row_pointers,
                                    info.column_index, heads, 0.2)
    assert_close_f64(Y.detach().cpu().numpy(), Y64.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what="directed forward")
    with pytest.raises(Exception, match="symmetric"):
        Y.sum().backward()


# ---- full size ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reddit():
    return graph.make_config_graph("reddit-like", device="cuda")


@pytest.mark.parametrize("heads,dim", [(1, 64), (4, 16)])
def test_reddit_like_fused_gat_layer(reddit, heads, dim):
    """One fused GAT layer forward and backward at full size: 256 sampled rows of Y and dX, all of dW, da_l, da_r, against the
    chunked fp64 formula run per head on the head's column block (given H the heads are independent)."""
    from gnnadvisor_osdi21_amd.ops import GATConv
    g = reddit
    info = _Info(g)
    torch.manual_seed(3)
    conv = GATConv(64, dim, heads=heads, fused=True).cuda()
    X = torch.randn(g.num_nodes, 64, device="cuda", requires_grad=True)
    Y = conv(X, info)
    G = torch.randn(Y.shape, device="cuda")
    (Y * G).sum().backward()
    assert "rows" not in info._edge_arrays()
    sample = torch.randperm(g.num_nodes, generator=torch.Generator().manual_seed(2))[:256].cuda()
    X64 = X.detach().double()
    dX_ref = torch.zeros(256, 64, dtype=torch.float64, device="cuda")
    for h in range(heads):
        blk = slice(h * dim, (h + 1) * dim)
        refs, sums = _gat64_chunked(X64, conv.weights.detach()[:, blk].double(), conv.att_l.detach()[h].double(),
                                    conv.att_r.detach()[h].double(), info.row_pointers, info.column_index, G[:, blk].double())
        dX_ref += refs[1][sample]
        gots = (Y.detach()[sample][:, blk], conv.weights.grad[:, blk], conv.att_l.grad[h], conv.att_r.grad[h])
        wants = (refs[0][sample], refs[2], refs[3], refs[4])
        scales = (np.full(wants[0].shape, float(wants[0].abs().max())),) + tuple(s.cpu().numpy() for s in sums)
        for got, ref, scale, name in zip(gots, wants, scales, ("Y", "dW", "da_l", "da_r")):
            assert_close_f64(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=scale,
                             what=f"Reddit-like fused GAT heads={heads} head {h} {name}")
        del refs, sums
    assert_close_f64(X.grad[sample].cpu().numpy(), dX_ref.cpu().numpy(), rtol=1e-4,
                     scale=np.full(dX_ref.shape, float(dX_ref.abs().max())), what=f"Reddit-like fused GAT heads={heads} dX")


# ---- driver ------------------------------------------------------------------------------------------------------------

def test_driver_fused_gat_trains():
    res = subprocess.run([sys.executable, "-m", "gnnadvisor_osdi21_amd.main", "--model", "gat", "--heads", "2",
                          "--fused_attention", "True", "--synthetic", "amazon0505-like", "--scale", "0.05", "--num_epoches", "20",
                          "--verbose_mode", "True"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "Time (ms):" in res.stdout
    first = float(re.search(r"# first loss: ([-\d.e+]+)", res.stdout).group(1))
    final = float(re.search(r"# final loss: ([-\d.e+]+)", res.stdout).group(1))
    assert final < first, (first, final)

"""Every autograd Function of ops.py on strided operands and strided incoming gradients, against the fp64 reference its own ops test
uses.

The rule under test: a Function of this package accepts every strided layout of its float operands and of the gradients that reach
its backward, and gives what its fp64 reference gives on the materialised values; it copies where the library cannot take the
layout and never raises because of strides.  One operand (or one incoming gradient) at a time takes a layout of tests/layouts.py,
everything else stays contiguous; the contiguous case of every operand is the control.

A case checks: every output and every gradient within the bound, the NaN padding of column_block / inner_stride_2 buffers still NaN,
no exception -- and, through a tensor hook on every output, that the gradient that ARRIVED at the Function had the strides the case
is about (a change in torch must not quietly turn these into contiguous cases).

Bounds: util.assert_close_f64 at 1e-4 * max(1, sum of |terms|) with the scale of the Function's own ops test; the fused attention
and the edge softmax at their tests' 1e-5 (x the score factor of gatv2_ref / dotattn_ref); max / min outputs exact; the 16-bit
neighbor sum at test_x16_ops_gpu.py's 1e-4 * max(1, scale) + u |ref| and the 16-bit layer at its 8 u * (sum of |terms|) + 1e-4,
u = 2^-8 (bfloat16) or 2^-11 (float16); SegmentNorm at segnorm_ref's bound_*; the std of NeighborStats at pna_ref's std tolerance.
No tolerance is introduced here.

Shapes: the directed graph of test_rgcn_ops_gpu.py (200 nodes, 2000 edges drawn) with three rows emptied (``directed`` set) and a symmetric
twin (the same edges and their reverses) for the reverse-edge / require_symmetric paths; one block sampled from the directed graph;
a batch of 5 graphs, one of them empty; W = 41 and W = 1; heads = 3, F = 5.  The worst error / bound of every Function is printed
by the last test."""
import time
import types

import numpy as np
import pytest
import torch
from torch.autograd import Function

import attnpool_ref
import dotattn_ref as tref
import edge_softmax_ref
import gat_drop_ref as dref
import gat_edge_ref as eref
import gat_rect_ref as gref
import gatv2_ref as vref
import layouts as L
import pna_ref
import pool_ref
import reduce_ref
import rgcn_ref
import segnorm_ref
import softagg_ref
from gnnadvisor_osdi21_amd import _lib, graph, ops
from gnnadvisor_osdi21_amd.batching import GraphBatch
from gnnadvisor_osdi21_amd.decider import inputProperty
from gnnadvisor_osdi21_amd.relational import RelationalGraph, synthetic_edge_types
from gnnadvisor_osdi21_amd.sampling import NeighborSampler
from util import assert_close_f64

pytestmark = pytest.mark.gpu

N, NNZ, W, HEADS, F, IN_DIM = 200, 2000, 41, 3, 5, 24
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SLOPE = 0.2
EMPTY_ROWS = [0, 77, N - 1]
STATS = ("mean", "std", "max", "min")

_made = {}
_worst = {}          # Function name -> (worst err / bound, the case it came from)
_clock = {"first": None, "last": None}


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _info(g, directed, partSize=8):
    ds = types.SimpleNamespace(num_nodes=g.num_nodes, avg_degree=g.avg_degree, avg_edgeSpan=g.avg_edgeSpan, num_features=IN_DIM)
    ip = inputProperty(g.row_pointers.cuda(), g.column_index.cuda(), g.degrees.cuda(), partSize, 32, 4, hiddenDim=16, dataset_obj=ds)
    pp, p2n = _lib.build_part(partSize, g.row_pointers)
    ip.partPtr, ip.part2Node = pp.cuda(), p2n.cuda()
    ip.directed = directed
    return ip


def _structure(rp, ci, n_out, n_in):
    """What the references index by: CPU and device row ids / column ids (int64) and the dense fp64 count matrix on the device."""
    rp, ci = rp.cpu(), ci.cpu()
    rows = torch.repeat_interleave(torch.arange(n_out), (rp[1:] - rp[:-1]).long())
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    A.index_put_((rows, ci.long()), torch.ones(rows.numel(), dtype=torch.float64), accumulate=True)
    return types.SimpleNamespace(rp=rp, ci=ci, rows=rows, src=ci.long(), A=A.cuda(), rows_d=rows.cuda(), src_d=ci.long().cuda(),
                                 n_out=n_out, n_in=n_in, nnz=int(ci.numel()))


def directed_graph():
    if "directed" not in _made:
        full = graph.uniform_graph(N, NNZ, symmetric=False)              # the graph of test_rgcn_ops_gpu.py ...
        rows = torch.repeat_interleave(torch.arange(N), (full.row_pointers[1:] - full.row_pointers[:-1]).long())
        keep = ~torch.isin(rows, torch.tensor(EMPTY_ROWS))                # ... with three rows emptied (the first, one inside, the last)
        g = graph.graph_from_edges(rows[keep], full.column_index.long()[keep], N)
        s = _structure(g.row_pointers, g.column_index, N, N)
        assert not torch.equal(s.A, s.A.t()) and bool((s.A.sum(1) == 0).any()), "directed, with rows without edges"
        s.info = _info(g, True)
        _made["directed"] = s
    return _made["directed"]


def symmetric_graph():
    """The twin: the directed graph's edges and their reverses."""
    if "symmetric" not in _made:
        d = directed_graph()
        g = graph.graph_from_edges(torch.cat([d.rows, d.src]), torch.cat([d.src, d.rows]), N)
        s = _structure(g.row_pointers, g.column_index, N, N)
        assert torch.equal(s.A, s.A.t())
        s.info = _info(g, False)
        _made["symmetric"] = s
    return _made["symmetric"]


def sampled_block():
    if "block" not in _made:
        d = directed_graph()
        seeds = torch.arange(0, N, 3, dtype=torch.int32).cuda()
        blocks, _ = NeighborSampler(d.info, [5], want_edge_ids=True).sample(seeds, 11)
        b = blocks[0]
        s = _structure(b.row_pointers, b.column_index, b.num_dst, b.num_src)
        assert b.num_src > b.num_dst == seeds.numel()
        s.info = b
        _made["block"] = s
    return _made["block"]


def graph_batch():
    """5 graphs, the third without nodes."""
    if "batch" not in _made:
        graphs = [graph.uniform_graph(n, 3 * n, seed=70 + k) for k, n in enumerate([13, 30, 0, 7, 21])]
        b = GraphBatch.from_graphs(graphs, partSize=8).to("cuda")
        _made["batch"] = types.SimpleNamespace(batch=b, gp=b.graph_pointers.cpu().tolist(), n=b.num_nodes)
    return _made["batch"]


def _rand(*shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


# ---- what a reference hands back ------------------------------------------------------------------------------------------
class Close:
    """|got - ref| <= rtol * max(1, scale) (util.assert_close_f64; scale None: |ref|), over the elements of `ok` when given."""

    def __init__(self, ref, scale=None, rtol=1e-4, ok=None):
        self.ref, self.scale, self.rtol, self.ok = ref, scale, rtol, ok

    def check(self, got, what):
        ref, scale = _t64(self.ref), None if self.scale is None else _t64(self.scale)
        got = got.detach().double().cpu()
        assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, the reference has {tuple(ref.shape)}"
        if self.ok is not None:
            ok = torch.as_tensor(self.ok).cpu()
            got, ref, scale = got[ok], ref[ok], None if scale is None else scale[ok]
        tol = self.rtol * (ref.abs() if scale is None else scale).clamp(min=1.0)
        worst = _ratio(got, ref, tol)
        assert_close_f64(got.numpy(), ref.numpy(), rtol=self.rtol, scale=None if scale is None else scale.numpy(), what=what)
        return worst


class Within:
    """|got - ref| <= tol, a bound the reference module states element by element."""

    def __init__(self, ref, tol):
        self.ref, self.tol = ref, tol

    def check(self, got, what):
        ref, tol = _t64(self.ref), _t64(self.tol)
        got = got.detach().double().cpu()
        assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, the reference has {tuple(ref.shape)}"
        worst = _ratio(got, ref, tol)
        assert not bool((~((got - ref).abs() <= tol)).any()), f"{what}: worst err / bound {worst:.3f}"
        return worst


def _t64(a):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach().cpu()).double()


def _ratio(got, ref, tol):
    if ref.numel() == 0:
        return 0.0
    r = (got - ref).abs() / tol
    r = torch.where((got - ref) == 0, torch.zeros_like(r), r)          # (0 / 0 where an exact result has the bound 0)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def _autograd(fn, tensors, dY):
    leaves = [t.detach().clone().requires_grad_() for t in tensors]
    Y = fn(*leaves)
    (Y * dY).sum().backward()
    return Y.detach(), [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves]


def sum_reference(dense, names, mask_from_output=False, unit=None, layer=False):
    """Operators that are sums with fixed non-negative coefficients (test_directed_ops_gpu.py, test_rgcn_ops_gpu.py): fp64 dense
    autograd, and as the scale of every result the same formula on the absolute values of every operand and of dY.
    mask_from_output: the op ends in a ReLU, whose step is taken where the path under test took it.  unit: 16-bit operands, the
    bound of test_x16_ops_gpu.py (layer: through bf16 / fp16 intermediates)."""
    def ref(v, dYs, outs):
        ts = [v[n] for n in names]
        mask = (outs[0].double() > 0).double() if mask_from_output else None
        Y, g = _autograd(lambda *t: dense(*t) if mask is None else dense(*t) * mask, ts, dYs[0])
        S, s = _autograd(dense, [t.abs() for t in ts], dYs[0].abs())

        def bound(r, sc):
            if unit is None:
                return Close(r, sc)
            return Within(r, 8 * unit * sc + 1e-4) if layer else Within(r, 1e-4 * sc.clamp(min=1.0) + unit * r.abs())
        exp = {"Y0": bound(Y, S)}
        exp.update({"d" + n: bound(gi, si) for n, gi, si in zip(names, g, s)})
        return exp
    return ref


# ---- the case table ---------------------------------------------------------------------------------------------------------
# name -> (Function, operands {name: "2d" | "col" | "1d"}, number of outputs, builder).  The builder returns (operands {name:
# contiguous tensor}, ours(**operands) -> output or tuple, ref(operands in fp64, [dY or None per output], outputs) -> {key:
# Close | Within} for the keys "Y<k>" and "d<operand>").  "col" is an [n, 1] operand, "1d" a vector.
SPECS = {}


def spec(name, fn, operands, outputs=1):
    def register(builder):
        SPECS[name] = types.SimpleNamespace(name=name, fn=fn, operands=operands, outputs=outputs, builder=builder)
        return builder
    return register


def _sag(s, w, dtype=torch.float32):
    X = _rand(s.n_in, w, seed=1, dtype=dtype)
    return ({"X": X}, lambda X: ops.ScatterAndGather.apply(X, s.info),
            sum_reference(lambda x: s.A @ x, ["X"], unit=UNIT.get(dtype)))


spec("ScatterAndGather", "ScatterAndGather", {"X": "2d"})(lambda: _sag(directed_graph(), W))
spec("ScatterAndGather W=1", "ScatterAndGather", {"X": "col"})(lambda: _sag(directed_graph(), 1))
spec("ScatterAndGather block", "ScatterAndGather", {"X": "2d"})(lambda: _sag(sampled_block(), W))
spec("ScatterAndGather bf16", "ScatterAndGather", {"X": "2d"})(lambda: _sag(directed_graph(), W, torch.bfloat16))
spec("ScatterAndGather fp16", "ScatterAndGather", {"X": "2d"})(lambda: _sag(directed_graph(), W, torch.float16))


def _gcn_matrix(s):
    deg = s.info.degrees.double()
    return deg[:, None] * s.A * deg[None, :]


def _gcn(fn, w, relu=False):
    s = directed_graph()
    M = _gcn_matrix(s)
    X, Wt = _rand(N, IN_DIM, seed=2), _rand(IN_DIM, w, seed=3) / 4
    return ({"X": X, "weight": Wt}, lambda X, weight: fn.apply(X, weight, s.info),
            sum_reference(lambda x, wt: M @ (x @ wt), ["X", "weight"], mask_from_output=relu))


spec("GNNAFunction", "GNNAFunction", {"X": "2d", "weight": "2d"})(lambda: _gcn(ops.GNNAFunction, W))
spec("GNNAFunction W=1", "GNNAFunction", {"X": "2d", "weight": "col"})(lambda: _gcn(ops.GNNAFunction, 1))
spec("GNNAFunction_ReLU", "GNNAFunction_ReLU", {"X": "2d", "weight": "2d"})(lambda: _gcn(ops.GNNAFunction_ReLU, W, relu=True))


@spec("GNNAFunction_GIN", "GNNAFunction_GIN", {"X": "2d", "weight": "2d"})
def _gin():
    s = directed_graph()
    X, Wt = _rand(N, IN_DIM, seed=4), _rand(IN_DIM, W, seed=5) / 4
    return ({"X": X, "weight": Wt}, lambda X, weight: ops.GNNAFunction_GIN.apply(X, weight, s.info, 0.5),
            sum_reference(lambda x, wt: (0.5 * (s.A @ x)) @ wt, ["X", "weight"]))


@spec("GNNAFunction_GIN_UpdateFirst", "GNNAFunction_GIN_UpdateFirst", {"X": "2d", "weight": "2d"})
def _gin_update_first():
    s = symmetric_graph()
    X, Wt = _rand(N, IN_DIM, seed=4), _rand(IN_DIM, W, seed=5) / 4
    return ({"X": X, "weight": Wt}, lambda X, weight: ops.GNNAFunction_GIN_UpdateFirst.apply(X, weight, s.info, 0.5, True),
            sum_reference(lambda x, wt: 0.5 * (s.A @ (x @ wt)), ["X", "weight"], mask_from_output=True))


def _x16(dtype, mode, update_first):
    s = symmetric_graph() if update_first else directed_graph()
    M = _gcn_matrix(s) if mode == 1 else 0.5 * s.A
    X, Wt = _rand(N, IN_DIM, seed=6, dtype=dtype), (_rand(IN_DIM, W, seed=7) / 4).to(dtype)
    dense = (lambda x, wt: M @ (x @ wt)) if update_first else (lambda x, wt: (M @ x) @ wt)
    return ({"X": X, "weight": Wt},
            lambda X, weight: ops.GNNAFunction_X16.apply(X, weight, s.info, mode, 0.5, update_first, False, dtype),
            sum_reference(dense, ["X", "weight"], unit=UNIT[dtype], layer=True))


spec("GNNAFunction_X16 bf16 gin", "GNNAFunction_X16", {"X": "2d", "weight": "2d"})(lambda: _x16(torch.bfloat16, 2, False))
spec("GNNAFunction_X16 fp16 gin", "GNNAFunction_X16", {"X": "2d", "weight": "2d"})(lambda: _x16(torch.float16, 2, False))
spec("GNNAFunction_X16 bf16 gcn", "GNNAFunction_X16", {"X": "2d", "weight": "2d"})(lambda: _x16(torch.bfloat16, 1, True))


def _extreme(fn, how, s, w):
    X = _rand(s.n_in, w, seed=8)

    def ref(v, dYs, outs):
        ext, dX = reduce_ref.first_edge_routing(v["X"], s.rows_d, s.src_d, s.n_out, how, dYs[0])
        _, scale = reduce_ref.first_edge_routing(v["X"], s.rows_d, s.src_d, s.n_out, how, dYs[0].abs())
        return {"Y0": Close(ext, rtol=0.0), "dX": Close(dX, scale)}           # (the forward is exact: test_reduce_ops_gpu.py)
    return {"X": X}, lambda X: fn.apply(X, s.info), ref


spec("NeighborMax", "NeighborMax", {"X": "2d"})(lambda: _extreme(ops.NeighborMax, "amax", directed_graph(), W))
spec("NeighborMax W=1", "NeighborMax", {"X": "col"})(lambda: _extreme(ops.NeighborMax, "amax", directed_graph(), 1))
spec("NeighborMax block", "NeighborMax", {"X": "2d"})(lambda: _extreme(ops.NeighborMax, "amax", sampled_block(), W))
spec("NeighborMin", "NeighborMin", {"X": "2d"})(lambda: _extreme(ops.NeighborMin, "amin", directed_graph(), W))
spec("NeighborMin block", "NeighborMin", {"X": "2d"})(lambda: _extreme(ops.NeighborMin, "amin", sampled_block(), W))


def _mean(s, w):
    inv = 1.0 / s.A.sum(1).clamp(min=1.0)
    X = _rand(s.n_in, w, seed=9)
    return {"X": X}, lambda X: ops.NeighborMean.apply(X, s.info), sum_reference(lambda x: inv[:, None] * (s.A @ x), ["X"])


spec("NeighborMean", "NeighborMean", {"X": "2d"})(lambda: _mean(directed_graph(), W))
spec("NeighborMean W=1", "NeighborMean", {"X": "col"})(lambda: _mean(directed_graph(), 1))
spec("NeighborMean block", "NeighborMean", {"X": "2d"})(lambda: _mean(sampled_block(), W))


def _stats(w, want=STATS):
    s = directed_graph()
    X = _rand(N, w, seed=10)

    def ref(v, dYs, outs):
        X64 = v["X"].cpu()
        g = [None if d is None else d.cpu() for d in dYs]
        leaf = X64.clone().requires_grad_()
        mean, std, _mx, _mn = pna_ref._stats64(leaf, s.rows, s.src, N)
        smooth = sum((y * gg).sum() for y, gg in zip((mean, std), g[:2]) if gg is not None)
        if torch.is_tensor(smooth):
            smooth.backward()
        dX = torch.zeros_like(X64) if leaf.grad is None else leaf.grad.clone()
        mabs, std_tol, dx_scale = pna_ref._bounds(X64, s.rows, s.src, N, [g[0], g[1], None, None], std.detach())
        ext = {}
        for k, how in ((2, "amax"), (3, "amin")):                  # the library's tie rule (a broadcast X is all ties)
            zero = torch.zeros(N, X64.shape[1], dtype=torch.float64)
            ext[k], routed = reduce_ref.first_edge_routing(X64, s.rows, s.src, N, how, zero if g[k] is None else g[k])
            dX += routed
            dx_scale = dx_scale + reduce_ref.first_edge_routing(X64, s.rows, s.src, N, how, zero if g[k] is None else g[k].abs())[1]
        return {"Y0": Close(mean.detach(), mabs), "Y1": Within(std.detach(), std_tol), "Y2": Close(ext[2], rtol=0.0),
                "Y3": Close(ext[3], rtol=0.0), "dX": Close(dX, dx_scale)}
    return {"X": X}, lambda X: ops.NeighborStats.apply(X, s.info, pna_ref.EPS, want), ref


spec("NeighborStats", "NeighborStats", {"X": "2d"}, outputs=4)(lambda: _stats(W))
# (without the std the backward aggregates g_mean / count itself, not the [a | b] buffer it fills)
spec("NeighborStats mean max", "NeighborStats", {"X": "2d"}, outputs=4)(lambda: _stats(W, ("mean", "max")))
spec("NeighborStats W=1", "NeighborStats", {"X": "col"}, outputs=4)(lambda: _stats(1))


def _softagg(s, w):
    X, temp = _rand(s.n_in, w, seed=11), (1.7 + 0.3 * _rand(w, seed=12))

    def ref(v, dYs, outs):
        r = softagg_ref.reference(v["X"], v["temp"], s.rp, s.ci, dYs[0])
        return {"Y0": Close(r["out"], r["out_scale"]), "dX": Close(r["dX"], r["dX_scale"]), "dtemp": Close(r["dt"], r["dt_scale"])}
    return {"X": X, "temp": temp}, lambda X, temp: ops.NeighborSoftmax.apply(X, temp, s.info), ref


spec("NeighborSoftmax", "NeighborSoftmax", {"X": "2d", "temp": "1d"})(lambda: _softagg(directed_graph(), W))
spec("NeighborSoftmax W=1", "NeighborSoftmax", {"X": "col", "temp": "1d"})(lambda: _softagg(directed_graph(), 1))


def _typed(w):
    s = directed_graph()
    R, B = 5, 3
    rel = RelationalGraph(s.info, synthetic_edge_types(s.info.row_pointers, s.info.column_index, R, seed=3), R)
    A = rgcn_ref.dense_relations(s.rp, s.ci, rel.edge_type, rel.edge_norm, R, N, N)
    X, coef = _rand(N, w, seed=1), _rand(R, B, seed=2)
    return ({"X": X, "coef": coef}, lambda X, coef: ops.TypedAggregate.apply(X, coef, rel),
            sum_reference(lambda x, c: rgcn_ref.dense_expand(A, x, c), ["X", "coef"]))


spec("TypedAggregate", "TypedAggregate", {"X": "2d", "coef": "2d"})(lambda: _typed(W))
spec("TypedAggregate W=1", "TypedAggregate", {"X": "col", "coef": "2d"})(lambda: _typed(1))


def _edge_weighted(heads, f):
    s = symmetric_graph()                       # (dX through the reverse-edge map)
    X = _rand(N, heads * f, seed=10)
    w = _rand(heads, s.nnz, seed=11) if heads > 1 else _rand(s.nnz, seed=11)

    def dense(x, wv):
        wv = wv.view(heads, -1)
        out = []
        for h in range(heads):
            Aw = torch.zeros(N, N, dtype=x.dtype, device=x.device).index_put((s.rows_d, s.src_d), wv[h], accumulate=True)
            out.append(Aw @ x[:, h * f:(h + 1) * f])
        return torch.cat(out, 1)
    return {"X": X, "w": w}, lambda X, w: ops.EdgeWeightedAggregate.apply(X, w, s.info), sum_reference(dense, ["X", "w"])


spec("EdgeWeightedAggregate heads", "EdgeWeightedAggregate", {"X": "2d", "w": "2d"})(lambda: _edge_weighted(HEADS, F))
spec("EdgeWeightedAggregate", "EdgeWeightedAggregate", {"X": "2d", "w": "1d"})(lambda: _edge_weighted(1, W))


def _edge_softmax(heads):
    s = directed_graph()
    scores = 4.0 * (_rand(heads, s.nnz, seed=13) if heads > 1 else _rand(s.nnz, seed=13))
    rp = s.info.row_pointers

    def ref(v, dYs, outs):
        sc, dp = v["scores"].view(heads, -1), dYs[0].view(heads, -1)
        p = edge_softmax_ref._softmax64(sc, rp)
        dot = torch.zeros(heads, N, dtype=torch.float64, device="cuda").index_add_(1, s.rows_d, p * dp)
        adot = torch.zeros_like(dot).index_add_(1, s.rows_d, p * dp.abs())
        shape = v["scores"].shape
        return {"Y0": Close(p.view(shape), rtol=edge_softmax_ref.SOFTMAX_RTOL),
                "dscores": Close((p * (dp - dot[:, s.rows_d])).view(shape), (p * (dp.abs() + adot[:, s.rows_d])).view(shape),
                                 rtol=edge_softmax_ref.SOFTMAX_RTOL)}
    return {"scores": scores}, lambda scores: ops.EdgeSoftmax.apply(scores, rp), ref


spec("EdgeSoftmax heads", "EdgeSoftmax", {"scores": "2d"})(lambda: _edge_softmax(HEADS))
spec("EdgeSoftmax", "EdgeSoftmax", {"scores": "1d"})(lambda: _edge_softmax(1))


def _gat(s, p=0.0, seed=0):
    H, el, er = _rand(s.n_in, HEADS * F, seed=14), _rand(s.n_out, HEADS, seed=15), _rand(s.n_in, HEADS, seed=16)
    rp, ci = s.info.row_pointers, s.info.column_index

    def ref(v, dYs, outs):
        if p > 0.0:
            r = dref.kernel_reference(v["H"], v["el"], v["er"], dYs[0], rp, ci, HEADS, SLOPE, p, seed, "GATAttention")
        else:
            r = gref.kernel_reference(v["H"], v["el"], v["er"], dYs[0], rp, ci, HEADS, SLOPE, "GATAttention")
        return {"Y0": Close(r.Y, r.s_Y, 1e-5), "dH": Close(r.dH, r.s_dH, 1e-5), "del": Close(r.d_el, r.s_el, 1e-5, r.ok_el),
                "der": Close(r.d_er, r.s_er, 1e-5, r.ok_er)}
    extra = (p, seed) if p > 0.0 else ()
    return {"H": H, "el": el, "er": er}, lambda H, el, er: ops.GATAttention.apply(H, el, er, s.info, SLOPE, *extra), ref


_GAT_OPERANDS = {"H": "2d", "el": "2d", "er": "2d"}
spec("GATAttention", "GATAttention", _GAT_OPERANDS)(lambda: _gat(directed_graph()))
spec("GATAttention block", "GATAttention", _GAT_OPERANDS)(lambda: _gat(sampled_block()))
spec("GATAttention attn_drop", "GATAttention", _GAT_OPERANDS)(lambda: _gat(symmetric_graph(), 0.5, 2 ** 40 + 7))


@spec("GATEdgeAttention", "GATEdgeAttention", {"H": "2d", "el": "2d", "er": "2d", "ee": "2d"})
def _gat_edge():
    s = symmetric_graph()                       # (ee of the source-side pass through the reverse-edge map)
    H, el, er, ee = _rand(N, HEADS * F, seed=14), _rand(N, HEADS, seed=15), _rand(N, HEADS, seed=16), _rand(s.nnz, HEADS, seed=17)
    rp, ci = s.info.row_pointers, s.info.column_index

    def ref(v, dYs, outs):
        r = eref.kernel_reference(v["H"], v["el"], v["er"], v["ee"], dYs[0], rp, ci, HEADS, SLOPE, what="GATEdgeAttention")
        return {"Y0": Close(r.Y, r.s_Y, 1e-5), "dH": Close(r.dH, r.s_dH, 1e-5), "del": Close(r.d_el, r.s_el, 1e-5, r.ok_el),
                "der": Close(r.d_er, r.s_er, 1e-5, r.ok_er), "dee": Close(r.d_ee, r.s_ee, 1e-5, r.ok_ee)}
    return ({"H": H, "el": el, "er": er, "ee": ee},
            lambda H, el, er, ee: ops.GATEdgeAttention.apply(H, el, er, ee, s.info, SLOPE), ref)


@spec("GATv2Attention", "GATv2Attention", {"Hs": "2d", "Hd": "2d", "att": "2d"})
def _gatv2():
    s = symmetric_graph()
    Hs, Hd, att = _rand(N, HEADS * F, seed=18), _rand(N, HEADS * F, seed=19), _rand(HEADS, F, seed=20)
    rp, ci = s.info.row_pointers, s.info.column_index

    def ref(v, dYs, outs):
        r = vref.kernel_reference(v["Hs"], v["Hd"], v["att"], dYs[0], rp, ci, HEADS, SLOPE, what="GATv2Attention")
        rtol = 1e-5 * r.factor
        return {"Y0": Close(r.Y, r.s_Y, rtol), "dHs": Close(r.dHs, r.s_dHs, rtol, r.ok_dHs), "dHd": Close(r.dHd, r.s_dHd, rtol, r.ok_dHd),
                "datt": Close(r.d_att, r.s_att, rtol)}
    return {"Hs": Hs, "Hd": Hd, "att": att}, lambda Hs, Hd, att: ops.GATv2Attention.apply(Hs, Hd, att, s.info, SLOPE), ref


@spec("DotAttention", "DotAttention", {"Q": "2d", "K": "2d", "V": "2d"})
def _dot():
    s = symmetric_graph()
    Q, K, V = _rand(N, HEADS * F, seed=21), _rand(N, HEADS * F, seed=22), _rand(N, HEADS * F, seed=23)
    rp, ci = s.info.row_pointers, s.info.column_index

    def ref(v, dYs, outs):
        r = tref.kernel_reference(v["Q"], v["K"], v["V"], dYs[0], rp, ci, HEADS, 1.0 / F ** 0.5)
        rtol = 1e-5 * r.factor
        return {"Y0": Close(r.Y, r.s_Y, rtol), "dQ": Close(r.dQ, r.s_dQ, rtol), "dK": Close(r.dK, r.s_dK, rtol),
                "dV": Close(r.dV, r.s_dV, rtol)}
    return {"Q": Q, "K": K, "V": V}, lambda Q, K, V: ops.DotAttention.apply(Q, K, V, s.info, HEADS), ref


def _segment_pool(w, mean):
    b = graph_batch()
    X = _rand(b.n, w, seed=24)
    segs = pool_ref.segments(b.gp, b.n)

    def ref(v, dYs, outs):
        X64 = v["X"].cpu()
        f = pool_ref.forward(X64.float().numpy(), b.gp)
        count = torch.as_tensor(f["count"]).double().clamp(min=1)[:, None]
        div = count if mean else torch.ones_like(count)
        dX, scale = torch.zeros_like(X64), torch.zeros_like(X64)
        for g, (a, e) in enumerate(segs):
            rows = torch.arange(a, e)[:, None]
            for k, arg in ((0, None), (1, f["argmax"]), (2, f["argmin"])):
                if dYs[k] is None or e <= a:
                    continue
                d = dYs[k][g].cpu()
                term = (d / div[g]).expand(e - a, -1) if arg is None else torch.where(torch.as_tensor(arg[g])[None, :] == rows, d, 0.0)
                dX[a:e] += term
                scale[a:e] += term.abs()
        return {"Y0": Close(torch.as_tensor(f["sum"]) / div, torch.as_tensor(f["abs"]) / div), "Y1": Close(f["max"], rtol=0.0),
                "Y2": Close(f["min"], rtol=0.0), "dX": Close(dX, scale)}
    return {"X": X}, lambda X: ops.SegmentPool.apply(X, b.batch, True, True, True, mean), ref


spec("SegmentPool", "SegmentPool", {"X": "2d"}, outputs=3)(lambda: _segment_pool(W, True))
spec("SegmentPool W=1", "SegmentPool", {"X": "col"}, outputs=3)(lambda: _segment_pool(1, False))


def _attention_pool(w, gate_w):
    b = graph_batch()
    X, gate = _rand(b.n, w, seed=25), _rand(b.n, gate_w, seed=26)

    def ref(v, dYs, outs):
        r = attnpool_ref.reference(v["X"].cpu().numpy(), v["gate"].cpu().numpy(), b.gp, dYs[0].cpu().numpy())
        return {"Y0": Close(r["out"], r["out_scale"]), "dX": Close(r["dX"], r["dX_scale"]), "dgate": Close(r["dGate"], r["dGate_scale"])}
    return {"X": X, "gate": gate}, lambda X, gate: ops.SegmentAttentionPool.apply(X, gate, b.batch), ref


spec("SegmentAttentionPool", "SegmentAttentionPool", {"X": "2d", "gate": "col"})(lambda: _attention_pool(W, 1))
spec("SegmentAttentionPool gate per element", "SegmentAttentionPool", {"X": "2d", "gate": "2d"})(lambda: _attention_pool(W, W))
spec("SegmentAttentionPool W=1", "SegmentAttentionPool", {"X": "col", "gate": "col"})(lambda: _attention_pool(1, 1))


def _selection():
    if "selection" not in _made:
        b = graph_batch()
        _made["selection"] = b.batch.coarsen(_rand(b.n, seed=27), ratio=0.5)[1]
        kept = int(_made["selection"].perm.numel())
        assert 0 < kept < b.n
    return _made["selection"]


def _select_rows(w):
    b, sel = graph_batch(), _selection()
    perm = sel.perm.long()
    X, scale = _rand(b.n, w, seed=28), _rand(b.n, seed=29)
    return ({"X": X, "scale": scale}, lambda X, scale: ops.SelectRows.apply(X, scale, sel),
            sum_reference(lambda x, sc: sc[perm, None] * x[perm], ["X", "scale"]))


spec("SelectRows", "SelectRows", {"X": "2d", "scale": "1d"})(lambda: _select_rows(W))
spec("SelectRows W=1", "SelectRows", {"X": "col", "scale": "1d"})(lambda: _select_rows(1))


def _unpool_rows(w):
    b, sel = graph_batch(), _selection()
    perm = sel.perm.long()
    X = _rand(perm.numel(), w, seed=30)
    return ({"X_small": X}, lambda X_small: ops.UnpoolRows.apply(X_small, sel),
            sum_reference(lambda x: torch.zeros(b.n, w, dtype=x.dtype, device=x.device).index_add(0, perm, x), ["X_small"]))


spec("UnpoolRows", "UnpoolRows", {"X_small": "2d"})(lambda: _unpool_rows(W))
spec("UnpoolRows W=1", "UnpoolRows", {"X_small": "col"})(lambda: _unpool_rows(1))


def _segment_norm(w):
    b = graph_batch()
    X = _rand(b.n, w, seed=31)
    weight, bias, alpha = 1.0 + 0.4 * _rand(w, seed=32), 0.4 * _rand(w, seed=33), 0.6 + 0.4 * _rand(w, seed=34)

    def ref(v, dYs, outs):
        host = lambda t: t.cpu().numpy()                                                       # noqa: E731
        r = segnorm_ref.graph_norm_f64(host(v["X"]), np.asarray(b.gp), host(v["weight"]), host(v["bias"]), host(v["alpha"]), 1e-5,
                                       host(dYs[0]))
        return {"Y0": Within(r["out"], r["bound_out"]), "dX": Within(r["d_input"], r["bound_d_input"]),
                "dweight": Within(r["d_weight"], r["bound_d_weight"]), "dbias": Within(r["d_bias"], r["bound_d_bias"]),
                "dalpha": Within(r["d_alpha"], r["bound_d_alpha"])}
    return ({"X": X, "weight": weight, "bias": bias, "alpha": alpha},
            lambda X, weight, bias, alpha: ops.SegmentNorm.apply(X, b.batch, weight, bias, alpha, 1e-5), ref)


_NORM_OPERANDS = {"weight": "1d", "bias": "1d", "alpha": "1d"}
spec("SegmentNorm", "SegmentNorm", {"X": "2d", **_NORM_OPERANDS})(lambda: _segment_norm(W))
spec("SegmentNorm W=1", "SegmentNorm", {"X": "col", **_NORM_OPERANDS})(lambda: _segment_norm(1))


# ---- the cases ------------------------------------------------------------------------------------------------------------
_OPERAND_KINDS = {"2d": L.KINDS, "col": tuple(k for k in L.KINDS if k != "column_major"), "1d": ("contiguous", "inner_stride_2")}
_OUTPUT_WIDTH_1 = {"ScatterAndGather W=1", "GNNAFunction W=1", "NeighborMax W=1", "NeighborMean W=1", "NeighborStats W=1",
                   "NeighborSoftmax W=1", "SegmentPool W=1", "SegmentAttentionPool W=1", "SelectRows W=1", "UnpoolRows W=1",
                   "SegmentNorm W=1"}
_OUTPUT_1D = {"EdgeSoftmax"}
ABSENT_OUTPUTS = {"NeighborStats mean max": (1, 3)}


def _gradient_kinds(name):
    if name in _OUTPUT_1D:
        return ("contiguous", "inner_stride_2", "full_broadcast")
    if name in _OUTPUT_WIDTH_1:
        return _OPERAND_KINDS["col"] + ("cat_block",)
    return L.KINDS + ("cat_block",)


def _cases():
    out = []
    for name, sp in SPECS.items():
        for operand, rank in sp.operands.items():
            out += [(name, operand, kind) for kind in _OPERAND_KINDS[rank]]
        for k in range(sp.outputs):
            if k in ABSENT_OUTPUTS.get(name, ()):
                continue
            out += [(name, f"grad{k}", kind) for kind in _gradient_kinds(name) if kind != "contiguous"]      # (the operands' control is it)
            if sp.outputs > 1:
                out.append((name, f"grad{k}", "unused"))
    return out


def _built(name):
    if ("case", name) not in _made:
        _made["case", name] = SPECS[name].builder()
    return _made["case", name]


def _read_strides(shape, strides):
    """The strides of the dimensions that have more than one element: the others are never read (torch leaves them free)."""
    return tuple(st for n, st in zip(shape, strides) if n > 1)


def _weights_like(Y, seed):
    return (torch.rand(*Y.shape, generator=torch.Generator().manual_seed(seed)) + 0.1).to(Y.dtype).cuda()


def test_the_table_names_every_function_of_ops():
    defined = {n for n, c in vars(ops).items() if isinstance(c, type) and issubclass(c, Function) and c is not Function
               and c.__module__ == ops.__name__}
    assert {sp.fn for sp in SPECS.values()} == defined, "one entry per autograd Function of ops.py, and none that is gone"
    assert len(defined) == 23
    with_block = {sp.fn for n, sp in SPECS.items() if n.endswith(" block")}
    assert with_block == {"ScatterAndGather", "NeighborMean", "NeighborMax", "NeighborMin", "GATAttention"}
    assert "GATAttention attn_drop" in SPECS


@pytest.mark.parametrize("name,which,kind", _cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_layout(name, which, kind):
    if _clock["first"] is None:
        _clock["first"] = time.perf_counter()
    sp = SPECS[name]
    operands, ours, ref = _built(name)
    keep, leaves, values = [], {}, {}
    for n, t in operands.items():
        if n == which:
            leaf, values[n] = L.relayout(t, kind, keep), L.materialised(t, kind)
            assert tuple(leaf.stride()) == L.expected_strides(tuple(t.shape), kind) and torch.equal(leaf, values[n])
        else:
            leaf, values[n] = t.detach().clone(), t
        leaves[n] = leaf.requires_grad_()
    outs = ours(**leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    assert len(outs) == sp.outputs
    loss, dYs, arrived, intended = 0.0, [], [], []
    for k, Y in enumerate(outs):
        here = kind if which == f"grad{k}" else "contiguous"
        if Y is None:                                        # an output that was not asked for
            assert here == "contiguous" or here == "unused", f"{name}: output {k} does not exist"
            dYs.append(None)
            continue
        if here == "unused":
            dYs.append(None)
            continue
        seen = []
        L.record_arrival(Y, seen)
        part, dY = L.layout_loss(Y, here, _weights_like(Y, 99 + k), keep)
        loss = loss + part
        dYs.append(dY.double())
        arrived.append(seen)
        intended.append(L.arrival_strides(tuple(Y.shape), here))
    loss.backward()
    torch.cuda.synchronize()
    assert len(arrived) == len(intended) and all(len(seen) == 1 for seen in arrived), arrived
    for Y, seen, want in zip([Y for Y, d in zip(outs, dYs) if d is not None], arrived, intended):      # (d is None: unused or absent)
        assert _read_strides(Y.shape, seen[0]) == _read_strides(Y.shape, want), \
            f"{name}, {which} {kind}: a gradient arrived with the strides {seen[0]}, the case is about {want}"
    expect = ref({n: v.double() for n, v in values.items()}, dYs, [None if Y is None else Y.detach() for Y in outs])
    expect = {key: e for key, e in expect.items() if not (key[0] == "Y" and outs[int(key[1:])] is None)}
    got = {f"Y{k}": Y for k, Y in enumerate(outs) if Y is not None}
    got.update({"d" + n: leaf.grad for n, leaf in leaves.items()})
    assert set(expect) == set(got), (sorted(expect), sorted(got))
    worst = 0.0
    for key, e in expect.items():
        what = f"{name}, {which} {kind}: {key}"
        if got[key] is None:
            assert float(_t64(e.ref).abs().max()) == 0.0, f"{what} is missing"
            continue
        worst = max(worst, e.check(got[key], what))
    assert L.padding_intact(keep), f"{name}, {which} {kind}: the NaN padding around a strided view was written"
    if worst >= _worst.get(sp.fn, (-1.0, ""))[0]:
        _worst[sp.fn] = (worst, f"{name}, {which} {kind}")
    _clock["last"] = time.perf_counter()


def test_two_rgcn_layers_under_a_sum_readout():
    """RGCNConv -> RGCNConv -> (Y.sum(0) * w).sum() against rgcn_ref.dense_layer: every gradient of a model whose loss is a sum
    readout.  (The readout's (0, 1) gradient meets the layer's torch.mm first; the aggregation alone under the same readout is the
    TypedAggregate row_broadcast case above.)"""
    s = directed_graph()
    R, B, HID, OUT = 5, 3, 16, 7
    rel = RelationalGraph(s.info, synthetic_edge_types(s.info.row_pointers, s.info.column_index, R, seed=3), R)
    A = rgcn_ref.dense_relations(s.rp, s.ci, rel.edge_type, rel.edge_norm, R, N, N)
    torch.manual_seed(7)
    c1 = ops.RGCNConv(IN_DIM, HID, R, num_bases=B).cuda()
    c2 = ops.RGCNConv(HID, OUT, R, num_bases=B).cuda()
    with torch.no_grad():
        c1.bias.uniform_(-0.5, 0.5)
        c2.bias.uniform_(-0.5, 0.5)
    X = _rand(N, IN_DIM, seed=4)
    w = torch.rand(OUT, generator=torch.Generator().manual_seed(99)).cuda() + 0.1
    names = ["X", "V1", "coef1", "W_self1", "bias1", "V2", "coef2", "W_self2", "bias2"]
    tensors = [X, c1.V, c1.coef, c1.W_self, c1.bias, c2.V, c2.coef, c2.W_self, c2.bias]

    def ours(x, v1, k1, w1, b1, v2, k2, w2, b2):
        h = torch.func.functional_call(c1, dict(V=v1, coef=k1, W_self=w1, bias=b1), (x, rel))
        return torch.func.functional_call(c2, dict(V=v2, coef=k2, W_self=w2, bias=b2), (h, rel))

    def dense(x, v1, k1, w1, b1, v2, k2, w2, b2):
        return rgcn_ref.dense_layer(A, rgcn_ref.dense_layer(A, x, k1, v1, w1, b1), k2, v2, w2, b2)

    def grads_of(fn, ts, wv):
        leaves = [t.detach().clone().requires_grad_() for t in ts]
        Y = fn(*leaves)
        seen = []
        L.record_arrival(Y, seen)
        (Y.sum(0) * wv).sum().backward()
        assert seen == [(0, 1)], f"the readout handed the model a gradient with the strides {seen}"
        return [Y.detach()] + [t.grad for t in leaves]

    got = grads_of(ours, tensors, w)
    ref = grads_of(dense, [t.double() for t in tensors], w.double())
    scale = grads_of(dense, [t.double().abs() for t in tensors], w.double())
    for name, g_, r_, s_ in zip(["Y"] + ["d" + n for n in names], got, ref, scale):
        worst = float(((g_.double() - r_).abs() / (1e-4 * s_.clamp(min=1.0))).max())
        print(f"two RGCN layers, sum readout {name}: worst err / tol {worst:.4f}")
        assert_close_f64(g_.cpu().numpy(), r_.cpu().numpy(), rtol=1e-4, scale=s_.cpu().numpy(), what=f"sum readout {name}")


def test_report():
    """The largest error-to-bound ratio of every Function over the cases above, and the wall time they took."""
    if _clock["first"] is not None:
        print(f"\ntest_layout: {_clock['last'] - _clock['first']:.1f} s wall for {len(_cases())} cases")
    for fn in sorted(_worst):
        print(f"{fn}: worst err / bound {_worst[fn][0]:.4f}  ({_worst[fn][1]})")
    assert all(v[0] <= 1.0 for v in _worst.values())

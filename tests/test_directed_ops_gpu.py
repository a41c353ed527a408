"""Backward passes on a DIRECTED graph (decider.inputProperty.directed = True): every gradient against fp64 dense autograd.

Bound: |got - ref| <= 1e-4 * max(1, scale) (util.assert_close_f64).  For the operators that are sums with fixed non-negative
coefficients (neighbor sum, GCN, GIN, mean, GraphSAGE, edge-weighted aggregation) the scale is the sum of |terms|: the same
dense formula evaluated on the absolute values of every input, whose outputs and gradients are exactly those sums.  A GAT
layer is no such sum (the softmax' coefficients depend on the inputs), so it takes the scale the project's GAT tests already
use for a layer: the largest |reference| of the tensor (tests/test_gat_fused_gpu.py, tests/test_edge_attention_gpu.py).
The bf16 layer uses the gradient bound of tests/test_x16_ops_gpu.py: 8 * 2^-8 * (sum of |terms|) + 1e-4."""
import types

import numpy as np
import pytest
import torch
from torch.func import functional_call

from gnnadvisor_osdi21_amd import _lib, graph, ops
from gnnadvisor_osdi21_amd.decider import inputProperty
from test_transpose_gpu import _hub
from util import assert_close_f64

pytestmark = pytest.mark.gpu
DIMS, PART_SIZES = [16, 41, 64], [3, 32]
IN_DIM = 24


def _make_graph(rp, ci, n):
    return graph.CSRGraph(n, rp, ci, graph.degrees_from_rowptr(rp), int(ci.numel()), ci.numel() / n, n / 3.0)


_graphs = {}


def _graph(name):
    """(graph, dense fp64 adjacency on the GPU with A[i, j] = number of edges i <- j)."""
    if name not in _graphs:
        g = graph.uniform_graph(300, 3000, symmetric=False) if name == "directed" else _make_graph(*_hub())
        rows = torch.repeat_interleave(torch.arange(g.num_nodes), (g.row_pointers[1:] - g.row_pointers[:-1]).long())
        A = torch.zeros(g.num_nodes, g.num_nodes, dtype=torch.float64)
        A.index_put_((rows, g.column_index.long()), torch.ones(rows.numel(), dtype=torch.float64), accumulate=True)
        assert not torch.equal(A, A.t()), "the graph must be directed"
        _graphs[name] = (g, A.cuda(), rows.cuda())
    return _graphs[name]


def _info(g, partSize, directed=True):
    ds = types.SimpleNamespace(num_nodes=g.num_nodes, avg_degree=g.avg_degree, avg_edgeSpan=g.avg_edgeSpan, num_features=IN_DIM)
    ip = inputProperty(g.row_pointers.cuda(), g.column_index.cuda(), g.degrees.cuda(), partSize, 32, 4, hiddenDim=16, dataset_obj=ds)
    pp, p2n = _lib.build_part(partSize, g.row_pointers)
    ip.partPtr, ip.part2Node = pp.cuda(), p2n.cuda()
    ip.directed = directed
    return ip


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _grads(fn, tensors, wgt):
    """Output and the gradients of sum(fn(*tensors) * wgt) with respect to every tensor."""
    leaves = [t.detach().clone().requires_grad_() for t in tensors]
    Y = fn(*leaves)
    (Y * wgt).sum().backward()
    return Y.detach(), [t.grad for t in leaves]


def _compare(ours, dense, tensors, names, what, mask_from_output=False):
    """ours(*fp32 tensors) against dense(*fp64 tensors, mask): output and every gradient within 1e-4 of the sum of |terms|.
    mask_from_output: the layer ends in a ReLU -- its step function is taken where the path under test took it (an element that
    cancels to fp32 rounding of zero has no defined sign), exactly as both paths then differentiate the same function."""
    wgt = _rand(*ours(*tensors).shape, seed=99).abs() + 0.1
    Y, got = _grads(ours, tensors, wgt)
    mask = (Y > 0).double() if mask_from_output else None
    Y64, ref = _grads(lambda *t: dense(*t, mask), [t.double() for t in tensors], wgt.double())
    ones = None if mask is None else torch.ones_like(mask)
    S, scale = _grads(lambda *t: dense(*t, ones), [t.double().abs() for t in tensors], wgt.double())
    worst = {}
    for name, g_, r_, s_ in zip(["Y"] + ["d" + n for n in names], [Y] + got, [Y64] + ref, [S] + scale):
        worst[name] = float(((g_.double() - r_).abs() / (1e-4 * s_.clamp(min=1.0))).max())
    print(f"{what}: worst err / tol {({k: round(v, 4) for k, v in worst.items()})}")
    for name, g_, r_, s_ in zip(["Y"] + ["d" + n for n in names], [Y] + got, [Y64] + ref, [S] + scale):
        assert_close_f64(g_.cpu().numpy(), r_.cpu().numpy(), rtol=1e-4, scale=s_.cpu().numpy(), what=f"{what} {name}")


def _masked(Y, mask):
    return Y if mask is None else Y * mask


# ---- the sum operators -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", ["directed", "hub"])
def test_scatter_and_gather(name, D, partSize):
    g, A, _rows = _graph(name)
    info = _info(g, partSize)
    X = _rand(g.num_nodes, D, seed=1)
    _compare(lambda x: ops.ScatterAndGather.apply(x, info), lambda x, m: A @ x, [X], ["X"], f"SAG {name} D={D} ps={partSize}")


def test_symmetric_assumption_misses_the_bound_on_a_directed_graph():
    """directed = False on the same directed graph: the backward pass applies A where A^T belongs, and this test can tell."""
    g, A, _rows = _graph("directed")
    info = _info(g, 32, directed=False)
    X = _rand(g.num_nodes, 16, seed=1)
    with pytest.raises(AssertionError, match="dX"):
        _compare(lambda x: ops.ScatterAndGather.apply(x, info), lambda x, m: A @ x, [X], ["X"], "SAG directed=False")


@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_gcn_conv(relu, D, partSize):
    g, A, _rows = _graph("directed")
    info = _info(g, partSize)
    deg = info.degrees.double()
    M = deg[:, None] * A * deg[None, :]
    conv = ops.GCNConv(IN_DIM, D).cuda()
    X, W = _rand(g.num_nodes, IN_DIM, seed=2), _rand(IN_DIM, D, seed=3) / 4
    ours = lambda x, w: functional_call(conv, {"weights": w}, (x, info), {"relu": relu})
    _compare(ours, lambda x, w, m: _masked(M @ (x @ w), m), [X, W], ["X", "W"], f"GCN relu={relu} D={D} ps={partSize}",
             mask_from_output=relu)


@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("update_first", [False, True], ids=["aggregate_first", "update_first"])
def test_gin_conv(update_first, D, partSize):
    g, A, _rows = _graph("directed")
    info = _info(g, partSize)
    conv = ops.GINConv(IN_DIM, D, update_first=update_first).cuda()
    X, W = _rand(g.num_nodes, IN_DIM, seed=4), _rand(IN_DIM, D, seed=5) / 4

    ours = lambda x, w: functional_call(conv, {"weights": w}, (x, info))
    _compare(ours, lambda x, w, m: (0.5 * (A @ x)) @ w, [X, W], ["X", "W"], f"GIN update_first={update_first} D={D} ps={partSize}")


@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("D", DIMS)
def test_neighbor_mean(D, partSize):
    g, A, _rows = _graph("directed")
    info = _info(g, partSize)
    inv = 1.0 / A.sum(1).clamp(min=1.0)
    X = _rand(g.num_nodes, D, seed=6)
    _compare(lambda x: ops.NeighborMean.apply(x, info), lambda x, m: inv[:, None] * (A @ x), [X], ["X"], f"mean D={D} ps={partSize}")


@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("D", DIMS)
def test_sage_conv_mean(D, partSize):
    g, A, _rows = _graph("directed")
    info = _info(g, partSize)
    inv = 1.0 / A.sum(1).clamp(min=1.0)
    conv = ops.SAGEConv(IN_DIM, D, aggregator="mean").cuda()
    X, Ws, Wn = _rand(g.num_nodes, IN_DIM, seed=7), _rand(IN_DIM, D, seed=8) / 4, _rand(IN_DIM, D, seed=9) / 4

    ours = lambda x, ws, wn: functional_call(conv, {"weights_self": ws, "weights_neigh": wn}, (x, info))
    _compare(ours, lambda x, ws, wn, m: x @ ws + (inv[:, None] * (A @ x)) @ wn, [X, Ws, Wn], ["X", "Ws", "Wn"],
             f"SAGE mean D={D} ps={partSize}")


# ---- edge values, attention -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("heads", [1, 4])
def test_edge_weighted_aggregate(heads, D, partSize):
    g, _A, rows = _graph("directed")
    info = _info(g, partSize)
    n, cols = g.num_nodes, info.column_index.long()
    X, w = _rand(n, heads * D, seed=10), _rand(heads, g.nnz, seed=11)

    def dense(x, wv, m):
        out = []
        for h in range(heads):
            Aw = torch.zeros(n, n, dtype=x.dtype, device=x.device).index_put((rows, cols), wv[h])
            out.append(Aw @ x[:, h * D:(h + 1) * D])
        return torch.cat(out, 1)

    _compare(lambda x, wv: ops.EdgeWeightedAggregate.apply(x, wv, info), dense, [X, w], ["X", "w"],
             f"edge-weighted heads={heads} D={D} ps={partSize}")
    assert "rev" not in info._edge_arrays(), "a directed graph has no reverse-edge map"


def _gat64(X, W, a_l, a_r, A, heads, out_dim, slope=0.2):
    n = X.shape[0]
    H = (X @ W).view(n, heads, out_dim)
    el, er = (H * a_l).sum(-1), (H * a_r).sum(-1)
    s = torch.nn.functional.leaky_relu(el[:, None, :] + er[None, :, :], slope)           # [i, j, h]
    has = A.sum(1) > 0
    s = s.masked_fill(((A == 0) & has[:, None])[:, :, None], float("-inf"))
    alpha = torch.softmax(s, dim=1) * has[:, None, None]                                 # rows without edges give 0
    return torch.einsum("ijh,jhf->ihf", alpha, H).reshape(n, heads * out_dim)


@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("heads,out_dim", [(1, 64), (4, 16)])
@pytest.mark.parametrize("fused", [False, True], ids=["composed", "fused"])
def test_gat_conv(fused, heads, out_dim, partSize):
    g, A, _rows = _graph("directed")
    info = _info(g, partSize)
    torch.manual_seed(heads)
    conv = ops.GATConv(IN_DIM, out_dim, heads=heads, fused=fused).cuda()
    X = _rand(g.num_nodes, IN_DIM, seed=12).requires_grad_()
    Y = conv(X, info)
    wgt = _rand(*Y.shape, seed=13)
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    Y64 = _gat64(X64, *P64, A, heads, out_dim)
    (Y64 * wgt.double()).sum().backward()
    pairs = [("Y", Y.detach(), Y64.detach()), ("dX", X.grad, X64.grad), ("dW", conv.weights.grad, P64[0].grad),
             ("da_l", conv.att_l.grad, P64[1].grad), ("da_r", conv.att_r.grad, P64[2].grad)]
    for name, got, ref in pairs:
        print(f"GAT fused={fused} {heads}x{out_dim} ps={partSize} {name}: max err / max |ref| = "
              f"{float((got.double() - ref).abs().max() / ref.abs().max()):.3e}")
    for name, got, ref in pairs:
        assert_close_f64(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=np.full(ref.shape, float(ref.abs().max())),
                         what=f"GAT fused={fused} {heads}x{out_dim} ps={partSize} {name}")
    assert "rev" not in info._edge_arrays() and "symmetric" not in info._edge_arrays()


def test_gat_attention_still_raises_on_a_directed_structure_when_not_told():
    """directed = False: today's behaviour -- the fused backward checks the symmetry and refuses."""
    g, _A, _rows = _graph("directed")
    info = _info(g, 32, directed=False)
    conv = ops.GATConv(IN_DIM, 16, heads=2, fused=True).cuda()
    X = _rand(g.num_nodes, IN_DIM, seed=12).requires_grad_()
    Y = conv(X, info)
    with pytest.raises(RuntimeError, match="not symmetric"):
        Y.sum().backward()


# ---- 16-bit layer ------------------------------------------------------------------------------------------------------------

def test_gcn_conv_bf16():
    """One bf16 GCNConv: dX and dW against fp64 on the bf16-representable inputs, with the bound tests/test_x16_ops_gpu.py uses
    for its bf16 gradients: |err| <= 8 * 2^-8 * (sum of |terms|) + 1e-4."""
    g, A, _rows = _graph("directed")
    info = _info(g, 32)
    info.degrees = (info.degrees / info.degrees.max()).contiguous()
    deg = info.degrees.double()
    M = deg[:, None] * A * deg[None, :]
    X = _rand(g.num_nodes, IN_DIM, seed=14).bfloat16()
    W = (_rand(IN_DIM, 64, seed=15) / 4).bfloat16()
    wgt = (_rand(g.num_nodes, 64, seed=16).abs() + 0.1).bfloat16()
    ours = lambda x, w: ops.GNNAFunction_X16.apply(x, w, info, 1, 1.0, True, False, torch.bfloat16)
    _Y, got = _grads(ours, [X, W], wgt)
    assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.bfloat16
    dense = lambda x, w: M @ (x @ w)
    _Y64, ref = _grads(dense, [X.double(), W.double()], wgt.double())
    _S, mag = _grads(dense, [X.double().abs(), W.double().abs()], wgt.double())
    for name, g_, r_, m_ in zip(("dX", "dW"), got, ref, mag):
        err, tol = (g_.double() - r_).abs(), 8 * 2.0 ** -8 * m_ + 1e-4
        print(f"bf16 GCN {name}: worst err / tol = {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), f"bf16 GCN {name}: worst err / tol {float((err / tol).max()):.3f}"


# ---- same structure, same bits; captured step ----------------------------------------------------------------------------------

def test_symmetric_graph_gives_identical_bits_with_and_without_directed():
    """A symmetric CSR with sorted rows is its own transpose, partition included: with the deterministic schedule the gradients
    of directed = True and directed = False are the same bits."""
    g = graph.uniform_graph(300, 3000, seed=2)
    X = _rand(g.num_nodes, 41, seed=17)
    wgt = _rand(g.num_nodes, 41, seed=18)
    _lib.set_tuning(deterministic=1)
    try:
        grads = []
        for directed in (False, True):
            info = _info(g, 3, directed=directed)
            if directed:
                t = info.transposed()
                assert torch.equal(t.column_index, info.column_index) and torch.equal(t.row_pointers, info.row_pointers)
                assert torch.equal(t.partPtr, info.partPtr) and torch.equal(t.part2Node, info.part2Node)
            grads.append(_grads(lambda x: ops.ScatterAndGather.apply(x, info), [X], wgt)[1][0])
        assert torch.equal(grads[0], grads[1])
    finally:
        _lib.reset_tuning()


def test_transposed_bundle_is_cached_per_column_index_and_part_size():
    g, _A, _rows = _graph("directed")
    info = _info(g, 32)
    t = info.transposed()
    assert info.transposed() is t and t.degrees is info.degrees and t._perm is None
    perm = t.perm
    assert perm.dtype == torch.int32 and t.perm is perm
    assert torch.equal(info.column_index[perm.long()], torch.repeat_interleave(
        torch.arange(g.num_nodes, dtype=torch.int32, device="cuda"), (t.row_pointers[1:] - t.row_pointers[:-1]).long()))
    info.partSize = 3
    pp, p2n = _lib.build_part(3, g.row_pointers)
    info.partPtr, info.part2Node = pp.cuda(), p2n.cuda()
    t3 = info.transposed()
    assert t3 is not t and t3.column_index is t.column_index and t3.partSize == 3 and t3.perm is perm
    info.column_index = info.column_index.clone()          # a renumbered CSR: another column_index object
    assert info.transposed().column_index is not t.column_index


def test_captured_directed_gcn_step_replays_to_the_eager_result():
    """torch.cuda.graph over forward + backward of a two-layer GCN on the directed graph, transposed() built beforehand.  Eager
    and replayed gradients are two fp32 evaluations of the same sums (the order of the float atomics may differ): they agree
    to 1e-5 of the largest gradient, ten times inside the 1e-4 bound each keeps against fp64."""
    g, _A, _rows = _graph("directed")
    info = _info(g, 32)
    info.transposed()
    torch.manual_seed(3)
    c1, c2 = ops.GCNConv(IN_DIM, 16).cuda(), ops.GCNConv(16, 8).cuda()
    X = _rand(g.num_nodes, IN_DIM, seed=19).requires_grad_()
    wgt = _rand(g.num_nodes, 8, seed=20)
    params = [X, c1.weights, c2.weights]

    def step():
        y = c2(c1(X, info, relu=True), info)
        return torch.autograd.grad((y * wgt).sum(), params)

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    side.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        static = step()
    for t in static:
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    for got, ref, name in zip(static, eager, ("dX", "dW1", "dW2")):
        assert_close_f64(got.cpu().numpy(), ref.double().cpu().numpy(), rtol=1e-5,
                         scale=np.full(ref.shape, float(ref.abs().max())), what=f"captured directed GCN {name}")

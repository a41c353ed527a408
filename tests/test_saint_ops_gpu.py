"""Layers on a sampled ``sampling.Subgraph``: outputs and every gradient against fp64 dense autograd on the dense induced adjacency,
which is built from the numpy restatement of the subgraph rule (tests/walk_ref.py), never from the library's arrays.

Bound: |got - ref| <= 1e-4 * max(1, scale), exactly as tests/test_directed_ops_gpu.py states it and with its helpers: for the sums
with fixed non-negative coefficients (GCN, GIN, GraphSAGE mean, edge-weighted aggregation) the scale is the sum of |terms|; a GAT
layer is no such sum and takes the scale the project's GAT tests use, the largest |reference| of the tensor.  The subgraph of a
symmetric graph is symmetric (its backward passes reuse the forward structure, and require_symmetric() passes); the subgraph of a
directed graph inherits ``directed`` and runs its backward passes on its own transposed structure."""
import functools

import numpy as np
import pytest
import torch
from torch.func import functional_call

import walk_ref as ref
from gnnadvisor_osdi21_amd import graph, ops, sampling
from test_directed_ops_gpu import IN_DIM, _compare, _gat64, _info, _masked, _rand
from util import assert_close_f64

pytestmark = pytest.mark.gpu
KINDS = ["symmetric", "directed"]
D = 41


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(parent bundle, sampler with estimated norms, one sampled Subgraph, its dense fp64 adjacency, the restated subgraph)."""
    g = graph.uniform_graph(600, 6000, seed=5, symmetric=kind == "symmetric")
    info = _info(g, 32, directed=kind == "directed")
    sampler = sampling.SaintRWSampler(info, num_roots=100, walk_length=2, seed=3)
    sampler.estimate_norms(6)
    sub = sampler.sample(0)
    walks, _ = sampler.walker.walk(sampler.roots(0), sampler._step_seed(0))
    want = ref.induced_subgraph(g.row_pointers.numpy(), g.column_index.numpy(), walks.reshape(-1).cpu().numpy())
    A = torch.from_numpy(ref.dense_adjacency(want)).cuda()
    return info, sampler, sub, A, want


@pytest.mark.parametrize("kind", KINDS)
def test_the_subgraph_is_the_restated_one_and_a_graph_batch(kind):
    info, _sampler, sub, A, want = _case(kind)
    n = len(want["nodes"])
    assert 100 < n < 600 and sub.num_nodes == n and sub.num_graphs == 1 and sub.graph_pointers.tolist() == [0, n]
    assert sub.nodes.tolist() == want["nodes"].tolist() and sub.edge_ids.tolist() == want["edge_ids"].tolist()
    assert sub.row_pointers.tolist() == want["row_pointers"].tolist() and sub.column_index.tolist() == want["column_index"].tolist()
    assert sub.parent_num_nodes == 600 and sub.directed == (kind == "directed") and sub.partSize == info.partSize
    assert (sub.dimWorker, sub.warpPerBlock) == (info.dimWorker, info.warpPerBlock)
    assert torch.equal(sub.degrees, graph.degrees_from_rowptr(sub.row_pointers))
    pp, p2n = ref.host_build_part(32, want["row_pointers"])
    assert sub.partPtr.tolist() == pp.tolist() and sub.part2Node.tolist() == p2n.tolist()
    assert torch.equal(A, A.t()) == (kind == "symmetric")
    if kind == "symmetric":
        sub.require_symmetric()
    else:
        with pytest.raises(Exception, match="not symmetric"):
            sub.require_symmetric()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_gcn_conv(kind, relu):
    _info_, _sampler, sub, A, _want = _case(kind)
    deg = sub.degrees.double()
    M = deg[:, None] * A * deg[None, :]
    conv = ops.GCNConv(IN_DIM, D).cuda()
    X, W = _rand(sub.num_nodes, IN_DIM, seed=2), _rand(IN_DIM, D, seed=3) / 4
    ours = lambda x, w: functional_call(conv, {"weights": w}, (x, sub), {"relu": relu})
    _compare(ours, lambda x, w, m: _masked(M @ (x @ w), m), [X, W], ["X", "W"], f"GCN on a {kind} subgraph relu={relu}",
             mask_from_output=relu)


@pytest.mark.parametrize("kind", KINDS)
def test_gin_conv(kind):
    _info_, _sampler, sub, A, _want = _case(kind)
    conv = ops.GINConv(IN_DIM, D).cuda()
    X, W = _rand(sub.num_nodes, IN_DIM, seed=4), _rand(IN_DIM, D, seed=5) / 4
    ours = lambda x, w: functional_call(conv, {"weights": w}, (x, sub))
    _compare(ours, lambda x, w, m: (0.5 * (A @ x)) @ w, [X, W], ["X", "W"], f"GIN on a {kind} subgraph")


@pytest.mark.parametrize("kind", KINDS)
def test_sage_conv_mean(kind):
    _info_, _sampler, sub, A, _want = _case(kind)
    inv = 1.0 / A.sum(1).clamp(min=1.0)
    conv = ops.SAGEConv(IN_DIM, D, aggregator="mean").cuda()
    X, Ws, Wn = _rand(sub.num_nodes, IN_DIM, seed=7), _rand(IN_DIM, D, seed=8) / 4, _rand(IN_DIM, D, seed=9) / 4
    ours = lambda x, ws, wn: functional_call(conv, {"weights_self": ws, "weights_neigh": wn}, (x, sub))
    _compare(ours, lambda x, ws, wn, m: x @ ws + (inv[:, None] * (A @ x)) @ wn, [X, Ws, Wn], ["X", "Ws", "Wn"],
             f"SAGE mean on a {kind} subgraph")


@pytest.mark.parametrize("kind", KINDS)
def test_gat_conv_fused(kind):
    _info_, _sampler, sub, A, _want = _case(kind)
    heads, out_dim = 4, 16
    torch.manual_seed(heads)
    conv = ops.GATConv(IN_DIM, out_dim, heads=heads, fused=True).cuda()
    X = _rand(sub.num_nodes, IN_DIM, seed=12).requires_grad_()
    Y = conv(X, sub)
    wgt = _rand(*Y.shape, seed=13)
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    Y64 = _gat64(X64, *P64, A, heads, out_dim)
    (Y64 * wgt.double()).sum().backward()
    pairs = [("Y", Y.detach(), Y64.detach()), ("dX", X.grad, X64.grad), ("dW", conv.weights.grad, P64[0].grad),
             ("da_l", conv.att_l.grad, P64[1].grad), ("da_r", conv.att_r.grad, P64[2].grad)]
    for name, got, want in pairs:
        print(f"fused GAT on a {kind} subgraph {name}: max err / max |ref| = {float((got.double() - want).abs().max() / want.abs().max()):.3e}")
    for name, got, want in pairs:
        assert_close_f64(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, scale=np.full(want.shape, float(want.abs().max())),
                         what=f"fused GAT on a {kind} subgraph {name}")


@pytest.mark.parametrize("kind", KINDS)
def test_edge_weighted_aggregate_with_the_saint_edge_weights(kind):
    _info_, sampler, sub, _A, want = _case(kind)
    n = sub.num_nodes
    w = sub.edge_weight
    assert w.dtype == torch.float32 and w.numel() == len(want["edge_ids"]) and float(w.min()) > 0 and float(w.max()) <= 1e4
    assert torch.equal(w, sampler.edge_weight[torch.from_numpy(want["edge_ids"]).cuda()])
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(want["row_pointers"]))).cuda()
    cols = torch.from_numpy(want["column_index"]).cuda()
    X = _rand(n, D, seed=10)

    def dense(x, wv, m):
        return torch.zeros(n, n, dtype=x.dtype, device=x.device).index_put((rows, cols), wv, accumulate=True) @ x

    _compare(lambda x, wv: ops.EdgeWeightedAggregate.apply(x, wv, sub), dense, [X, w], ["X", "w"],
             f"edge-weighted aggregation on a {kind} subgraph")


@pytest.mark.parametrize("kind", KINDS)
def test_estimate_norms_counts_equal_a_numpy_recount(kind):
    info, _sampler, _sub, _A, _want = _case(kind)
    T = 5
    sampler = sampling.SaintRWSampler(info, num_roots=100, walk_length=2, seed=9)
    assert sampler.node_weight is None and sampler.sample(0).node_weight is None and sampler.sample(0).edge_weight is None
    node_weight, edge_weight = sampler.estimate_norms(T)
    rp, ci = info.row_pointers.cpu().numpy(), info.column_index.cpu().numpy()
    c_v, c_e = np.zeros(600, np.int64), np.zeros(len(ci), np.int64)
    for i in range(T):
        step = -(i + 1)
        walks = ref.random_walks(rp, ci, sampler.roots(step).cpu().numpy(), 2, sampler._step_seed(step))[0]
        want = ref.induced_subgraph(rp, ci, walks.reshape(-1))
        c_v[want["nodes"]] += 1
        c_e[want["edge_ids"]] += 1
    assert sampler.node_count.dtype == torch.int64 and (sampler.node_count.cpu().numpy() == c_v).all()
    assert (sampler.edge_count.cpu().numpy() == c_e).all() and c_v.max() > 1 and (c_v == 0).any()
    cv = np.where(c_v == 0, 0.1, c_v.astype(np.float64))
    ce = np.where(c_e == 0, 0.1, c_e.astype(np.float64))
    rows = np.repeat(np.arange(600), np.diff(rp))
    assert np.allclose(node_weight.cpu().numpy(), T / (600 * cv), rtol=1e-6)
    assert np.allclose(edge_weight.cpu().numpy(), np.clip(cv[rows] / ce, 0, 1e4), rtol=1e-6)
    sub = sampler.sample(0)
    assert torch.equal(sub.node_weight, node_weight[sub.nodes.long()]) and torch.equal(sub.edge_weight, edge_weight[sub.edge_ids.long()])


def test_the_sampler_is_a_function_of_seed_and_step_and_resizes_its_edge_buffer():
    info, _sampler, _sub, _A, _want = _case("symmetric")
    a, b = sampling.SaintRWSampler(info, 100, 2, seed=4), sampling.SaintRWSampler(info, 100, 2, seed=4)
    first = a.sample(7)
    for _ in range(2):                              # (b's second call runs with the 1.25x capacity)
        again = b.sample(7)
        assert torch.equal(first.nodes, again.nodes) and torch.equal(first.column_index, again.column_index)
    assert not torch.equal(first.nodes, a.sample(8).nodes)
    assert a.max_edges >= first.column_index.numel() > 0
    a.max_edges = 1                                 # a remembered size that is far too small: one retry from the reported counts
    retried = a.sample(7)
    assert torch.equal(retried.column_index, first.column_index) and torch.equal(retried.partPtr, first.partPtr)
    assert a.max_edges == first.column_index.numel()

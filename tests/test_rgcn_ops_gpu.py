"""ops.TypedAggregate / ops.RGCNConv on relational.RelationalGraph against fp64 dense autograd, on a DIRECTED graph whose types
are not symmetric, and on one sampled block.

Dense reference: one [num_dst, num_src] matrix per relation, A_r[i, j] = sum of the factors n[e] of the edges i <- j of type r;
T[:, b] = sum_r coef[r, b] A_r X and Y = T V + X_dst W_self + bias.  Bound: |got - ref| <= 1e-4 * max(1, sum of |terms|)
(util.assert_close_f64); the sum of |terms| of every output and gradient is the same network evaluated on the absolute values of
every input, parameter and loss weight (A_r is non-negative, and there is no ReLU between the layers: nothing has a kink)."""
import types

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph, ops
from gnnadvisor_osdi21_amd.decider import inputProperty
from gnnadvisor_osdi21_amd.relational import RelationalGraph, synthetic_edge_types
from gnnadvisor_osdi21_amd.sampling import NeighborSampler
from rgcn_ref import dense_expand, dense_layer, dense_relations
from util import assert_close_f64

pytestmark = pytest.mark.gpu
N, IN_DIM, HID, OUT = 200, 24, 16, 7
CONFIGS = [(5, 3), (4, None)]          # (relations, bases): with bases, and one weight per relation

_shared = {}


def shared_graph():
    if not _shared:
        g = graph.uniform_graph(N, 2000, symmetric=False)
        ds = types.SimpleNamespace(num_nodes=N, avg_degree=g.avg_degree, avg_edgeSpan=g.avg_edgeSpan, num_features=IN_DIM)
        ip = inputProperty(g.row_pointers.cuda(), g.column_index.cuda(), g.degrees.cuda(), 8, 32, 4, hiddenDim=HID, dataset_obj=ds)
        pp, p2n = _lib.build_part(8, g.row_pointers)
        ip.partPtr, ip.part2Node = pp.cuda(), p2n.cuda()
        ip.directed = False                       # (RelationalGraph does not consult it)
        _shared.update(g=g, info=ip)
    return _shared["g"], _shared["info"]


def relational(R, norm="relation"):
    g, info = shared_graph()
    ety = synthetic_edge_types(info.row_pointers, info.column_index, R, seed=3)
    return RelationalGraph(info, ety, R, norm=norm)


def numpy_norm(rp, ety, R):
    """1 / (edges of row(e) with type t[e]), counted edge by edge."""
    rp, ety = np.asarray(rp, np.int64), np.asarray(ety, np.int64)
    out = np.zeros(len(ety))
    for i in range(len(rp) - 1):
        t = ety[rp[i]: rp[i + 1]]
        out[rp[i]: rp[i + 1]] = 1.0 / np.bincount(t, minlength=R)[t]
    return out


def grads_of(fn, tensors, wgt, needs=None):
    needs = [True] * len(tensors) if needs is None else needs
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip(tensors, needs)]
    Y = fn(*leaves)
    (Y * wgt).sum().backward()
    return [Y.detach()] + [t.grad for t in leaves]


def compare(ours, dense, tensors, names, what, needs=None):
    """ours(*fp32 tensors) against dense(*fp64 tensors): the output and every gradient asked for."""
    with torch.no_grad():
        shape = ours(*tensors).shape
    wgt = torch.rand(*shape, generator=torch.Generator().manual_seed(99)).cuda() + 0.1
    got = grads_of(ours, tensors, wgt, needs)
    ref = grads_of(dense, [t.double() for t in tensors], wgt.double(), needs)
    scale = grads_of(dense, [t.double().abs() for t in tensors], wgt.double(), needs)
    for name, g_, r_, s_ in zip(["Y"] + ["d" + n for n in names], got, ref, scale):
        if r_ is None:
            assert g_ is None, f"{what}: {name} was not asked for"
            continue
        worst = float(((g_.double() - r_).abs() / (1e-4 * s_.clamp(min=1.0))).max())
        print(f"{what} {name}: worst err / tol {worst:.4f}")
        assert_close_f64(g_.cpu().numpy(), r_.cpu().numpy(), rtol=1e-4, scale=s_.cpu().numpy(), what=f"{what} {name}")


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_relation_norm_against_a_numpy_count():
    g, info = shared_graph()
    rel = relational(5)
    assert rel.edge_type.dtype == torch.int32 and rel.edge_type.is_cuda and rel.edge_type.numel() == g.column_index.numel()
    ety = rel.edge_type.cpu().numpy()
    assert set(ety.tolist()) == set(range(5))
    want = numpy_norm(g.row_pointers.numpy(), ety, 5)
    assert np.allclose(rel.edge_norm.cpu().numpy().astype(np.float64), want, rtol=1e-6, atol=0)
    assert relational(5, norm=None).edge_norm is None
    # the types are not symmetric: some edge i <- j has a reverse edge j <- i of another type
    A = dense_relations(g.row_pointers, g.column_index, ety, None, 5, N, N)
    assert not torch.equal(A, A.transpose(1, 2))


def test_relation_norm_leaves_out_of_range_types_out_of_the_count():
    g, info = shared_graph()
    ety = synthetic_edge_types(info.row_pointers, info.column_index, 5, seed=3).cpu().numpy().astype(np.int64)
    ety[::7] = 5                                   # skipped by the kernels: in nobody's count
    ety[3::11] = -1
    rel = RelationalGraph(info, torch.from_numpy(ety), 5)
    valid = (ety >= 0) & (ety < 5)
    rp = g.row_pointers.numpy().astype(np.int64)
    want = np.zeros(len(ety))
    for i in range(N):
        t = ety[rp[i]: rp[i + 1]]
        ok = valid[rp[i]: rp[i + 1]]
        cnt = np.bincount(t[ok], minlength=5)
        want[rp[i]: rp[i + 1]][ok] = 1.0 / cnt[t[ok]]
    got = rel.edge_norm.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.allclose(got[valid], want[valid], rtol=1e-6, atol=0)


@pytest.mark.parametrize("R,B", CONFIGS)
@pytest.mark.parametrize("x_grad", [True, False], ids=["dX", "no_dX"])
def test_typed_aggregate(R, B, x_grad):
    g, info = shared_graph()
    rel = relational(R)
    A = dense_relations(g.row_pointers, g.column_index, rel.edge_type, rel.edge_norm, R, N, N)
    X = rand(N, 41, seed=1)
    coef = rand(R, B, seed=2) if B else torch.eye(R).cuda()
    needs = [x_grad, B is not None]
    if not any(needs):
        needs = [False, True]
    compare(lambda x, c: ops.TypedAggregate.apply(x, c, rel), lambda x, c: dense_expand(A, x, c), [X, coef], ["X", "coef"],
            f"TypedAggregate R={R} B={B}", needs)
    assert (rel._transposed is not None) == x_grad, "the transposed structure is built for dX only"


@pytest.mark.parametrize("R,B", CONFIGS)
@pytest.mark.parametrize("x_grad", [True, False], ids=["dX", "no_dX"])
def test_two_layer_stack(R, B, x_grad):
    g, info = shared_graph()
    rel = relational(R)
    A = dense_relations(g.row_pointers, g.column_index, rel.edge_type, rel.edge_norm, R, N, N)
    torch.manual_seed(7)
    c1 = ops.RGCNConv(IN_DIM, HID, R, num_bases=B).cuda()
    c2 = ops.RGCNConv(HID, OUT, R, num_bases=B).cuda()
    with torch.no_grad():
        c1.bias.uniform_(-0.5, 0.5)
        c2.bias.uniform_(-0.5, 0.5)
    X = rand(N, IN_DIM, seed=4)
    names = ["X", "V1", "coef1", "W_self1", "bias1", "V2", "coef2", "W_self2", "bias2"]
    tensors = [X, c1.V, c1.coef, c1.W_self, c1.bias, c2.V, c2.coef, c2.W_self, c2.bias]
    needs = [x_grad, True, B is not None, True, True, True, B is not None, True, True]

    def ours(x, v1, k1, w1, b1, v2, k2, w2, b2):
        h = torch.func.functional_call(c1, dict(V=v1, coef=k1, W_self=w1, bias=b1), (x, rel))
        return torch.func.functional_call(c2, dict(V=v2, coef=k2, W_self=w2, bias=b2), (h, rel))

    def dense(x, v1, k1, w1, b1, v2, k2, w2, b2):
        return dense_layer(A, dense_layer(A, x, k1, v1, w1, b1), k2, v2, w2, b2)

    compare(ours, dense, tensors, names, f"two layers R={R} B={B}", needs)


@pytest.mark.parametrize("R,B", CONFIGS)
def test_first_layer_builds_no_transposed_structure(R, B):
    rel = relational(R)
    conv = ops.RGCNConv(IN_DIM, HID, R, num_bases=B).cuda()
    X = rand(N, IN_DIM, seed=5)
    conv(X, rel).sum().backward()
    assert rel._transposed is None and conv.V.grad is not None and (B is None or conv.coef.grad is not None)
    conv(X.requires_grad_(), rel).sum().backward()
    assert rel._transposed is not None and X.grad is not None


def test_layer_refuses_16_bit():
    rel = relational(4)
    conv = ops.RGCNConv(IN_DIM, HID, 4).cuda()
    X = rand(N, IN_DIM, seed=6)
    with pytest.raises(TypeError, match="float32 only"):
        conv(X.bfloat16(), rel)
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(TypeError, match="float32 only"):
        conv(X, rel)


@pytest.mark.parametrize("R,B", CONFIGS)
def test_layer_on_a_sampled_block(R, B):
    g, info = shared_graph()
    types_full = synthetic_edge_types(info.row_pointers, info.column_index, R, seed=3)
    sampler = NeighborSampler(info, [5], want_edge_ids=True)
    seeds = torch.arange(0, N, 3, dtype=torch.int32).cuda()
    blocks, input_nodes = sampler.sample(seeds, 11)
    block = blocks[0]
    rel = RelationalGraph.for_block(block, types_full, R)
    assert rel.is_block and rel.num_dst == seeds.numel() and rel.num_src == block.num_src > rel.num_dst
    ety = types_full.cpu()[block.edge_ids.cpu().long()]
    assert torch.equal(rel.edge_type.cpu(), ety)
    nrm = numpy_norm(block.row_pointers.cpu().numpy(), ety.numpy(), R)
    assert np.allclose(rel.edge_norm.cpu().numpy().astype(np.float64), nrm, rtol=1e-6, atol=0)
    A = dense_relations(block.row_pointers, block.column_index, ety, nrm, R, block.num_dst, block.num_src)
    conv = ops.RGCNConv(IN_DIM, HID, R, num_bases=B).cuda()
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    X = rand(block.num_src, IN_DIM, seed=8)

    def ours(x, v, k, w, b):
        return torch.func.functional_call(conv, dict(V=v, coef=k, W_self=w, bias=b), (x, rel))

    compare(ours, lambda x, v, k, w, b: dense_layer(A, x, k, v, w, b), [X, conv.V, conv.coef, conv.W_self, conv.bias],
            ["X", "V", "coef", "W_self", "bias"], f"block R={R} B={B}", [True, True, B is not None, True, True])

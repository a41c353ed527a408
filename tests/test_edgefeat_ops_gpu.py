"""Edge features through the operators: edgeconv.EdgeFeatureSum, GINEConv and CFConv against fp64 autograd of the composed formula
(the same modules in float64 with fused=False) on a symmetric graph, a directed one, a SampledBlock and a GraphBatch with an empty
graph; fused against composed; strided operands and an expanded gradient; no transposed structure when X needs no gradient; a
coarsened batch with carried edge attributes.

Bound: 1e-4 * max(1, max |ref|) per tensor, the bound of test_gat_edge_ops_gpu.py for outputs and input gradients.  It holds for
the parameter gradients too: each is a sum of at most 2e4 terms here, fp32 summation loses about 1e-7 of the sum of |terms|, and
the largest element of such a gradient is no smaller than 1e-3 of that sum."""
import copy

import numpy as np
import pytest
import torch

import edgefeat_ref as ref
from gnnadvisor_osdi21_amd import graph
from gnnadvisor_osdi21_amd.batching import GraphBatch
from gnnadvisor_osdi21_amd.edgeconv import CFConv, EdgeFeatureSum, GINEConv, composed_edge_feature_sum
from test_directed_ops_gpu import _info as _property
from test_edge_attention_gpu import _Info
from test_gat_block_ops_gpu import _max_scale, bundle, one_block
from util import assert_close_f64

pytestmark = pytest.mark.gpu
F, EDGE_DIM = 20, 5


def _batch_with_an_empty_graph():
    graphs = []
    for k, n in enumerate((9, 0, 14, 1, 30)):
        rp, ci = ref.small_rows_graph(n, max(n, 1), seed=50 + k, lo=0, hi=4) if n else (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
        graphs.append((torch.from_numpy(rp), torch.from_numpy(ci)))
    b = GraphBatch.from_graphs(graphs, directed=True).to("cuda")
    assert b.num_graphs == 5 and int(b.graph_pointers[2] - b.graph_pointers[1]) == 0 and b.directed
    return b


def _structure(kind):
    """(inputInfo, rows of the result, source rows, edge rows: None or the positions of the block's edges in its graph)"""
    if kind == "symmetric":
        g = graph.powerlaw_graph(1200, 20000, 300, seed=8)
        return _Info(g), g.num_nodes, g.num_nodes, None
    if kind == "directed":
        g = graph.uniform_graph(300, 3000, symmetric=False)
        return _property(g, 32, directed=True), g.num_nodes, g.num_nodes, None
    if kind == "batch":
        b = _batch_with_an_empty_graph()
        return b, b.num_nodes, b.num_nodes, None
    block = one_block()
    assert block.num_dst == 65 and block.num_src > 65
    return block, block.num_dst, block.num_src, block.edge_ids.long()


KINDS = ["symmetric", "directed", "block", "batch"]


def _n(t):
    return t.detach().cpu().numpy()


def _close(got, want, what):
    assert_close_f64(_n(got), _n(want), rtol=1e-4, scale=_max_scale(want.detach()), what=what)


def _edge_rows(kind, edge_ids, nnz, width, seed):
    """The E (or edge_attr) rows of the structure's own edges: a block's are gathered from its graph's through edge_ids."""
    gen = torch.Generator().manual_seed(seed)
    if edge_ids is None:
        return torch.randn(nnz, width, generator=gen).cuda()
    whole = torch.randn(bundle().column_index.numel(), width, generator=gen).cuda()
    return whole[edge_ids]


@pytest.mark.parametrize("combine, act", ref.MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_function_against_fp64(kind, combine, act):
    info, n_dst, n_src, edge_ids = _structure(kind)
    nnz = info.column_index.numel()
    gen = torch.Generator().manual_seed(5)
    X = torch.randn(n_src, F, generator=gen).cuda().requires_grad_()
    E = _edge_rows(kind, edge_ids, nnz, F, 6).requires_grad_()
    G = torch.randn(n_dst, F, generator=gen).cuda()
    Y = EdgeFeatureSum.apply(X, E, info, combine, act)
    assert Y.shape == (n_dst, F)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == X.data_ptr() and saved[1].data_ptr() == E.data_ptr(), "saved: X and E only"
    (Y * G).sum().backward()
    X64, E64 = X.detach().double().requires_grad_(), E.detach().double().requires_grad_()
    Y64 = composed_edge_feature_sum(X64, E64, info, combine, act)
    (Y64 * G.double()).sum().backward()
    _close(Y, Y64, f"{kind} {combine}/{act}: Y")
    _close(X.grad, X64.grad, f"{kind} {combine}/{act}: dX")
    _close(E.grad, E64.grad, f"{kind} {combine}/{act}: dE")


def _layers(which):
    torch.manual_seed(13)
    if which == "gine":
        return GINEConv(torch.nn.Sequential(torch.nn.Linear(F, 24), torch.nn.ReLU(), torch.nn.Linear(24, 12)), eps=0.3, train_eps=True,
                        edge_dim=EDGE_DIM).cuda()
    if which == "gine_plain":                                        # edge_attr already has the width of x
        return GINEConv(torch.nn.Linear(F, 12)).cuda()
    return CFConv(F, 12, 16, torch.nn.Sequential(torch.nn.Linear(EDGE_DIM, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16))).cuda()


def _run_layer(layer, X, EA, info, wgt):
    X, EA = X.detach().clone().requires_grad_(), EA.detach().clone().requires_grad_()
    Y = layer(X, info, EA)
    (Y * wgt.to(Y.dtype)).sum().backward()
    grads = {"Y": Y, "dX": X.grad, "d_edge_attr": EA.grad}
    grads.update({"d_" + name: p.grad for name, p in layer.named_parameters()})
    return grads


@pytest.mark.parametrize("which", ["gine", "gine_plain", "cfconv"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_layers_against_the_fp64_composed_layers(kind, which):
    info, n_dst, n_src, edge_ids = _structure(kind)
    nnz = info.column_index.numel()
    layer = _layers(which)
    X = torch.randn(n_src, F, generator=torch.Generator().manual_seed(7)).cuda()
    EA = _edge_rows(kind, edge_ids, nnz, F if which == "gine_plain" else EDGE_DIM, 8)
    wgt = torch.randn(n_dst, 12, generator=torch.Generator().manual_seed(9)).cuda()
    got = _run_layer(layer, X, EA, info, wgt)
    composed32 = copy.deepcopy(layer)
    composed32.fused = False
    composed64 = copy.deepcopy(composed32).double()
    for p in list(composed32.parameters()) + list(composed64.parameters()):
        p.grad = None
    want = _run_layer(composed64, X.double(), EA.double(), info, wgt)
    assert set(got) == set(want) and len(got) >= 5 and all(v is not None for v in got.values())
    for name in got:
        _close(got[name], want[name], f"{which} fused, {kind}: {name}")
    other = _run_layer(composed32, X, EA, info, wgt)                 # fused=True against fused=False, both within the same bound
    for name in other:
        _close(other[name], want[name], f"{which} composed, {kind}: {name}")


def test_strided_operands_and_an_expanded_gradient():
    info, n, _, _ = _structure("directed")
    nnz = info.column_index.numel()
    gen = torch.Generator().manual_seed(21)
    Xbig = torch.randn(n, F + 7, generator=gen).cuda().requires_grad_()
    Ebig = torch.randn(nnz, F + 3, generator=gen).cuda().requires_grad_()
    X, E = Xbig[:, 4:4 + F], Ebig[:, :F]                             # a column slice and a padded buffer: no copy is made
    assert not X.is_contiguous() and not E.is_contiguous()
    Y = EdgeFeatureSum.apply(X, E, info, "add", "relu")
    saved = Y.grad_fn.saved_tensors
    assert saved[0].data_ptr() == X.data_ptr() and saved[1].data_ptr() == E.data_ptr(), "the strided operands were copied"
    Y.sum().backward()                                               # the incoming gradient is an expanded scalar (strides 0, 0)
    X64, E64 = Xbig.detach().double().requires_grad_(), Ebig.detach().double().requires_grad_()
    composed_edge_feature_sum(X64[:, 4:4 + F], E64[:, :F], info, "add", "relu").sum().backward()
    _close(Xbig.grad, X64.grad, "strided: dX")
    _close(Ebig.grad, E64.grad, "strided: dE")
    # a gradient with transposed strides goes through a copy
    Xbig.grad = Ebig.grad = None
    W = torch.randn(F, n, generator=gen).cuda()
    (EdgeFeatureSum.apply(X, E, info, "mul", "none") * W.t()).sum().backward()
    X64.grad = E64.grad = None
    (composed_edge_feature_sum(X64[:, 4:4 + F], E64[:, :F], info, "mul", "none") * W.t().double()).sum().backward()
    _close(Xbig.grad, X64.grad, "column-major gradient: dX")
    _close(Ebig.grad, E64.grad, "column-major gradient: dE")


def test_no_transposed_structure_is_built_when_x_needs_no_gradient():
    info, n, _, _ = _structure("directed")
    nnz = info.column_index.numel()
    X = torch.randn(n, F, device="cuda")
    E = torch.randn(nnz, F, device="cuda", requires_grad=True)
    EdgeFeatureSum.apply(X, E, info, "add", "relu").sum().backward()
    assert E.grad is not None and "transposed" not in info._edge_arrays()
    X.requires_grad_()
    EdgeFeatureSum.apply(X, E.detach(), info, "add", "relu").sum().backward()
    assert X.grad is not None and "transposed" in info._edge_arrays()
    block = one_block()
    Eb = torch.randn(block.column_index.numel(), F, device="cuda", requires_grad=True)
    EdgeFeatureSum.apply(torch.randn(block.num_src, F, device="cuda"), Eb, block).sum().backward()
    assert Eb.grad is not None and block._transposed is None


def test_a_coarsened_batch_carries_its_edge_attributes():
    b = _batch_with_an_empty_graph()
    nnz = b.column_index.numel()
    b.edge_attr = torch.randn(nnz, EDGE_DIM, generator=torch.Generator().manual_seed(31)).cuda()
    score = torch.randn(b.num_nodes, generator=torch.Generator().manual_seed(32)).cuda()
    small, sel = b.coarsen(score, ratio=0.6, want_edge_ids=True)
    assert b.carry_edge_attr(small, sel) is small and small.column_index.numel() > 0
    ids = sel.edge_ids.long()
    assert torch.equal(small.edge_attr, b.edge_attr[ids])
    # the carried rows sit on the right edges: new edge p joins the new rows of the old edge's two ends
    perm = sel.perm.long()
    assert torch.equal(perm[small.edge_rows().long()], b.edge_rows().long()[ids])
    assert torch.equal(perm[small.column_index.long()], b.column_index.long()[ids])
    layer = _layers("gine")
    X = torch.randn(small.num_nodes, F, generator=torch.Generator().manual_seed(33)).cuda()
    wgt = torch.randn(small.num_nodes, 12, generator=torch.Generator().manual_seed(34)).cuda()
    got = _run_layer(layer, X, small.edge_attr, small, wgt)
    composed64 = copy.deepcopy(layer).double()
    composed64.fused = False
    for p in composed64.parameters():
        p.grad = None
    want = _run_layer(composed64, X.double(), small.edge_attr.double(), small, wgt)
    for name in got:
        _close(got[name], want[name], f"coarsened batch: {name}")
    # the pooling layers carry them on their own
    from gnnadvisor_osdi21_amd.ops import TopKPooling
    for fused in (True, False):
        pool = TopKPooling(F, ratio=0.6, fused=fused).cuda()
        _, pooled, selection, _ = pool(torch.randn(b.num_nodes, F, device="cuda"), b)
        assert pooled.edge_attr is not None and pooled.edge_attr.shape == (pooled.column_index.numel(), EDGE_DIM)
        assert torch.equal(pooled.edge_attr, b.edge_attr[selection.edge_ids.long()])

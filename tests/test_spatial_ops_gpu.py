"""spatial.radius_graph / knn_graph as the layers see them, on the GPU: the GraphBatch they give is accepted by GCNConv, GINEConv
and CFConv; without a cap it is symmetric (reverse_edges() exists, directed is False), with a cap it is directed and the backward
walks the transposed structure; the fused and the composed construction give identical structures; SchNetInteraction against fp64
autograd of the same modules composed from torch ops.

Bound: 1e-4 * max(1, max |ref|) per tensor, the bound of test_edgefeat_ops_gpu.py for outputs, input and parameter gradients (the
sums here are shorter than there: 40 point sets of 3 .. 40 points)."""
import copy

import numpy as np
import pytest
import torch

import spatial_ref as ref
from gnnadvisor_osdi21_amd import graph, spatial
from gnnadvisor_osdi21_amd.edgeconv import CFConv, GINEConv
from gnnadvisor_osdi21_amd.ops import GCNConv
from gnnadvisor_osdi21_amd.structure import TransposedGraph, backward_structure
from util import assert_close_f64

pytestmark = pytest.mark.gpu
CUTOFF = 1.6


def clouds():
    pos, gp, _ = graph.small_point_clouds(40, 3, 40, seed=7, device="cuda")
    return pos, gp


def _close(got, want, what):
    assert_close_f64(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=1e-4, scale=float(want.detach().abs().max()), what=what)


@pytest.mark.parametrize("cap", [None, 6])
def test_the_layers_accept_the_batch(cap):
    pos, gp = clouds()
    batch = spatial.radius_graph(pos, CUTOFF, gp, max_num_neighbors=cap, hiddenDim=16)
    n, nnz = pos.shape[0], batch.column_index.numel()
    assert batch.num_nodes == n and batch.num_graphs == 40 and batch.edge_dist2.shape == (nnz,) and nnz > 2 * n
    assert batch.directed == (cap is not None)
    torch.manual_seed(0)
    x = torch.randn(n, 16, device="cuda", requires_grad=True)
    e = torch.randn(nnz, 16, device="cuda")
    lin = torch.nn.Linear(16, 16).cuda()
    for layer, args in ((GCNConv(16, 16).cuda(), ()), (GINEConv(lin).cuda(), (e,)),
                        (CFConv(16, 16, 16, torch.nn.Linear(1, 16)).cuda(), (batch.edge_dist2[:, None],))):
        out = layer(x, batch, *args)
        assert out.shape == (n, 16) and bool(torch.isfinite(out).all())
        out.sum().backward()
        assert bool(torch.isfinite(x.grad).all())


def test_without_a_cap_the_batch_is_symmetric_and_with_one_it_is_directed():
    pos, gp = clouds()
    plain = spatial.radius_graph(pos, CUTOFF, gp)
    rev = plain.reverse_edges()                                   # (raises on a structure that is not symmetric)
    assert not plain.directed and rev.numel() == plain.column_index.numel()
    assert torch.equal(plain.edge_dist2[rev.long()].view(torch.int32), plain.edge_dist2.view(torch.int32))       # d2(i,j) == d2(j,i)
    assert backward_structure(plain) is plain
    capped = spatial.radius_graph(pos, CUTOFF, gp, max_num_neighbors=3)
    assert capped.directed and isinstance(backward_structure(capped), TransposedGraph)
    assert int((capped.row_pointers[1:] - capped.row_pointers[:-1]).max()) == 3
    with pytest.raises(Exception):
        capped.reverse_edges()                                    # nearest-3 is not a symmetric relation on these sets
    knn = spatial.knn_graph(pos, 5, gp)
    sizes = (gp[1:] - gp[:-1]).long()
    want = torch.repeat_interleave((sizes - 1).clamp(max=5), sizes)
    assert knn.directed and torch.equal((knn.row_pointers[1:] - knn.row_pointers[:-1]).long(), want)


@pytest.mark.parametrize("cap, loop", [(None, False), (None, True), (4, False), (64, True)])
def test_fused_and_composed_give_identical_structures(cap, loop):
    pos, gp = clouds()
    a = spatial.radius_graph(pos, CUTOFF, gp, loop=loop, max_num_neighbors=cap, fused=True)
    b = spatial.radius_graph(pos, CUTOFF, gp, loop=loop, max_num_neighbors=cap, fused=False)
    for key in ("row_pointers", "column_index", "partPtr", "part2Node"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(a.edge_dist2.view(torch.int32), b.edge_dist2.view(torch.int32))
    want = ref.radius_graph(pos.cpu().numpy(), gp.cpu().numpy(), CUTOFF, max_neighbors=cap, loop=loop)
    assert np.array_equal(a.column_index.cpu().numpy(), want["column_index"])


@pytest.mark.parametrize("hidden", [16, 64])
@pytest.mark.parametrize("cap", [None, 8])
def test_the_interaction_matches_fp64_autograd(hidden, cap):
    pos, gp = clouds()
    batch = spatial.radius_graph(pos, CUTOFF, gp, max_num_neighbors=cap, hiddenDim=hidden)
    torch.manual_seed(hidden)
    layer = spatial.SchNetInteraction(hidden, hidden, 12, CUTOFF, fused=True).cuda()
    twin = copy.deepcopy(layer).double()
    twin.conv.fused = False
    x = torch.randn(pos.shape[0], hidden, device="cuda", requires_grad=True)
    x64 = x.detach().double().requires_grad_()
    weight = torch.randn(pos.shape[0], hidden, device="cuda")
    out = layer(x, batch)
    (out * weight).sum().backward()
    want = twin(x64, batch, edge_dist2=batch.edge_dist2.double())
    (want * weight.double()).sum().backward()
    _close(out, want, "out")
    _close(x.grad, x64.grad, "d x")
    theirs = dict(twin.named_parameters())
    for name, p in layer.named_parameters():
        _close(p.grad, theirs[name].grad, "d " + name)

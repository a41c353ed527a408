"""ops.GATAttention / GATConv(fused=True) on sampled blocks against the fp64 layer on the block's [num_dst x num_src] edge list
(tests/gat_rect_ref.py).  Bounds: layer outputs and input gradients 1e-4 of max|ref|, parameter gradients 1e-4 of their sum of
|terms|, two fp32 paths over the same H within the kernel bound 1e-5 of max(1, sum of |terms|)."""
import functools
import types

import numpy as np
import pytest
import torch

import gat_rect_ref as gref
import sampling_ref as sref
from gnnadvisor_osdi21_amd import _lib, ops
from gnnadvisor_osdi21_amd.sampling import NeighborSampler, SampledBlock
from util import assert_close_f64

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_graph():
    rp, ci = sref.shared_graph()
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


def bundle(partSize=32):
    rp, ci = device_graph()
    return types.SimpleNamespace(row_pointers=rp, column_index=ci, partSize=partSize)


def one_block(seeds=65, fanout=5, rng_seed=77):
    b = bundle()
    return SampledBlock.sample(b.row_pointers, b.column_index, torch.from_numpy(sref.seed_sets()[seeds]).cuda(), fanout, rng_seed,
                               partSize=32)


def _max_scale(ref):
    return np.full(ref.shape, float(ref.abs().max()))


@pytest.mark.parametrize("fin,fout,heads,concat", [(8, 4, 1, True), (41, 16, 4, True), (16, 8, 4, False)])
def test_fused_gatconv_on_a_block_matches_the_fp64_layer(fin, fout, heads, concat):
    block = one_block()
    assert block.num_dst == 65 and block.num_src > 65
    torch.manual_seed(fin + heads)
    conv = ops.GATConv(fin, fout, heads=heads, concat=concat, fused=True).cuda()
    X = torch.randn(block.num_src, fin, device="cuda", requires_grad=True)
    Y = conv(X, block)
    assert Y.shape == (65, heads * fout if concat else fout)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    assert X.grad.shape == X.shape

    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    keep = {}
    Y64 = gref.gat_layer64(X64, *P64, block.row_pointers, block.column_index, block.num_dst, heads, fout, concat, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    what = f"GATConv on a block in={fin} out={fout} heads={heads} concat={concat}"
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=_max_scale(ref), what=f"{what} {name}")
    for got, ref, scale, name in zip((conv.weights.grad, conv.att_l.grad, conv.att_r.grad), P64,
                                     gref.param_scales(X64, keep, heads, fout), ("dW", "da_l", "da_r")):
        assert_close_f64(got.cpu().numpy(), ref.grad.cpu().numpy(), rtol=1e-4, scale=scale.cpu().numpy(), what=f"{what} {name}")


def test_the_transpose_is_built_by_the_first_backward_that_needs_it_and_by_nothing_else():
    """What a sum operator's rule (`ops._sum_backward`: no transpose when X needs no gradient) becomes for attention.  The
    gradient of the layer's own weight is X^T dH with dH[j] = sum_i alpha(i, j) dY[i], a sum over the edges that leave source j:
    the source-side pass, which walks block.transposed().  So unlike SAGEConv a first GAT layer with a trainable weight does
    build the transpose even though X needs no gradient.  What holds, and is checked: the forward builds none; a backward that
    does not reach the attention (the layer frozen, a trainable head on top) builds none; the first backward that needs
    H / el / er gradients builds it once, and it is kept."""
    block = one_block(seeds=64, rng_seed=3)
    conv = ops.GATConv(8, 4, heads=2, fused=True).cuda()
    X = torch.randn(block.num_src, 8, device="cuda")                  # X needs no gradient
    with torch.no_grad():
        conv(X, block)
    Y = conv(X, block)
    assert block._transposed is None
    frozen = ops.GATConv(8, 4, heads=2, fused=True).cuda().requires_grad_(False)
    head = torch.nn.Linear(8, 3).cuda()
    head(frozen(X, block)).sum().backward()
    assert block._transposed is None and head.weight.grad is not None
    Y.sum().backward()
    t = block._transposed
    assert t is not None and conv.weights.grad is not None and t.row_pointers.numel() == block.num_src + 1
    conv(X, block).sum().backward()
    assert block._transposed is t


def test_two_blocks_chain_through_two_layers():
    sampler = NeighborSampler(bundle(), [5, 5])
    blocks, input_nodes = sampler.sample(torch.from_numpy(sref.seed_sets()[65]).cuda(), 9)
    assert blocks[0].num_dst == blocks[1].num_src and blocks[1].num_dst == 65
    torch.manual_seed(4)
    conv1 = ops.GATConv(8, 8, heads=2, fused=True).cuda()
    conv2 = ops.GATConv(16, 4, heads=1, fused=True).cuda()
    X = torch.randn(blocks[0].num_src, 8, device="cuda", requires_grad=True)
    Y = conv2(conv1(X, blocks[0]), blocks[1])
    assert Y.shape == (65, 4)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    p1 = [p.detach().double() for p in (conv1.weights, conv1.att_l, conv1.att_r)]
    p2 = [p.detach().double() for p in (conv2.weights, conv2.att_l, conv2.att_r)]
    h = gref.gat_layer64(X64, *p1, blocks[0].row_pointers, blocks[0].column_index, blocks[0].num_dst, 2, 8, True)
    Y64 = gref.gat_layer64(h, *p2, blocks[1].row_pointers, blocks[1].column_index, 65, 1, 4, True)
    (Y64 * wgt.double()).sum().backward()
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=_max_scale(ref), what=f"two layers {name}")
    assert (X.grad != 0).any() and blocks[0]._transposed is not None and blocks[1]._transposed is not None


def test_the_full_block_equals_the_full_graph():
    rp, ci = device_graph()
    n = rp.numel() - 1
    block = SampledBlock.sample(rp, ci, torch.arange(n, dtype=torch.int32, device="cuda"), -1, 5, partSize=32)
    assert block.num_src == block.num_dst == n and torch.equal(block.column_index, ci) and torch.equal(block.row_pointers, rp)
    pp, p2n = _lib.build_part(32, rp.cpu())
    info = types.SimpleNamespace(row_pointers=rp, column_index=ci, partPtr=pp.int().cuda(), part2Node=p2n.int().cuda(), partSize=32,
                                 directed=True)                       # (no symmetry is needed or assumed)
    torch.manual_seed(6)
    conv = ops.GATConv(16, 8, heads=4, fused=True).cuda()
    X = torch.randn(n, 16, device="cuda")
    with torch.no_grad():
        want, got = conv(X, info), conv(X, block)
        H = torch.mm(X, conv.weights).double()
        Hh = H.view(n, 4, 8)
        rows, cl = gref.edges_of(rp, ci, n)
        Y64, _lse, _has, scale = gref.attention64(H, (Hh * conv.att_l.double()).sum(-1), (Hh * conv.att_r.double()).sum(-1), rows, cl,
                                                  n, 4, 0.2)
    for t, name in ((got, "block"), (want, "graph")):
        assert_close_f64(t.cpu().numpy(), Y64.cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what=f"full {name} against fp64")
    assert_close_f64(got.cpu().numpy(), want.double().cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what="full block vs graph")


def test_refusals():
    block = one_block(seeds=64, rng_seed=3)
    X = torch.randn(block.num_src, 8, device="cuda")
    with pytest.raises(TypeError, match="GraphSAGE operators.*GATConv\\(fused=True\\)"):
        ops.GATConv(8, 4).cuda()(X, block)
    with pytest.raises(TypeError, match="float32"):
        ops.GATConv(8, 4, fused=True).cuda().half()(X.half(), block)
    with pytest.raises(TypeError, match="float32"):
        ops.GATConv(8, 4, fused=True).cuda().bfloat16()(X.bfloat16(), block)
    with pytest.raises(ValueError, match="num_src"):
        ops.GATConv(8, 4, fused=True).cuda()(X[:-1], block)
    for layer in (ops.GCNConv(8, 4), ops.GINConv(8, 4)):
        with pytest.raises(TypeError, match="GraphSAGE operators"):
            layer.cuda()(X, block)

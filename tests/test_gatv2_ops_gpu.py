"""ops.GATv2Attention / ops.GATv2Conv (fused) against the fp64 layer of tests/gatv2_ref.py on a full (symmetric) graph, a directed
graph and a two-layer chain of sampled blocks.  Bounds as test_gat_block_ops_gpu.py -- layer outputs and input gradients 1e-4 of
max|ref|, parameter gradients 1e-4 of their sum of |terms| -- each times max(1, S), S = the largest sum_d |att| |lrelu(t)| of an
edge (gatv2_ref's docstring)."""
import functools
import types

import numpy as np
import pytest
import torch

import gatv2_ref as vref
import sampling_ref as sref
from gnnadvisor_osdi21_amd import _lib, graph, ops
from gnnadvisor_osdi21_amd.decider import inputProperty
from gnnadvisor_osdi21_amd.sampling import NeighborSampler, SampledBlock
from util import assert_close_f64

pytestmark = pytest.mark.gpu


def _info(g, partSize=32, directed=False):
    ds = types.SimpleNamespace(num_nodes=g.num_nodes, avg_degree=g.avg_degree, avg_edgeSpan=g.avg_edgeSpan, num_features=16)
    ip = inputProperty(g.row_pointers.cuda(), g.column_index.cuda(), g.degrees.cuda(), partSize, 32, 4, hiddenDim=16, dataset_obj=ds)
    pp, p2n = _lib.build_part(partSize, g.row_pointers)
    ip.partPtr, ip.part2Node = pp.cuda(), p2n.cuda()
    ip.directed = directed
    return ip


@functools.lru_cache(maxsize=None)
def _graph(kind):
    if kind == "symmetric":
        return graph.powerlaw_graph(500, 8000, 300, seed=4)
    return graph.uniform_graph(300, 3000, symmetric=False)


@functools.lru_cache(maxsize=None)
def device_graph():
    rp, ci = sref.shared_graph()
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


def one_block(seeds=65, fanout=5, rng_seed=77):
    rp, ci = device_graph()
    return SampledBlock.sample(rp, ci, torch.from_numpy(sref.seed_sets()[seeds]).cuda(), fanout, rng_seed, partSize=32)


def _max_scale(ref):
    return np.full(ref.shape, float(ref.abs().max()))


def _params64(conv):
    return [None if p is None else p.detach().double().requires_grad_() for p in (conv.W_l, conv.W_r, conv.att)]


def _check_layer(conv, X, info, rp, ci, n_dst, what, p=0.0, rng_seed=0):
    """One forward and backward of `conv` against gatv2_layer64: Y, dX and every parameter gradient."""
    heads, fout, concat = conv.heads, conv.out_dim, conv.concat
    Y = conv(X, info, rng_seed=rng_seed) if p > 0 else conv(X, info)
    assert Y.shape == (n_dst, heads * fout if concat or heads == 1 else fout)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = _params64(conv)
    keep = {}
    Y64 = vref.gatv2_layer64(X64, *P64, rp, ci, n_dst, heads, fout, concat, conv.negative_slope, p, rng_seed, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    s_Wl, s_Wr, s_att, S = vref.param_scales(X64, keep)
    rtol = 1e-4 * max(1.0, S)
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=rtol, scale=_max_scale(ref), what=f"{what} {name}")
    for got, ref, scale, name in ((conv.W_l, P64[0], s_Wl, "dW_l"), (conv.W_r, P64[1], s_Wr, "dW_r"), (conv.att, P64[2], s_att, "d_att")):
        if ref is not None:
            assert_close_f64(got.grad.cpu().numpy(), ref.grad.cpu().numpy(), rtol=rtol, scale=scale.cpu().numpy(), what=f"{what} {name}")


@pytest.mark.parametrize("kind", ["symmetric", "directed"])
@pytest.mark.parametrize("fin,fout,heads,concat,share", [(8, 4, 1, True, False), (41, 16, 4, True, True), (16, 8, 4, False, False),
                                                         (12, 5, 3, False, True)])
def test_fused_layer_on_a_graph_matches_the_fp64_layer(kind, fin, fout, heads, concat, share):
    g = _graph(kind)
    info = _info(g, 32 if heads == 1 else 3, directed=kind == "directed")
    torch.manual_seed(fin + heads)
    conv = ops.GATv2Conv(fin, fout, heads=heads, concat=concat, share_weights=share).cuda()
    assert conv.fused and (conv.W_r is None) == share
    X = torch.randn(g.num_nodes, fin, device="cuda", requires_grad=True)
    _check_layer(conv, X, info, info.row_pointers, info.column_index, g.num_nodes,
                 f"GATv2Conv {kind} in={fin} out={fout} heads={heads} concat={concat} share={share}")


@pytest.mark.parametrize("fin,fout,heads,concat,share", [(8, 4, 1, True, True), (41, 16, 4, True, False), (16, 8, 4, False, True)])
def test_fused_layer_on_a_block_matches_the_fp64_layer(fin, fout, heads, concat, share):
    block = one_block()
    assert block.num_dst == 65 and block.num_src > 65
    torch.manual_seed(fin + heads)
    conv = ops.GATv2Conv(fin, fout, heads=heads, concat=concat, share_weights=share).cuda()
    X = torch.randn(block.num_src, fin, device="cuda", requires_grad=True)
    _check_layer(conv, X, block, block.row_pointers, block.column_index, 65,
                 f"GATv2Conv on a block in={fin} out={fout} heads={heads} concat={concat} share={share}")
    assert block._transposed is not None


def test_attention_function_with_the_mask_and_node_sized_saved_tensors():
    """GATv2Attention.apply with attn_drop on a directed graph: (dHs, dHd, d_att) against fp64 autograd with the restated mask."""
    g = _graph("directed")
    info = _info(g, 3, directed=True)
    heads, dim, p, seed = 4, 16, 0.5, 2 ** 63 + 11
    Hs, Hd, att, G = [t.cuda() for t in vref.inputs(g.num_nodes, g.num_nodes, heads, dim, 6)]
    for t in (Hs, Hd, att):
        t.requires_grad_()
    Y = ops.GATv2Attention.apply(Hs, Hd, att, info, 0.2, p, seed)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 5 and all(t.numel() <= g.num_nodes * heads * dim for t in saved), "saved tensors are node-sized"
    (Y * G).sum().backward()
    r = vref.kernel_reference(Hs, Hd, att, G, info.row_pointers, info.column_index, heads, 0.2, p, seed, "GATv2Attention")
    n = lambda t: t.detach().cpu().numpy()
    rtol = 1e-5 * r.factor
    assert_close_f64(n(Y), n(r.Y), rtol=rtol, scale=n(r.s_Y), what="Y")
    assert_close_f64(n(Hs.grad[r.ok_dHs]), n(r.dHs[r.ok_dHs]), rtol=rtol, scale=n(r.s_dHs[r.ok_dHs]), what="dHs")
    assert_close_f64(n(Hd.grad[r.ok_dHd]), n(r.dHd[r.ok_dHd]), rtol=rtol, scale=n(r.s_dHd[r.ok_dHd]), what="dHd")
    assert_close_f64(n(att.grad), n(r.d_att), rtol=rtol, scale=n(r.s_att), what="d_att")
    # only what needs a gradient gets one, and a graph that needs none runs no backward kernel
    Hs2, att2 = Hs.detach().requires_grad_(), att.detach()
    ops.GATv2Attention.apply(Hs2, Hd.detach(), att2, info, 0.2).sum().backward()
    assert Hs2.grad is not None and att2.grad is None


def test_two_blocks_chain_through_two_layers():
    sampler = NeighborSampler(types.SimpleNamespace(row_pointers=device_graph()[0], column_index=device_graph()[1], partSize=32), [5, 5])
    blocks, input_nodes = sampler.sample(torch.from_numpy(sref.seed_sets()[65]).cuda(), 9)
    assert blocks[0].num_dst == blocks[1].num_src and blocks[1].num_dst == 65
    torch.manual_seed(4)
    conv1 = ops.GATv2Conv(8, 8, heads=2).cuda()
    conv2 = ops.GATv2Conv(16, 4, heads=1, share_weights=True).cuda()
    X = torch.randn(blocks[0].num_src, 8, device="cuda", requires_grad=True)
    Y = conv2(conv1(X, blocks[0]), blocks[1])
    assert Y.shape == (65, 4)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    p1, p2 = [None if p is None else p.detach().double() for p in _params64(conv1)], \
        [None if p is None else p.detach().double() for p in _params64(conv2)]
    k1, k2 = {}, {}
    h = vref.gatv2_layer64(X64, *p1, blocks[0].row_pointers, blocks[0].column_index, blocks[0].num_dst, 2, 8, True, keep=k1)
    Y64 = vref.gatv2_layer64(h, *p2, blocks[1].row_pointers, blocks[1].column_index, 65, 1, 4, True, keep=k2)
    (Y64 * wgt.double()).sum().backward()
    S = max(vref.param_scales(X64, k1)[3], vref.param_scales(h, k2)[3])
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-4 * max(1.0, S), scale=_max_scale(ref),
                         what=f"two layers {name}")
    assert (X.grad != 0).any() and blocks[0]._transposed is not None and blocks[1]._transposed is not None


def test_fused_equals_composed_on_a_small_graph():
    g = _graph("symmetric")
    info = _info(g, 32)
    torch.manual_seed(3)
    fused = ops.GATv2Conv(12, 8, heads=2).cuda()
    composed = ops.GATv2Conv(12, 8, heads=2, fused=False).cuda()
    composed.load_state_dict(fused.state_dict())
    X = torch.randn(g.num_nodes, 12, device="cuda")
    wgt = torch.randn(g.num_nodes, 16, device="cuda")
    res = []
    for conv in (fused, composed):
        Xc = X.clone().requires_grad_()
        Y = conv(Xc, info)
        (Y * wgt).sum().backward()
        res.append((Y.detach(), Xc.grad, conv.W_l.grad, conv.W_r.grad, conv.att.grad))
    X64 = X.double().requires_grad_()
    keep = {}
    P64 = _params64(fused)
    Y64 = vref.gatv2_layer64(X64, *P64, info.row_pointers, info.column_index, g.num_nodes, 2, 8, True, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    s_Wl, s_Wr, s_att, S = vref.param_scales(X64, keep)
    scales = (_max_scale(Y64.detach()), _max_scale(X64.grad), s_Wl.cpu().numpy(), s_Wr.cpu().numpy(), s_att.cpu().numpy())
    for a, b, scale, name in zip(res[0], res[1], scales, ("Y", "dX", "dW_l", "dW_r", "d_att")):
        # (each path is within 1e-4 of the fp64 layer on this scale: the two are within twice that of each other)
        assert_close_f64(a.cpu().numpy(), b.double().cpu().numpy(), rtol=2e-4 * max(1.0, S), scale=scale, what=f"fused vs composed {name}")
    with pytest.raises(TypeError, match="GATv2Conv\\(fused=False\\) does not take a SampledBlock"):
        composed(torch.randn(one_block().num_src, 12, device="cuda"), one_block())


def test_dropout_trains_with_the_restated_mask_and_eval_ignores_it():
    g = _graph("symmetric")
    info = _info(g, 32)
    torch.manual_seed(9)
    conv = ops.GATv2Conv(10, 6, heads=3, attn_drop=0.5).cuda()
    X = torch.randn(g.num_nodes, 10, device="cuda", requires_grad=True)
    _check_layer(conv, X, info, info.row_pointers, info.column_index, g.num_nodes, "GATv2Conv attn_drop=0.5", p=0.5, rng_seed=1234567)
    assert conv.last_rng_seed == 1234567
    with torch.no_grad():
        a = conv(X, info)
        assert isinstance(conv.last_rng_seed, int) and conv.last_rng_seed != 1234567      # a seed drawn on the host
        first = conv.last_rng_seed
        b = conv(X, info)
        assert conv.last_rng_seed != first and not torch.equal(a, b)
        conv.eval()
        plain = ops.GATv2Conv(10, 6, heads=3).cuda()
        plain.load_state_dict(conv.state_dict())
        e1, e2, want = conv(X, info), conv(X, info, rng_seed=5), plain(X, info)
        # the layer without the mask, in fp64: what both must compute (layer bound, S of this layer's attention)
        keep = {}
        Y64 = vref.gatv2_layer64(X.detach().double(), *[q.detach() for q in _params64(conv)], info.row_pointers, info.column_index,
                                 g.num_nodes, 3, 6, True, keep=keep)
        S = vref.magnitudes(keep["Hs"], keep["Hd"], keep["att"], torch.zeros_like(keep["Y"]), keep["lse"], keep["rows"], keep["cl"],
                            3, 0.2).S
    for e in (e1, e2, want):
        assert_close_f64(e.cpu().numpy(), Y64.cpu().numpy(), rtol=1e-4 * max(1.0, S), scale=_max_scale(Y64),
                         what="eval() ignores attn_drop")


def test_an_unsymmetric_undirected_graph_raises_at_the_first_backward():
    g = _graph("directed")
    info = _info(g, 32, directed=False)               # the structure is not symmetric and nobody says it is directed
    conv = ops.GATv2Conv(8, 4, heads=2).cuda()
    X = torch.randn(g.num_nodes, 8, device="cuda")
    Y = conv(X, info)                                 # the forward needs nothing of the kind
    with pytest.raises(Exception, match="symmetric"):
        Y.sum().backward()

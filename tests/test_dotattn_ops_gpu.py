"""ops.DotAttention / ops.TransformerConv (fused) against the fp64 layer of tests/dotattn_ref.py on a full (symmetric) graph, a
directed graph and a two-layer chain of sampled blocks.  Bounds as test_gatv2_ops_gpu.py -- layer outputs and input gradients 1e-4
of max|ref|, weight gradients 1e-4 of their sum of |terms| -- each times max(1, S), S = the largest |scale| sum_d |Q| |K| of an
edge (dotattn_ref's docstring)."""
import functools
import types

import numpy as np
import pytest
import torch

import dotattn_ref as tref
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
    return [None if p is None else p.detach().double().requires_grad_() for p in (conv.weights, conv.W_skip)]


def _check_layer(conv, X, info, rp, ci, n_dst, what, p=0.0, rng_seed=0):
    """One forward and backward of `conv` against transformer_layer64: Y, dX and every weight gradient."""
    heads, fout, concat = conv.heads, conv.out_dim, conv.concat
    Y = conv(X, info, rng_seed=rng_seed) if p > 0 else conv(X, info)
    assert Y.shape == (n_dst, heads * fout if concat or heads == 1 else fout)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = _params64(conv)
    keep = {}
    Y64 = tref.transformer_layer64(X64, *P64, rp, ci, n_dst, heads, fout, concat, p, rng_seed, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    s_W, s_skip, S = tref.param_scales(X64, keep)
    print(f"{what}: S = {S:.3f}")
    rtol = 1e-4 * max(1.0, S)
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=rtol, scale=_max_scale(ref), what=f"{what} {name}")
    for got, ref, scale, name in ((conv.weights, P64[0], s_W, "dW"), (conv.W_skip, P64[1], s_skip, "dW_skip")):
        if ref is not None:
            assert_close_f64(got.grad.cpu().numpy(), ref.grad.cpu().numpy(), rtol=rtol, scale=scale.cpu().numpy(), what=f"{what} {name}")


@pytest.mark.parametrize("kind", ["symmetric", "directed"])
@pytest.mark.parametrize("fin,fout,heads,concat,root", [(8, 4, 1, True, True), (41, 16, 4, True, False), (16, 8, 4, False, True),
                                                        (12, 5, 3, False, False)])
def test_fused_layer_on_a_graph_matches_the_fp64_layer(kind, fin, fout, heads, concat, root):
    g = _graph(kind)
    info = _info(g, 32 if heads == 1 else 3, directed=kind == "directed")
    torch.manual_seed(fin + heads)
    conv = ops.TransformerConv(fin, fout, heads=heads, concat=concat, root_weight=root).cuda()
    assert conv.fused and (conv.W_skip is not None) == root
    X = torch.randn(g.num_nodes, fin, device="cuda", requires_grad=True)
    _check_layer(conv, X, info, info.row_pointers, info.column_index, g.num_nodes,
                 f"TransformerConv {kind} in={fin} out={fout} heads={heads} concat={concat} root_weight={root}")


@pytest.mark.parametrize("fin,fout,heads,concat,root", [(8, 4, 1, True, False), (41, 16, 4, True, True), (16, 8, 4, False, True)])
def test_fused_layer_on_a_block_matches_the_fp64_layer(fin, fout, heads, concat, root):
    block = one_block()
    assert block.num_dst == 65 and block.num_src > 65
    torch.manual_seed(fin + heads)
    conv = ops.TransformerConv(fin, fout, heads=heads, concat=concat, root_weight=root).cuda()
    X = torch.randn(block.num_src, fin, device="cuda", requires_grad=True)
    _check_layer(conv, X, block, block.row_pointers, block.column_index, 65,
                 f"TransformerConv on a block in={fin} out={fout} heads={heads} concat={concat} root_weight={root}")
    assert block._transposed is not None


def test_attention_function_with_the_mask_and_node_sized_saved_tensors():
    """DotAttention.apply with attn_drop on a directed graph, Q, K and V as column slices of one matrix: the gradient of that
    matrix against fp64 autograd with the restated mask; an explicit scale."""
    g = _graph("directed")
    info = _info(g, 3, directed=True)
    heads, dim, p, seed, scale = 4, 16, 0.5, 2 ** 63 + 11, 0.3
    W = heads * dim
    gen = torch.Generator().manual_seed(6)
    P = torch.randn(g.num_nodes, 3 * W, generator=gen).cuda().requires_grad_()
    G = torch.randn(g.num_nodes, W, generator=gen).cuda()
    Q, K, V = P[:, :W], P[:, W:2 * W], P[:, 2 * W:]
    Y = ops.DotAttention.apply(Q, K, V, info, heads, scale, p, seed)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 5 and all(t.numel() <= g.num_nodes * W for t in saved), "saved tensors are node-sized"
    assert saved[1].data_ptr() == K.data_ptr() and saved[1].stride(0) == 3 * W, "the slices are passed on, not copied"
    (Y * G).sum().backward()
    r = tref.kernel_reference(Q, K, V, G, info.row_pointers, info.column_index, heads, scale, p, seed)
    n = lambda t: t.detach().cpu().numpy()
    rtol = 1e-5 * r.factor
    assert_close_f64(n(Y), n(r.Y), rtol=rtol, scale=n(r.s_Y), what="Y")
    for lo, ref, s, name in ((0, r.dQ, r.s_dQ, "dQ"), (W, r.dK, r.s_dK, "dK"), (2 * W, r.dV, r.s_dV, "dV")):
        assert_close_f64(n(P.grad[:, lo:lo + W]), n(ref), rtol=rtol, scale=n(s), what=name)
    # the default scale is 1 / sqrt(dim)
    Yd = ops.DotAttention.apply(Q.detach(), K.detach(), V.detach(), info, heads)
    rd = tref.kernel_reference(Q, K, V, G, info.row_pointers, info.column_index, heads, 1 / dim ** 0.5)
    assert_close_f64(n(Yd), n(rd.Y), rtol=1e-5 * rd.factor, scale=n(rd.s_Y), what="default scale")
    # only what needs a gradient gets one
    Q2, K2 = Q.detach().clone().requires_grad_(), K.detach().clone()
    ops.DotAttention.apply(Q2, K2, V.detach(), info, heads).sum().backward()
    assert Q2.grad is not None and K2.grad is None


def test_two_blocks_chain_through_two_layers():
    sampler = NeighborSampler(types.SimpleNamespace(row_pointers=device_graph()[0], column_index=device_graph()[1], partSize=32), [5, 5])
    blocks, input_nodes = sampler.sample(torch.from_numpy(sref.seed_sets()[65]).cuda(), 9)
    assert blocks[0].num_dst == blocks[1].num_src and blocks[1].num_dst == 65
    torch.manual_seed(4)
    conv1 = ops.TransformerConv(8, 8, heads=2).cuda()
    conv2 = ops.TransformerConv(16, 4, heads=1, root_weight=False).cuda()
    X = torch.randn(blocks[0].num_src, 8, device="cuda", requires_grad=True)
    Y = conv2(conv1(X, blocks[0]), blocks[1])
    assert Y.shape == (65, 4)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    p1, p2 = [None if p is None else p.detach() for p in _params64(conv1)], [None if p is None else p.detach() for p in _params64(conv2)]
    k1, k2 = {}, {}
    h = tref.transformer_layer64(X64, *p1, blocks[0].row_pointers, blocks[0].column_index, blocks[0].num_dst, 2, 8, True, keep=k1)
    Y64 = tref.transformer_layer64(h, *p2, blocks[1].row_pointers, blocks[1].column_index, 65, 1, 4, True, keep=k2)
    (Y64 * wgt.double()).sum().backward()
    S = max(tref.param_scales(X64, k1)[2], tref.param_scales(h, k2)[2])
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-4 * max(1.0, S), scale=_max_scale(ref),
                         what=f"two layers {name}")
    assert (X.grad != 0).any() and blocks[0]._transposed is not None and blocks[1]._transposed is not None


def test_fused_equals_composed_on_a_small_graph():
    g = _graph("symmetric")
    info = _info(g, 32)
    torch.manual_seed(3)
    fused = ops.TransformerConv(12, 8, heads=2).cuda()
    composed = ops.TransformerConv(12, 8, heads=2, fused=False).cuda()
    composed.load_state_dict(fused.state_dict())
    X = torch.randn(g.num_nodes, 12, device="cuda")
    wgt = torch.randn(g.num_nodes, 16, device="cuda")
    res = []
    for conv in (fused, composed):
        Xc = X.clone().requires_grad_()
        Y = conv(Xc, info)
        (Y * wgt).sum().backward()
        res.append((Y.detach(), Xc.grad, conv.weights.grad, conv.W_skip.grad))
    X64 = X.double().requires_grad_()
    keep = {}
    P64 = _params64(fused)
    Y64 = tref.transformer_layer64(X64, *P64, info.row_pointers, info.column_index, g.num_nodes, 2, 8, True, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    s_W, s_skip, S = tref.param_scales(X64, keep)
    scales = (_max_scale(Y64.detach()), _max_scale(X64.grad), s_W.cpu().numpy(), s_skip.cpu().numpy())
    for a, b, scale, name in zip(res[0], res[1], scales, ("Y", "dX", "dW", "dW_skip")):
        # (each path is within 1e-4 of the fp64 layer on this scale: the two are within twice that of each other)
        assert_close_f64(a.cpu().numpy(), b.double().cpu().numpy(), rtol=2e-4 * max(1.0, S), scale=scale, what=f"fused vs composed {name}")
    with pytest.raises(TypeError, match="TransformerConv\\(fused=False\\) does not take a SampledBlock"):
        composed(torch.randn(one_block().num_src, 12, device="cuda"), one_block())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(TypeError, match="inside torch.autocast"):
            fused(X, info)


def test_dropout_trains_with_the_restated_mask_and_eval_ignores_it():
    g = _graph("symmetric")
    info = _info(g, 32)
    torch.manual_seed(9)
    conv = ops.TransformerConv(10, 6, heads=3, attn_drop=0.5).cuda()
    X = torch.randn(g.num_nodes, 10, device="cuda", requires_grad=True)
    _check_layer(conv, X, info, info.row_pointers, info.column_index, g.num_nodes, "TransformerConv attn_drop=0.5", p=0.5, rng_seed=1234567)
    assert conv.last_rng_seed == 1234567
    with torch.no_grad():
        a = conv(X, info)
        assert isinstance(conv.last_rng_seed, int) and conv.last_rng_seed != 1234567      # a seed drawn on the host
        first = conv.last_rng_seed
        b = conv(X, info)
        assert conv.last_rng_seed != first and not torch.equal(a, b)
        conv.eval()
        plain = ops.TransformerConv(10, 6, heads=3).cuda()
        plain.load_state_dict(conv.state_dict())
        e1, e2, want = conv(X, info), conv(X, info, rng_seed=5), plain(X, info)
        # the layer without the mask, in fp64: what both must compute (layer bound, S of this layer's attention)
        keep = {}
        Y64 = tref.transformer_layer64(X.detach().double(), *[q.detach() for q in _params64(conv)], info.row_pointers,
                                       info.column_index, g.num_nodes, 3, 6, True, keep=keep)
        P, Wd = keep["P"], keep["Wd"]
        S = tref.magnitudes(P[:, :Wd], P[:, Wd:2 * Wd], P[:, 2 * Wd:], torch.zeros_like(keep["Y"]), keep["lse"], keep["rows"],
                            keep["cl"], 3, keep["scale"]).S
    for e in (e1, e2, want):
        assert_close_f64(e.cpu().numpy(), Y64.cpu().numpy(), rtol=1e-4 * max(1.0, S), scale=_max_scale(Y64),
                         what="eval() ignores attn_drop")


def test_an_unsymmetric_undirected_graph_raises_at_the_first_backward():
    g = _graph("directed")
    info = _info(g, 32, directed=False)               # the structure is not symmetric and nobody says it is directed
    conv = ops.TransformerConv(8, 4, heads=2).cuda()
    X = torch.randn(g.num_nodes, 8, device="cuda")
    Y = conv(X, info)                                 # the forward needs nothing of the kind
    with pytest.raises(Exception, match="symmetric"):
        Y.sum().backward()

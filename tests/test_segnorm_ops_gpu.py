"""Per-graph normalisation through the operators on the GPU: ops.SegmentNorm, ops.graph_norm and ops.GraphNorm (fused and composed)
against fp64 autograd of the plain formula (segnorm_ref.graph_norm_f64), on a batching.GraphBatch, after a conv layer and on a
coarsened batch; what the op saves; and the two bindings.

Bound: |got - ref| <= 1e-4 * max(1, sum |terms|), the sum of the absolute values of the terms of each output's formula, written
out in segnorm_ref.graph_norm_f64 for the output, the gradient of x and the three parameter gradients."""
import numpy as np
import pytest
import torch

import segnorm_ref
from gnnadvisor_osdi21_amd import _lib, graph, load_extension, ops
from gnnadvisor_osdi21_amd.batching import GraphBatch

pytestmark = pytest.mark.gpu

_made = {}
SIZES = [1] + [int(v) for v in np.random.default_rng(321).integers(1, 91, size=39)]
EPS = 1e-5


def _batch():
    """40 graphs of 1 .. 90 nodes, seeded."""
    if "batch" not in _made:
        graphs = [graph.uniform_graph(n, 3 * n, seed=700 + k) for k, n in enumerate(SIZES)]
        _made["batch"] = GraphBatch.from_graphs(graphs, partSize=8).to("cuda")
    return _made["batch"]


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _set_parameters(layer, seed):
    """Values away from the initial ones, so that every gradient has something to show."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, centre in (("weight", 1.0), ("bias", 0.0), ("mean_scale", 0.6)):
            p = getattr(layer, name)
            if p is not None:
                p.copy_((centre + 0.4 * torch.randn(p.shape, generator=g)).cuda())
    return layer


def _host(t):
    return None if t is None else t.detach().cpu().numpy()


def _check_layer(layer, x, batch, what):
    """layer(x, batch) and the gradients of x and of every parameter the layer has against fp64 autograd of the plain formula."""
    gp = batch.graph_pointers if hasattr(batch, "graph_pointers") else batch
    wgt = _rand(*x.shape, seed=99)
    leaf = x.detach().clone().requires_grad_()
    layer.zero_grad(set_to_none=True)
    y = layer(leaf, batch)
    (y * wgt).sum().backward()
    ref = segnorm_ref.graph_norm_f64(_host(x), _host(gp), _host(layer.weight), _host(layer.bias), _host(layer.mean_scale), layer.eps,
                                     _host(wgt))
    got = {"out": y, "d_input": leaf.grad, "d_weight": None if layer.weight is None else layer.weight.grad,
           "d_bias": None if layer.bias is None else layer.bias.grad, "d_alpha": None if layer.mean_scale is None else layer.mean_scale.grad}
    for name, t in got.items():
        if t is None:
            continue
        err, bound = np.abs(_host(t).astype(np.float64) - ref[name]), ref["bound_" + name]
        print(f"{what} {name}: worst err / bound {float((err / bound).max()):.4f}")
        assert (err <= bound).all(), f"{what} {name}: worst err / bound {float((err / bound).max()):.3f}"
    return y


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("F", [7, 64])
def test_graph_norm_and_all_its_gradients_against_fp64(F, fused):
    b = _batch()
    x = 0.7 + 1.3 * _rand(b.num_nodes, F, seed=F)
    layer = _set_parameters(ops.GraphNorm(F, fused=fused).cuda(), seed=1)
    assert sorted(n for n, _ in layer.named_parameters()) == ["bias", "mean_scale", "weight"]
    _check_layer(layer, x, b, f"GraphNorm F={F} {'fused' if fused else 'composed'}")


@pytest.mark.parametrize("F", [7, 64])
def test_fused_against_composed(F):
    b = _batch()
    x = 0.7 + 1.3 * _rand(b.num_nodes, F, seed=F + 1)
    fused, composed = _set_parameters(ops.GraphNorm(F).cuda(), seed=2), _set_parameters(ops.GraphNorm(F, fused=False).cuda(), seed=2)
    yf, yc = _check_layer(fused, x, b, "fused"), _check_layer(composed, x, b, "composed")      # each inside the bound of fp64
    print("fused - composed:", float((yf - yc).detach().abs().max()))
    for name in ("weight", "bias", "mean_scale"):
        print(name, float((getattr(fused, name).grad - getattr(composed, name).grad).abs().max()))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mean_scale, affine", [(False, True), (True, False), (False, False)])
def test_without_the_mean_scale_and_without_the_affine_part(mean_scale, affine, fused):
    b = _batch()
    x = 0.7 + 1.3 * _rand(b.num_nodes, 16, seed=5)
    layer = _set_parameters(ops.GraphNorm(16, mean_scale=mean_scale, affine=affine, fused=fused).cuda(), seed=3)
    assert (layer.mean_scale is None) == (not mean_scale) and (layer.weight is None) == (layer.bias is None) == (not affine)
    _check_layer(layer, x, b, f"GraphNorm mean_scale={mean_scale} affine={affine} {'fused' if fused else 'composed'}")


def test_the_initial_layer_and_the_function_form():
    b = _batch()
    x = 0.7 + 1.3 * _rand(b.num_nodes, 16, seed=6)
    layer = ops.GraphNorm(16).cuda()
    assert bool((layer.weight == 1).all() and (layer.bias == 0).all() and (layer.mean_scale == 1).all())
    y = _check_layer(layer, x, b, "initial")
    # graph_norm with graph_pointers alone, and without parameters: the same bits (ones, zeros and ones are the defaults' values)
    assert torch.equal(ops.graph_norm(x, b.graph_pointers), y.detach())
    assert torch.equal(ops.graph_norm(x, b, layer.weight, layer.bias, layer.mean_scale, EPS), y.detach())
    assert torch.equal(ops.SegmentNorm.apply(x, b, None, None, None, EPS), y.detach())
    with pytest.raises(TypeError, match="float32 only"):
        layer(x.half(), b)
    with pytest.raises(ValueError, match="eps must be finite and > 0"):
        ops.GraphNorm(16, eps=0.0)


def test_after_a_conv_layer_and_on_a_coarsened_batch():
    b = _batch()
    torch.manual_seed(11)
    conv, pool = ops.GINConv(12, 32).cuda(), ops.TopKPooling(32).cuda()
    norm = _set_parameters(ops.GraphNorm(32).cuda(), seed=4)
    x = _rand(b.num_nodes, 12, seed=7)
    h = conv(x, b)
    _check_layer(norm, h.detach(), b, "after GINConv")
    small_x, small, _sel, _gate = pool(torch.relu(norm(h, b)), b)
    assert small.num_graphs == b.num_graphs and 0 < small.num_nodes < b.num_nodes
    _check_layer(norm, small_x.detach(), small, "on the coarsened batch")
    # a gradient reaches the conv layer's weights through the normalisation on the coarsened batch
    norm.zero_grad(set_to_none=True)
    norm(conv(small_x.detach()[:, :12].contiguous(), small), small).square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in list(conv.parameters()) + list(norm.parameters()))


def test_the_op_saves_nothing_of_the_size_of_x_besides_x():
    b = _batch()
    N, G, F = b.num_nodes, b.num_graphs, 16
    x = _rand(N, F, seed=8).requires_grad_()
    layer = _set_parameters(ops.GraphNorm(F).cuda(), seed=5)
    y = layer(x, b)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert sorted(tuple(t.shape) for t in saved) == sorted([(N, F), (G, F), (G, F), (G + 1,), (F,), (F,)])
    assert [t.data_ptr() for t in saved if tuple(t.shape) == (N, F)] == [x.data_ptr()]
    # x needs no gradient: the pass over the rows is skipped, the parameter gradients are the same bits
    y.sum().backward()
    with_x = [p.grad.clone() for p in layer.parameters()]
    layer.zero_grad(set_to_none=True)
    layer(x.detach(), b).sum().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(with_x, layer.parameters()))


def test_the_two_bindings_agree_bit_for_bit():
    GNNA = load_extension()
    b = _batch()
    gp = b.graph_pointers
    for F in (7, 64):
        x, dy = 0.7 + 1.3 * _rand(b.num_nodes, F, seed=9), _rand(b.num_nodes, F, seed=10)
        w, bias, a = (_rand(F, seed=s) for s in (11, 12, 13))
        mean, m2 = GNNA.segment_moments(x, gp)
        res = _lib.segment_moments(x, gp)
        assert torch.equal(mean, res["mean"]) and torch.equal(m2, res["m2"])
        for params in ((w, bias, a), (None, None, None), (w, None, None), (None, None, a)):
            y, mean, rstd = GNNA.segment_norm(x, gp, *params, EPS)
            res = _lib.segment_norm(x, gp, *params, eps=EPS)
            assert torch.equal(y, res["out"]) and torch.equal(mean, res["mean"]) and torch.equal(rstd, res["rstd"])
            for need_input in (True, False):
                dx, A, B = GNNA.segment_norm_backward(dy, x, mean, rstd, gp, params[0], params[2], need_input)
                dx2, A2, B2 = _lib.segment_norm_backward(dy, x, mean, rstd, gp, params[0], params[2], need_input=need_input)
                assert torch.equal(A, A2) and torch.equal(B, B2)
                assert (dx is None and dx2 is None) if not need_input else torch.equal(dx, dx2)

"""NeighborSoftmax, SoftmaxAggregation and GENConv on the GPU, against fp64 autograd of the dense formula
(softagg_ref.dense_forward) on graphs of about 300 rows: a symmetric one, a directed one and a block sampled from a power-law
graph.

Bounds, all of the project's form 1e-4 * max(1, sum of |terms|) (assert_close_f64), the scales those of softagg_ref.reference for
the loss sum(Y * G): sum alpha |x| for Y, sum alpha |G| (1 + |t| (|x_j| + |Y_i|)) for dX, sum |G| (sq + Y^2) for dt.  GENConv's
scales are the layer on magnitudes (|X|, |W|, |b|, relu' <= 1, the aggregation's own scales where a gradient crosses it)."""
import types

import pytest
import torch

from gnnadvisor_osdi21_amd import ops
from gnnadvisor_osdi21_amd.sampling import NeighborSampler
from util import assert_close_f64, make_case

import softagg_ref as S
from test_pna_ops_gpu import _directed_info, _directed_structure
from test_reduce_ops_gpu import _Info

pytestmark = pytest.mark.gpu

N = 300


def _randn(n, d, seed):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


def _powerlaw():
    g, _, _, _ = make_case(N, 4000, 1, 32, seed=3, kind="powerlaw")
    return g


def _structure(kind):
    """(inputInfo, row_pointers, column_index, num_out_rows, num_in_rows), the CSR on the CPU"""
    if kind == "symmetric":
        g = _powerlaw()
        return _Info(g.row_pointers, g.column_index), g.row_pointers, g.column_index, N, N
    if kind == "directed":
        rp, ci = _directed_structure(n=N, edges=3500)
        return _directed_info(rp, ci), rp, ci, N, N
    g = _powerlaw()
    bundle = types.SimpleNamespace(row_pointers=g.row_pointers.cuda(), column_index=g.column_index.cuda(), partSize=32)
    blocks, _ = NeighborSampler(bundle, [5]).sample(torch.arange(0, N, 3, dtype=torch.int32).cuda(), 11)
    block = blocks[0]
    assert block.num_src > block.num_dst
    return block, block.row_pointers.cpu(), block.column_index.cpu(), block.num_dst, block.num_src


def _temp(which, d):
    if which == "scalar":
        return torch.tensor([1.3])
    t = 2.0 * torch.randn(d, generator=torch.Generator().manual_seed(21))
    t[0], t[1] = 0.0, -1.5
    return t


def _dense64(X, t, rp, ci, n_in, G):
    """(Y, dX, dt) by fp64 autograd of the dense formula for the loss sum(Y * G)"""
    X64, t64 = X.double().requires_grad_(True), t.double().requires_grad_(True)
    Y = S.dense_forward(X64, t64, S.counts_matrix(rp, ci, n_in))
    (Y * G.double()).sum().backward()
    return Y.detach(), X64.grad, t64.grad


@pytest.mark.parametrize("which", ["scalar", "per_channel"])
@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
def test_neighbor_softmax_gradients_against_dense_fp64_autograd(kind, which):
    info, rp, ci, n_out, n_in = _structure(kind)
    d = 20
    X, G, t = _randn(n_in, d, 31), _randn(n_out, d, 32), _temp(which, d)
    Y64, dX64, dt64 = _dense64(X, t, rp, ci, n_in, G)
    scales = S.reference(X, t, rp, ci, G)
    # (the dense formula and the index form are the same function)
    assert_close_f64(scales["dX"].numpy(), dX64.numpy(), rtol=1e-9, scale=scales["dX_scale"].numpy(), what="index form against dense")
    Xd, td = X.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    Y = ops.NeighborSoftmax.apply(Xd, td, info)
    assert Y.shape == (n_out, d)
    (Y * G.cuda()).sum().backward()
    assert td.grad.shape == t.shape
    for name, got, ref in (("out", Y.detach(), Y64), ("dX", Xd.grad, dX64), ("dt", td.grad, dt64)):
        print(f"{kind} {which} {name}: worst error / bound {S.worst_ratio(got, ref, scales[name + '_scale']):.5f}")
        assert_close_f64(got.cpu().numpy(), ref.numpy(), scale=scales[name + "_scale"].numpy(), what=f"{kind} {which}: {name}")


def test_what_needs_no_gradient_is_not_computed():
    rp, ci = _directed_structure(n=N, edges=3500)
    info = _directed_info(rp, ci)
    X, t = _randn(N, 8, 41).cuda(), torch.tensor([0.7]).cuda()
    # a temperature that needs no gradient: no sq is made or saved
    Xd = X.clone().requires_grad_(True)
    Y = ops.NeighborSoftmax.apply(Xd, t, info)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 5 and saved[4] is None and all(s is not None for s in saved[:4])
    # an X that needs no gradient builds no transposed structure, in the forward or in the backward
    td = t.clone().requires_grad_(True)
    Y = ops.NeighborSoftmax.apply(X, td, info)
    assert Y.grad_fn.saved_tensors[4] is not None
    assert info._edge_arrays().get("transposed") is None
    Y.sum().backward()
    assert td.grad is not None and info._edge_arrays().get("transposed") is None
    # neither needs one: no graph at all
    assert not ops.NeighborSoftmax.apply(X, t, info).requires_grad
    # and the first backward for X builds it
    ops.NeighborSoftmax.apply(Xd, t, info).sum().backward()
    assert Xd.grad is not None and info._edge_arrays().get("transposed") is not None


@pytest.mark.parametrize("learn", [False, True], ids=["fixed", "learn"])
@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_fused_and_composed_aggregation_agree(kind, learn):
    info, rp, ci, n_out, n_in = _structure(kind)
    d = 12
    X, G = _randn(n_in, d, 51), _randn(n_out, d, 52)
    got = {}
    for fused in (True, False):
        agg = ops.SoftmaxAggregation(t=1.7, learn=learn, channels=d if learn else 1, fused=fused).cuda()
        Xd = X.cuda().requires_grad_(True)
        Y = agg(Xd, info)
        (Y * G.cuda()).sum().backward()
        got[fused] = dict(out=Y.detach(), dX=Xd.grad, dt=agg.t.grad if learn else None)
    scales = S.reference(X, torch.full((d if learn else 1,), 1.7), rp, ci, G)
    for name in ("out", "dX", "dt"):
        a, b = got[True][name], got[False][name]
        if a is None:
            assert b is None and not learn
            continue
        # both paths are held to fp64, and to each other, within the same bound
        for path, v in (("fused", a), ("composed", b)):
            assert_close_f64(v.cpu().numpy(), scales[name].numpy(), scale=scales[name + "_scale"].numpy(), what=f"{kind} {path}: {name}")
        assert_close_f64(a.cpu().numpy(), b.cpu().double().numpy(), scale=scales[name + "_scale"].numpy(),
                         what=f"{kind}: fused against composed {name}")
    if kind == "symmetric":
        block = _structure("block")[0]
        with pytest.raises(TypeError, match="does not take a SampledBlock"):
            ops.SoftmaxAggregation(fused=False).cuda()(torch.zeros(block.num_src, d, device="cuda"), block)


def _gen64(conv, X, rp, ci, n_out, G):
    """GENConv in fp64 from torch ops (dense aggregation), the gradients of sum(Y * G) by autograd, and the sum of |terms| of
    every result."""
    n_in = X.shape[0]
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in conv.named_parameters()}
    Xr = X.double().requires_grad_(True)
    A = S.counts_matrix(rp, ci, n_in)
    t = p["aggr.t"] if "aggr.t" in p else conv.aggr.t.detach().double().cpu()
    h = Xr @ p["weights_in"] if "weights_in" in p else Xr
    m = torch.relu(h) + conv.eps
    a = S.dense_forward(m, t, A)
    z = h[:n_out] + a
    u = z @ p["weights_mlp1"] + (p["bias_mlp1"] if "bias_mlp1" in p else 0.0)
    Y = torch.relu(u) @ p["weights_mlp2"] + (p["bias_mlp2"] if "bias_mlp2" in p else 0.0)
    (Y * G).sum().backward()
    ref = dict(Y=Y.detach(), dX=Xr.grad, **{k: v.grad for k, v in p.items()})
    # ---- magnitudes: forward ...
    pa = {k: v.detach().abs() for k, v in p.items()}
    Xa, Ga = X.double().abs(), G.abs()
    ha = Xa @ pa["weights_in"] if "weights_in" in pa else Xa
    agg = S.reference(m.detach(), t.detach(), rp, ci)
    za = ha[:n_out] + agg["out_scale"]
    ua = za @ pa["weights_mlp1"] + (pa["bias_mlp1"] if "bias_mlp1" in pa else 0.0)
    scale = dict(Y=ua @ pa["weights_mlp2"] + (pa["bias_mlp2"] if "bias_mlp2" in pa else 0.0))
    # ... and backward (relu' <= 1)
    dua = Ga @ pa["weights_mlp2"].t()
    scale["weights_mlp2"] = ua.t() @ Ga
    scale["weights_mlp1"] = za.t() @ dua
    if "bias_mlp1" in pa:
        scale["bias_mlp1"], scale["bias_mlp2"] = dua.sum(0), Ga.sum(0)
    dza = dua @ pa["weights_mlp1"].t()
    through = S.reference(m.detach(), t.detach(), rp, ci, dza)         # the aggregation's own scales for the gradient dza
    if "aggr.t" in pa:
        scale["aggr.t"] = through["dt_scale"]
    dha = through["dX_scale"].clone()
    dha[:n_out] += dza
    if "weights_in" in pa:
        scale["weights_in"] = Xa.t() @ dha
        scale["dX"] = dha @ pa["weights_in"].t()
    else:
        scale["dX"] = dha
    return ref, scale


CONFIGS = {
    "plain": dict(),
    "learn-scalar-bias": dict(learn_t=True, bias=True, t=0.5),
    "learn-per-channel": dict(learn_t=True, channels=24, t=2.0),
}


def _check_gen(conv, info, X, rp, ci, n_out, what):
    Xd = X.cuda().requires_grad_(True)
    Y = conv(Xd, info)
    assert Y.shape == (n_out, conv.weights_mlp2.shape[1])
    G = _randn(n_out, Y.shape[1], 62).double()
    (Y * G.float().cuda()).sum().backward()
    ref, scale = _gen64(conv, X, rp, ci, n_out, G)
    got = dict(Y=Y.detach(), dX=Xd.grad, **{k: v.grad for k, v in conv.named_parameters()})
    assert set(got) == set(ref) and all(v is not None for v in got.values())
    for name in ref:
        print(f"GENConv {what} {name}: worst error / bound {S.worst_ratio(got[name], ref[name], scale[name]):.5f}")
        assert_close_f64(got[name].cpu().numpy(), ref[name].numpy(), scale=scale[name].numpy(), what=f"GENConv {what}: {name}")
    return ref, scale


@pytest.mark.parametrize("config", list(CONFIGS))
def test_gen_conv_on_a_full_graph(config):
    info, rp, ci, n_out, n_in = _structure("symmetric")
    torch.manual_seed(61)
    conv = ops.GENConv(16, 24, **CONFIGS[config])
    if conv.bias_mlp1 is not None:
        with torch.no_grad():
            conv.bias_mlp1.uniform_(-0.5, 0.5)
            conv.bias_mlp2.uniform_(-0.5, 0.5)
    conv = conv.cuda()
    X = _randn(n_in, 16, 63)
    ref, scale = _check_gen(conv, info, X, rp, ci, n_out, config)
    Yr = conv(X.cuda(), info, relu=True)             # the same bits again, clamped
    assert float(Yr.detach().min()) == 0.0
    assert_close_f64(Yr.detach().cpu().numpy(), torch.relu(ref["Y"]).numpy(), scale=scale["Y"].numpy(), what=f"GENConv {config}: relu")


def test_gen_conv_without_an_input_weight_and_on_a_block():
    info, rp, ci, n_out, n_in = _structure("block")
    torch.manual_seed(64)
    square = ops.GENConv(16, 16, learn_t=True).cuda()
    assert square.weights_in is None
    _check_gen(square, info, _randn(n_in, 16, 65), rp, ci, n_out, "block, square")
    conv = ops.GENConv(16, 8, t=-1.0, bias=True).cuda()
    X = _randn(n_in, 16, 66)
    _check_gen(conv, info, X, rp, ci, n_out, "block")
    with pytest.raises(TypeError, match="float32 only"):
        conv.bfloat16()(X.cuda().bfloat16(), info)
    conv = conv.float()
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(TypeError, match="float32 only"):
        conv(X.cuda(), info)
    with pytest.raises(TypeError, match="float32 only"):
        ops.NeighborSoftmax.apply(X.cuda().half(), torch.ones(1, device="cuda"), info)
    with pytest.raises(TypeError, match="does not take a SampledBlock"):
        ops.GENConv(16, 8, fused=False).cuda()(X.cuda(), info)

"""ops.DotAttentionRows and ops.TransformerConv(fused="rows") against the fp64 restatements of tests/dotattn_ref.py on a symmetric
graph, a directed graph and a sampled block, at the bounds of test_dotattn_ops_gpu.py (kernel outputs 1e-5 of the sum of |terms|,
layer outputs and input gradients 1e-4 of max|ref|, weight gradients 1e-4 of their sum of |terms|, each times max(1, S)); one run of
the driver."""
import pytest
import torch

import dotattn_ref as tref
from gnnadvisor_osdi21_amd import ops
from test_dotattn_driver_gpu import _run as run_driver
from test_dotattn_ops_gpu import _check_layer
from test_gat_rows_ops_gpu import _input
from util import assert_close_f64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
def test_the_gradients_match_fp64_autograd(kind):
    info, n_src, n_dst = _input(kind)
    heads, dim = 4, 16
    W = heads * dim
    gen = torch.Generator().manual_seed(6)
    P = torch.randn(n_src, 3 * W, generator=gen).cuda().requires_grad_()
    G = torch.randn(n_dst, W, generator=gen).cuda()
    Q, K, V = P[:n_dst, :W], P[:, W:2 * W], P[:, 2 * W:]
    Y = ops.DotAttentionRows.apply(Q, K, V, info, heads)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 5 and all(t.numel() <= n_src * W for t in saved), "saved tensors are node-sized"
    assert saved[1].data_ptr() == K.data_ptr() and saved[1].stride(0) == 3 * W, "the slices are passed on, not copied"
    (Y * G).sum().backward()
    r = tref.kernel_reference(Q, K, V, G, info.row_pointers, info.column_index, heads, 1 / dim ** 0.5)
    n = lambda t: t.detach().cpu().numpy()
    rtol = 1e-5 * r.factor
    assert_close_f64(n(Y), n(r.Y), rtol=rtol, scale=n(r.s_Y), what=f"{kind} Y")
    for rows, lo, ref, s, name in ((n_dst, 0, r.dQ, r.s_dQ, "dQ"), (n_src, W, r.dK, r.s_dK, "dK"), (n_src, 2 * W, r.dV, r.s_dV, "dV")):
        assert_close_f64(n(P.grad[:rows, lo:lo + W]), n(ref), rtol=rtol, scale=n(s), what=f"{kind} {name}")
    # only what needs a gradient gets one
    Q2, K2 = Q.detach().clone().requires_grad_(), K.detach().clone()
    ops.DotAttentionRows.apply(Q2, K2, V.detach(), info, heads).sum().backward()
    assert Q2.grad is not None and K2.grad is None


def test_the_layer_trains_with_the_restated_mask_to_the_same_bits_twice():
    info, n, _ = _input("symmetric")
    torch.manual_seed(9)
    conv = ops.TransformerConv(10, 6, heads=3, attn_drop=0.5, fused="rows").cuda()
    assert conv.rows and conv.fused and conv.training
    X = torch.randn(n, 10, device="cuda", requires_grad=True)
    _check_layer(conv, X, info, info.row_pointers, info.column_index, n, 'TransformerConv(fused="rows") attn_drop=0.5', p=0.5,
                 rng_seed=1234567)
    assert conv.last_rng_seed == 1234567
    steps = []
    for _ in range(2):
        X.grad = None
        conv.zero_grad()
        Y = conv(X, info, rng_seed=1234567)
        Y.square().sum().backward()
        steps.append((Y.detach().clone(), X.grad.clone(), conv.weights.grad.clone()))
    # (the layer's GEMMs repeat themselves too: the same bits from one seed, through the whole step)
    assert all(torch.equal(a, b) for a, b in zip(*steps))
    with pytest.raises(ValueError, match='fused must be True, False or "rows"'):
        ops.TransformerConv(8, 4, fused="columns")


def test_the_driver_trains_the_transformer_on_the_rows_kernels():
    out = run_driver(["--fused_attention", "rows", "--heads", "2"])
    assert "TransformerConv" in out

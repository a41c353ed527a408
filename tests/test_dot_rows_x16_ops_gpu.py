"""ops.DotAttentionRows on bfloat16 / float16 leaves and ops.TransformerConv(fused="rows") as a cast model and under autocast
(include/gnna_dot_rows_x16.h): the op against tests/dotattn_ref.py's fp64 function of the 16-bit inputs under the bounds of
test_dot_rows_x16_gpu.py, the layer against the hand composition of the same ops (equal bits), one run of the driver."""
import itertools

import pytest
import torch

import dotattn_ref as tref
from gnnadvisor_osdi21_amd import ops
from test_dot_rows_x16_gpu import TYPES, both_types, within_the_bound
from test_dotattn_driver_gpu import _run as run_driver
from test_gat_rows_ops_gpu import _input

pytestmark = pytest.mark.gpu
HEADS, DIM = 4, 16
W = HEADS * DIM


def _leaves(kind, dtype):
    info, n_src, n_dst = _input(kind)
    gen = torch.Generator().manual_seed(6)
    P = torch.randn(n_src, 3 * W, generator=gen).cuda().to(dtype).requires_grad_()
    G = torch.randn(n_dst, W, generator=gen).cuda().to(dtype)
    return info, P, G, (P[:n_dst, :W], P[:, W:2 * W], P[:, 2 * W:])


@both_types
@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
def test_the_op_on_16_bit_leaves_against_fp64(kind, dtype):
    info, P, G, (Q, K, V) = _leaves(kind, dtype)
    Y = ops.DotAttentionRows.apply(Q, K, V, info, HEADS)
    saved = Y.grad_fn.saved_tensors
    assert Y.dtype == dtype and [t.dtype for t in saved] == [dtype, dtype, dtype, torch.float32, dtype]
    assert all(t.numel() <= P.shape[0] * W for t in saved), "saved tensors are node-sized"
    assert saved[1].data_ptr() == K.data_ptr() and saved[1].stride(0) == 3 * W, "the slices are passed on, not copied"
    (Y * G).sum().backward()
    assert P.grad.dtype == dtype
    r = tref.kernel_reference(Q.detach(), K.detach(), V.detach(), G, info.row_pointers, info.column_index, HEADS, 1 / DIM ** 0.5)
    n_dst = Q.shape[0]
    got = (Y.detach(), saved[3], P.grad[:n_dst, :W], P.grad[:, W:2 * W], P.grad[:, 2 * W:])
    within_the_bound(f"{kind} {dtype}", got, r, dtype)


def test_only_the_gradients_that_are_needed_are_made_and_mixed_dtypes_are_refused():
    info, _, _, qkv = _leaves("directed", torch.bfloat16)
    for need in itertools.product((False, True), repeat=3):
        leaves = [t.detach().clone().requires_grad_(n) for t, n in zip(qkv, need)]
        Y = ops.DotAttentionRows.apply(*leaves, info, HEADS)
        if any(need):
            Y.float().sum().backward()
        assert [t.grad is not None for t in leaves] == list(need), need
        assert all(t.grad is None or t.grad.dtype == torch.bfloat16 for t in leaves)
    Q, K, V = (t.detach() for t in qkv)
    for bad in ((Q, K.float(), V), (Q.float(), K, V), (Q, K, V.half()), (Q.double(), K.double(), V.double())):
        with pytest.raises(TypeError, match="DotAttentionRows: float32, or Q, K and V all bfloat16 or all float16"):
            ops.DotAttentionRows.apply(*bad, info, HEADS)


@pytest.mark.parametrize("mode", ["cast", "autocast"])
def test_the_layer_is_the_hand_composition_of_its_ops(mode):
    info, n, _ = _input("symmetric")
    torch.manual_seed(9)
    conv = ops.TransformerConv(10, 6, heads=3, fused="rows").cuda()
    X = torch.randn(n, 10, device="cuda")
    if mode == "cast":
        conv, X = conv.to(torch.bfloat16), X.to(torch.bfloat16)
    X.requires_grad_()
    Xh = X.detach().clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
        Y = conv(X, info)
        Xc = Xh.to(torch.bfloat16)
        P = torch.mm(Xc, conv.weights.detach().to(torch.bfloat16))
        hand = ops.DotAttentionRows.apply(P[:, :18], P[:, 18:36], P[:, 36:], info, 3) + torch.mm(Xc, conv.W_skip.detach().to(torch.bfloat16))
    assert Y.dtype == torch.bfloat16 and torch.equal(Y, hand)
    wgt = torch.randn_like(Y)
    (Y * wgt).sum().backward()
    (hand * wgt).sum().backward()
    assert X.grad.dtype == X.dtype and torch.equal(X.grad, Xh.grad)
    for q in conv.parameters():
        assert q.grad is not None and q.grad.dtype == q.dtype and torch.isfinite(q.grad).all()
    fused = ops.TransformerConv(10, 6, heads=3, fused=True).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(TypeError, match="TransformerConv computes in float32 only: .*inside torch.autocast"):
            fused(torch.randn(n, 10, device="cuda"), info)


def test_the_driver_trains_the_transformer_in_bfloat16_on_the_rows_kernels():
    out = run_driver(["--fused_attention", "rows", "--heads", "2", "--dtype", "bfloat16"], falling=False)
    assert "TransformerConv" in out and "dtype='bfloat16'" in out

"""ops.GATv2AttentionRows and ops.GATv2Conv(fused="rows") on a symmetric graph, a directed graph and a sampled block: the gradients
of the Function against the fp64 reference of tests/gatv2_ref.py under the bounds test_gatv2_ops_gpu.py uses for GATv2Attention
(1e-5 * max(1, S) of the sum of |terms|); the layer against its hand composition, against fused=True under one seed, and twice from
one seed; the driver's run."""
import numpy as np
import pytest
import torch

import gatv2_ref as vref
from gnnadvisor_osdi21_amd import main as driver, ops
from test_gat_rows_ops_gpu import _input
from util import assert_close_f64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
@pytest.mark.parametrize("heads,dim,p", [(4, 16, 0.0), (3, 5, 0.5)])
def test_the_function_matches_the_fp64_reference(kind, heads, dim, p):
    info, n_src, n_dst = _input(kind)
    seed = 2 ** 63 + 11
    Hs, Hd, att, G = [t.cuda() for t in vref.inputs(n_dst, n_src, heads, dim, heads + dim)]
    for t in (Hs, Hd, att):
        t.requires_grad_()
    Y = ops.GATv2AttentionRows.apply(Hs, Hd, att, info, 0.2, p, seed)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 5 and all(t.numel() <= n_src * heads * dim for t in saved), "saved tensors are node-sized"
    (Y * G).sum().backward()
    r = vref.kernel_reference(Hs, Hd, att, G, info.row_pointers, info.column_index, heads, 0.2, p, seed, "GATv2AttentionRows")
    n = lambda t: t.detach().cpu().numpy()
    rtol = 1e-5 * r.factor
    assert_close_f64(n(Y), n(r.Y), rtol=rtol, scale=n(r.s_Y), what=f"{kind} Y")
    assert_close_f64(n(Hs.grad[r.ok_dHs]), n(r.dHs[r.ok_dHs]), rtol=rtol, scale=n(r.s_dHs[r.ok_dHs]), what=f"{kind} dHs")
    assert_close_f64(n(Hd.grad[r.ok_dHd]), n(r.dHd[r.ok_dHd]), rtol=rtol, scale=n(r.s_dHd[r.ok_dHd]), what=f"{kind} dHd")
    assert_close_f64(n(att.grad), n(r.d_att), rtol=rtol, scale=n(r.s_att), what=f"{kind} d_att")


def _step(conv, X, info, wgt, rng_seed=None):
    """One forward and backward -> the bits of (Y, dX, every parameter gradient)."""
    conv.zero_grad()
    Xc = X.clone().requires_grad_()
    Y = conv(Xc, info, rng_seed=rng_seed)
    (Y * wgt).sum().backward()
    return [Y.detach(), Xc.grad] + [q.grad.clone() for q in conv.parameters()]


@pytest.mark.parametrize("kind,share,concat", [("symmetric", True, True), ("directed", False, False), ("block", True, False)])
def test_the_layer_is_its_hand_composition_and_repeats_its_bits(kind, share, concat):
    info, n_src, n_dst = _input(kind)
    heads, fin, fout = 3, 12, 5
    torch.manual_seed(11)
    conv = ops.GATv2Conv(fin, fout, heads=heads, concat=concat, share_weights=share, attn_drop=0.5, fused="rows").cuda()
    assert conv.rows and conv.fused
    X = torch.randn(n_src, fin, device="cuda")
    wgt = torch.randn(n_dst, heads * fout if concat else fout, device="cuda")
    first, second = _step(conv, X, info, wgt, 99), _step(conv, X, info, wgt, 99)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), "two training steps from one seed give the same bits"
    with torch.no_grad():
        Hs = torch.mm(X, conv.W_l)
        Hd = Hs[:n_dst] if share else torch.mm(X[:n_dst], conv.W_r)
        Y = ops.GATv2AttentionRows.apply(Hs, Hd, conv.att, info, conv.negative_slope, 0.5, 99)
        assert torch.equal(first[0], Y if concat else Y.view(n_dst, heads, fout).mean(1))
    # fused=True with the same seed drops the same edges: both are within the layer bound of the fp64 layer, so within twice that
    atomic = ops.GATv2Conv(fin, fout, heads=heads, concat=concat, share_weights=share, attn_drop=0.5).cuda()
    atomic.load_state_dict(conv.state_dict())
    X64 = X.double().requires_grad_()
    keep = {}
    P64 = [None if q is None else q.detach().double().requires_grad_() for q in (conv.W_l, conv.W_r, conv.att)]
    Y64 = vref.gatv2_layer64(X64, *P64, info.row_pointers, info.column_index, n_dst, heads, fout, concat, 0.2, 0.5, 99, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    s_Wl, s_Wr, s_att, S = vref.param_scales(X64, keep)
    full = lambda ref: np.full(ref.shape, float(ref.abs().max()))
    scales = [full(Y64.detach()), full(X64.grad), s_Wl.cpu().numpy()] + ([] if share else [s_Wr.cpu().numpy()]) + [s_att.cpu().numpy()]
    for a, b, scale in zip(first, _step(atomic, X, info, wgt, 99), scales):
        assert_close_f64(a.cpu().numpy(), b.double().cpu().numpy(), rtol=2e-4 * max(1.0, S), scale=scale, what=f"rows vs fused=True {kind}")


def test_fused_takes_rows_and_no_other_string():
    with pytest.raises(ValueError, match='GATv2Conv: fused must be True, False or "rows"'):
        ops.GATv2Conv(8, 4, fused="columns")
    plain = ops.GATv2Conv(8, 4)
    assert plain.fused and not plain.rows and not ops.GATv2Conv(8, 4, fused=False).fused


def test_the_driver_trains_on_the_rows_kernels_with_attention_dropout():
    cap = {}
    assert driver.main(["--model", "gatv2", "--synthetic", "cora-like", "--scale", "0.5", "--dim", "16", "--hidden", "16", "--classes", "4",
                        "--num_epoches", "3", "--heads", "2", "--fused_attention", "rows", "--attn_drop", "0.5"], capture=cap) == 0
    assert cap["model"].conv1.rows and cap["model"].conv2.rows
    assert np.isfinite(cap["first_loss"]) and np.isfinite(cap["final_loss"])

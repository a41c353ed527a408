"""Edge features through the operators: ops.GATEdgeAttention and GATConv(edge_dim=5, heads=4, out=16) against the fp64 layer of
tests/gat_edge_ref.py on a symmetric graph, a directed one and a SampledBlock; fused against composed; the attention weights;
the dropout seed; the memory of a fused step.  Bounds are those of test_gat_block_ops_gpu.py: outputs and input gradients 1e-4
of max|ref|, parameter gradients 1e-4 of their sum of |terms|."""
import pytest
import torch

import gat_edge_ref as eref
from gnnadvisor_osdi21_amd import graph, ops
from test_directed_ops_gpu import _info as _property
from test_edge_attention_gpu import _Info
from test_gat_block_ops_gpu import _max_scale, one_block
from util import assert_close_f64

pytestmark = pytest.mark.gpu
FIN, FOUT, HEADS, EDGE_DIM = 12, 16, 4, 5


def _structure(kind):
    """(inputInfo, rows of the result, source rows)"""
    if kind == "symmetric":
        g = graph.powerlaw_graph(1200, 20000, 300, seed=8)
        return _Info(g), g.num_nodes, g.num_nodes
    if kind == "directed":
        g = graph.uniform_graph(300, 3000, symmetric=False)
        return _property(g, 32, directed=True), g.num_nodes, g.num_nodes
    block = one_block()
    assert block.num_dst == 65 and block.num_src > 65
    return block, block.num_dst, block.num_src


def _n(t):
    return t.detach().cpu().numpy()


def _layer_case(kind, fused, p=0.0, seed=None, concat=True):
    """One forward and backward of the layer and of the fp64 layer on the same values -> (conv, got, ref, scales, keep)."""
    info, n_dst, n_src = _structure(kind)
    nnz = info.column_index.numel()
    torch.manual_seed(11)
    conv = ops.GATConv(FIN, FOUT, heads=HEADS, concat=concat, fused=fused, attn_drop=p, edge_dim=EDGE_DIM).cuda()
    if p == 0.0:
        conv.eval()
    X = torch.randn(n_src, FIN, device="cuda", requires_grad=True)
    EA = torch.randn(nnz, EDGE_DIM, device="cuda", requires_grad=True)
    Y = conv(X, info, rng_seed=seed, edge_attr=EA)
    assert Y.shape == (n_dst, HEADS * FOUT if concat else FOUT)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    params = (conv.weights, conv.att_l, conv.att_r, conv.weights_edge, conv.att_e)
    X64, EA64 = X.detach().double().requires_grad_(), EA.detach().double().requires_grad_()
    P64 = [q.detach().double().requires_grad_() for q in params]
    keep = {}
    Y64 = eref.gat_layer64(X64, *P64, EA64, info.row_pointers, info.column_index, n_dst, HEADS, FOUT, concat, p=p,
                           rng_seed=conv.last_rng_seed or 0, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    scales = eref.param_scales(X64, EA64, P64[3], P64[4], keep, HEADS, FOUT)
    got = dict(Y=Y, dX=X.grad, dEA=EA.grad, dW=params[0].grad, da_l=params[1].grad, da_r=params[2].grad, dW_e=params[3].grad,
               da_e=params[4].grad)
    ref = dict(Y=Y64.detach(), dX=X64.grad, dEA=EA64.grad, dW=P64[0].grad, da_l=P64[1].grad, da_r=P64[2].grad, dW_e=P64[3].grad,
               da_e=P64[4].grad)
    s_W, s_l, s_r, s_We, s_ae, s_ea = scales
    scale = dict(Y=_max_scale(ref["Y"]), dX=_max_scale(ref["dX"]), dEA=_max_scale(ref["dEA"]), dW=_n(s_W), da_l=_n(s_l), da_r=_n(s_r),
                 dW_e=_n(s_We), da_e=_n(s_ae))
    return conv, got, ref, scale, keep


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
def test_fused_gatconv_with_edge_features_matches_the_fp64_layer(kind, concat):
    conv, got, ref, scale, keep = _layer_case(kind, fused=True, concat=concat)
    assert float(keep["ee"].detach().abs().max()) > 0.1, "the edge term must matter in this case"
    for name in got:
        assert_close_f64(_n(got[name]), _n(ref[name]), rtol=1e-4, scale=scale[name], what=f"GATConv(edge_dim) fused, {kind}: {name}")


@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_fused_and_composed_agree(kind):
    """Both against the same fp64 layer with the same bound (the composed path refuses a block)."""
    for fused in (True, False):
        conv, got, ref, scale, _ = _layer_case(kind, fused=fused)
        for name in got:
            assert_close_f64(_n(got[name]), _n(ref[name]), rtol=1e-4, scale=scale[name],
                             what=f"GATConv(edge_dim) fused={fused}, {kind}: {name}")
    with pytest.raises(TypeError, match="does not take a SampledBlock"):
        block = one_block()
        ops.GATConv(FIN, FOUT, heads=HEADS, edge_dim=EDGE_DIM).cuda()(torch.randn(block.num_src, FIN, device="cuda"), block,
                                                                     edge_attr=torch.randn(block.column_index.numel(), EDGE_DIM, device="cuda"))


@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
def test_the_function_against_fp64(kind):
    """ops.GATEdgeAttention alone: Y and the gradients of H, el, er and ee against gat_edge_ref.kernel_reference."""
    info, n_dst, n_src = _structure(kind)
    nnz = info.column_index.numel()
    gen = torch.Generator().manual_seed(5)
    mk = lambda *shape: torch.randn(*shape, generator=gen).cuda().requires_grad_()
    H, el, er, ee = mk(n_src, HEADS * FOUT), mk(n_dst, HEADS), mk(n_src, HEADS), mk(nnz, HEADS)
    G = torch.randn(n_dst, HEADS * FOUT, generator=gen).cuda()
    Y = ops.GATEdgeAttention.apply(H, el, er, ee, info, 0.2)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 6 and all(t.numel() <= max(n_src * HEADS * FOUT, nnz * HEADS) for t in saved), "saved: node-sized tensors and ee"
    (Y * G).sum().backward()
    r = eref.kernel_reference(H, el, er, ee, G, info.row_pointers, info.column_index, HEADS, 0.2, what=kind)
    assert_close_f64(_n(Y), _n(r.Y), rtol=1e-5, scale=_n(r.s_Y), what=f"{kind} Y")
    assert_close_f64(_n(H.grad), _n(r.dH), rtol=1e-5, scale=_n(r.s_dH), what=f"{kind} dH")
    assert_close_f64(_n(el.grad[r.ok_el]), _n(r.d_el[r.ok_el]), rtol=1e-5, scale=_n(r.s_el[r.ok_el]), what=f"{kind} d_el")
    assert_close_f64(_n(er.grad[r.ok_er]), _n(r.d_er[r.ok_er]), rtol=1e-5, scale=_n(r.s_er[r.ok_er]), what=f"{kind} d_er")
    assert_close_f64(_n(ee.grad[r.ok_ee]), _n(r.d_ee[r.ok_ee]), rtol=1e-5, scale=_n(r.s_ee[r.ok_ee]), what=f"{kind} d_ee")


@pytest.mark.parametrize("edge_dim", [EDGE_DIM, None], ids=["edge_dim", "plain"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_attention_weights(fused, edge_dim):
    info, n, _ = _structure("symmetric")
    nnz = info.column_index.numel()
    torch.manual_seed(3)
    conv = ops.GATConv(FIN, FOUT, heads=HEADS, fused=fused, edge_dim=edge_dim).cuda()
    X = torch.randn(n, FIN, device="cuda")
    EA = torch.randn(nnz, EDGE_DIM, device="cuda") if edge_dim else None
    Y, alpha = conv(X, info, edge_attr=EA, return_attention_weights=True)
    assert Y.shape == (n, HEADS * FOUT) and alpha.shape == (nnz, HEADS) and not alpha.requires_grad
    assert (alpha >= 0).all()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (info.row_pointers[1:] - info.row_pointers[:-1]).long())
    sums = torch.zeros(n, HEADS, device="cuda", dtype=torch.float64).index_add_(0, rows, alpha.double())
    has = torch.bincount(rows, minlength=n) > 0
    assert (sums[has] - 1).abs().max().item() <= 1e-5 * 300 and (sums[~has] == 0).all()      # (at most 300 edges per row, 1e-5 each)
    keep = {}
    P64 = [q.detach().double() for q in (conv.weights, conv.att_l, conv.att_r)]
    if edge_dim:
        P64 += [conv.weights_edge.detach().double(), conv.att_e.detach().double(), EA.double()]
    else:
        P64 += [torch.zeros(1, HEADS * FOUT, dtype=torch.float64, device="cuda"), torch.zeros(HEADS, FOUT, dtype=torch.float64, device="cuda"),
                torch.zeros(nnz, 1, dtype=torch.float64, device="cuda")]
    eref.gat_layer64(X.double().requires_grad_(), *P64[:3], P64[3].requires_grad_(), P64[4], P64[5], info.row_pointers, info.column_index, n,
                     HEADS, FOUT, True, keep=keep)
    err = (alpha.double() - keep["alpha"]).abs().max().item()
    print(f"attention weights fused={fused} edge_dim={edge_dim}: max err {err:.3e}")
    assert err <= 1e-5


def test_training_with_attn_drop_uses_the_seed_as_the_plain_layer_does():
    conv, got, ref, scale, _ = _layer_case("symmetric", fused=True, p=0.6, seed=None)
    seed = conv.last_rng_seed
    assert isinstance(seed, int) and 0 <= seed < 2 ** 63
    for name in got:
        assert_close_f64(_n(got[name]), _n(ref[name]), rtol=1e-4, scale=scale[name], what=f"GATConv(edge_dim) attn_drop=0.6: {name}")
    conv2, got2, ref2, scale2, _ = _layer_case("block", fused=True, p=0.6, seed=12345)
    assert conv2.last_rng_seed == 12345
    for name in got2:
        assert_close_f64(_n(got2[name]), _n(ref2[name]), rtol=1e-4, scale=scale2[name], what=f"GATConv(edge_dim) on a block, seed given: {name}")
    conv2.eval()
    info, _, n_src = _structure("block")
    conv2(torch.randn(n_src, FIN, device="cuda"), info, edge_attr=torch.randn(info.column_index.numel(), EDGE_DIM, device="cuda"))
    assert conv2.last_rng_seed == 12345                   # eval mode draws no seed


def test_a_fused_step_allocates_nothing_of_the_size_of_edges_times_width():
    """Peak torch memory of a training step above what is allocated before it, against a budget that has no room for one
    [nnz, heads * out] tensor: 16 node-sized tensors of [N, heads * out] floats (H, Y, their gradients and the pieces autograd
    makes on the way to the parameters: 10 counted, 16 allowed), 3 x nnz x heads x 4 bytes (ee, d_ee and one more) and nnz x 4 for
    the position map, plus 256 KiB for everything small (el, er, lse, their gradients, the parameters' gradients).  The library's
    own scratch is node-sized and not torch's."""
    heads, out = 4, 64
    g = graph.uniform_graph(300, 36000, seed=2)
    info = _Info(g)
    n, nnz = g.num_nodes, info.column_index.numel()
    assert 25000 <= nnz <= 40000
    torch.manual_seed(0)
    conv = ops.GATConv(32, out, heads=heads, fused=True, edge_dim=8).cuda()
    X, EA = torch.randn(n, 32, device="cuda"), torch.randn(nnz, 8, device="cuda")
    wgt = torch.randn(n, heads * out, device="cuda")

    def step():
        conv.zero_grad(set_to_none=True)
        (conv(X, info, edge_attr=EA) * wgt).sum().backward()
    step()                                  # (the reverse-edge map, the symmetry answer and torch's GEMM workspace: made here)
    torch.cuda.synchronize()
    conv.zero_grad(set_to_none=True)
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    edge_wide = nnz * heads * out * 4
    budget = 16 * n * heads * out * 4 + 3 * nnz * heads * 4 + nnz * 4 + (256 << 10)
    print(f"fused step: peak {peak / 2 ** 20:.2f} MiB above the resident set, budget {budget / 2 ** 20:.2f} MiB, "
          f"one [nnz, heads * out] tensor {edge_wide / 2 ** 20:.2f} MiB")
    assert budget < edge_wide, "the budget must have no room for an [nnz, heads * out] tensor"
    assert peak <= budget

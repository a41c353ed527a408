"""Attention dropout through the operators and the driver: GATConv(fused=True, attn_drop=p) in training mode against the fp64
layer with the mask of ``layer.last_rng_seed`` (tests/gat_drop_ref.py), on a symmetric graph, a directed one and a SampledBlock;
eval mode; seeding; the composed path's torch dropout; main.py --attn_drop.  Bounds are those of test_gat_block_ops_gpu.py: layer
outputs and input gradients 1e-4 of max|ref|, parameter gradients 1e-4 of their sum of |terms|."""
import math

import pytest
import torch

import gat_drop_ref as dref
import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import graph, ops
from gnnadvisor_osdi21_amd import main as driver
from test_directed_ops_gpu import _info as _property
from test_edge_attention_gpu import _Info
from test_gat_block_ops_gpu import _max_scale, one_block
from util import assert_close_f64

pytestmark = pytest.mark.gpu
P = 0.6


def _structure(kind):
    """(inputInfo, rows of the result)"""
    if kind == "symmetric":
        g = graph.powerlaw_graph(1200, 20000, 300, seed=8)
        return _Info(g), g.num_nodes
    if kind == "directed":
        g = graph.uniform_graph(300, 3000, symmetric=False)
        return _property(g, 32, directed=True), g.num_nodes
    block = one_block()
    assert block.num_dst == 65 and block.num_src > 65
    return block, block.num_dst


@pytest.mark.parametrize("fin,fout,heads,concat", [(41, 16, 4, True), (16, 8, 4, False), (8, 4, 1, True)])
@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
def test_fused_gatconv_with_dropout_matches_the_fp64_layer_with_the_mask(kind, fin, fout, heads, concat):
    info, n_dst = _structure(kind)
    n_src = info.num_src if kind == "block" else n_dst
    torch.manual_seed(fin + heads)
    conv = ops.GATConv(fin, fout, heads=heads, concat=concat, fused=True, attn_drop=P).cuda()
    assert conv.training and conv.last_rng_seed is None
    X = torch.randn(n_src, fin, device="cuda", requires_grad=True)
    Y = conv(X, info)
    seed = conv.last_rng_seed
    assert isinstance(seed, int) and 0 <= seed < 2 ** 63
    assert Y.shape == (n_dst, heads * fout if concat else fout)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()

    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    keep = {}
    Y64 = dref.gat_layer64(X64, *P64, info.row_pointers, info.column_index, n_dst, heads, fout, concat, P, seed, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    plain = gref.gat_layer64(X64.detach(), *[p.detach() for p in P64], info.row_pointers, info.column_index, n_dst, heads, fout, concat)
    assert float((Y64.detach() - plain).abs().max()) > 1e-2 * float(plain.abs().max()), "the mask must matter in this case"
    what = f"GATConv attn_drop={P} on a {kind} structure in={fin} out={fout} heads={heads} concat={concat}"
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=_max_scale(ref), what=f"{what} {name}")
    for got, ref, scale, name in zip((conv.weights.grad, conv.att_l.grad, conv.att_r.grad), P64,
                                     gref.param_scales(X64, keep, heads, fout), ("dW", "da_l", "da_r")):
        assert_close_f64(got.cpu().numpy(), ref.grad.cpu().numpy(), rtol=1e-4, scale=scale.cpu().numpy(), what=f"{what} {name}")
    # an explicit seed is used as given, and the same seed gives the same bits of the mask (the sums are atomics: compare to fp64)
    Y2 = conv(X.detach(), info, rng_seed=seed)
    assert conv.last_rng_seed == seed
    assert_close_f64(Y2.detach().cpu().numpy(), Y64.detach().cpu().numpy(), rtol=1e-4, scale=_max_scale(Y64.detach()), what=f"{what} Y again")


def test_saved_state_stays_node_sized():
    info, n = _structure("symmetric")
    H = torch.randn(n, 32, device="cuda", requires_grad=True)
    el, er = torch.randn(n, 4, device="cuda", requires_grad=True), torch.randn(n, 4, device="cuda", requires_grad=True)
    Y = ops.GATAttention.apply(H, el, er, info, 0.2, 0.5, 2 ** 64 - 5)
    fn = Y.grad_fn
    assert type(fn.rng_seed) is int and fn.rng_seed == 2 ** 64 - 5 and fn.attn_drop == 0.5
    assert all(t.shape[0] == n and t.numel() <= n * 32 for t in fn.saved_tensors)
    Y.sum().backward()
    assert H.grad is not None and el.grad is not None and er.grad is not None
    with pytest.raises(ValueError, match="attn_drop"):
        ops.GATAttention.apply(H, el, er, info, 0.2, 1.0, 3)


@pytest.mark.parametrize("kind", ["symmetric", "block"])
def test_eval_mode_and_attn_drop_zero_take_the_plain_path(kind, monkeypatch):
    info, n_dst = _structure(kind)
    n_src = info.num_src if kind == "block" else n_dst

    def refuse(*a, **k):
        raise AssertionError("the drop entry was called")
    monkeypatch.setattr(ops.GNNA, "gat_forward_drop", refuse)
    monkeypatch.setattr(ops.GNNA, "gat_backward_drop", refuse)
    torch.manual_seed(3)
    for conv in (ops.GATConv(16, 8, heads=4, fused=True, attn_drop=P).cuda().eval(), ops.GATConv(16, 8, heads=4, fused=True).cuda()):
        X = torch.randn(n_src, 16, device="cuda", requires_grad=True)
        Y = conv(X, info)
        Y.sum().backward()
        assert conv.last_rng_seed is None and X.grad is not None
        Y64 = gref.gat_layer64(X.detach().double(), *[p.detach().double() for p in (conv.weights, conv.att_l, conv.att_r)],
                               info.row_pointers, info.column_index, n_dst, 4, 8, True)
        assert_close_f64(Y.detach().cpu().numpy(), Y64.cpu().numpy(), rtol=1e-4, scale=_max_scale(Y64), what=f"{kind}: no mask")
    with pytest.raises(AssertionError, match="the drop entry was called"):       # (the patch does see a call that drops)
        ops.GATConv(16, 8, heads=4, fused=True, attn_drop=P).cuda()(torch.randn(n_src, 16, device="cuda"), info)


def test_seeding():
    info, n = _structure("symmetric")
    conv = ops.GATConv(8, 4, heads=2, fused=True, attn_drop=P).cuda()
    X = torch.randn(n, 8, device="cuda")
    seeds = []
    for _ in range(2):
        torch.manual_seed(1234)
        conv(X, info)
        seeds.append(conv.last_rng_seed)
        conv(X, info)
        seeds.append(conv.last_rng_seed)
    assert seeds[0] == seeds[2] and seeds[1] == seeds[3], "torch.manual_seed must reproduce the seeds of a run"
    assert seeds[0] != seeds[1], "two consecutive forwards must draw different seeds"


def test_composed_path_drops_with_torch_dropout(monkeypatch):
    """fused=False: torch.nn.functional.dropout on alpha.  The kept share of the heads * nnz draws (at least 35,000) lies within
    5 sigma of 1 - p (binomial), a kept alpha is scaled by 1 / (1 - p), and eval mode drops nothing."""
    g = graph.powerlaw_graph(1500, 40000, 900, seed=4)
    info = _Info(g)
    heads = 2
    seen = []

    class Recorder:
        @staticmethod
        def apply(H, alpha, inputInfo, _real=ops.EdgeWeightedAggregate):
            seen.append(alpha.detach().clone())
            return _real.apply(H, alpha, inputInfo)
    monkeypatch.setattr(ops, "EdgeWeightedAggregate", Recorder)
    torch.manual_seed(2)
    conv = ops.GATConv(16, 8, heads=heads, attn_drop=P).cuda()
    X = torch.randn(g.num_nodes, 16, device="cuda")
    conv(X, info)
    conv.eval()
    conv(X, info)
    dropped, plain = seen
    draws = plain.numel()
    assert draws == heads * info.column_index.numel() >= 35000 and (plain > 0).all()
    kept = dropped != 0
    share = float(kept.double().mean())
    sigma = math.sqrt(P * (1 - P) / draws)
    print(f"composed path: kept share {share:.4f} of {draws} draws (1 - p = {1 - P}, sigma {sigma:.5f})")
    assert abs(share - (1 - P)) < 5 * sigma
    assert torch.allclose(dropped[kept], plain[kept] / (1 - P), rtol=1e-6, atol=0)


@pytest.mark.parametrize("extra", [[], ["--fanout", "5,5"]], ids=["full_graph", "fanout"])
def test_driver_trains_with_attention_dropout(extra, capsys):
    cap = {}
    rc = driver.main(["--synthetic", "cora-like", "--model", "gat", "--fused_attention", "True", "--attn_drop", "0.6", "--num_epoches", "3"]
                     + extra, capture=cap)
    out = capsys.readouterr().out
    assert rc == 0 and "Time (ms):" in out
    assert math.isfinite(cap["first_loss"]) and math.isfinite(cap["final_loss"])
    model = cap["model"]
    assert model.conv1.attn_drop == 0.6 and model.conv2.attn_drop == 0.6
    assert isinstance(model.conv1.last_rng_seed, int) and isinstance(model.conv2.last_rng_seed, int)
    assert model.conv1.last_rng_seed != model.conv2.last_rng_seed

"""ops.GATConv(fused="rows") (ops.GATAttentionRows) against the fp64 layer of tests/gat_rect_ref.py on a symmetric graph, a directed
graph and a sampled block, at the bounds of test_gat_block_ops_gpu.py (layer outputs and input gradients 1e-4 of max|ref|,
parameter gradients 1e-4 of their sum of |terms|); the driver's training steps twice from one seed; the layer's refusals."""
import types

import numpy as np
import pytest
import torch

import gat_rect_ref as gref
import sampling_ref as sref
from gnnadvisor_osdi21_amd import _lib, graph, main as driver, ops
from gnnadvisor_osdi21_amd.decider import inputProperty
from gnnadvisor_osdi21_amd.sampling import SampledBlock
from util import assert_close_f64

pytestmark = pytest.mark.gpu


def _info(g, directed):
    ds = types.SimpleNamespace(num_nodes=g.num_nodes, avg_degree=g.avg_degree, avg_edgeSpan=g.avg_edgeSpan, num_features=16)
    ip = inputProperty(g.row_pointers.cuda(), g.column_index.cuda(), g.degrees.cuda(), 32, 32, 4, hiddenDim=16, dataset_obj=ds)
    pp, p2n = _lib.build_part(32, g.row_pointers)
    ip.partPtr, ip.part2Node, ip.directed = pp.cuda(), p2n.cuda(), directed
    return ip


def _input(kind):
    """(inputInfo, source rows, destination rows)"""
    if kind == "block":
        rp, ci = sref.shared_graph()
        b = SampledBlock.sample(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(sref.seed_sets()[65]).cuda(),
                                5, 77, partSize=32)
        return b, b.num_src, b.num_dst
    g = graph.powerlaw_graph(500, 8000, 300, seed=4) if kind == "symmetric" else graph.uniform_graph(300, 3000, symmetric=False)
    return _info(g, kind == "directed"), g.num_nodes, g.num_nodes


@pytest.mark.parametrize("kind", ["symmetric", "directed", "block"])
@pytest.mark.parametrize("fin,fout,heads,concat", [(41, 16, 4, True), (16, 5, 3, False)])
def test_gatconv_rows_matches_the_fp64_layer(kind, fin, fout, heads, concat):
    info, n_src, n_dst = _input(kind)
    torch.manual_seed(fin + heads)
    conv = ops.GATConv(fin, fout, heads=heads, concat=concat, fused="rows").cuda()
    X = torch.randn(n_src, fin, device="cuda", requires_grad=True)
    Y = conv(X, info)
    assert Y.shape == (n_dst, heads * fout if concat else fout)
    wgt = torch.randn(Y.shape, device="cuda")
    (Y * wgt).sum().backward()
    X64 = X.detach().double().requires_grad_()
    P64 = [p.detach().double().requires_grad_() for p in (conv.weights, conv.att_l, conv.att_r)]
    keep = {}
    Y64 = gref.gat_layer64(X64, *P64, info.row_pointers, info.column_index, n_dst, heads, fout, concat, keep=keep)
    (Y64 * wgt.double()).sum().backward()
    what = f"GATConv(fused='rows') {kind} in={fin} out={fout} heads={heads}"
    for got, ref, name in ((Y, Y64.detach(), "Y"), (X.grad, X64.grad, "dX")):
        assert_close_f64(got.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, scale=np.full(ref.shape, float(ref.abs().max())),
                         what=f"{what} {name}")
    for got, ref, scale, name in zip((conv.weights.grad, conv.att_l.grad, conv.att_r.grad), P64,
                                     gref.param_scales(X64, keep, heads, fout), ("dW", "da_l", "da_r")):
        assert_close_f64(got.cpu().numpy(), ref.grad.cpu().numpy(), rtol=1e-4, scale=scale.cpu().numpy(), what=f"{what} {name}")


def test_the_driver_trains_to_the_same_bits_twice_from_one_seed():
    losses = []
    for _ in range(2):
        torch.manual_seed(7)
        cap = {}
        assert driver.main(["--synthetic", "cora-like", "--model", "gat", "--fused_attention", "rows", "--heads", "4",
                            "--num_epoches", "1"], capture=cap) == 0
        assert cap["model"].conv1.rows and cap["model"].conv2.rows
        losses.append((cap["first_loss"], cap["final_loss"]))       # the first training step and the eleventh
    assert losses[0] == losses[1] and all(np.isfinite(losses[0])) and losses[0][0] != losses[0][1]


def test_rows_refuses_attention_dropout_and_edge_features():
    for kw in (dict(attn_drop=0.1), dict(edge_dim=4)):
        with pytest.raises(ValueError, match='fused="rows"\\) has no attention dropout and no edge features'):
            ops.GATConv(8, 4, fused="rows", **kw)
    with pytest.raises(ValueError, match='fused must be True, False or "rows"'):
        ops.GATConv(8, 4, fused="columns")
    for extra in (["--attn_drop", "0.5"], ["--edge_dim", "4"]):
        with pytest.raises(SystemExit, match="--fused_attention rows has no attention dropout and no edge features"):
            driver.main(["--synthetic", "no-such-config", "--model", "gat", "--fused_attention", "rows"] + extra)

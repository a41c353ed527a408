"""Hierarchical pooling through the operators on the GPU: GraphBatch.coarsen, ops.SelectRows / unpool, ops.TopKPooling and
ops.SAGPooling (fused and composed) against fp64 dense restatements, and the existing layers on a coarsened batch.

Bound: |got - ref| <= 1e-4 * max(1, sum |terms|) (util.assert_close_f64), with the sums of |terms| written out for every output:
  X'[i, f]   = m g_r x[r, f], r = perm[i]: one product of a gate that carries the error of its score; scale |X'|.
  d_gate_r   = m sum_f dY[i, f] x[r, f]: S1_r = sum_f |dY x|; through the gate, d_score_r = d_gate_r (1 - g_r^2) with the sum of
               |terms| A_r = m S1_r (1 - g_r^2).
  dX[r, f]   = m g_r dY[i, f] + sum_q d_score_q (d score_q / d x[r, f]): |m g dY| + sum_q A_q |d score_q / d x[r, f]|.
  dw, dW     = sum_q d_score_q (d score_q / d w): sum_q A_q sum |terms of d score_q / d w|.
The rows are chosen by comparisons of scores, so the fp32 paths and the fp64 restatement pick the same rows only when no two
scores around a cut are closer than the rounding of the fp32 score: `_gap_check` asserts on the CPU, in fp64, that the smallest
gap at any cut exceeds twice the bound (terms + 2) * 2^-24 * sum |terms| of either score."""
import numpy as np
import pytest
import torch
from torch.func import functional_call

import topk_ref
from gnnadvisor_osdi21_amd import graph, ops
from gnnadvisor_osdi21_amd.batching import GraphBatch
from util import assert_close_f64

pytestmark = pytest.mark.gpu

_made = {}
SIZES = [int(v) for v in np.random.default_rng(123).integers(3, 91, size=40)]


def _batch():
    """40 graphs of 3 .. 90 nodes, seeded, symmetric: random edges plus a ring, so that no node is without edges (two such nodes
    get the same score from a conv layer, 0 -- an exact tie, which every path breaks alike but the gap check cannot pass)."""
    if "batch" not in _made:
        graphs = []
        for k, n in enumerate(SIZES):
            g = graph.uniform_graph(n, 3 * n, seed=300 + k)
            rows = torch.repeat_interleave(torch.arange(n), (g.row_pointers[1:] - g.row_pointers[:-1]).long())
            ring = torch.arange(n)
            nxt = (ring + 1) % n
            graphs.append(graph.graph_from_edges(torch.cat([rows, ring, nxt]), torch.cat([g.column_index.long(), nxt, ring]), n))
        _made["batch"] = GraphBatch.from_graphs(graphs, partSize=8).to("cuda")
    return _made["batch"]


def _dense(b):
    """The 0/1 adjacency of a batch in fp64 on the device."""
    n = b.num_nodes
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (b.row_pointers[1:] - b.row_pointers[:-1]).long())
    A = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    A[rows, b.column_index.long()] = 1.0
    return A


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _close(got, ref, scale, what):
    worst = float(((got.double() - ref).abs() / (1e-4 * scale.clamp(min=1.0))).max()) if ref.numel() else 0.0
    print(f"{what}: worst err / tol {worst:.4f}")
    assert_close_f64(got.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=1e-4, scale=scale.detach().cpu().numpy(), what=what)


def _gap_check(score64, score_terms, num_terms, gp, how):
    """The fp64 selection, after asserting that no fp32 evaluation of the score can choose other rows."""
    s = score64.cpu().numpy()
    err = (num_terms + 2) * 2.0 ** -24 * score_terms.cpu().numpy()
    smallest = np.inf
    for a, b in zip(gp[:-1], gp[1:]):
        k = topk_ref.keep_count(b - a, **how)
        if k >= b - a:
            continue
        order = np.argsort(-s[a:b], kind="stable")
        lo, hi = a + order[k], a + order[k - 1]                  # the best row that is dropped, the worst that is kept
        gap = s[hi] - s[lo]
        assert gap > 2 * (err[lo] + err[hi]), (a, b, gap, err[lo], err[hi])
        smallest = min(smallest, gap / (err[lo] + err[hi]))
    print(f"smallest gap at a cut: {smallest:.1f} x the fp32 rounding of the two scores")
    mask = topk_ref.keep_mask(s.astype(np.float32), gp, **how)
    return torch.from_numpy(np.flatnonzero(mask)).cuda()


def _pool_grads(layer, params, X, b, wgt):
    """(X', perm, gate[perm], [dX, d params...]) of a pooling layer under the loss sum(wgt * X')."""
    leaves = [X.detach().clone().requires_grad_()] + [p.detach().clone().requires_grad_() for p in params.values()]
    out, small, sel, gate = functional_call(layer, dict(zip(params, leaves[1:])), (leaves[0], b))
    (out * wgt).sum().backward()
    return out.detach(), small, sel, gate.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("how", [dict(ratio=0.5), dict(k=7)], ids=["ratio0.5", "k7"])
@pytest.mark.parametrize("F", [8, 64])
def test_topk_pooling_fused_composed_and_fp64(F, how):
    b = _batch()
    gp = b.graph_pointers.tolist()
    m = 1.5
    X, w = _rand(b.num_nodes, F, seed=F), _rand(F, seed=F + 1)
    x64, w64 = X.double(), w.double()
    nw = w64.norm()
    perm = _gap_check((x64 @ w64) / nw, (x64.abs() @ w64.abs()) / nw, F, gp, how)
    wgt = _rand(perm.numel(), F, seed=F + 2).abs() + 0.1

    def dense(x, w_):
        score = (x @ w_) / w_.norm()
        return (m * torch.tanh(score))[perm].unsqueeze(1) * x[perm], score

    xl, wl = x64.clone().requires_grad_(), w64.clone().requires_grad_()
    ref, score = dense(xl, wl)
    (ref * wgt.double()).sum().backward()
    g = torch.tanh(score.detach())
    # the sums of |terms| (module docstring)
    dY = wgt.double()
    A_ = m * (dY * x64[perm].abs()).sum(1) * (1 - g[perm] ** 2)
    scale_dx = torch.zeros_like(x64)
    scale_dx[perm] = (m * g[perm].abs()).unsqueeze(1) * dY + A_.unsqueeze(1) * w64.abs().unsqueeze(0) / nw
    scale_dw = (A_.unsqueeze(1) * (x64[perm].abs() / nw + score.detach()[perm].abs().unsqueeze(1) * w64.abs().unsqueeze(0) / nw ** 2)).sum(0)
    outs = {}
    for fused in (True, False):
        layer = ops.TopKPooling(F, multiplier=m, fused=fused, **how).cuda()
        out, small, sel, gate, (dX, dw) = _pool_grads(layer, {"weight": w}, X, b, wgt)
        name = f"TopKPooling F={F} {how} {'fused' if fused else 'composed'}"
        assert torch.equal(sel.perm.long(), perm), name                              # identical rows
        assert small.num_nodes == perm.numel() and small.num_graphs == b.num_graphs
        _close(out, ref.detach(), ref.detach().abs(), name + " X'")
        _close(gate, g[perm], g[perm].abs(), name + " gate[perm]")
        _close(dX, xl.grad, scale_dx, name + " dX")
        _close(dw, wl.grad, scale_dw, name + " dw")
        outs[fused] = (out, small, sel)
    # both paths multiply the same two fp32 numbers, and build the same batch
    assert torch.equal(outs[True][0], outs[False][0])
    for name in ("row_pointers", "column_index", "graph_pointers", "partPtr", "part2Node"):
        assert torch.equal(getattr(outs[True][1], name), getattr(outs[False][1], name)), name
    assert torch.equal(outs[True][2].new_id, outs[False][2].new_id) and torch.equal(outs[True][1].degrees, outs[False][1].degrees)


@pytest.mark.parametrize("F", [8, 64])
def test_sag_pooling_fused_composed_and_fp64(F):
    b = _batch()
    gp = b.graph_pointers.tolist()
    how = dict(ratio=0.5)
    deg = b.degrees.double()
    M = deg[:, None] * _dense(b) * deg[None, :]                                      # the GCN layer's matrix (test_directed_ops_gpu.py)
    X, W = _rand(b.num_nodes, F, seed=60 + F), _rand(F, 1, seed=61 + F) / (4 * F ** 0.5)    # (seeds that pass _gap_check)
    x64, W64 = X.double(), W.double()
    terms = M @ (x64.abs() @ W64.abs())
    perm = _gap_check((M @ (x64 @ W64)).reshape(-1), terms.reshape(-1), F + int((M != 0).sum(1).max()), gp, how)
    wgt = _rand(perm.numel(), F, seed=62 + F).abs() + 0.1

    xl, Wl = x64.clone().requires_grad_(), W64.clone().requires_grad_()
    score = (M @ (xl @ Wl)).reshape(-1)
    ref = torch.tanh(score)[perm].unsqueeze(1) * xl[perm]
    (ref * wgt.double()).sum().backward()
    g = torch.tanh(score.detach())
    dY = wgt.double()
    A_ = torch.zeros_like(g)
    A_[perm] = (dY * x64[perm].abs()).sum(1) * (1 - g[perm] ** 2)
    scale_dx = (M.t() @ A_).unsqueeze(1) * W64.abs().reshape(1, -1)
    scale_dx[perm] += g[perm].abs().unsqueeze(1) * dY
    scale_dW = ((M.t() @ A_).unsqueeze(1) * x64.abs()).sum(0).reshape(-1, 1)
    outs = {}
    for fused in (True, False):
        layer = ops.SAGPooling(F, fused=fused, **how).cuda()
        out, small, sel, gate, (dX, dW) = _pool_grads(layer, {"gnn.weights": W}, X, b, wgt)
        name = f"SAGPooling F={F} {'fused' if fused else 'composed'}"
        assert torch.equal(sel.perm.long(), perm), name
        _close(out, ref.detach(), ref.detach().abs() + (terms.reshape(-1)[perm].unsqueeze(1) * x64[perm].abs()), name + " X'")
        _close(gate, g[perm], terms.reshape(-1)[perm], name + " gate[perm]")
        _close(dX, xl.grad, scale_dx, name + " dX")
        _close(dW, Wl.grad, scale_dW, name + " dW")
        outs[fused] = sel
    assert torch.equal(outs[True].new_id, outs[False].new_id)


def _coarse(seed=21, ratio=0.6):
    """(the batch, a coarsened batch, its selection, the dense adjacency of the coarsened batch cut out of the old one)."""
    b = _batch()
    small, sel = b.coarsen(_rand(b.num_nodes, seed=seed), ratio=ratio, want_edge_ids=True)
    perm = sel.perm.long()
    return b, small, sel, _dense(b)[perm][:, perm]


def test_coarsen_cuts_the_induced_subgraph_out():
    b, small, sel, A = _coarse()
    assert torch.equal(_dense(small), A) and small.num_nodes == sel.perm.numel() and sel.num_nodes == b.num_nodes
    sizes = np.diff(small.graph_pointers.cpu().numpy())
    assert sizes.tolist() == [topk_ref.keep_count(n, ratio=0.6) for n in SIZES]
    assert small.directed == b.directed and small.partSize == b.partSize and small.dimWorker == b.dimWorker and small.x is None
    assert torch.equal(small.degrees, graph.degrees_from_rowptr(small.row_pointers))
    fresh = GraphBatch(small.row_pointers, small.column_index, small.graph_pointers, partSize=b.partSize)
    assert torch.equal(fresh.partPtr, small.partPtr) and torch.equal(fresh.part2Node, small.part2Node)
    # the edge ids name the edges that survived
    assert torch.equal(sel.new_id[b.column_index[sel.edge_ids.long()].long()], small.column_index)
    with pytest.raises(ValueError, match="exactly one of ratio and k"):
        b.coarsen(_rand(b.num_nodes, seed=1))
    with pytest.raises(TypeError, match="score must be float32"):
        b.coarsen(_rand(b.num_nodes + 1, seed=1), ratio=0.5)


def _layer_check(ours, dense, tensors, names, what):
    """ours(*fp32) against dense(*fp64), the output and every gradient; the scales are `dense` on the absolute values."""
    wgt = _rand(*ours(*tensors).shape, seed=99).abs() + 0.1

    def grads(fn, ts, wg):
        leaves = [t.detach().clone().requires_grad_() for t in ts]
        Y = fn(*leaves)
        (Y * wg).sum().backward()
        return [Y.detach()] + [t.grad for t in leaves]

    got = grads(ours, tensors, wgt)
    ref = grads(dense, [t.double() for t in tensors], wgt.double())
    scale = grads(dense, [t.double().abs() for t in tensors], wgt.double())
    for name, g_, r_, s_ in zip(["Y"] + ["d" + n for n in names], got, ref, scale):
        _close(g_, r_, s_, f"{what} {name}")


@pytest.mark.parametrize("layer", ["gcn", "gin", "sage", "readout"])
def test_layers_on_a_coarsened_batch_against_fp64(layer):
    _, small, _, A = _coarse()
    n, Fin, H = small.num_nodes, 12, 16
    gp = small.graph_pointers.tolist()
    X, W, W2 = _rand(n, Fin, seed=31), _rand(Fin, H, seed=32) / 4, _rand(Fin, H, seed=33) / 4
    if layer == "gcn":
        deg = small.degrees.double()
        M = deg[:, None] * A * deg[None, :]
        conv = ops.GCNConv(Fin, H).cuda()
        _layer_check(lambda x, w: functional_call(conv, {"weights": w}, (x, small)), lambda x, w: M @ (x @ w), [X, W], ["X", "W"], "GCN")
    elif layer == "gin":
        conv = ops.GINConv(Fin, H, update_first=False).cuda()
        _layer_check(lambda x, w: functional_call(conv, {"weights": w}, (x, small)), lambda x, w: (0.5 * (A @ x)) @ w, [X, W], ["X", "W"],
                     "GIN")
    elif layer == "sage":
        conv = ops.SAGEConv(Fin, H, aggregator="mean").cuda()
        inv = 1.0 / A.sum(1).clamp(min=1.0)
        _layer_check(lambda x, w, v: functional_call(conv, {"weights_self": w, "weights_neigh": v}, (x, small)),
                     lambda x, w, v: x @ w + (inv[:, None] * (A @ x)) @ v, [X, W, W2], ["X", "W_self", "W_neigh"], "SAGE")
    else:
        readout = ops.Readout(("sum", "mean"))

        def dense(x):
            rows = [x[a:b].sum(0) if b > a else x.new_zeros(x.shape[1]) for a, b in zip(gp[:-1], gp[1:])]
            means = [x[a:b].mean(0) if b > a else x.new_zeros(x.shape[1]) for a, b in zip(gp[:-1], gp[1:])]
            return torch.cat((torch.stack(rows), torch.stack(means)), 1)

        _layer_check(lambda x: readout(x, small), dense, [X], ["X"], "Readout")


def test_fused_gat_on_a_coarsened_batch_against_fp64():
    """One head.  The weights of the softmax sum to 1 over a row's edges: the scale of Y is alpha |H|, H = |X| |W|."""
    _, small, _, A = _coarse()
    n, Fin, H = small.num_nodes, 12, 16
    conv = ops.GATConv(Fin, H, heads=1, fused=True).cuda()
    X = _rand(n, Fin, seed=41)
    with torch.no_grad():
        Y = conv(X, small)
        W, al, ar = conv.weights.double(), conv.att_l.double().reshape(-1), conv.att_r.double().reshape(-1)
        Hd = X.double() @ W
        s = torch.nn.functional.leaky_relu((Hd @ al)[:, None] + (Hd @ ar)[None, :], conv.negative_slope)
        s = torch.where(A > 0, s, torch.full_like(s, float("-inf")))
        alpha = torch.where(A.sum(1, keepdim=True) > 0, torch.softmax(s, 1), torch.zeros_like(s)).nan_to_num(0.0)
        _close(Y, alpha @ Hd, alpha @ (X.double().abs() @ W.abs()), "fused GAT on a coarsened batch")
    # the backward gathers through the structure again: it runs, and a row without edges gets what its own term gives
    Xg = X.clone().requires_grad_()
    conv(Xg, small).sum().backward()
    assert bool(torch.isfinite(Xg.grad).all())


def test_two_levels_of_pooling_in_a_row():
    b = _batch()
    gp = b.graph_pointers.tolist()
    F = 8
    X, w1, w2 = _rand(b.num_nodes, F, seed=51), _rand(F, seed=52), _rand(F, seed=53)
    how = dict(ratio=0.5)
    # fp64: level 1, then level 2 on what level 1 kept
    x64 = X.double()
    s1 = (x64 @ w1.double()) / w1.double().norm()
    p1 = _gap_check(s1, (x64.abs() @ w1.double().abs()) / w1.double().norm(), F, gp, how)
    x1 = torch.tanh(s1)[p1].unsqueeze(1) * x64[p1]
    gp1 = [0] + list(np.cumsum([topk_ref.keep_count(n, **how) for n in SIZES]))
    s2 = (x1 @ w2.double()) / w2.double().norm()
    p2 = _gap_check(s2, (x1.abs() @ w2.double().abs()) / w2.double().norm(), F + 1, gp1, how)
    x2 = torch.tanh(s2)[p2].unsqueeze(1) * x1[p2]
    l1, l2 = ops.TopKPooling(F, **how).cuda(), ops.TopKPooling(F, **how).cuda()
    with torch.no_grad():
        l1.weight.copy_(w1)
        l2.weight.copy_(w2)
    Xg = X.clone().requires_grad_()
    y1, b1, sel1, _ = l1(Xg, b)
    y2, b2, sel2, _ = l2(y1, b1)
    assert torch.equal(sel1.perm.long(), p1) and torch.equal(sel2.perm.long(), p2) and b1.graph_pointers.tolist() == [int(v) for v in gp1]
    _close(y2, x2, x2.abs() + 1e-3, "two levels X''")
    assert torch.equal(_dense(b2), _dense(b)[p1][:, p1][p2][:, p2])
    ops.Readout(("sum",))(y2, b2).sum().backward()
    assert bool(torch.isfinite(Xg.grad).all()) and int((Xg.grad.abs().sum(1) > 0).sum()) >= p2.numel()


def test_select_rows_and_unpool_round_trip():
    b, small, sel, _ = _coarse()
    n, F = b.num_nodes, 20
    X = _rand(n, F, seed=61).requires_grad_()
    scale = _rand(n, seed=62).requires_grad_()
    perm = sel.perm.long()
    Y = ops.SelectRows.apply(X, scale, sel)
    assert torch.equal(Y, scale[perm].unsqueeze(1) * X[perm])
    # what the op keeps for the backward: new_id, and X and scale because both need a gradient
    saved = sorted(tuple(t.shape) for t in Y.grad_fn.saved_tensors if t is not None)
    assert saved == sorted([(n,), (n,), (n, F)])
    back = ops.unpool(Y, sel)
    kept = torch.zeros(n, dtype=torch.bool, device="cuda")
    kept[perm] = True
    assert torch.equal(back[perm], Y) and bool((back[~kept] == 0).all()) and tuple(back.shape) == (n, F)
    wgt = _rand(n, F, seed=63)
    (back * wgt).sum().backward()
    ref_dx = torch.zeros(n, F, device="cuda")
    ref_dx[perm] = scale.detach()[perm].unsqueeze(1) * wgt[perm]
    assert torch.equal(X.grad, ref_dx)
    ref_ds = torch.zeros(n, dtype=torch.float64, device="cuda")
    ref_ds[perm] = (wgt[perm].double() * X.detach()[perm].double()).sum(1)
    terms = torch.zeros(n, dtype=torch.float64, device="cuda")
    terms[perm] = (wgt[perm].double() * X.detach()[perm].double()).abs().sum(1)
    _close(scale.grad, ref_ds, terms, "d_scale")
    # a plain gather saves no X; X without a gradient saves no scale
    plain = ops.SelectRows.apply(X, None, sel)
    assert torch.equal(plain, X.detach()[perm]) and sorted(tuple(t.shape) for t in plain.grad_fn.saved_tensors if t is not None) == [(n,)]
    only_scale = ops.SelectRows.apply(X.detach(), scale, sel)
    assert sorted(tuple(t.shape) for t in only_scale.grad_fn.saved_tensors if t is not None) == sorted([(n,), (n, F)])
    assert not ops.SelectRows.apply(X.detach(), scale.detach(), sel).requires_grad
    with pytest.raises(ValueError, match="X must be"):
        ops.SelectRows.apply(X[:-1], None, sel)
    with pytest.raises(ValueError, match="X_small must be"):
        ops.unpool(Y[:-1], sel)

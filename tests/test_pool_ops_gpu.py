"""The readout operators (ops.SegmentPool, global_*_pool, Readout) and batches of graphs (batching.GraphBatch, GraphDataset) on the
GPU, against fp64 dense autograd.

Bound: |got - ref| <= 1e-4 * max(1, scale) (util.assert_close_f64), as tests/test_directed_ops_gpu.py: for a sum or a mean the
scale is the sum of |terms| (the same formula on the absolute values of the inputs); a max or a min copies one input element, and
its gradient one gradient element, so their scale is |reference| itself."""
import numpy as np
import pytest
import torch
from torch.func import functional_call

from gnnadvisor_osdi21_amd import graph, ops
from gnnadvisor_osdi21_amd.batching import GraphBatch, GraphDataset
from util import assert_close_f64

pytestmark = pytest.mark.gpu

_made = {}


def _graphs():
    """21 graphs of 0 .. 40 nodes (one without nodes, one of a single node), seeded."""
    if "graphs" not in _made:
        sizes = [7, 40, 0, 1, 23, 12, 31, 5, 18, 2, 36, 9, 27, 14, 3, 40, 21, 11, 6, 33, 16]
        _made["graphs"] = [graph.uniform_graph(n, 3 * n, seed=50 + k) for k, n in enumerate(sizes)]
    return _made["graphs"]


def _batch(partSize=32):
    if ("batch", partSize) not in _made:
        _made["batch", partSize] = GraphBatch.from_graphs(_graphs(), partSize=partSize).to("cuda")
    return _made["batch", partSize]


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _dense_pool(X, gp, mode):
    """One statistic over the segments with torch ops a segment at a time: differentiable in any dtype."""
    rows = []
    for a, b in zip(gp[:-1], gp[1:]):
        seg = X[a:b]
        if b <= a:
            rows.append(X.new_zeros(X.shape[1]))
        else:
            rows.append({"sum": seg.sum(0), "mean": seg.mean(0), "max": seg.amax(0), "min": seg.amin(0)}[mode])
    return torch.stack(rows)


def _dense_readout(X, gp, modes):
    return torch.cat([_dense_pool(X, gp, m) for m in modes], 1)


def _grads(fn, tensors, wgt):
    leaves = [t.detach().clone().requires_grad_() for t in tensors]
    Y = fn(*leaves)
    (Y * wgt).sum().backward()
    return Y.detach(), [t.grad for t in leaves]


def _check(ours, dense, dense_scale, tensors, names, what):
    """ours(*fp32) against dense(*fp64): the output and every gradient.  dense_scale(*|fp64|) gives the scales, None: |ref|."""
    wgt = _rand(*ours(*tensors).shape, seed=99).abs() + 0.1
    Y, got = _grads(ours, tensors, wgt)
    Y64, ref = _grads(dense, [t.double() for t in tensors], wgt.double())
    if dense_scale is None:
        S, scale = Y64.abs(), [r.abs() for r in ref]
    else:
        S, scale = _grads(dense_scale, [t.double().abs() for t in tensors], wgt.double())
    for name, g_, r_, s_ in zip(["Y"] + ["d" + n for n in names], [Y] + got, [Y64] + ref, [S] + scale):
        worst = float(((g_.double() - r_).abs() / (1e-4 * s_.clamp(min=1.0))).max()) if r_.numel() else 0.0
        print(f"{what} {name}: worst err / tol {worst:.4f}")
        assert_close_f64(g_.cpu().numpy(), r_.cpu().numpy(), rtol=1e-4, scale=s_.cpu().numpy(), what=f"{what} {name}")


@pytest.mark.parametrize("F", [5, 64])
@pytest.mark.parametrize("mode", ops.POOL_MODES)
def test_global_pools_against_fp64(mode, F):
    b = _batch()
    gp = b.graph_pointers.tolist()
    X = _rand(b.num_nodes, F, seed=1)
    fn = {"sum": ops.global_add_pool, "mean": ops.global_mean_pool, "max": ops.global_max_pool, "min": ops.global_min_pool}[mode]
    dense = lambda x: _dense_pool(x, gp, mode)
    _check(lambda x: fn(x, b), dense, dense if mode in ("sum", "mean") else None, [X], ["X"], f"global {mode} F={F}")
    # graph_pointers alone stand for the batch
    assert torch.equal(fn(X, b.graph_pointers), fn(X, b))


@pytest.mark.parametrize("modes", [("sum", "max"), ("mean", "min", "max"), ("sum", "mean", "max", "min"), ("min",)], ids="+".join)
def test_readout_against_fp64_and_the_composition(modes):
    b = _batch()
    gp = b.graph_pointers.tolist()
    X = _rand(b.num_nodes, 33, seed=2)
    fused, composed = ops.Readout(modes), ops.Readout(modes, fused=False)
    assert tuple(fused(X, b).shape) == (b.num_graphs, 33 * len(modes))
    sums = all(m in ("sum", "mean") for m in modes)
    # (the extrema next to sums: the scale of a sum, which is no smaller than that of an element)
    scale = lambda x: _dense_readout(x, gp, ["sum" if m in ("max", "min") else m for m in modes])
    for name, layer in (("fused", fused), ("composed", composed)):
        _check(lambda x: layer(x, b), lambda x: _dense_readout(x, gp, modes), scale if not sums else
               (lambda x: _dense_readout(x, gp, modes)), [X], ["X"], f"Readout {name} {modes}")
    # both paths pick the same elements: the extrema agree bit for bit, the sums to the order of their additions
    Yf, Yc = fused(X, b), composed(X, b)
    for k, m in enumerate(modes):
        f, c = Yf[:, 33 * k: 33 * k + 33], Yc[:, 33 * k: 33 * k + 33]
        if m in ("max", "min"):
            assert torch.equal(f, c), m
        else:
            S = _dense_pool(X.double().abs(), gp, m)
            assert bool(((f.double() - c.double()).abs() <= 1e-4 * S.clamp(min=1.0)).all()), m


def test_segment_pool_saves_nothing_of_the_size_of_x_and_skips_what_needs_no_gradient():
    b = _batch()
    X = _rand(b.num_nodes, 16, seed=3).requires_grad_()
    s, mx, mn = ops.SegmentPool.apply(X, b, True, True, False, False)
    assert mn is None and s.shape == mx.shape == (b.num_graphs, 16)
    saved = [t for t in s.grad_fn.saved_tensors if t is not None]
    assert sorted(tuple(t.shape) for t in saved) == sorted([(b.num_graphs + 1,), (b.num_graphs, 16)])
    # only the sum is used: the backward runs without the max's gradient
    s.sum().backward()
    counts = torch.tensor(np.diff(b.graph_pointers.cpu().numpy()), device="cuda")
    assert torch.equal(X.grad, torch.ones_like(X)) and int(counts.sum()) == b.num_nodes
    # X needs no gradient: nothing runs, nothing is returned
    Xn = X.detach()
    out = ops.SegmentPool.apply(Xn, b, True, False, False, True)[0]
    assert not out.requires_grad


def test_gin_readout_linear_model_against_fp64():
    b = _batch()
    gp = b.graph_pointers.tolist()
    n, Fin, H, C = b.num_nodes, 12, 16, 3
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (b.row_pointers[1:] - b.row_pointers[:-1]).long())
    A = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    A.index_put_((rows, b.column_index.long()), torch.ones(rows.numel(), dtype=torch.float64, device="cuda"), accumulate=True)
    conv = ops.GINConv(Fin, H, update_first=False).cuda()
    readout = ops.Readout(("sum", "mean"))
    X, W, Wl, bl = _rand(n, Fin, seed=4), _rand(Fin, H, seed=5) / 4, _rand(2 * H, C, seed=6) / 4, _rand(C, seed=7)

    def ours(x, w, wl, b_):
        return readout(functional_call(conv, {"weights": w}, (x, b)), b) @ wl + b_

    def dense(x, w, wl, b_):
        return _dense_readout((0.5 * (A @ x)) @ w, gp, ("sum", "mean")) @ wl + b_

    _check(ours, dense, dense, [X, W, Wl, bl], ["X", "W", "W_lin", "b_lin"], "GIN -> Readout -> Linear")


def test_dataset_batch_equals_from_graphs():
    graphs = _graphs()
    ds = GraphDataset.from_graphs(graphs, x=torch.arange(sum(g.num_nodes for g in graphs), dtype=torch.float32).reshape(-1, 1),
                                  y=torch.arange(len(graphs)), device="cuda")
    starts = np.cumsum([0] + [g.num_nodes for g in graphs])
    for ids in ([0, 1, 2, 3, 4], [20, 3, 3, 2, 7, 0, 20], [2], [2, 2], list(range(len(graphs)))[::-1], []):
        got = ds.batch(ids, partSize=4)
        ref = GraphBatch.from_graphs([graphs[i] for i in ids], partSize=4)
        for name in ("row_pointers", "column_index", "graph_pointers", "partPtr", "part2Node"):
            a, r = getattr(got, name), getattr(ref, name)
            assert a.dtype == torch.int32 and a.is_cuda and a.cpu().tolist() == r.tolist(), (ids, name)
        assert got.num_graphs == len(ids) and got.batch.cpu().tolist() == ref.batch.tolist()
        assert torch.allclose(got.degrees.cpu(), ref.degrees)
        assert got.y.cpu().tolist() == list(ids)
        want_x = [float(starts[i] + r) for i in ids for r in range(graphs[i].num_nodes)]
        assert got.x.reshape(-1).cpu().tolist() == want_x


@pytest.mark.parametrize("layer", ["gcn", "sage"])
def test_existing_layers_take_a_batch_and_give_the_per_graph_outputs(layer):
    """The block-diagonal CSR keeps the graphs apart: a layer on the batch gives the rows a layer on each graph gives.  Every row
    here sums at most 40 + 12 products, in an order that may differ between the two calls: at most 52 * 2^-24 < 1e-5 of the sum of
    |terms|, which the same layer gives on the absolute values."""
    b = _batch()
    graphs = _graphs()
    conv = (ops.GCNConv(12, 8) if layer == "gcn" else ops.SAGEConv(12, 8, aggregator="mean")).cuda()
    params = {k: v.detach() for k, v in conv.named_parameters()}
    X = _rand(b.num_nodes, 12, seed=8)
    with torch.no_grad():
        Y = conv(X, b)
        S = functional_call(conv, {k: v.abs() for k, v in params.items()}, (X.abs(), b))
        parts, at = [], 0
        for g in graphs:
            if g.num_nodes:
                one = GraphBatch.from_graphs([g]).to("cuda")
                parts.append(conv(X[at: at + g.num_nodes].contiguous(), one))
            at += g.num_nodes
        ref = torch.cat(parts)
    assert Y.shape == ref.shape
    assert bool(((Y - ref).abs() <= 1e-5 * S.clamp(min=1.0)).all()), float((Y - ref).abs().max())

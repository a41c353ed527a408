"""Hierarchical pooling, the parts that need no GPU (the binding surface of include/gnna_topk.h and the build lists are pinned by
test_binding_table_host.py): the header's constant, the refusals the three entries make before any device work, the rule for the
rows a segment keeps, the numpy reference against a brute-force statement of the selection, the wrappers, and GraphBatch without
the new keywords."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import topk_ref
from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOPK, FWD, BWD = "gnna_segment_topk_i32", "gnna_gather_rows_scale_ld_f32", "gnna_gather_rows_scale_backward_ld_f32"


def test_the_header_defines_the_constant_the_binding_restates():
    header = open(os.path.join(ROOT, "include", "gnna_topk.h")).read()
    assert "#define GNNA_TOPK_WAVE_ROWS %d\n" % _lib.TOPK_WAVE_ROWS in header


_B = [(ctypes.c_float * 64)() for _ in range(8)]
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = [ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p).value for _ in range(12)]
INVALID, UNSUPPORTED = -1, -3                                                # include/gnna.h


def _last():
    return _lib.load().gnna_last_error().decode()


def _topk(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(score=F[0], n=6, gp=I[0], g=2, ratio=0.5, k=0, rp=I[1], ci=I[2], nnz=8, part=4, new_id=I[3], perm=I[4], new_gp=I[5],
             new_rp=I[6], new_ci=I[7], eid=I[8], pp=I[9], p2n=I[10], row_cap=6, edge_cap=8, part_cap=8)
    a.update(kw)
    counts = a.get("counts", (ctypes.c_int64 * 3)())
    return _lib.load().gnna_segment_topk_i32(a["score"], a["n"], a["gp"], a["g"], a["ratio"], a["k"], a["rp"], a["ci"], a["nnz"], a["part"],
                                             a["new_id"], a["perm"], a["new_gp"], a["new_rp"], a["new_ci"], a["eid"], a["pp"], a["p2n"],
                                             a["row_cap"], a["edge_cap"], a["part_cap"], counts, None)


def test_refusals_of_the_structure_entry():
    assert _topk(counts=None) == INVALID and _last() == TOPK + ": null counts"
    assert _topk(n=-1) == INVALID and _last() == TOPK + ": negative size (num_rows=-1 num_segments=2 nnz=8)"
    assert _topk(g=-2) == INVALID and _last() == TOPK + ": negative size (num_rows=6 num_segments=-2 nnz=8)"
    assert _topk(nnz=-3) == INVALID and _last() == TOPK + ": negative size (num_rows=6 num_segments=2 nnz=-3)"
    assert _topk(g=1 << 29) == UNSUPPORTED and _last() == TOPK + ": 536870912 segments in one call (at most 536870911): shard the batch"
    assert _topk(n=1 << 31) == UNSUPPORTED and _last() == TOPK + ": 2147483648 rows in one call (at most 2147483647: graph_pointers is int32)"
    assert _topk(nnz=1 << 31) == UNSUPPORTED and _last() == TOPK + ": 2147483648 edges in one call (at most 2147483647: row_pointers is int32)"
    # exactly one of ratio and k_fixed
    assert _topk(ratio=0.5, k=3) == INVALID and _last() == TOPK + ": ratio and k_fixed are both given (ratio=0.5 k_fixed=3): one of them is 0"
    assert _topk(ratio=0.0, k=0) == INVALID and _last() == TOPK + ": neither ratio nor k_fixed is given"
    assert _topk(ratio=0.0, k=-1) == INVALID and _last() == TOPK + ": k_fixed must be >= 1 (got -1)"
    for ratio, shown in ((-0.25, "-0.25"), (1.5, "1.5"), (float("inf"), "inf")):
        assert _topk(ratio=ratio) == INVALID and _last() == TOPK + f": ratio must be in (0, 1] (got {shown})"
    assert _topk(ratio=float("nan")) == INVALID and _last().startswith(TOPK + ": ratio must be in (0, 1] (got ") and "nan" in _last()
    for cap in ("row_cap", "edge_cap", "part_cap"):
        assert _topk(**{cap: -1}) == INVALID and _last().startswith(TOPK + ": negative capacity (") and "=-1" in _last(), cap
    assert _topk(part=-1) == INVALID and _last() == TOPK + ": partSize must not be negative (got -1)"
    assert _topk(rp=None) == INVALID and _last() == TOPK + ": row_pointers and column_index come together"
    assert _topk(ci=None) == INVALID and _last() == TOPK + ": row_pointers and column_index come together"
    assert _topk(rp=None, ci=None) == INVALID and _last() == TOPK + ": a partition (partSize=4) needs row_pointers and column_index"
    for name in ("gp", "new_gp"):
        assert _topk(**{name: None}) == INVALID and _last() == TOPK + ": null graph_pointers or new_graph_pointers"
    for name in ("score", "new_id"):
        assert _topk(**{name: None}) == INVALID and _last() == TOPK + ": null score or new_id"
    assert _topk(perm=None) == INVALID and _last() == TOPK + ": null perm"
    for name in ("new_rp", "new_ci"):
        assert _topk(**{name: None}) == INVALID and _last() == TOPK + ": null new_row_pointers or new_column_index"
    for name in ("pp", "p2n"):
        assert _topk(**{name: None}) == INVALID and _last() == TOPK + ": null partPtr or part2Node"
    # an output that is an input or another output
    outputs = ("new_id", "perm", "new_gp", "new_rp", "new_ci", "eid", "pp", "p2n")
    for name in outputs:
        for inp in (F[0], I[0], I[1], I[2]):
            assert _topk(**{name: inp}) == INVALID and _last() == TOPK + ": an output must not alias an input", name
    for a, b in zip(outputs, outputs[1:]):
        assert _topk(**{a: I[11], b: I[11]}) == INVALID and _last() == TOPK + ": the outputs must not alias each other", (a, b)
    # every refusal leaves counts at zero
    counts = (ctypes.c_int64 * 3)(7, 7, 7)
    assert _topk(counts=counts, part=-1) == INVALID and list(counts) == [0, 0, 0]


def _fwd(**kw):
    a = dict(x=F[0], ld_in=8, n=6, perm=I[0], scale=F[1], out=F[2], ld_out=8, m=3, dim=4)
    a.update(kw)
    return _lib.load().gnna_gather_rows_scale_ld_f32(a["x"], a["ld_in"], a["n"], a["perm"], a["scale"], a["out"], a["ld_out"], a["m"],
                                                     a["dim"], None)


def _bwd(**kw):
    a = dict(dy=F[0], ld_dout=8, m=3, new_id=I[0], x=F[1], ld_in=8, scale=F[2], dx=F[3], ld_din=8, ds=F[4], n=6, dim=4)
    a.update(kw)
    return _lib.load().gnna_gather_rows_scale_backward_ld_f32(a["dy"], a["ld_dout"], a["m"], a["new_id"], a["x"], a["ld_in"], a["scale"],
                                                              a["dx"], a["ld_din"], a["ds"], a["n"], a["dim"], None)


@pytest.mark.parametrize("call, name", [(_fwd, FWD), (_bwd, BWD)], ids=["forward", "backward"])
def test_refusals_both_gathers_make_alike(call, name):
    assert call(dim=0) == INVALID and _last() == f"{name}: dim must be >= 1 (got 0)"
    assert call(dim=-3) == INVALID and _last() == f"{name}: dim must be >= 1 (got -3)"
    assert call(n=-1) == INVALID and _last() == f"{name}: negative size (num_in_rows=-1 num_out_rows=3)"
    assert call(m=-2) == INVALID and _last() == f"{name}: negative size (num_in_rows=6 num_out_rows=-2)"
    for size in ("n", "m"):
        assert call(**{size: 1 << 31}) == UNSUPPORTED and _last() == f"{name}: 2147483648 rows in one call (at most 2147483647: the row ids are int32)"
    assert call(ld_in=3) == INVALID and _last().startswith(name + ": row strides must be >= dim and < 2^29 elements (") and "ld_in=3" in _last()
    assert call(ld_in=1 << 29) == INVALID and "ld_in=536870912" in _last()


def test_refusals_of_the_forward_gather():
    for ld in ("ld_in", "ld_out"):
        assert _fwd(**{ld: 3}) == INVALID and f"{ld}=3" in _last() and _last().endswith("dim=4)"), ld
        assert _fwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    for name in ("x", "perm", "scale", "out"):
        assert _fwd(**{name: F[7] + 2}) == INVALID and _last() == FWD + ": feature, scale, row id and output pointers must be 4-byte aligned"
    for inp in (F[0], I[0], F[1]):
        assert _fwd(out=inp) == INVALID and _last() == FWD + ": an output must not alias an input"
    assert _fwd(out=None) == INVALID and _last() == FWD + ": null output pointer"
    assert _fwd(perm=None) == INVALID and _last() == FWD + ": null perm"
    assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
    assert _fwd(m=0) == 0                                                     # no row to gather: nothing to write
    assert _fwd(m=0, x=None, perm=None, scale=None, out=None) == 0


def test_refusals_of_the_backward_gather():
    for ld in ("ld_dout", "ld_in", "ld_din"):
        assert _bwd(**{ld: 3}) == INVALID and f"{ld}=3" in _last() and _last().endswith("dim=4)"), ld
        assert _bwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    # (a null output's stride strides nothing: the call gets past the stride check to the next refusal)
    assert _bwd(dx=None, ld_din=3, new_id=None) == INVALID and _last() == BWD + ": null new_id"
    assert _bwd(ds=None, ld_in=3, new_id=None) == INVALID and _last() == BWD + ": null new_id"
    assert _bwd(dx=None, ds=None) == INVALID and _last() == BWD + ": null output pointers: d_input and d_scale are both null"
    for name in ("dy", "new_id", "x", "scale", "dx", "ds"):
        assert _bwd(**{name: F[7] + 2}) == INVALID and _last() == BWD + ": gradient, feature, scale and row id pointers must be 4-byte aligned"
    for name in ("dx", "ds"):
        for inp in (F[0], I[0], F[1], F[2]):
            assert _bwd(**{name: inp}) == INVALID and _last() == BWD + ": an output must not alias an input", name
    assert _bwd(dx=F[5], ds=F[5]) == INVALID and _last() == BWD + ": the outputs must not alias each other"
    assert _bwd(new_id=None) == INVALID and _last() == BWD + ": null new_id"
    assert _bwd(x=None) == INVALID and _last() == BWD + ": d_scale needs the feature pointer"
    assert _bwd(dy=None) == INVALID and _last() == BWD + ": null gradient pointer"
    assert _bwd(n=0) == 0                                                     # no row: nothing to write
    assert _bwd(n=0, dy=None, new_id=None, x=None, scale=None) == 0


def test_deterministic_tuning_does_not_refuse_the_entries():
    try:
        _lib.set_tuning(deterministic=1)
        # (the next refusal is met instead of GNNA_ERR_UNSUPPORTED: no device is touched here)
        assert _topk(perm=None) == INVALID and _last() == TOPK + ": null perm"
        assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
        assert _bwd(new_id=None) == INVALID and _last() == BWD + ": null new_id"
    finally:
        _lib.reset_tuning()


@pytest.mark.parametrize("ratio", [0.5, 0.8, 0.1, 1.0 / 3.0, 1.0])
def test_the_rows_a_segment_keeps_under_a_ratio(ratio):
    """min(n, ceil(ratio * n)) with one IEEE double multiplication: the C side against numpy, bit for bit, and against exact
    rational arithmetic where the product is exact."""
    for n in range(0, 301):
        want = int(min(n, np.ceil(np.float64(ratio) * np.float64(n))))
        assert _lib.topk_keep_count(n, ratio=ratio) == want == topk_ref.keep_count(n, ratio=ratio), n
        assert (want >= 1) == (n >= 1) and want <= n
    if ratio in (0.5, 1.0):
        assert [_lib.topk_keep_count(n, ratio=ratio) for n in (1, 2, 3, 7, 300)] == [-(-n * int(ratio * 2) // 2) for n in (1, 2, 3, 7, 300)]


def test_the_rows_a_segment_keeps_under_a_fixed_k_and_what_the_helper_refuses():
    for k in (1, 5, 300):
        assert [_lib.topk_keep_count(n, k=k) for n in range(0, 302)] == [min(n, k) for n in range(0, 302)]
    assert _lib.topk_keep_count(5, ratio=0.5, k=2) == -1 and _lib.topk_keep_count(5) == -1 and _lib.topk_keep_count(-1, ratio=0.5) == -1
    assert _lib.topk_keep_count(5, ratio=1.5) == -1 and _lib.topk_keep_count(5, ratio=float("nan")) == -1 and _lib.topk_keep_count(5, k=-2) == -1


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0], dtype=np.float32)


def _nan(sign):
    return np.array([0x7FC00000 | (sign << 31)], dtype=np.uint32).view(np.float32)[0]


def test_the_reference_agrees_with_the_brute_force_check():
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(0, 14))
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 5))))
        gp = [int(rng.integers(0, 3))] + [int(c) for c in cuts] + [n - int(rng.integers(0, 3))]
        if trial % 3 == 0:
            score = rng.integers(0, 3, size=n).astype(np.float32)               # many ties
        elif trial % 3 == 1:
            score = rng.choice(np.concatenate((SPECIALS, [_nan(0), _nan(1)])), size=n).astype(np.float32)
        else:
            score = rng.standard_normal(n).astype(np.float32)
        how = dict(ratio=float(rng.choice([0.01, 0.5, 0.8, 1.0]))) if trial % 2 else dict(k=int(rng.integers(1, 6)))
        assert np.array_equal(topk_ref.keep_mask(score, gp, **how), topk_ref.brute_force_keep(score, gp, **how)), (trial, gp, score, how)


def test_the_reference_on_a_case_worked_by_hand():
    # two graphs: rows 0..3 and 4..6; ratio 0.5 keeps 2 of each; ties go to the smaller row; -0 < +0; NaN(+) is the largest
    score = np.array([1.0, 3.0, 3.0, 3.0, -0.0, 0.0, _nan(0)], dtype=np.float32)
    rp = [0, 2, 4, 5, 6, 8, 9, 10]
    ci = [1, 2, 0, 2, 1, 7, 5, 6, -1, 4]           # row 0: 1 2; row 1: 0 2; row 2: 1; row 3: 7 (outside); row 4: 5 6; row 5: -1; row 6: 4
    r = topk_ref.segment_topk(score, [0, 4, 7], ratio=0.5, row_pointers=rp, column_index=ci, partSize=1)
    assert r["perm"].tolist() == [1, 2, 5, 6] and r["new_id"].tolist() == [-1, 0, 1, -1, -1, 2, 3]
    assert r["graph_pointers"].tolist() == [0, 2, 4]
    assert r["row_pointers"].tolist() == [0, 1, 2, 2, 2] and r["column_index"].tolist() == [1, 0] and r["edge_ids"].tolist() == [3, 4]
    assert r["partPtr"].tolist() == [0, 1, 2] and r["part2Node"].tolist() == [0, 1]
    assert topk_ref.segment_topk(score, [0, 4, 7], k=1)["perm"].tolist() == [1, 6]


def test_the_wrappers_and_the_ops():
    sig = inspect.signature(_lib.segment_topk).parameters
    assert list(sig)[:8] == ["score", "graph_pointers", "ratio", "k", "row_pointers", "column_index", "partSize", "want_edge_ids"]
    assert sig["ratio"].default is None and sig["k"].default is None and sig["want_edge_ids"].default is False
    assert list(inspect.signature(_lib.gather_rows_scale).parameters) == ["X", "perm", "scale", "out"]
    assert list(inspect.signature(_lib.gather_rows_scale_backward).parameters) == ["dY", "new_id", "X", "scale", "need_input", "need_scale", "out"]
    assert TOPK in _lib.segment_topk.__doc__ and FWD in _lib.gather_rows_scale.__doc__ and BWD in _lib.gather_rows_scale_backward.__doc__
    gp = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.segment_topk(torch.zeros(4), gp, ratio=0.5)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.gather_rows_scale(torch.zeros(2, 4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs need_input or need_scale"):
        _lib.gather_rows_scale_backward(torch.zeros(2, 4), torch.zeros(3, dtype=torch.int32), need_input=False, need_scale=False)
    with pytest.raises(ValueError, match="need_scale needs X"):
        _lib.gather_rows_scale_backward(torch.zeros(2, 4), torch.zeros(3, dtype=torch.int32))
    from gnnadvisor_osdi21_amd import load_extension, ops
    GNNA = load_extension()
    assert "ties to the smaller row" in GNNA.segment_topk.__doc__ and "row of zeros" in GNNA.gather_rows_scale.__doc__
    assert "unpooling" in GNNA.gather_rows_scale_backward.__doc__
    for layer in (ops.TopKPooling, ops.SAGPooling):
        params = inspect.signature(layer.__init__).parameters
        assert params["ratio"].default == 0.5 and params["k"].default is None and params["nonlinearity"].default == "tanh" and params["fused"].default is True
        with pytest.raises(ValueError, match="ratio must be in \\(0, 1\\]"):
            layer(8, ratio=0.0)
        with pytest.raises(ValueError, match="k must be >= 1"):
            layer(8, k=0)
        with pytest.raises(ValueError, match="nonlinearity must be"):
            layer(8, nonlinearity="relu")
    assert inspect.signature(ops.SAGPooling.__init__).parameters["GNN"].default is ops.GCNConv
    assert inspect.signature(ops.TopKPooling.__init__).parameters["multiplier"].default == 1.0
    pool = ops.TopKPooling(6)
    assert tuple(pool.weight.shape) == (6,) and pool.ratio == 0.5 and pool.k is None
    assert ops.TopKPooling(6, k=3).ratio is None and tuple(ops.SAGPooling(6).gnn.weights.shape) == (6, 1)
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="TopKPooling computes in float32 only"):
            pool(torch.zeros(3, 6, dtype=dtype), None)
    assert "nothing of the size of X beyond X itself" in " ".join(ops.SelectRows.__doc__.split())
    assert "timing baseline" in " ".join(ops.TopKPooling.__doc__.split())


def test_a_graph_batch_without_the_new_keywords_is_unchanged():
    from gnnadvisor_osdi21_amd.batching import GraphBatch
    params = inspect.signature(GraphBatch.__init__).parameters
    assert list(params)[-2:] == ["partPtr", "part2Node"] and params["partPtr"].default is None and params["part2Node"].default is None
    rp = torch.tensor([0, 2, 3, 3, 40], dtype=torch.int32)
    ci = torch.arange(40, dtype=torch.int32) % 4
    gp = torch.tensor([0, 3, 4], dtype=torch.int32)
    b = GraphBatch(rp, ci, gp, partSize=16)
    pp, p2n = _lib.build_part(16, rp)
    assert torch.equal(b.partPtr, pp) and torch.equal(b.part2Node, p2n) and b.num_graphs == 2 and b.num_nodes == 4
    assert b.partPtr.tolist() == [0, 2, 3, 19, 35, 40] and b.part2Node.tolist() == [0, 1, 3, 3, 3]
    given = GraphBatch(rp, ci, gp, partSize=16, partPtr=pp, part2Node=p2n)
    assert given.partPtr is pp and given.part2Node is p2n and torch.equal(given.degrees, b.degrees)
    with pytest.raises(ValueError, match="partPtr and part2Node come together"):
        GraphBatch(rp, ci, gp, partPtr=pp)
    with pytest.raises(_lib.GnnaError, match="needs a batch on the device"):
        b.coarsen(torch.zeros(4), ratio=0.5)


@pytest.mark.parametrize("value", ["max", "", "TopK", "topk,sag"])
def test_the_driver_refuses_an_unknown_pool(value):
    from gnnadvisor_osdi21_amd import graph_main as driver
    text = driver.build_parser().format_help()
    assert "--pool" in text and "none, topk or sag" in text and "--pool_ratio" in text
    args = driver.build_parser().parse_args([])
    assert args.pool == "none" and args.pool_ratio == 0.5
    with pytest.raises(SystemExit) as refusal:
        driver.main(["--pool", value])
    assert str(refusal.value) == "--pool takes none, topk or sag (got %r)" % value
    with pytest.raises(SystemExit) as refusal:
        driver.main(["--pool", "topk", "--pool_ratio", "0"])
    assert str(refusal.value) == "--pool_ratio must be in (0, 1] (got 0.0)"

"""Graph-level readout and batches of graphs, the parts that need no GPU (the binding surface of include/gnna_pool.h and the
build lists are pinned by test_binding_table_host.py): the header's constants, the refusals both entries make before any device
work, the wrappers, GraphBatch.from_graphs against a hand-written case, the seeded generator and the driver's refusals."""
import ctypes
import inspect
import os

import pytest
import torch

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD, BWD = "gnna_segment_pool_ld_f32", "gnna_segment_pool_backward_ld_f32"


def test_the_header_defines_the_constants_the_binding_restates():
    header = open(os.path.join(ROOT, "include", "gnna_pool.h")).read()
    assert f"#define GNNA_POOL_LONG_STEPS {_lib.POOL_LONG_STEPS}\n" in header
    assert f"#define GNNA_POOL_TILE_ROWS {_lib.POOL_TILE_ROWS}\n" in header and f"#define GNNA_POOL_MEAN {_lib.POOL_MEAN}u" in header


_B = [(ctypes.c_float * 64)() for _ in range(12)]
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = [ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p).value for _ in range(4)]


def _fwd(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(x=F[0], ld_in=8, n=6, gp=I[0], g=2, sum=F[1], ld_sum=8, mx=F[2], ld_max=8, amx=I[1], ld_argmax=8, mn=F[3], ld_min=8,
             amn=I[2], ld_argmin=8, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_pool_ld_f32(a["x"], a["ld_in"], a["n"], a["gp"], a["g"], a["sum"], a["ld_sum"], a["mx"], a["ld_max"],
                                                a["amx"], a["ld_argmax"], a["mn"], a["ld_min"], a["amn"], a["ld_argmin"], a["dim"],
                                                a["flags"], None)


def _bwd(**kw):
    a = dict(dsum=F[1], ld_dsum=8, dmax=F[2], ld_dmax=8, amx=I[1], ld_argmax=8, dmin=F[3], ld_dmin=8, amn=I[2], ld_argmin=8, gp=I[0],
             g=2, dx=F[4], ld_din=8, n=6, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_pool_backward_ld_f32(a["dsum"], a["ld_dsum"], a["dmax"], a["ld_dmax"], a["amx"], a["ld_argmax"],
                                                         a["dmin"], a["ld_dmin"], a["amn"], a["ld_argmin"], a["gp"], a["g"], a["dx"],
                                                         a["ld_din"], a["n"], a["dim"], a["flags"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


INVALID, UNSUPPORTED = -1, -3                                                # include/gnna.h


@pytest.mark.parametrize("call, name", [(_fwd, FWD), (_bwd, BWD)], ids=["forward", "backward"])
def test_refusals_both_entries_make_alike(call, name):
    for flags in (2, 4, 0x80000000):
        assert call(flags=flags) == INVALID
        assert _last() == f"{name}: unknown flag bits 0x{flags:x} (GNNA_POOL_MEAN is the only flag)"
    assert call(flags=3) == INVALID and _last() == f"{name}: unknown flag bits 0x2 (GNNA_POOL_MEAN is the only flag)"
    assert call(dim=0) == INVALID and _last() == f"{name}: dim must be >= 1 (got 0)"
    assert call(dim=-3) == INVALID and _last() == f"{name}: dim must be >= 1 (got -3)"
    assert call(n=-1) == INVALID and _last() == f"{name}: negative size (num_rows=-1 num_segments=2)"
    assert call(g=-2) == INVALID and _last() == f"{name}: negative size (num_rows=6 num_segments=-2)"
    assert call(g=1 << 29) == UNSUPPORTED and _last() == f"{name}: 536870912 segments in one call (at most 536870911): shard the batch"
    assert call(n=1 << 31) == UNSUPPORTED and _last() == f"{name}: 2147483648 rows in one call (at most 2147483647: graph_pointers is int32)"
    assert call(gp=I[3] + 2) == INVALID and "must be 4-byte aligned" in _last() and _last().startswith(name + ": ")
    assert call(gp=None) == INVALID and _last() == f"{name}: null graph_pointers"


def test_refusals_of_the_forward_entry():
    assert _fwd(sum=None, mx=None, amx=None, mn=None, amn=None) == INVALID
    assert _last() == FWD + ": no statistic asked for: sum, max_out and min_out are all null"
    assert _fwd(mx=None) == INVALID and _last() == FWD + ": argmax without max_out: rows come with their values"
    assert _fwd(mn=None) == INVALID and _last() == FWD + ": argmin without min_out: rows come with their values"
    for ld in ("ld_in", "ld_sum", "ld_max", "ld_argmax", "ld_min", "ld_argmin"):
        assert _fwd(**{ld: 3}) == INVALID and _last().startswith(FWD + ": row strides must be >= dim and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
        assert _fwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    # (a null output's stride strides nothing: the call gets past the stride check to the next refusal)
    assert _fwd(sum=None, ld_sum=3, x=None) == INVALID and _last() == FWD + ": null feature pointer"
    assert _fwd(mx=None, amx=None, ld_max=1, ld_argmax=2, x=None) == INVALID and _last() == FWD + ": null feature pointer"
    for name in ("x", "sum", "mx", "amx", "mn", "amn"):
        assert _fwd(**{name: F[7] + 2}) == INVALID
        assert _last() == FWD + ": feature, pointer, statistic and arg pointers must be 4-byte aligned", name
    for name in ("sum", "mx", "amx", "mn", "amn"):
        assert _fwd(**{name: F[0]}) == INVALID and _last() == FWD + ": an output must not alias an input", name
        assert _fwd(**{name: I[0]}) == INVALID and _last() == FWD + ": an output must not alias an input", name
    for a, b in (("sum", "mx"), ("sum", "mn"), ("mx", "mn"), ("amx", "amn"), ("sum", "amx"), ("mn", "amn")):
        assert _fwd(**{a: F[8], b: F[8]}) == INVALID and _last() == FWD + ": the outputs must not alias each other", (a, b)
    assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
    assert _fwd(g=0) == 0                                                     # no graph: nothing to write
    assert _fwd(g=0, gp=None, x=None) == 0


def test_refusals_of_the_backward_entry():
    assert _bwd(dsum=None, dmax=None, amx=None, dmin=None, amn=None) == INVALID
    assert _last() == BWD + ": no gradient given: d_sum, d_max and d_min are all null"
    for kw, pair in ((dict(dmax=None), "d_max and argmax"), (dict(amx=None), "d_max and argmax"), (dict(dmin=None), "d_min and argmin"),
                     (dict(amn=None), "d_min and argmin")):
        assert _bwd(**kw) == INVALID and _last() == f"{BWD}: {pair} come together", kw
    for ld in ("ld_dsum", "ld_dmax", "ld_argmax", "ld_dmin", "ld_argmin", "ld_din"):
        assert _bwd(**{ld: 3}) == INVALID and _last().startswith(BWD + ": row strides must be >= dim and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
        assert _bwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    assert _bwd(dsum=None, ld_dsum=3, dx=None) == INVALID and _last() == BWD + ": null output pointer"
    for name in ("dsum", "dmax", "amx", "dmin", "amn", "dx"):
        assert _bwd(**{name: F[7] + 2}) == INVALID and _last() == BWD + ": gradient, arg and pointer pointers must be 4-byte aligned", name
    for inp in (F[1], F[2], F[3], I[0], I[1], I[2]):
        assert _bwd(dx=inp) == INVALID and _last() == BWD + ": an output must not alias an input"
    assert _bwd(dx=None) == INVALID and _last() == BWD + ": null output pointer"
    assert _bwd(n=0) == 0                                                     # no row: nothing to write


def test_deterministic_tuning_does_not_refuse_the_entries():
    try:
        _lib.set_tuning(deterministic=1)
        # (the next refusal is met instead of GNNA_ERR_UNSUPPORTED: no device is touched here)
        assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
        assert _bwd(dx=None) == INVALID and _last() == BWD + ": null output pointer"
    finally:
        _lib.reset_tuning()


def test_the_wrappers_and_the_ops():
    sig = inspect.signature(_lib.segment_pool).parameters
    assert list(sig) == ["X", "graph_pointers", "want", "mean", "out"] and sig["want"].default == ("sum",) and sig["mean"].default is False
    sig = inspect.signature(_lib.segment_pool_backward).parameters
    assert list(sig) == ["graph_pointers", "num_rows", "d_sum", "d_max", "argmax", "d_min", "argmin", "mean", "out"]
    assert FWD in _lib.segment_pool.__doc__ and BWD in _lib.segment_pool_backward.__doc__
    gp = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.segment_pool(torch.zeros(2, 4), gp)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.segment_pool_backward(gp, 2, d_sum=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="want must name some of"):
        _lib.segment_pool(torch.zeros(2, 4), gp, want=("sumsq",))
    with pytest.raises(ValueError, match="needs d_sum, d_max or d_min"):
        _lib.segment_pool_backward(gp, 2)
    with pytest.raises(ValueError, match="d_max comes with argmax"):
        _lib.segment_pool_backward(gp, 2, d_max=torch.zeros(2, 4))
    from gnnadvisor_osdi21_amd import load_extension, ops
    GNNA = load_extension()
    assert "(sum, max, argmax, min, argmin)" in GNNA.segment_pool.__doc__ and "graph_pointers" in GNNA.segment_pool.__doc__
    assert "row of no graph" in GNNA.segment_pool_backward.__doc__
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="SegmentPool computes in float32 only: 16-bit features and torch.autocast are not supported"):
            ops.global_add_pool(torch.zeros(3, 6, dtype=dtype), gp)
        for fused in (True, False):
            with pytest.raises(TypeError, match="Readout computes in float32 only"):
                ops.Readout(("sum", "max"), fused=fused)(torch.zeros(3, 6, dtype=dtype), gp)
    with pytest.raises(TypeError, match="an unsorted `batch` vector is not supported"):
        ops.global_max_pool(torch.zeros(3, 6), torch.zeros(3, dtype=torch.int64))
    for modes in ((), ("sum", "sum"), ("median",), "avg"):
        with pytest.raises(ValueError, match="modes must name some of"):
            ops.Readout(modes)
    assert ops.Readout("mean").modes == ("mean",) and ops.Readout().fused is True
    assert "nothing of the size of X" in " ".join(ops.SegmentPool.__doc__.split())
    assert "timing baseline" in " ".join(ops.Readout.__doc__.split())


def _csr(rp, ci):
    return torch.tensor(rp, dtype=torch.int32), torch.tensor(ci, dtype=torch.int32)


def test_from_graphs_against_a_hand_written_case():
    from gnnadvisor_osdi21_amd.batching import GraphBatch, GraphDataset
    # a triangle with a tail (4 nodes), a graph without nodes, three nodes without edges, a pair
    graphs = [_csr([0, 2, 4, 7, 8], [1, 2, 0, 2, 0, 1, 3, 2]), _csr([0], []), _csr([0, 0, 0, 0], []), _csr([0, 1, 2], [1, 0])]
    b = GraphBatch.from_graphs(graphs, partSize=2)
    assert b.num_graphs == 4 and b.num_nodes == 9
    assert b.graph_pointers.dtype == torch.int32 and b.graph_pointers.tolist() == [0, 4, 4, 7, 9]
    assert b.row_pointers.dtype == torch.int32 and b.row_pointers.tolist() == [0, 2, 4, 7, 8, 8, 8, 8, 9, 10]
    assert b.column_index.dtype == torch.int32 and b.column_index.tolist() == [1, 2, 0, 2, 0, 1, 3, 2, 8, 7]
    assert b.batch.tolist() == [0, 0, 0, 0, 2, 2, 2, 3, 3]
    assert b.inv_counts.tolist() == [0.25, 1.0, pytest.approx(1 / 3), 0.5]
    assert b.degrees.tolist() == pytest.approx([2 ** 0.5, 2 ** 0.5, 3 ** 0.5, 1, 1, 1, 1, 1, 1])
    # the partition is the library's for these row pointers: groups of at most 2 edges
    pp, p2n = _lib.build_part(2, b.row_pointers)
    assert b.partPtr.tolist() == pp.tolist() == [0, 2, 4, 6, 7, 8, 9, 10] and b.part2Node.tolist() == p2n.tolist() == [0, 1, 2, 2, 3, 7, 8]
    assert (b.partSize, b.directed) == (2, False) and b.set_input() is b and b.set_hidden() is b
    for name in ("row_pointers", "column_index", "degrees", "partPtr", "part2Node", "partSize", "dimWorker", "warpPerBlock", "directed",
                 "transposed", "graph_pointers", "num_graphs"):
        assert hasattr(b, name), name
    assert GraphBatch.from_graphs([]).graph_pointers.tolist() == [0]
    d = GraphDataset.from_graphs(graphs)
    assert d.column_index.tolist() == [1, 2, 0, 2, 0, 1, 3, 2, 1, 0] and d.graph_pointers.tolist() == [0, 4, 4, 7, 9] and len(d) == 4
    for bad, message in ((_csr([0, 2, 1, 3], [0, 1, 2]), "graph 1: row_pointers must start at 0, ascend and end at the number of edges"),
                         (_csr([1, 2], [0, 0]), "graph 1: row_pointers must start at 0"), (_csr([0, 1], [1]), "graph 1: a column id lies outside its 1 nodes")):
        with pytest.raises(ValueError, match=message):
            GraphBatch.from_graphs([graphs[0], bad])
    with pytest.raises(TypeError, match="graph_pointers must be a 1-D int32 tensor"):
        GraphBatch(b.row_pointers, b.column_index, b.graph_pointers.long())


def test_small_graphs_is_seeded_and_symmetric_inside_each_graph():
    from gnnadvisor_osdi21_amd.graph import small_graphs
    a, b, c = small_graphs(40, 1, 30, 3.0, seed=11), small_graphs(40, 1, 30, 3.0, seed=11), small_graphs(40, 1, 30, 3.0, seed=12)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert not torch.equal(a[2], c[2])
    rp, ci, gp = (t.long() for t in a)
    assert a[0].dtype == a[1].dtype == a[2].dtype == torch.int32
    sizes = gp[1:] - gp[:-1]
    assert gp[0] == 0 and sizes.min() >= 1 and sizes.max() <= 30 and rp.numel() == gp[-1] + 1 and rp[-1] == ci.numel()
    assert bool((rp[1:] >= rp[:-1]).all())
    rows = torch.repeat_interleave(torch.arange(int(gp[-1])), rp[1:] - rp[:-1])
    graph_of = torch.repeat_interleave(torch.arange(40), sizes)
    assert bool((ci >= 0).all()) and bool((ci < sizes[graph_of[rows]]).all())            # ids are local to their graph
    cols = ci + gp[graph_of[rows]]
    edges, back = set(zip(rows.tolist(), cols.tolist())), set(zip(cols.tolist(), rows.tolist()))
    assert edges == back and len(edges) == ci.numel()                                     # symmetric, no duplicate
    assert small_graphs(0, 1, 5)[2].tolist() == [0]
    with pytest.raises(ValueError, match="small_graphs: need"):
        small_graphs(3, 5, 4)


@pytest.mark.parametrize("extra, message", [
    (["--model", "gat"], "--model gat: graph_main trains gcn or gin"),
    (["--model", "sage"], "--model sage: graph_main trains gcn or gin"),
    (["--dtype", "bfloat16"], "--dtype bfloat16: the readout .* is float32 only; run graph_main with --dtype float32"),
    (["--readout", "sum,median"], "--readout takes a comma list of sum, mean, max, min, each once \\(got 'sum,median'\\)"),
    (["--readout", "max,max"], "each once"),
    (["--readout", ""], "--readout takes a comma list"),
    (["--graph_nodes", "12"], "--graph_nodes takes MIN,MAX, e.g. 8,72 \\(got '12'\\)"),
    (["--graph_nodes", "9,3"], "--graph_nodes needs 1 <= MIN <= MAX"),
    (["--graph_nodes", "0,3"], "--graph_nodes needs 1 <= MIN <= MAX"),
    (["--num_graphs", "0"], "--num_graphs must be >= 1"),
    (["--batch_graphs", "0"], "--batch_graphs must be >= 1"),
    (["--num_layers", "1"], "--num_layers must be >= 2 \\(got 1\\)"),
    (["--num_epoches", "0"], "--num_epoches must be >= 1"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import graph_main as driver
    text = driver.build_parser().format_help()
    for flag in ("--model", "--num_graphs", "--graph_nodes", "--batch_graphs", "--readout", "--hidden", "--classes", "--num_epoches"):
        assert flag in text
    with pytest.raises(SystemExit, match=message):
        driver.main(extra)
    with pytest.raises(SystemExit):
        driver.main(["--fused_readout", "maybe"])

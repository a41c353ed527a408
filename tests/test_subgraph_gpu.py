"""gnna_induced_subgraph_i32 on the GPU, exact against the numpy restatement of the subgraph rule (tests/walk_ref.py), and the
agreement of the ctypes binding and the GNNAdvisor module for both entries of include/gnna_walk.h."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import walk_ref as ref
from gnnadvisor_osdi21_amd import _lib, load_extension

pytestmark = pytest.mark.gpu

SENTINEL = -77
LISTS = ["empty", "hub", "64", "65", "1000", "all", "walk"]


@functools.lru_cache(maxsize=None)
def device_graph():
    rp, ci = ref.shared_graph()
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


@functools.lru_cache(maxsize=None)
def id_list(name):
    if name == "walk":                                         # the flattened output of a walk: repeats, and -1 rows of bad roots
        rp, ci = ref.shared_graph()
        return ref.random_walks(rp, ci, ref.root_sets()[1000], 4, 2024)[0].reshape(-1).astype(np.int32)
    return ref.id_lists()[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    rp, ci = ref.shared_graph()
    return ref.induced_subgraph(rp, ci, id_list(name))


def run(name, partSize=None, **kw):
    rp, ci = device_graph()
    return _lib.induced_subgraph(rp, ci, torch.from_numpy(id_list(name)).cuda(), partSize=partSize, **kw)


def same(got, want):
    got = got.cpu().numpy().astype(np.int64)
    return got.shape == want.shape and (got == want).all()


def check(got, want, partSize=None, edge_ids=True, new_id=True):
    assert got["num_nodes"] == len(want["nodes"])
    assert same(got["nodes"], want["nodes"])
    assert same(got["row_pointers"], want["row_pointers"])
    assert same(got["column_index"], want["column_index"])
    assert (same(got["edge_ids"], want["edge_ids"])) if edge_ids else got["edge_ids"] is None
    assert (same(got["new_id"], want["new_id"])) if new_id else got["new_id"] is None
    if partSize is None:
        assert got["partPtr"] is None and got["part2Node"] is None
    else:
        pp, p2n = ref.host_build_part(partSize, want["row_pointers"])
        assert same(got["partPtr"], pp) and same(got["part2Node"], p2n)


@pytest.mark.parametrize("partSize", [1, 32])
@pytest.mark.parametrize("name", LISTS)
def test_subgraph_equals_the_restatement(name, partSize):
    check(run(name, partSize, want_new_id=True), expected(name), partSize)


@pytest.mark.parametrize("name", ["hub", "65", "1000"])
def test_the_optional_outputs_are_optional(name):
    want = expected(name)
    check(run(name, None, want_edge_ids=False), want, None, edge_ids=False, new_id=False)
    check(run(name, 32, want_edge_ids=False, want_new_id=True), want, 32, edge_ids=False)
    check(run(name, None, want_edge_ids=True), want, None, new_id=False)


def test_the_hub_alone_keeps_its_self_loops_and_duplicates():
    got, (rp, ci) = run("hub"), ref.shared_graph()
    loops = np.flatnonzero(ci[rp[10]:rp[11]] == 10) + rp[10]
    assert len(loops) >= 1 and got["row_pointers"].tolist() == [0, len(loops)]
    assert got["column_index"].tolist() == [0] * len(loops) and same(got["edge_ids"], loops)


def test_every_id_gives_the_graph_itself():
    got, (rp, ci) = run("all", 32, want_new_id=True), device_graph()
    assert torch.equal(got["row_pointers"], rp) and torch.equal(got["column_index"], ci)
    assert torch.equal(got["edge_ids"], torch.arange(ci.numel(), dtype=torch.int32, device="cuda"))
    assert torch.equal(got["nodes"], torch.arange(ref.N, dtype=torch.int32, device="cuda")) and torch.equal(got["new_id"], got["nodes"])
    pp, p2n = _lib.build_part(32, rp.cpu())
    assert torch.equal(got["partPtr"].cpu(), pp.int()) and torch.equal(got["part2Node"].cpu(), p2n.int())


def test_column_ids_outside_the_graph_are_dropped():
    rp, ci = ref.dead_end_graph()
    want = ref.induced_subgraph(rp, ci, id_list("1000"), partSize=32)
    got = _lib.induced_subgraph(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(id_list("1000")).cuda(),
                                partSize=32, want_new_id=True)
    check(got, want, 32)
    assert len(want["edge_ids"]) < len(expected("1000")["edge_ids"])


@pytest.mark.parametrize("bad", [ref.N, -2])
def test_an_id_outside_the_graph_names_its_index_and_the_next_call_succeeds(bad):
    rp, ci = device_graph()
    ids = torch.tensor([5, -1, 7, bad, 9], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.GnnaError, match=r"nodes\[3\] is outside \[0, num_nodes = 3000\)"):
        _lib.induced_subgraph(rp, ci, ids, partSize=32)
    check(run("65", 32, want_new_id=True), expected("65"), 32)


def _raw_call(name, node_cap, edge_cap, slack=8):
    """The C entry on buffers with `slack` sentinel words behind every capacity -> (rc, counts, buffers)."""
    rp, ci = device_graph()
    ids = torch.from_numpy(id_list(name)).cuda()
    full = lambda n: torch.full((n + slack,), SENTINEL, dtype=torch.int32, device="cuda")            # noqa: E731
    buf = {"nodes": full(node_cap), "row_pointers": full(node_cap + 1), "column_index": full(edge_cap), "edge_ids": full(edge_cap),
           "partPtr": full(edge_cap + 1), "part2Node": full(edge_cap)}
    counts = (ctypes.c_int64 * 3)()
    rc = _lib.load().gnna_induced_subgraph_i32(rp.data_ptr(), ci.data_ptr(), ref.N, ci.numel(), ids.data_ptr(), ids.numel(), 32,
                                               buf["nodes"].data_ptr(), None, buf["row_pointers"].data_ptr(),
                                               buf["column_index"].data_ptr(), buf["edge_ids"].data_ptr(), buf["partPtr"].data_ptr(),
                                               buf["part2Node"].data_ptr(), node_cap, edge_cap, counts,
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, tuple(int(c) for c in counts), buf


def _sizes(name):
    want = expected(name)
    return len(want["nodes"]), len(want["edge_ids"]), len(ref.host_build_part(32, want["row_pointers"])[1])


def test_exact_capacities_are_enough_and_nothing_is_written_behind_them():
    n, e, parts = _sizes("1000")
    rc, counts, buf = _raw_call("1000", n, e)
    assert rc == 0 and counts == (n, e, parts)
    want = expected("1000")
    lengths = {"nodes": n, "row_pointers": n + 1, "column_index": e, "edge_ids": e, "partPtr": parts + 1, "part2Node": parts}
    for key, length in lengths.items():
        assert bool((buf[key][length:] == SENTINEL).all()), key
    assert same(buf["column_index"][:e], want["column_index"]) and same(buf["row_pointers"][:n + 1], want["row_pointers"])


@pytest.mark.parametrize("short", ["edges", "nodes"])
def test_a_capacity_one_short_reports_the_needed_sizes_and_writes_nothing_beyond(short):
    n, e, parts = _sizes("1000")
    node_cap, edge_cap = (n, e - 1) if short == "edges" else (n - 1, e)
    rc, counts, buf = _raw_call("1000", node_cap, edge_cap)
    assert rc == -1 and "capacity too small" in _lib.load().gnna_last_error().decode()               # GNNA_ERR_INVALID_ARGUMENT
    assert counts == (n, e, parts)
    capacity = {"nodes": node_cap, "row_pointers": node_cap + 1, "column_index": edge_cap, "edge_ids": edge_cap,
                "partPtr": edge_cap + 1, "part2Node": edge_cap}
    for key, length in capacity.items():
        assert bool((buf[key][length:] == SENTINEL).all()), key
    with pytest.raises(_lib.GnnaError, match="capacity too small") as info:
        run("1000", 32, **({"edge_capacity": e - 1} if short == "edges" else {"node_capacity": n - 1}))
    assert info.value.counts == (n, e, parts)
    check(run("1000", 32, want_new_id=True), expected("1000"), 32)                                   # the next call succeeds


def test_decreasing_row_pointers_on_a_kept_row_make_it_empty():
    rp, ci = ref.shared_graph()
    rp = rp.copy()
    rp[8] = rp[9] + 5                      # row 8 = [rp[9] + 5, rp[9]): decreasing; row 7 grows over it and stays valid
    rp[3000] = len(ci) + 1                 # the last row leaves [0, nnz]
    ids = np.concatenate([np.arange(12), [2999, 2999, 40]]).astype(np.int32)
    want = ref.induced_subgraph(rp, ci, ids, partSize=1)
    assert np.diff(want["row_pointers"])[8] == 0 and np.diff(want["row_pointers"])[-1] == 0
    got = _lib.induced_subgraph(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(ids).cuda(), partSize=1,
                                want_new_id=True)
    check(got, want, 1)


def test_refused_inside_a_stream_capture():
    rp, ci = device_graph()
    ids = torch.from_numpy(id_list("64")).cuda()
    _lib.induced_subgraph(rp, ci, ids)                       # (scratch exists: the capture below has nothing to allocate)
    sub_rp = torch.empty(65, dtype=torch.int32, device="cuda")
    counts = (ctypes.c_int64 * 3)()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = None
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lib = _lib.load()
            rc = lib.gnna_induced_subgraph_i32(rp.data_ptr(), ci.data_ptr(), ref.N, ci.numel(), ids.data_ptr(), 64, 0, None, None,
                                               sub_rp.data_ptr(), None, None, None, None, 0, 0, counts, side.cuda_stream)
            sub_rp.add_(0)                                   # (a capture must record something)
    assert rc == -3 and "stream capture" in lib.gnna_last_error().decode()      # GNNA_ERR_UNSUPPORTED


def test_two_calls_give_equal_bits():
    a, b = run("walk", 32, want_new_id=True), run("walk", 32, want_new_id=True)
    for key in ("row_pointers", "column_index", "edge_ids", "nodes", "new_id", "partPtr", "part2Node"):
        assert torch.equal(a[key], b[key]), key


# ---- the two bindings ----

def test_the_bindings_agree_on_the_walks():
    GNNA = load_extension()
    rp, ci = device_graph()
    roots = torch.from_numpy(ref.root_sets()[1000]).cuda()
    for rng_seed in (2024, (1 << 64) - 3):
        a = _lib.random_walk(rp, ci, roots, 4, rng_seed, want_edge_ids=True)
        b = GNNA.random_walk(rp, ci, roots, 4, rng_seed, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert GNNA.random_walk(rp, ci, roots, 4, 1)[1] is None


@pytest.mark.parametrize("name", ["empty", "1000", "walk"])
def test_the_bindings_agree_on_the_subgraph(name):
    GNNA = load_extension()
    rp, ci = device_graph()
    ids = torch.from_numpy(id_list(name)).cuda()
    a = _lib.induced_subgraph(rp, ci, ids, partSize=32, want_new_id=True)
    b = GNNA.induced_subgraph(rp, ci, ids, 32, True, True)
    for key, other in zip(("row_pointers", "column_index", "edge_ids", "nodes", "new_id", "partPtr", "part2Node"), b):
        assert torch.equal(a[key], other), key
    c = GNNA.induced_subgraph(rp, ci, ids)
    assert c[4] is None and c[5] is None and c[6] is None and torch.equal(c[2], a["edge_ids"])

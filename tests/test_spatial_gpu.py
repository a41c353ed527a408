"""gnna_radius_graph_f32 on the GPU, exact against the numpy restatement of the rule (tests/spatial_ref.py): every array is compared
with ==.  Shapes: the segment sizes around the lane groups (4 .. 64), around the longest segment the lanes-per-row kernel takes
(_lib.SPATIAL_LONG_ROWS) and around a whole number of staged source tiles (_lib.SPATIAL_SOURCE_TILE // dim rows), shuffled so that
segments straddle the 256-row tiles; the widths on both sides of _lib.SPATIAL_REGISTER_DIM and the widest one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import spatial_ref as ref
from gnnadvisor_osdi21_amd import _lib, load_extension

pytestmark = pytest.mark.gpu

T = _lib.SPATIAL_LONG_ROWS
SENTINEL = -77
SIZES = sorted({0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1})


def tile_rows(dim):
    return min(256, _lib.SPATIAL_SOURCE_TILE // dim)


@functools.lru_cache(maxsize=None)
def size_batch(dim=3, seed=0, extra=()):
    rng = np.random.default_rng(100 + seed)
    sizes = rng.permutation(np.array(SIZES + list(extra)))
    return ref.random_batch(sizes, dim, seed=seed, specials=False)


@functools.lru_cache(maxsize=None)
def expected(case, radius, cap, loop, partSize=None):
    pos, gp = CASES[case]()
    return ref.radius_graph(pos, gp, radius, max_neighbors=cap, loop=loop, partSize=partSize)


CASES = {
    "sizes": size_batch,
    "lattice": ref.lattice,
    "small": lambda: ref.random_batch([1, 2, 3, 5, 0, 4, 9, 6, 2, 7, 3, 8, 1, 5, 4, 6], 3, seed=11),        # 4 lanes per row, two rounds
    "coincident": lambda: (np.ones((T + 5 + 70 + 3, 2), np.float32), ref.pointers_of([T + 5, 70, 3])),
}


def run(case, radius, cap=None, loop=False, partSize=None, **kw):
    pos, gp = CASES[case]()
    return _lib.radius_graph(torch.from_numpy(pos).cuda(), torch.from_numpy(gp).cuda(), radius, cap, loop, partSize=partSize, **kw)


def same(t, a):
    return t.dtype in (torch.int32, torch.float32) and np.array_equal(t.cpu().numpy().view(np.int32), np.asarray(a).astype(t.cpu().numpy().dtype).view(np.int32))


def check(got, want, partSize=None):
    assert same(got["row_pointers"], want["row_pointers"])
    assert same(got["column_index"], want["column_index"])
    assert same(got["dist2"], want["dist2"])                             # the bits
    assert got["num_edges"] == len(want["column_index"])
    if partSize is not None:
        assert same(got["partPtr"], want["partPtr"]) and same(got["part2Node"], want["part2Node"])


# ---- segment sizes, the lattice ----

@pytest.mark.parametrize("loop", [False, True])
def test_every_segment_size_in_one_batch(loop):
    check(run("sizes", 1.0, loop=loop, partSize=32), expected("sizes", 1.0, None, loop, 32), 32)
    got = run("sizes", 1.0, loop=loop)
    edges = ref.edge_set({k: v.cpu().numpy() for k, v in got.items() if k in ("row_pointers", "column_index")})
    assert all((j, i) in edges for i, j in edges)                        # without a cap the structure is symmetric


@pytest.mark.parametrize("radius", list(ref.LATTICE_RADII))
@pytest.mark.parametrize("loop", [False, True])
def test_the_lattice(radius, loop):
    check(run("lattice", radius, loop=loop), expected("lattice", radius, None, loop))


@pytest.mark.parametrize("cap", [1, 4, 64])
def test_the_lattice_under_a_cap(cap):
    check(run("lattice", 2.0, cap), expected("lattice", 2.0, cap, False))
    check(run("lattice", np.inf, cap, True), expected("lattice", np.inf, cap, True))


def test_few_lanes_per_row():
    for radius, cap in ((1.0, None), (np.inf, None), (np.inf, 2), (1.5, 1)):
        check(run("small", radius, cap, partSize=3), expected("small", radius, cap, False, 3), 3)


# ---- random floats: widths, a column slice, special values ----

@pytest.mark.parametrize("dim", [1, 2, 3, _lib.SPATIAL_REGISTER_DIM, _lib.SPATIAL_REGISTER_DIM + 1, 7, _lib.SPATIAL_MAX_DIM])
def test_random_floats_at_every_width(dim):
    t = tile_rows(dim)
    sizes = [40, 7, T + 1, 0, 2 * t - 1, 64, 2 * t + 1, 13, 2 * t]
    pos, gp = ref.random_batch(sizes, dim, seed=dim)                  # rows 3, 5, 7 hold NaN, +inf, 1e30; rows 8 and 9 coincide
    radius = float(np.sqrt(dim) * 0.6)
    for r, cap, loop in ((radius, None, False), (np.inf, 16, True)):
        want = ref.radius_graph(pos, gp, r, max_neighbors=cap, loop=loop)
        check(_lib.radius_graph(torch.from_numpy(pos).cuda(), torch.from_numpy(gp).cuda(), r, cap, loop), want)
    # the same as a column slice (ld_pos > dim)
    wide = torch.full((len(pos), dim + 3), float("nan"), device="cuda")
    wide[:, 2:2 + dim] = torch.from_numpy(pos).cuda()
    check(_lib.radius_graph(wide[:, 2:2 + dim], torch.from_numpy(gp).cuda(), radius), ref.radius_graph(pos, gp, radius))


def test_special_values_at_an_infinite_radius():
    pos, gp = ref.random_batch([12, 8, T + 9], 3, seed=3)
    pos[25, :] = 1e30                                                  # in the long segment as well
    pos[26, 1] = np.nan
    pos[27, 2] = np.inf
    for loop in (False, True):
        want = ref.radius_graph(pos, gp, np.inf, loop=loop)
        got = _lib.radius_graph(torch.from_numpy(pos).cuda(), torch.from_numpy(gp).cuda(), np.inf, None, loop)
        check(got, want)
    edges = ref.edge_set(want)
    assert (7, 7) in edges and (7, 0) in edges and (5, 5) not in edges and not any(3 in e for e in edges)
    assert np.isinf(want["dist2"][want["row_pointers"][7]])            # 1e30: d2 overflows to +inf, and radius = inf keeps it


# ---- caps ----

@pytest.mark.parametrize("cap", [1, 2, 32, 64])
@pytest.mark.parametrize("radius", [1.0, np.inf])
def test_caps_over_segments_smaller_equal_and_larger(cap, radius):
    sizes = (cap - 1, cap, cap + 1, cap + 2, 3 * cap + 1)
    case = "caps%d" % cap
    CASES.setdefault(case, lambda: size_batch(3, cap, sizes))
    check(run(case, radius, cap, partSize=32), expected(case, radius, cap, False, 32), 32)
    check(run(case, radius, cap, True), expected(case, radius, cap, True))


@pytest.mark.parametrize("cap", [1, 32, 64])
def test_coincident_points_leave_the_cap_to_the_row_ids(cap):
    check(run("coincident", 0.0, cap), expected("coincident", 0.0, cap, False))
    check(run("coincident", np.inf, cap, True), expected("coincident", np.inf, cap, True))


# ---- pointers ----

def _call(pos, gp, radius, **kw):
    return _lib.radius_graph(torch.from_numpy(pos).cuda(), torch.tensor(gp, dtype=torch.int32, device="cuda"), radius, **kw)


def test_pointers_outside_the_batch_and_rows_outside_every_segment():
    pos, _ = ref.random_batch([700], 3, seed=8)
    for gp in ([-5, 4, 4, 10, 99999], [2, 6], [30, 30 + T + 2, 650], [0, 0], [700, 700], [5]):
        check(_call(pos, gp, 1.0, partSize=32), ref.radius_graph(pos, gp, 1.0, partSize=32), 32)


def test_an_empty_batch():
    empty = np.zeros((0, 3), np.float32)
    for gp in ([0], [0, 0, 0], [3, 9]):
        got = _call(empty, gp, 1.0, partSize=32)
        assert got["row_pointers"].tolist() == [0] and got["num_edges"] == 0 and got["partPtr"].tolist() == [0]
        assert got["column_index"].numel() == got["dist2"].numel() == got["part2Node"].numel() == 0


def test_decreasing_pointers_name_the_first_segment_and_the_next_call_succeeds():
    pos, _ = ref.random_batch([700], 3, seed=8)
    with pytest.raises(_lib.GnnaError, match="graph_pointers decreases at segment 2 "):
        _call(pos, [0, 9, 400, 4, 650, 20, 700], 1.0, partSize=32)
    with pytest.raises(_lib.GnnaError, match="graph_pointers decreases at segment 0 "):
        _call(pos, [9999, 0], 1.0)
    check(_call(pos, [0, 9, 400, 700], 1.0), ref.radius_graph(pos, [0, 9, 400, 700], 1.0))


# ---- capacity ----

def _raw_call(case, radius, edge_cap, slack=8, partSize=32):
    pos, gp = CASES[case]()
    pos, gp = torch.from_numpy(pos).cuda(), torch.from_numpy(gp).cuda()
    full = lambda n, dtype=torch.int32: torch.full((n + slack,), SENTINEL, dtype=dtype, device="cuda")            # noqa: E731
    buf = {"row_pointers": full(len(pos) + 1), "column_index": full(edge_cap), "dist2": full(edge_cap, torch.float32),
           "partPtr": full(edge_cap + 1), "part2Node": full(edge_cap)}
    counts = (ctypes.c_int64 * 3)()
    rc = _lib.load().gnna_radius_graph_f32(pos.data_ptr(), pos.stride(0), len(pos), pos.shape[1], gp.data_ptr(), gp.numel() - 1, radius,
                                           0, 0, partSize, *(buf[k].data_ptr() for k in buf), edge_cap, counts,
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, tuple(int(c) for c in counts), buf


def test_a_capacity_one_short_reports_the_needed_sizes_and_writes_only_the_row_pointers():
    want = expected("sizes", 1.0, None, False, 32)
    n, e, parts = len(want["row_pointers"]) - 1, len(want["column_index"]), len(want["part2Node"])
    rc, counts, buf = _raw_call("sizes", 1.0, e - 1)
    assert rc == -1 and "capacity too small" in _lib.load().gnna_last_error().decode()               # GNNA_ERR_INVALID_ARGUMENT
    assert counts == (n, e, parts)
    assert same(buf["row_pointers"][:n + 1], want["row_pointers"]) and bool((buf["row_pointers"][n + 1:] == SENTINEL).all())
    for key in ("column_index", "dist2", "partPtr", "part2Node"):
        assert bool((buf[key] == SENTINEL).all()), key
    with pytest.raises(_lib.GnnaError, match="capacity too small") as info:
        run("sizes", 1.0, partSize=32, edge_capacity=e - 1)
    assert info.value.counts == (n, e, parts)
    check(run("sizes", 1.0, partSize=32), want, 32)                                                  # the next call succeeds


def test_an_exact_capacity_is_enough_and_nothing_is_written_behind_it():
    want = expected("sizes", 1.0, None, False, 32)
    n, e, parts = len(want["row_pointers"]) - 1, len(want["column_index"]), len(want["part2Node"])
    rc, counts, buf = _raw_call("sizes", 1.0, e)
    assert rc == 0 and counts == (n, e, parts)
    lengths = {"row_pointers": n + 1, "column_index": e, "dist2": e, "partPtr": parts + 1, "part2Node": parts}
    for key, length in lengths.items():
        assert bool((buf[key][length:] == SENTINEL).all()), key
        assert same(buf[key][:length], want[key]), key


def test_the_default_capacity_is_retried_once_at_the_reported_size(monkeypatch):
    monkeypatch.setattr(_lib, "SPATIAL_DEFAULT_EDGES", 16)
    pos = np.zeros((600, 1), np.float32)                               # 600 coincident points: 359,400 edges > 64 * 600
    got = _call(pos, [0, 600], 0.0)
    assert got["num_edges"] == 600 * 599 and got["row_pointers"][-1].item() == 600 * 599


def test_more_than_2_31_edges_are_unsupported_and_counted_in_64_bits():
    n = 46400
    pos = torch.rand((n, 3), device="cuda")
    gp = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.GnnaError, match=r"libgnna error -3: gnna_radius_graph_f32: the graph has 2152960000 edges") as info:
        _lib.radius_graph(pos, gp, np.inf, None, True, edge_capacity=0)                              # (the count pass alone)
    assert info.value.counts[1] == n * n >= 2 ** 31


# ---- the partition, determinism, capture, the bindings ----

@pytest.mark.parametrize("partSize", [1, 3, 32])
def test_the_partition_is_build_part_of_the_row_pointers(partSize):
    for cap in (None, 5):
        got = run("sizes", 1.0, cap, partSize=partSize)
        pp, p2n = _lib.build_part_device(partSize, got["row_pointers"])
        assert torch.equal(got["partPtr"], pp) and torch.equal(got["part2Node"], p2n)
        check(got, expected("sizes", 1.0, cap, False, partSize), partSize)


def test_two_calls_give_equal_bits_and_the_deterministic_mode_accepts_the_call():
    a = run("sizes", 1.0, 7, True, partSize=32)
    _lib.set_tuning(deterministic=1)
    try:
        b = run("sizes", 1.0, 7, True, partSize=32)
    finally:
        _lib.reset_tuning()
    for key in ("row_pointers", "column_index", "dist2", "partPtr", "part2Node"):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key


def test_refused_inside_a_stream_capture():
    pos, gp = (torch.from_numpy(a).cuda() for a in ref.lattice())
    _lib.radius_graph(pos, gp, 1.0)                            # (scratch exists: the capture below has nothing to allocate)
    rp = torch.empty(len(pos) + 1, dtype=torch.int32, device="cuda")
    counts = (ctypes.c_int64 * 3)()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = None
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lib = _lib.load()
            rc = lib.gnna_radius_graph_f32(pos.data_ptr(), 3, len(pos), 3, gp.data_ptr(), gp.numel() - 1, 1.0, 0, 0, 0, rp.data_ptr(),
                                           None, None, None, None, 0, counts, side.cuda_stream)
            rp.add_(0)                                         # (a capture must record something)
    assert rc == -3 and "stream capture" in lib.gnna_last_error().decode()      # GNNA_ERR_UNSUPPORTED


@pytest.mark.parametrize("cap, loop", [(None, False), (5, True)])
def test_the_bindings_agree(cap, loop):
    GNNA = load_extension()
    pos, gp = (torch.from_numpy(a).cuda() for a in size_batch())
    a = _lib.radius_graph(pos, gp, 1.0, cap, loop, partSize=32)
    b = GNNA.radius_graph(pos, gp, 1.0, cap or 0, loop, 32, True)
    for key, other in zip(("row_pointers", "column_index", "dist2", "partPtr", "part2Node"), b):
        assert torch.equal(a[key].view(torch.int32), other.view(torch.int32)), key
    c = GNNA.radius_graph(pos, gp, 1.0, cap or 0, loop, 0, False)
    assert c[2] is None and c[3] is None and c[4] is None and torch.equal(c[1], a["column_index"])

"""gnna_segment_topk_i32 on the GPU, through the C ABI with sentinel-filled buffers, through _lib and through GNNA, against
tests/topk_ref.py.  Every array is compared exactly: the selection is a rule on bit patterns, not arithmetic.

Shapes: the segment sizes around the wavefront (64) and around the longest segment one wavefront selects (_lib.TOPK_WAVE_ROWS),
one segment of 5,000 and three of about 3,000 rows for the workgroup path and a scan over more than one 4,096-element tile, and the
inputs that break the contract of graph_pointers or column_index."""
import ctypes

import numpy as np
import pytest
import torch

import topk_ref
from gnnadvisor_osdi21_amd import _lib, load_extension

pytestmark = pytest.mark.gpu

W = _lib.TOPK_WAVE_ROWS
SENTINEL = -7777
SLACK = 8                                  # entries behind every capacity that must keep the sentinel
MIXED = [0, 1, 2, 63, 64, 65, W - 1, W, W + 1, 0, 1000, 3]
HOW = [dict(ratio=0.01), dict(ratio=0.5), dict(ratio=0.8), dict(ratio=1.0), dict(k=1), dict(k=5), dict(k=300)]
HOW_IDS = ["ratio0.01", "ratio0.5", "ratio0.8", "ratio1.0", "k1", "k5", "k300"]


def _nan(sign):
    return np.array([0x7FC00000 | (sign << 31)], dtype=np.uint32).view(np.float32)[0]


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, _nan(0), _nan(1), 1e-45, -1e-45, 1e-39, 1.0, -1.0, 0.0, -0.0, _nan(0), np.inf],
                    dtype=np.float32)


def pointers(sizes, first=0):
    return [first] + [int(v) for v in first + np.cumsum(sizes)]


def block_graph(gp, n, degree, seed, symmetric=True):
    """(row_pointers, column_index) of a random graph whose edges stay inside the segments of gp; ids ascend inside a row."""
    rng = np.random.default_rng(seed)
    pairs = set()
    for a, b in topk_ref.segments(gp, n):
        if b - a < 2:
            continue
        m = max(1, (b - a) * degree // (2 if symmetric else 1))
        src, dst = rng.integers(a, b, size=m), rng.integers(a, b, size=m)
        for s, d in zip(src.tolist(), dst.tolist()):
            if s != d:
                pairs.add((s, d))
                if symmetric:
                    pairs.add((d, s))
    edges = sorted(pairs)
    rows = np.array([e[0] for e in edges], dtype=np.int64)
    rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return rp, np.array([e[1] for e in edges], dtype=np.int32)


def _buf(n):
    return torch.full((n + SLACK,), SENTINEL, dtype=torch.int32, device="cuda")


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def run(score, gp, ratio=None, k=None, rp=None, ci=None, partSize=None, row_cap=None, edge_cap=None, part_cap=None, stream=None):
    """One call of the C entry with sentinel-filled outputs -> (rc, counts, dict of the trimmed numpy arrays, dict of the raw
    buffers).  Checks that nothing behind a capacity was written."""
    n, G = len(score), len(gp) - 1
    csr, parts = rp is not None, partSize is not None
    nnz = len(ci) if csr else 0
    row_cap = n if row_cap is None else row_cap
    edge_cap = nnz if edge_cap is None else edge_cap
    part_cap = (nnz if part_cap is None else part_cap) if parts else 0
    sd, gpd = _dev(score, torch.float32), _dev(gp, torch.int32)
    rpd, cid = (_dev(rp, torch.int32), _dev(ci, torch.int32)) if csr else (None, None)
    b = dict(new_id=_buf(n), perm=_buf(row_cap), graph_pointers=_buf(G + 1))
    if csr:
        b.update(row_pointers=_buf(row_cap + 1), column_index=_buf(edge_cap), edge_ids=_buf(edge_cap))
    if parts:
        b.update(partPtr=_buf(part_cap + 1), part2Node=_buf(part_cap))
    ptr = lambda name: b[name].data_ptr() if name in b else None                                      # noqa: E731
    counts = (ctypes.c_int64 * 3)()
    torch.cuda.synchronize()
    rc = _lib.load().gnna_segment_topk_i32(sd.data_ptr(), n, gpd.data_ptr(), G, 0.0 if ratio is None else ratio, 0 if k is None else k,
                                           rpd.data_ptr() if csr else None, cid.data_ptr() if csr else None, nnz, partSize if parts else 0,
                                           ptr("new_id"), ptr("perm"), ptr("graph_pointers"), ptr("row_pointers"), ptr("column_index"),
                                           ptr("edge_ids"), ptr("partPtr"), ptr("part2Node"), row_cap, edge_cap, part_cap, counts,
                                           torch.cuda.current_stream().cuda_stream if stream is None else stream)
    torch.cuda.synchronize()
    counts = tuple(int(c) for c in counts)
    caps = dict(new_id=n, perm=row_cap, graph_pointers=G + 1, row_pointers=row_cap + 1, column_index=edge_cap, edge_ids=edge_cap,
                partPtr=part_cap + 1, part2Node=part_cap)
    for name, t in b.items():
        assert bool((t[caps[name]:] == SENTINEL).all()), f"{name}: written behind its capacity"
    used = dict(new_id=n, perm=counts[0], graph_pointers=G + 1, row_pointers=counts[0] + 1, column_index=counts[1], edge_ids=counts[1],
                partPtr=counts[2] + 1, part2Node=counts[2])
    out = {}
    if rc == 0:
        for name, t in b.items():
            assert bool((t[used[name]: caps[name]] == SENTINEL).all()), f"{name}: written behind its count"
            out[name] = t[:used[name]].cpu().numpy()
    return rc, counts, out, b


def check(score, gp, how, rp=None, ci=None, partSize=None):
    """The call against the reference, array by array; -> the call's arrays."""
    ref = topk_ref.segment_topk(score, gp, row_pointers=rp, column_index=ci, partSize=partSize, **how)
    rc, counts, got, _ = run(score, gp, rp=rp, ci=ci, partSize=partSize, **how)
    assert rc == 0, _lib.load().gnna_last_error().decode()
    assert counts == (len(ref["perm"]), len(ref.get("column_index", ())), len(ref.get("part2Node", ())))
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], ref[name]), name
    return got


def tied_scores(n, seed):
    """Normal scores rounded to one decimal: ties inside every larger segment."""
    return np.round(np.random.default_rng(seed).standard_normal(n), 1).astype(np.float32)


@pytest.mark.parametrize("how", HOW, ids=HOW_IDS)
def test_segments_around_the_wavefront_and_the_workgroup(how):
    gp = pointers(MIXED)
    n = gp[-1]
    rp, ci = block_graph(gp, n, 4, seed=1)
    got = check(tied_scores(n, 2), gp, how, rp, ci, partSize=3)
    sizes = np.diff(got["graph_pointers"])
    assert sizes.tolist() == [topk_ref.keep_count(s, **how) for s in MIXED]


@pytest.mark.parametrize("values", [3, 1], ids=["three_values", "all_equal"])
@pytest.mark.parametrize("how", [dict(ratio=0.5), dict(k=1700)], ids=["ratio0.5", "k1700"])
def test_long_segments_whose_cut_falls_inside_a_run_of_equal_scores(values, how):
    sizes = [5000, 2999, 3000, 3001]
    gp = pointers(sizes)
    n = gp[-1]
    assert n + 1 > 3 * 4096                                                        # the scan of the keep flags takes several tiles
    score = np.random.default_rng(7).integers(0, values, size=n).astype(np.float32)
    rp, ci = block_graph(gp, n, 3, seed=8)
    assert len(ci) + 1 > 2 * 4096
    got = check(score, gp, how, rp, ci, partSize=32)
    if values == 1:                                                                # all equal: the first rows of every graph
        want = np.concatenate([np.arange(a, a + topk_ref.keep_count(s, **how)) for a, s in zip(gp[:-1], sizes)])
        assert np.array_equal(got["perm"], want)


@pytest.mark.parametrize("reps", [1, 20], ids=["wavefront", "workgroup"])
def test_special_values_follow_the_order_of_the_keys(reps):
    score = np.tile(SPECIALS, reps)
    n = len(score)
    assert (n <= W) == (reps == 1)
    for k in sorted(set([1, 2, 3, 5, 8, n // 2, n - 1, n])):
        got = check(score, [0, n], dict(k=k))
        # what is kept is not below what is dropped, in the order of gnna_keys.h
        key = topk_ref.order_key(score).astype(np.int64)
        kept = np.zeros(n, dtype=bool)
        kept[got["perm"]] = True
        assert kept.sum() == k and (k == n or key[kept].min() >= key[~kept].max())
    order = sorted(range(len(SPECIALS)), key=lambda r: (-int(topk_ref.order_key(SPECIALS)[r]), r))
    # NaN(+) > +inf > 1 > 1e-39 > 1e-45 > +0 > -0 > -1e-45 > -1 > -inf > NaN(-)
    assert order == [4, 13, 2, 14, 9, 8, 6, 0, 11, 1, 12, 7, 10, 3, 5]


def test_pointers_that_leave_rows_out_descend_or_lie_outside():
    n = 700
    score = tied_scores(n, 11)
    rp, ci = block_graph([0, n], n, 3, seed=12)
    for gp in ([5, 40, 300, 650],                   # rows before p[0] and from p[G] on belong to no graph
               [-9, 100, 100, 9000],                # clamped to [0, n]; an empty segment
               [0, 300, 200, 200, 700],             # a descending pair: empty; the next segment holds rows twice
               [600, 100],                          # only a descending pair
               [0]):                                # no graph
        for how in (dict(ratio=0.5), dict(k=7)):
            got = check(score, gp, how, rp, ci, partSize=4)
            if len(gp) == 1 or gp == [600, 100]:
                assert len(got["perm"]) == 0 and got["row_pointers"].tolist() == [0] and got["partPtr"].tolist() == [0]
    assert topk_ref.segments([0, 300, 200, 200, 700], n) == [(0, 300), (300, 300), (200, 200), (200, 700)]


def test_no_rows_no_edges_and_a_graph_without_edges():
    empty_f, empty_i = np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32)
    got = check(empty_f, [0, 0, 0], dict(ratio=0.5), np.zeros(1, dtype=np.int32), empty_i, partSize=4)
    assert got["graph_pointers"].tolist() == [0, 0, 0] and got["row_pointers"].tolist() == [0]
    check(empty_f, [0], dict(k=3))
    # the middle graph has no edge; the call without a CSR; the CSR without a partition
    gp = [0, 30, 50, 90]
    rp, ci = block_graph([0, 30], 90, 4, seed=3)
    rp2, ci2 = block_graph([50, 90], 90, 4, seed=4)
    rp, ci = (rp + rp2).astype(np.int32), np.concatenate((ci, ci2))
    score = tied_scores(90, 5)
    got = check(score, gp, dict(ratio=0.5), rp, ci, partSize=2)
    a, b = got["graph_pointers"][1], got["graph_pointers"][2]
    assert b - a == 10 and np.all(np.diff(got["row_pointers"][a: b + 1]) == 0)
    check(score, gp, dict(ratio=0.5))
    check(score, gp, dict(ratio=0.5), rp, ci)
    check(score, gp, dict(ratio=0.5), np.zeros(91, dtype=np.int32), empty_i, partSize=2)


def test_column_ids_outside_the_rows_are_dropped():
    gp = pointers([40, 300])
    n = gp[-1]
    rp, ci = block_graph(gp, n, 5, seed=21)
    ci = ci.copy()
    rng = np.random.default_rng(22)
    bad = rng.choice(len(ci), size=60, replace=False)
    ci[bad[:20]], ci[bad[20:40]], ci[bad[40:]] = -1, n, 2 ** 31 - 1
    got = check(tied_scores(n, 23), gp, dict(ratio=0.8), rp, ci, partSize=3)
    assert not np.isin(got["edge_ids"], bad).any() and got["column_index"].min() >= 0 and got["column_index"].max() < len(got["perm"])


def test_row_pointers_that_break_the_contract_are_refused_after_the_read_back():
    gp, n = [0, 50], 50
    rp, ci = block_graph(gp, n, 4, seed=31)
    for broken, where in ((np.r_[1, rp[1:]], 0), (np.r_[rp[:-1], rp[-1] + 3], n), (np.r_[rp[:20], rp[21], rp[20], rp[22:]], None)):
        if where is None and rp[20] == rp[21]:
            continue
        rc, counts, _, _ = run(tied_scores(n, 32), gp, ratio=0.5, rp=broken.astype(np.int32), ci=ci, partSize=4)
        assert rc == -1 and "row_pointers must start at 0, ascend and end at nnz = %d" % len(ci) in _lib.load().gnna_last_error().decode()
        assert counts[0] == 25


def test_ratio_one_gives_the_batch_back():
    gp = pointers([3, 70, 300, 1, 0, 26])
    n = gp[-1]
    rp, ci = block_graph(gp, n, 4, seed=41)
    got = check(tied_scores(n, 42), gp, dict(ratio=1.0), rp, ci, partSize=5)
    assert np.array_equal(got["perm"], np.arange(n)) and np.array_equal(got["new_id"], np.arange(n))
    assert np.array_equal(got["graph_pointers"], gp) and np.array_equal(got["row_pointers"], rp) and np.array_equal(got["column_index"], ci)
    assert np.array_equal(got["edge_ids"], np.arange(len(ci)))
    pp, p2n = _lib.build_part_device(5, _dev(rp, torch.int32))
    assert np.array_equal(got["partPtr"], pp.cpu().numpy()) and np.array_equal(got["part2Node"], p2n.cpu().numpy())


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "directed"])
def test_the_structure_of_the_output_and_its_edge_ids(symmetric):
    gp = pointers([90, 5, 400, 33])
    n = gp[-1]
    rp, ci = block_graph(gp, n, 5, seed=51, symmetric=symmetric)
    got = check(tied_scores(n, 52), gp, dict(ratio=0.5), rp, ci, partSize=8)
    new_rp, new_ci, eid, perm = got["row_pointers"], got["column_index"], got["edge_ids"], got["perm"]
    # every surviving edge is the relabelled edge of the input at edge_ids
    new_rows = np.repeat(np.arange(len(perm)), np.diff(new_rp))
    old_rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(perm[new_rows], old_rows[eid]) and np.array_equal(perm[new_ci], ci[eid]) and np.all(np.diff(eid) > 0)
    if symmetric:                                   # a symmetric input gives a symmetric output (reverse_edges raises otherwise)
        rev = _lib.reverse_edges(torch.from_numpy(new_rp), torch.from_numpy(new_ci)).cpu().numpy()
        assert np.array_equal(new_ci[rev], new_rows) and np.array_equal(new_rows[rev], new_ci)


def test_capacities_one_too_small():
    gp = pointers([90, 5, 400, 33])
    n = gp[-1]
    rp, ci = block_graph(gp, n, 5, seed=61)
    score = tied_scores(n, 62)
    ref = topk_ref.segment_topk(score, gp, ratio=0.5, row_pointers=rp, column_index=ci, partSize=2)
    need = (len(ref["perm"]), len(ref["column_index"]), len(ref["part2Node"]))
    assert min(need) > 0
    for which, name in enumerate(("row_cap", "edge_cap", "part_cap")):
        caps = dict(row_cap=need[0], edge_cap=need[1], part_cap=need[2])
        rc, counts, got, _ = run(score, gp, ratio=0.5, rp=rp, ci=ci, partSize=2, **caps)          # exactly enough
        assert rc == 0 and counts == need and np.array_equal(got["partPtr"], ref["partPtr"])
        caps[name] -= 1
        rc, counts, _, _ = run(score, gp, ratio=0.5, rp=rp, ci=ci, partSize=2, **caps)            # (run() checks the sentinels)
        message = _lib.load().gnna_last_error().decode()
        assert rc == -1 and counts == need and "capacity too small" in message and "%d rows, %d edges and %d neighbor-groups" % need in message
    # the wrapper hands the counts on
    with pytest.raises(_lib.GnnaError, match="capacity too small") as info:
        _lib.segment_topk(_dev(score, torch.float32), _dev(gp, torch.int32), ratio=0.5, row_pointers=_dev(rp, torch.int32),
                          column_index=_dev(ci, torch.int32), partSize=2, edge_capacity=need[1] - 1)
    assert info.value.counts == need


def test_refused_inside_a_stream_capture():
    gp = pointers([30, 40])
    score = _dev(tied_scores(70, 71), torch.float32)
    gpd = _dev(gp, torch.int32)
    _lib.segment_topk(score, gpd, ratio=0.5)                  # (scratch exists: the capture below has nothing to allocate)
    new_id, perm, new_gp = _buf(70), _buf(70), _buf(3)
    counts = (ctypes.c_int64 * 3)()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = None
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lib = _lib.load()
            rc = lib.gnna_segment_topk_i32(score.data_ptr(), 70, gpd.data_ptr(), 2, 0.5, 0, None, None, 0, 0, new_id.data_ptr(),
                                           perm.data_ptr(), new_gp.data_ptr(), None, None, None, None, None, 70, 0, 0, counts,
                                           side.cuda_stream)
            new_id.add_(0)                                    # (a capture must record something)
    assert rc == -3 and "stream capture" in lib.gnna_last_error().decode()      # GNNA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((perm == SENTINEL).all())


def test_the_same_bits_on_every_run_and_under_the_deterministic_tuning():
    gp = pointers(MIXED + [3000])
    n = gp[-1]
    rp, ci = block_graph(gp, n, 4, seed=81)
    score = np.random.default_rng(82).integers(0, 4, size=n).astype(np.float32)
    first = run(score, gp, ratio=0.5, rp=rp, ci=ci, partSize=3)
    assert first[0] == 0
    try:
        _lib.set_tuning(deterministic=1)
        again = run(score, gp, ratio=0.5, rp=rp, ci=ci, partSize=3)
    finally:
        _lib.reset_tuning()
    assert again[0] == 0 and again[1] == first[1]
    for name in first[3]:
        assert torch.equal(first[3][name], again[3][name]), name


def test_the_wrapper_and_the_module_agree_with_the_reference():
    GNNA = load_extension()
    gp = pointers([90, 5, 400, 33], first=2)
    n = gp[-1] + 4
    rp, ci = block_graph(gp, n, 5, seed=91)
    score = tied_scores(n, 92)
    sd, gpd, rpd, cid = _dev(score, torch.float32), _dev(gp, torch.int32), _dev(rp, torch.int32), _dev(ci, torch.int32)
    for how in (dict(ratio=0.3), dict(k=9)):
        ref = topk_ref.segment_topk(score, gp, row_pointers=rp, column_index=ci, partSize=4, **how)
        got = _lib.segment_topk(sd, gpd, row_pointers=rpd, column_index=cid, partSize=4, want_edge_ids=True, **how)
        assert got.pop("num_rows") == len(ref["perm"])
        for name in ref:
            assert np.array_equal(got[name].cpu().numpy(), ref[name]), name
        mod = GNNA.segment_topk(sd, gpd, how.get("ratio", 0.0), how.get("k", 0), rpd, cid, 4, True)
        for t, name in zip(mod, ("new_id", "perm", "graph_pointers", "row_pointers", "column_index", "edge_ids", "partPtr", "part2Node")):
            assert np.array_equal(t.cpu().numpy(), ref[name]), name
        bare = _lib.segment_topk(sd, gpd, **how)
        assert bare["row_pointers"] is None and bare["partPtr"] is None and np.array_equal(bare["perm"].cpu().numpy(), ref["perm"])
        assert GNNA.segment_topk(sd, gpd, how.get("ratio", 0.0), how.get("k", 0))[3] is None

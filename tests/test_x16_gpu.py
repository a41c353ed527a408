"""gnna_agg_ld_x16: features stored in bfloat16 / float16, accumulated in fp32, written as fp32 or in the input's type.

Reference: the 16-bit inputs converted exactly to fp64 and aggregated in fp64 (never the fp32 path of the code under
test, except in the exactness test).  Tolerance (derived, not tuned), with scale = sum |coef * x| from the same fp64 formula
on |X|:
    fp32 output:    |err| <= 1e-4 * max(1, scale)                 -- the project's bound for an fp32 accumulation
    16-bit output:  |err| <= 1e-4 * max(1, scale) + u * |ref|      -- plus one round-to-nearest: u = 2^-8 (bf16), 2^-11 (fp16)
Every element is compared and a NaN counts as wrong; the suite runs with GNNA_DEBUG_POISON=1, so an element the library
leaves unwritten shows as NaN."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph

pytestmark = pytest.mark.gpu

SAG, GCN, GIN = 0, 1, 2
DTYPES = [torch.bfloat16, torch.float16]
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
WIDTHS = [1, 3, 7, 8, 16, 32, 41, 64, 100, 128, 256]
PART_SIZES = [1, 3, 32, 64]
EPS = 0.37


def _rows_of(pp, p2n):
    """Destination row of every edge position a partition covers, and those positions (any partition: groups with a
    negative range are empty)."""
    pp, p2n = pp.long(), p2n.long()
    lens = (pp[1:] - pp[:-1]).clamp(min=0)
    rows = torch.repeat_interleave(p2n, lens)
    starts = torch.repeat_interleave(pp[:-1], lens)
    first = torch.cumsum(lens, 0) - lens
    pos = starts + (torch.arange(rows.numel(), device=pp.device) - torch.repeat_interleave(first, lens))
    return rows, pos


def _agg64(mode, X, ci, pp, p2n, num_out_rows, deg_out=None, deg_in=None, eps=1.0):
    """fp64 aggregation over the partition itself and its magnitude scale sum |coef * x| (on X's device)."""
    rows, pos = _rows_of(pp, p2n)
    cols = ci.long()[pos]
    Xd = X.double()
    ref = torch.zeros(num_out_rows, X.shape[1], dtype=torch.float64, device=X.device)
    scale = torch.zeros_like(ref)
    for c0 in range(0, cols.numel(), 1 << 21):
        sl = slice(c0, c0 + (1 << 21))
        src = Xd[cols[sl]]
        if mode == GCN:
            src = src * (deg_out.double()[rows[sl]] * deg_in.double()[cols[sl]])[:, None]
        ref.index_add_(0, rows[sl], src)
        scale.index_add_(0, rows[sl], src.abs())
    if mode == GIN:
        ref, scale = ref * float(np.float32(eps)), scale * abs(float(np.float32(eps)))
    return ref, scale


def _check(got, ref, scale, what, relu=False):
    """Every element inside the bound of the module docstring (NaN counts as off); prints the worst error / tolerance."""
    u = UNIT[got.dtype]
    if relu:
        ref = ref.clamp(min=0)
    g = got.double()
    tol = 1e-4 * scale.clamp(min=1.0) + u * ref.abs()
    both_inf = torch.isinf(g) & (g == ref)
    err = torch.where(both_inf, torch.zeros_like(ref), (g - ref).abs())
    bad = ~(err <= tol)
    worst = float((err / tol).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    print(f"{what}: worst err / tol = {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} elements off, worst err / tol {worst:.3f}"


def _graph(kind, seed, n=3000, nnz=120000):
    if kind == "powerlaw":
        return graph.powerlaw_graph(n, nnz, 900, seed=seed)
    return graph.uniform_graph(n, nnz, seed=seed)


def _features(n, dim, dtype, seed):
    return torch.randn(n, dim, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _degrees(g, dtype):
    """fp32 degrees; for fp16 scaled so that the GCN outputs stay finite (coefficients are products of sqrt-degrees)."""
    deg = g.degrees.clone()
    if dtype == torch.float16:
        deg = deg / deg.max()
    return deg.cuda()


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("dim", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_modes_outputs_part_sizes(dtype, dim, kind):
    """{SAG, GCN, GIN} x {fp32 out, 16-bit out} x partSizes {1, 3, 32, 64} at one width on one graph."""
    g = _graph(kind, seed=dim)
    ci, deg = g.column_index.cuda(), _degrees(g, dtype)
    X = _features(g.num_nodes, dim, dtype, seed=dim + 1)
    for partSize in PART_SIZES:
        pp, p2n = [t.cuda() for t in _lib.build_part(partSize, g.row_pointers)]
        for mode in (SAG, GCN, GIN):
            ref, scale = _agg64(mode, X, ci, pp, p2n, g.num_nodes, deg, deg, EPS)
            for out_dtype in (torch.float32, dtype):
                Y = _lib.agg_ld_x16(mode, X, ci, pp, p2n, g.num_nodes, partSize, degrees_out=deg, degrees_in=deg,
                                    epsilon=EPS, out_dtype=out_dtype)
                assert Y.dtype == out_dtype
                _check(Y, ref, scale, f"{kind} {dtype} D={dim} ps={partSize} mode={mode} out={out_dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_hub_empty_rows_isolated_nodes(dtype):
    """A hub of >= 10,000 edges, rows without edges and nodes nobody points at."""
    n, hub_deg = 20000, 12000
    gen = torch.Generator().manual_seed(3)
    counts = torch.randint(0, 12, (n,), generator=gen)
    counts[torch.rand(n, generator=gen) < 0.3] = 0          # empty rows
    counts[7] = hub_deg
    rp = torch.zeros(n + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(counts, 0).int()
    ci = torch.randint(0, n // 2, (int(rp[-1]),), generator=gen, dtype=torch.int32)   # ids >= n / 2: isolated sources
    assert int(counts.max()) >= 10000 and int((counts == 0).sum()) > 1000
    deg = torch.sqrt(counts.clamp(min=1).float())
    deg = (deg / deg.max() if dtype == torch.float16 else deg).cuda()
    X = _features(n, 64, dtype, seed=4)
    for partSize in (3, 32):
        pp, p2n = [t.cuda() for t in _lib.build_part(partSize, rp)]
        for mode in (SAG, GCN, GIN):
            ref, scale = _agg64(mode, X, ci.cuda(), pp, p2n, n, deg, deg, EPS)
            for out_dtype in (torch.float32, dtype):
                Y = _lib.agg_ld_x16(mode, X, ci.cuda(), pp, p2n, n, partSize, degrees_out=deg, degrees_in=deg, epsilon=EPS,
                                    out_dtype=out_dtype)
                _check(Y, ref, scale, f"hub {dtype} ps={partSize} mode={mode} out={out_dtype}")
                assert (Y[counts.cuda() == 0] == 0).all(), "a row without edges is zero"


@pytest.mark.parametrize("dim", [7, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_non_canonical_partition(dtype, dim):
    """Groups in shuffled order (part2Node not sorted, rows split over distant groups), an empty group and a group with a
    negative range: the answer is the sum over the partition as given."""
    g = _graph("powerlaw", seed=21)
    pp0, p2n0 = _lib.build_part(8, g.row_pointers)
    P = p2n0.numel()
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(1))
    # a shuffled partition cannot share one pointer array, so every group gets its own [start, end) pair through a
    # column_index that repeats the group's ids in the new order
    lens = (pp0[1:] - pp0[:-1]).long()[perm]
    pp = torch.zeros(P + 1, dtype=torch.int64)
    pp[1:] = torch.cumsum(lens, 0)
    starts = pp0[:-1].long()[perm]
    ci_new = torch.cat([g.column_index[int(s): int(s) + int(l)] for s, l in zip(starts.tolist(), lens.tolist())])
    p2n = p2n0[perm].clone()
    pp = pp.int()
    # an empty group and a negative range in the middle: insert two extra groups
    mid = P // 2
    cut = int(pp[mid])
    pp = torch.cat([pp[:mid + 1], torch.tensor([cut, cut - 5], dtype=torch.int32), pp[mid + 1:]])
    # groups: ..., [pp[mid-1], cut), [cut, cut) empty, [cut, cut-5) negative, [cut-5, pp[mid+1]) -- the last one re-reads 5 ids
    p2n = torch.cat([p2n[:mid], torch.tensor([5, 6], dtype=torch.int32), p2n[mid:]])
    X = _features(g.num_nodes, dim, dtype, seed=5)
    deg = _degrees(g, dtype)
    ci_d, pp_d, p2n_d = ci_new.cuda(), pp.cuda(), p2n.cuda()
    for mode in (SAG, GCN):
        ref, scale = _agg64(mode, X, ci_d, pp_d, p2n_d, g.num_nodes, deg, deg)
        for out_dtype in (torch.float32, dtype):
            Y = _lib.agg_ld_x16(mode, X, ci_d, pp_d, p2n_d, g.num_nodes, 8, degrees_out=deg, degrees_in=deg, out_dtype=out_dtype)
            _check(Y, ref, scale, f"non-canonical {dtype} D={dim} mode={mode} out={out_dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rectangular(dtype):
    """num_in_rows != num_out_rows: a destination shard gathering from all source rows."""
    g = _graph("uniform", seed=8, n=4000, nnz=100000)
    lo, hi = 1000, 2500
    rp = (g.row_pointers[lo:hi + 1] - g.row_pointers[lo]).int()
    ci = g.column_index[int(g.row_pointers[lo]): int(g.row_pointers[hi])].cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, rp)]
    X = _features(g.num_nodes, 64, dtype, seed=9)
    deg_in = _degrees(g, dtype)
    deg_out = deg_in[lo:hi].contiguous()
    for mode in (SAG, GCN, GIN):
        ref, scale = _agg64(mode, X, ci, pp, p2n, hi - lo, deg_out, deg_in, EPS)
        for out_dtype in (torch.float32, dtype):
            Y = _lib.agg_ld_x16(mode, X, ci, pp, p2n, hi - lo, 32, degrees_out=deg_out, degrees_in=deg_in, epsilon=EPS,
                                out_dtype=out_dtype)
            assert Y.shape == (hi - lo, 64)
            _check(Y, ref, scale, f"rect {dtype} mode={mode} out={out_dtype}")


@pytest.mark.parametrize("dim", [16, 41, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_leading_dimensions_relu_accumulate(dtype, dim):
    """ld_in / ld_out > dim (a column block of a wider matrix, output into a slice), the ReLU epilogue with both output types,
    ACCUMULATE into fp32 and its refusal with a 16-bit output; the elements around the views are never touched."""
    g = _graph("powerlaw", seed=11, n=2500, nnz=150000)
    ci = g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    n = g.num_nodes
    wide = _features(n, dim + 24, dtype, seed=dim)
    for off in (8, 3):                       # a 16-byte aligned block and one that is not
        X = wide[:, off: off + dim]
        ref, scale = _agg64(SAG, X, ci, pp, p2n, n)
        for out_dtype in (torch.float32, dtype):
            buf = torch.full((n, dim + 10), 7.0, dtype=out_dtype, device="cuda")
            out = buf[:, 5: 5 + dim]
            _lib.agg_ld_x16(SAG, X, ci, pp, p2n, n, 32, out=out, relu=True)
            _check(out, ref, scale, f"ld relu {dtype} D={dim} off={off} out={out_dtype}", relu=True)
            assert (buf[:, :5] == 7).all() and (buf[:, 5 + dim:] == 7).all()
        acc = torch.full((n, dim), 2.5, dtype=torch.float32, device="cuda")
        _lib.agg_ld_x16(SAG, X, ci, pp, p2n, n, 32, out=acc, accumulate=True)
        _check(acc, ref + 2.5, scale + 2.5, f"accumulate {dtype} D={dim} off={off}")
        with pytest.raises(_lib.GnnaError, match="round"):
            _lib.agg_ld_x16(SAG, X, ci, pp, p2n, n, 32, out=torch.zeros(n, dim, dtype=dtype, device="cuda"), accumulate=True)


def test_output_type_rules():
    g = _graph("uniform", seed=2, n=500, nnz=4000)
    ci = g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    X = _features(g.num_nodes, 16, torch.bfloat16, seed=1)
    with pytest.raises(_lib.GnnaError):
        _lib.agg_ld_x16(SAG, X, ci, pp, p2n, g.num_nodes, 32, out_dtype=torch.float16)
    L = _lib.load()
    out = torch.zeros(g.num_nodes, 16, dtype=torch.float16, device="cuda")
    rc = L.gnna_agg_ld_x16(SAG, _lib.BF16, X.data_ptr(), 16, g.num_nodes, ci.data_ptr(), None, None, 1.0, pp.data_ptr(),
                           p2n.data_ptr(), out.data_ptr(), _lib.F16, 16, g.num_nodes, 16, p2n.numel(), 32, 0, None)
    assert rc == -1, "out_type must be GNNA_F32 or in_type: GNNA_ERR_INVALID_ARGUMENT"
    rc = L.gnna_agg_ld_x16(SAG, _lib.F32, X.data_ptr(), 16, g.num_nodes, ci.data_ptr(), None, None, 1.0, pp.data_ptr(),
                           p2n.data_ptr(), out.data_ptr(), _lib.F32, 16, g.num_nodes, 16, p2n.numel(), 32, 0, None)
    assert rc == -1, "GNNA_F32 is an output type only"
    with pytest.raises(_lib.GnnaError):
        _lib.agg_ld_x16(SAG, X.float(), ci, pp, p2n, g.num_nodes, 32)


def test_fp16_overflow_is_inf():
    """An fp16 output row whose sum exceeds 65504 is +-inf (IEEE rounding), not NaN or garbage; its neighbours stay exact."""
    n, d = 64, 16
    rp = torch.zeros(n + 1, dtype=torch.int32)
    rp[1:] = torch.arange(1, n + 1, dtype=torch.int32) * 4
    ci = torch.arange(4 * n, dtype=torch.int32)
    ci[8:] = 8 + (ci[8:] - 8) % (n - 8)          # rows 0 and 1 read ids 0..7, every other row ids >= 8
    X = torch.ones(n, d, dtype=torch.float16)
    X[0:4] = 30000.0            # row 0 sums ids 0..3: 120000 > 65504
    X[4:8, :8] = -30000.0       # row 1: -inf in its first 8 columns, 4 in the others
    X[4:8, 8:] = 1.0
    pp, p2n = [t.cuda() for t in _lib.build_part(32, rp)]
    Y = _lib.agg_ld_x16(SAG, X.cuda(), ci.cuda(), pp, p2n, n, 32).cpu()
    assert Y.dtype == torch.float16
    assert (Y[0] == float("inf")).all() and (Y[1, :8] == float("-inf")).all() and (Y[1, 8:] == 4).all()
    assert (Y[2:] == 4).all()
    Y32 = _lib.agg_ld_x16(SAG, X.cuda(), ci.cuda(), pp, p2n, n, 32, out_dtype=torch.float32).cpu()
    assert (Y32[0] == 120000).all() and (Y32[1, :8] == -120000).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_exact_on_small_integers(dtype):
    """X of integers in [-8, 8] is exact in both formats and every sum stays far below 2^24: unweighted SAG with fp32 output
    equals _lib.agg_ld on X.float() bit for bit, and the 16-bit output equals that result rounded once."""
    g = _graph("powerlaw", seed=17)
    ci = g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    Xi = torch.randint(-8, 9, (g.num_nodes, 64), generator=torch.Generator().manual_seed(2)).float()
    X = Xi.to(dtype).cuda()
    assert (X.float().cpu() == Xi).all()
    want = _lib.agg_ld(SAG, X.float(), ci, pp, p2n, g.num_nodes, 32)
    assert float(want.abs().max()) < 2 ** 24
    got32 = _lib.agg_ld_x16(SAG, X, ci, pp, p2n, g.num_nodes, 32, out_dtype=torch.float32)
    assert torch.equal(got32, want)
    got16 = _lib.agg_ld_x16(SAG, X, ci, pp, p2n, g.num_nodes, 32)
    assert got16.dtype == dtype and torch.equal(got16, want.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_prepared_graph_counters_stay_flat(dtype):
    """On a prepared graph (gnna_prepare_graph + gnna_prepare_x16) the 16-bit calls neither synchronise, free nor allocate."""
    g = _graph("powerlaw", seed=23, n=6000, nnz=400000)
    ci = g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    deg = _degrees(g, dtype)
    _lib.prepare_graph(ci, pp, p2n, g.num_nodes, g.num_nodes, 32, dims=(41, 64))
    _lib.prepare_x16(g.num_nodes, g.num_nodes, (41, 64))
    try:
        before = _lib.runtime_counters()
        for dim in (41, 64):
            X = _features(g.num_nodes, dim, dtype, seed=dim)
            for mode in (SAG, GCN, GIN):
                for out_dtype in (torch.float32, dtype):
                    Y = _lib.agg_ld_x16(mode, X, ci, pp, p2n, g.num_nodes, 32, degrees_out=deg, degrees_in=deg, out_dtype=out_dtype)
            ref, scale = _agg64(GIN, X, ci, pp, p2n, g.num_nodes)
            _check(Y, ref, scale, f"prepared {dtype} D={dim}")
        after = _lib.runtime_counters()
        for name in ("launch_syncs", "launch_frees", "launch_mallocs"):
            assert after[name] == before[name], (name, before, after)
    finally:
        _lib.release_graph(ci)


@pytest.mark.parametrize("out32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_capture_replays_next_to_eager(dtype, out32):
    """A torch.cuda.graph capture of a 16-bit call (no warm-up on the capture stream) replays correctly while eager calls of
    another shape use the library's scratch in between: the capture owns its scratch."""
    g = _graph("powerlaw", seed=29)
    ci = g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    out_dtype = torch.float32 if out32 else dtype
    X = _features(g.num_nodes, 41, dtype, seed=1)          # (41: staged source rows AND fp32 sums in library scratch)
    Y = torch.zeros(g.num_nodes, 41, dtype=out_dtype, device="cuda")
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        _lib.agg_ld_x16(GIN, X, ci, pp, p2n, g.num_nodes, 32, epsilon=EPS, out=Y)
    X2 = _features(g.num_nodes, 100, dtype, seed=2)
    ref2, scale2 = _agg64(SAG, X2, ci, pp, p2n, g.num_nodes)
    for rep in range(3):
        X.copy_(_features(g.num_nodes, 41, dtype, seed=10 + rep))
        Y.fill_(float("nan"))
        cg.replay()
        E = _lib.agg_ld_x16(SAG, X2, ci, pp, p2n, g.num_nodes, 32, out_dtype=out_dtype)     # eager, same stream family
        cg.replay()
        torch.cuda.synchronize()
        ref, scale = _agg64(GIN, X, ci, pp, p2n, g.num_nodes, eps=EPS)
        _check(Y, ref, scale, f"captured {dtype} out={out_dtype} rep={rep}")
        _check(E, ref2, scale2, f"eager next to the capture {dtype} out={out_dtype} rep={rep}")


def test_deterministic_is_refused():
    """gnna_tuning.deterministic = 1: the 16-bit call adds its rows with float atomics and says so instead of running."""
    g = _graph("uniform", seed=2, n=500, nnz=4000)
    ci = g.column_index.cuda()
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers)]
    X = _features(g.num_nodes, 16, torch.bfloat16, seed=1)
    try:
        _lib.set_tuning(deterministic=1)
        with pytest.raises(_lib.GnnaError, match="deterministic"):
            _lib.agg_ld_x16(SAG, X, ci, pp, p2n, g.num_nodes, 32)
    finally:
        _lib.reset_tuning()
    _lib.agg_ld_x16(SAG, X, ci, pp, p2n, g.num_nodes, 32)

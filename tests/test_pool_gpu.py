"""gnna_segment_pool_ld_f32 / gnna_segment_pool_backward_ld_f32 on the GPU, through the C ABI (_lib) and through GNNA, against
tests/pool_ref.py.  The layouts are derived from the tile (T = _lib.POOL_TILE_ROWS) and from the number of tiles at which a
segment's join moves from a wavefront to the workgroup (_lib.POOL_LONG_STEPS per slot).

Extrema, rows and the backward's selection are exact (bit patterns).  Sums are exact on integer-valued inputs (|x| <= 8: every
order of addition is exact in fp32) and within 1e-4 * max(1, sum |terms|) of fp64 on normal inputs, with every segment <= 1600
rows: any order of n fp32 additions errs by at most (n - 1) * 2^-24 * sum |terms| < 1e-4 * sum |terms| for n <= 1600."""
import numpy as np
import pytest
import torch

import pool_ref
from gnnadvisor_osdi21_amd import _lib, load_extension

pytestmark = pytest.mark.gpu

T = _lib.POOL_TILE_ROWS
DIMS = (1, 3, 4, 16, 33, 64, 100, 128, 257)
NAN = float("nan")


def _slots(dim):
    """Partial rows of a wavefront at this width: 64 / lanes per row."""
    lanes = 1
    while lanes < 64 and 4 * lanes < dim:
        lanes *= 2
    return 64 // lanes


def _cum(first, lengths):
    return [first] + list(first + np.cumsum(lengths))


def _layouts(dim):
    """name -> (num_rows, graph_pointers)"""
    long_tiles = _lib.POOL_LONG_STEPS * _slots(dim) + 2        # joined by the whole workgroup
    return {
        "one_segment": (2 * T + 7, [0, 2 * T + 7]),
        "single_rows": (T + 3, list(range(T + 4))),
        "empties": (T + 9, [0, 0, 5, 5, T, T, T + 9, T + 9]),     # first, middle, on the tile boundary, last
        "len_63_64_65": (192, _cum(0, [63, 64, 65])),
        "len_T-1_T_T+1": (3 * T, _cum(0, [T - 1, T, T + 1])),
        "two_tiles": (T + 20, [0, T - 10, T + 10, T + 20]),
        "three_tiles_and_5": (3 * T + 20, [0, 7, 3 * T + 12, 3 * T + 20]),       # the tile [T, 2T) and [2T, 3T) are wholly its
        "begins_on_a_tile": (2 * T + 5, [0, T, 2 * T + 5]),
        "less_than_a_tile": (37, [0, 10, 37]),
        "rows_of_no_graph": (T + 30, [3, 40, T + 2]),
        "long_join": (long_tiles * T + 5, [2, 9, long_tiles * T - 3, long_tiles * T + 5]),
    }


LAYOUT_NAMES = tuple(_layouts(1))


def _ints(n, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(n, dim)).astype(np.float32)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _padded(rows, dim, pad, dtype=torch.float32):
    """A NaN-filled (INT_MIN-filled) buffer [rows, dim + pad] and its view [rows, dim]."""
    fill = NAN if dtype == torch.float32 else -(2 ** 31)
    buf = torch.full((rows, dim + pad), fill, dtype=dtype, device="cuda")
    return buf, buf[:, :dim]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _forward(X, gp, want=_lib.POOL_STATS, mean=False, pad=3):
    """Through the C ABI with leading dimensions > dim on the input and every output; checks that the padding is untouched."""
    n, dim = X.shape
    G = len(gp) - 1
    xbuf, xv = _padded(n, dim, pad)
    xv.copy_(_dev(X))
    out, bufs = {}, {}
    for name in want:
        bufs[name], out[name] = _padded(G, dim, pad)
        if name != "sum":
            bufs["arg" + name], out["arg" + name] = _padded(G, dim, pad, torch.int32)
    res = _lib.segment_pool(xv, _dev(gp, torch.int32), want=want, mean=mean, out=out)
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert set(res) == set(bufs) and res[name] is out[name]
        tail = buf[:, dim:]
        assert bool(torch.isnan(tail).all() if buf.dtype == torch.float32 else (tail == -(2 ** 31)).all()), name
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_extrema(got, ref):
    for name in ("max", "min"):
        if name in got:
            assert np.array_equal(_bits(got[name]), _bits(ref[name])), name
            assert np.array_equal(got["arg" + name], ref["arg" + name]), "arg" + name


def _backward(gp, n, dim, grads, mean, pad=2):
    """Through the C ABI into a NaN-filled padded d_input: every element of the dim columns written, the padding untouched."""
    buf, view = _padded(n, dim, pad)
    dev = {k: (None if v is None else _dev(v)) for k, v in grads.items()}
    _lib.segment_pool_backward(_dev(gp, torch.int32), n, mean=mean, out=view, **dev)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, dim:]).all())
    return view.cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dim", DIMS)
def test_forward_and_backward_are_exact_on_integer_valued_inputs(dim, layout):
    n, gp = _layouts(dim)[layout]
    X = _ints(n, dim, 100 + dim)
    ref = pool_ref.forward(X, gp)
    got = _forward(X, gp)
    assert np.array_equal(got["sum"], ref["sum"].astype(np.float32))
    _check_extrema(got, ref)
    mean = _forward(X, gp, want=("sum",), mean=True)["sum"]
    assert np.array_equal(_bits(mean), _bits(pool_ref.mean_f32(X, gp)))
    # backward: integer-valued gradients, the rows the forward found
    G = len(gp) - 1
    rng = np.random.default_rng(7 + dim)
    grads = dict(d_sum=rng.integers(-4, 5, (G, dim)).astype(np.float32), d_max=rng.integers(-4, 5, (G, dim)).astype(np.float32),
                 argmax=ref["argmax"], d_min=rng.integers(-4, 5, (G, dim)).astype(np.float32), argmin=ref["argmin"])
    for is_mean in (False, True):
        dX = _backward(gp, n, dim, grads, is_mean)
        assert np.array_equal(dX, pool_ref.backward(gp, n, dim, mean=is_mean, **grads)), is_mean


# (long_join has a segment of more than 1600 rows, where the bound would test the order of the additions: it is covered by the
# integer-valued inputs above)
@pytest.mark.parametrize("layout", [name for name in LAYOUT_NAMES if name != "long_join"])
@pytest.mark.parametrize("dim", DIMS)
def test_sums_of_normal_inputs_are_within_the_bound_of_fp64(dim, layout):
    n, gp = _layouts(dim)[layout]
    assert max(b - a for a, b in pool_ref.segments(gp, n)) <= 1600
    X = np.random.default_rng(dim).standard_normal((n, dim)).astype(np.float32)
    ref = pool_ref.forward(X, gp)
    got = _forward(X, gp)
    bound = 1e-4 * np.maximum(1.0, ref["abs"])
    assert (np.abs(got["sum"].astype(np.float64) - ref["sum"]) <= bound).all()
    _check_extrema(got, ref)
    count = np.maximum(ref["count"], 1)[:, None]
    mean = _forward(X, gp, want=("sum",), mean=True)["sum"]
    assert (np.abs(mean.astype(np.float64) - ref["sum"] / count) <= bound / count).all()


def test_a_batch_without_graphs():
    gp = _dev([0], torch.int32)
    X = _dev(_ints(40, 5, 1))
    res = _lib.segment_pool(X, gp, want=_lib.POOL_STATS)
    assert all(tuple(v.shape) == (0, 5) for v in res.values()) and set(res) == {"sum", "max", "argmax", "min", "argmin"}
    # the C entry itself: nothing is written
    keep = torch.full((2, 5), 7.0, device="cuda")
    _lib._call(X.device, "gnna_segment_pool_ld_f32", X.data_ptr(), 5, 40, gp.data_ptr(), 0, keep.data_ptr(), 5, None, 5, None, 5, None, 5,
               None, 5, 5, 0)
    assert bool((keep == 7.0).all())
    # backward: every row is a row of no graph
    d_sum = torch.ones(1, 5, device="cuda")
    out = torch.full((40, 5), NAN, device="cuda")
    _lib._call(X.device, "gnna_segment_pool_backward_ld_f32", d_sum.data_ptr(), 5, None, 5, None, 5, None, 5, None, 5, gp.data_ptr(), 0,
               out.data_ptr(), 5, 40, 5, 0)
    assert bool((out == 0).all())
    # ... and the wrapper, whose empty gradient has no address
    out.fill_(NAN)
    assert _lib.segment_pool_backward(gp, 40, d_sum=torch.zeros(0, 5, device="cuda"), out=out) is out and bool((out == 0).all())


def test_pointers_are_clamped_and_a_descending_pair_is_an_empty_segment():
    """The forward of pointers that break the contract in the two ways the header names (inside one tile: the search for a tile's
    first segment assumes pointers that do not descend)."""
    n, dim, gp = 50, 5, [-5, 20, 10, 10, 70]                      # -> [0, 20), empty, empty, [10, 50)
    assert pool_ref.segments(gp, n) == [(0, 20), (20, 20), (10, 10), (10, 50)]
    X = _ints(n, dim, 3)
    ref = pool_ref.forward(X, gp)
    got = _forward(X, gp)
    assert np.array_equal(got["sum"], ref["sum"].astype(np.float32))
    _check_extrema(got, ref)


SUBSETS = [w for k in range(1, 8) for w in [tuple(n for b, n in enumerate(_lib.POOL_STATS) if k >> b & 1)]]


@pytest.mark.parametrize("want", SUBSETS, ids=["+".join(w) for w in SUBSETS])
@pytest.mark.parametrize("dim, layout", [(3, "two_tiles"), (64, "three_tiles_and_5"), (100, "empties"), (16, "long_join")])
def test_any_subset_of_the_outputs(dim, layout, want):
    n, gp = _layouts(dim)[layout]
    X = _ints(n, dim, 5)
    ref = pool_ref.forward(X, gp)
    got = _forward(X, gp, want=want)
    assert set(got) == set(want) | {"arg" + w for w in want if w != "sum"}
    if "sum" in want:
        assert np.array_equal(got["sum"], ref["sum"].astype(np.float32))
    _check_extrema(got, ref)
    # values without their rows
    if "max" in want:
        only = _lib.segment_pool(_dev(X), _dev(gp, torch.int32), want=("max",), out={"max": torch.empty(len(gp) - 1, dim, device="cuda")})
        assert set(only) == {"max"} and np.array_equal(_bits(only["max"].cpu().numpy()), _bits(ref["max"]))
    # the matching subset of the backward's terms
    G = len(gp) - 1
    rng = np.random.default_rng(3)
    grads = {}
    if "sum" in want:
        grads["d_sum"] = rng.integers(-4, 5, (G, dim)).astype(np.float32)
    for name in ("max", "min"):
        if name in want:
            grads["d_" + name], grads["arg" + name] = rng.integers(-4, 5, (G, dim)).astype(np.float32), ref["arg" + name]
    assert np.array_equal(_backward(gp, n, dim, grads, True), pool_ref.backward(gp, n, dim, mean=True, **grads))


@pytest.mark.parametrize("dim, layout", [(4, "single_rows"), (33, "two_tiles"), (64, "len_63_64_65"), (128, "three_tiles_and_5")])
def test_ties_signed_zeros_and_nan_rows(dim, layout):
    n, gp = _layouts(dim)[layout]
    rng = np.random.default_rng(9)
    X = rng.integers(-1, 2, size=(n, dim)).astype(np.float32)           # -1, 0, 1: ties everywhere
    zeros = X == 0
    X[zeros & (rng.random((n, dim)) < 0.5)] = np.float32(-0.0)          # -0 sorts below +0
    X[n // 2] = np.float32(NAN)                                          # a NaN with a clear sign bit: above +inf
    X[n // 3, ::2] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]   # one with the sign bit set: below -inf
    ref = pool_ref.forward(X, gp)
    got = _forward(X, gp, want=("max", "min"))
    _check_extrema(got, ref)
    # the winning rows select the gradient, whatever the values were
    G = len(gp) - 1
    grads = dict(d_max=np.ones((G, dim), np.float32), argmax=got["argmax"], d_min=np.full((G, dim), 2, np.float32), argmin=got["argmin"])
    assert np.array_equal(_backward(gp, n, dim, grads, False), pool_ref.backward(gp, n, dim, **grads))


@pytest.mark.parametrize("dim, layout", [(33, "three_tiles_and_5"), (64, "long_join"), (257, "len_T-1_T_T+1")])
def test_the_same_bits_on_two_runs_and_deterministic_tuning_accepts_the_call(dim, layout):
    n, gp = _layouts(dim)[layout]
    X = np.random.default_rng(4).standard_normal((n, dim)).astype(np.float32)
    first = _forward(X, gp)
    try:
        _lib.set_tuning(deterministic=1)
        second = _forward(X, gp)
        G = len(gp) - 1
        grads = dict(d_sum=np.random.default_rng(5).standard_normal((G, dim)).astype(np.float32))
        a, b = _backward(gp, n, dim, grads, True), _backward(gp, n, dim, grads, True)
    finally:
        _lib.reset_tuning()
    for name in first:
        assert np.array_equal(first[name].view(np.uint32), second[name].view(np.uint32)), name
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dim, layout", [(64, "three_tiles_and_5"), (3, "empties"), (100, "rows_of_no_graph")])
def test_through_the_extension_module(dim, layout):
    GNNA = load_extension()
    n, gp = _layouts(dim)[layout]
    X = _ints(n, dim, 21)
    ref = pool_ref.forward(X, gp)
    gpd = _dev(gp, torch.int32)
    s, mx, amx, mn, amn = GNNA.segment_pool(_dev(X), gpd, True, True, True, False)
    got = dict(sum=s.cpu().numpy(), max=mx.cpu().numpy(), argmax=amx.cpu().numpy(), min=mn.cpu().numpy(), argmin=amn.cpu().numpy())
    assert np.array_equal(got["sum"], ref["sum"].astype(np.float32))
    _check_extrema(got, ref)
    m, none_mx, none_amx, none_mn, none_amn = GNNA.segment_pool(_dev(X), gpd, True, False, False, True)
    assert none_mx is None and none_amx is None and none_mn is None and none_amn is None
    assert np.array_equal(_bits(m.cpu().numpy()), _bits(pool_ref.mean_f32(X, gp)))
    G = len(gp) - 1
    rng = np.random.default_rng(2)
    grads = dict(d_sum=rng.integers(-4, 5, (G, dim)).astype(np.float32), d_max=rng.integers(-4, 5, (G, dim)).astype(np.float32),
                 argmax=ref["argmax"], d_min=rng.integers(-4, 5, (G, dim)).astype(np.float32), argmin=ref["argmin"])
    dX = GNNA.segment_pool_backward(_dev(grads["d_sum"]), _dev(grads["d_max"]), amx, _dev(grads["d_min"]), amn, gpd, n, True)
    assert np.array_equal(dX.cpu().numpy(), pool_ref.backward(gp, n, dim, mean=True, **grads))
    dX = GNNA.segment_pool_backward(None, _dev(grads["d_max"]), amx, None, None, gpd, n, False)
    assert np.array_equal(dX.cpu().numpy(), pool_ref.backward(gp, n, dim, d_max=grads["d_max"], argmax=ref["argmax"]))


def test_one_captured_call_replayed_on_new_inputs():
    """torch.cuda.graph without stream=, as in test_capture_gpu.py: forward and backward in one graph, replayed twice on new
    input values; every output is NaN-filled before a replay and compared after it."""
    dim = 64
    n, gp = _layouts(dim)["three_tiles_and_5"]
    G = len(gp) - 1
    gpd = _dev(gp, torch.int32)
    X = torch.empty(n, dim, device="cuda")
    d_sum = torch.empty(G, dim, device="cuda")
    out = {k: torch.empty(G, dim, device="cuda") for k in ("sum", "max", "min")}
    out.update({k: torch.empty(G, dim, dtype=torch.int32, device="cuda") for k in ("argmax", "argmin")})
    dX = torch.empty(n, dim, device="cuda")

    def step():
        _lib.segment_pool(X, gpd, want=_lib.POOL_STATS, out=out)
        _lib.segment_pool_backward(gpd, n, d_sum=d_sum, d_max=out["max"], argmax=out["argmax"], mean=True, out=dX)

    X.copy_(_dev(_ints(n, dim, 0)))
    d_sum.fill_(1.0)
    if torch.cuda.graph.default_capture_stream is None:
        torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.graph.default_capture_stream):
        step()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    torch.cuda.synchronize()
    for seed in (1, 2):
        Xh = _ints(n, dim, seed)
        gh = np.random.default_rng(seed).integers(-4, 5, (G, dim)).astype(np.float32)
        X.copy_(_dev(Xh))
        d_sum.copy_(_dev(gh))
        for t in list(out.values()) + [dX]:
            t.fill_(NAN if t.dtype == torch.float32 else -(2 ** 31))
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        ref = pool_ref.forward(Xh, gp)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert np.array_equal(got["sum"], ref["sum"].astype(np.float32)), seed
        _check_extrema(got, ref)
        want = pool_ref.backward(gp, n, dim, d_sum=gh, d_max=ref["max"], argmax=ref["argmax"], mean=True)
        assert np.array_equal(dX.cpu().numpy(), want), seed

"""gnna_segment_moments_ld_f32 / gnna_segment_norm_ld_f32 / gnna_segment_norm_backward_ld_f32 on the GPU, through the C ABI
(_lib), against tests/segnorm_ref.py.

The statistics are held to the contract of include/gnna_segnorm.h, per segment with u = 2^-24 max|x|: |mean - mean64| <= 4 u and
|m2 / n - var64| <= 1e-5 var64 + 4 u sqrt(var64) -- the bounds the fp32 restatement is shown to keep in test_segnorm_host.py and a
sum of x^2 is shown to miss.  rstd is held to what those two bounds allow: var_t = m2 / n + (1 - alpha)^2 mean^2 may be off by
b = bound_var + (1 - alpha)^2 (2 |mean64| bound_mean + bound_mean^2) + 2^-22 var_t64 (the two statistics' bounds carried through the
formula, plus four roundings), so rstd lies between 1 / sqrt(var_t64 +- b + eps), widened by 2^-22 relative for the square root, the
division and the sum.  Everything else -- out, d_input, seg_a, seg_b -- is within 1e-4 * max(1, sum |terms|) of fp64, the sum of the
absolute values of the terms of that output's formula (segnorm_ref.graph_norm_f64).  A lane adds at most 256 rows in sequence and
the slots, pieces and wavefronts meet in trees, so the roundings of a sum stay far below 1600, the count at which that bound would
test the order of the additions.

Operands past 4 GiB: tests/test_segnorm_far_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import segnorm_ref
from gnnadvisor_osdi21_amd import _lib

pytestmark = pytest.mark.gpu

T = _lib.POOL_TILE_ROWS
DIMS = (1, 3, 4, 7, 41, 64, 100, 256, 260, 300)
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 600)            # in one batch; 600: three tiles
FIRST, LAST = 3, 4                                              # rows of no graph before p[0] and from p[G] on
NAN = float("nan")
EPS = 1e-5
WORST = {}                                                      # what -> the worst error / bound seen (printed by every test)


def _batch():
    gp = FIRST + np.r_[0, np.cumsum(SIZES)]
    return int(gp[-1]) + LAST, [int(v) for v in gp]


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _padded(rows, dim, pad):
    buf = torch.full((rows, dim + pad), NAN, device="cuda")
    return buf, buf[:, :dim]


def _params(dim, alpha, affine, seed=3):
    """(weight, bias, alpha) as float32 arrays or None.  alpha: None, 1, 0 or "0.37": 0.37 .. 0.43, a value per column."""
    rng = np.random.default_rng(seed)
    w = (1.0 + 0.5 * rng.standard_normal(dim)).astype(np.float32) if affine else None
    b = rng.standard_normal(dim).astype(np.float32) if affine else None
    a = None if alpha is None else (0.37 + 0.01 * (np.arange(dim) % 7) if alpha == "0.37" else np.full(dim, float(alpha))).astype(np.float32)
    return w, b, a


def _run(x, gp, w=None, b=None, a=None, dy=None, pad=3, need_input=True, eps=EPS):
    """The three entries through the C ABI with leading dimensions > dim on every operand but the parameters, every output
    NaN-filled first; checks that the columns from dim to the leading dimension are untouched."""
    n, dim = x.shape
    G = len(gp) - 1
    xbuf, xv = _padded(n, dim, pad)
    xv.copy_(_dev(x))
    gpd = _dev(gp, torch.int32)
    bufs, out = {}, {}
    for name, rows in (("mean", G), ("m2", G), ("out", n), ("mean_n", G), ("rstd", G), ("d_input", n), ("seg_a", G), ("seg_b", G)):
        bufs[name], out[name] = _padded(rows, dim, pad + (1 if name == "out" else 0))
    res = _lib.segment_moments(xv, gpd, out=dict(mean=out["mean"], m2=out["m2"]))
    assert res["mean"] is out["mean"] and res["m2"] is out["m2"]
    wd, bd, ad = _dev(w), _dev(b), _dev(a)
    res = _lib.segment_norm(xv, gpd, wd, bd, ad, eps, out=dict(out=out["out"], mean=out["mean_n"], rstd=out["rstd"]))
    assert res["out"] is out["out"]
    used = ["mean", "m2", "out", "mean_n", "rstd"]
    if dy is not None:
        dbuf, dv = _padded(n, dim, pad + 2)
        dv.copy_(_dev(dy))
        given = dict(seg_a=out["seg_a"], seg_b=out["seg_b"])
        if need_input:
            given["d_input"] = out["d_input"]
        dx, A, B = _lib.segment_norm_backward(dv, xv, out["mean_n"], out["rstd"], gpd, wd, ad, need_input=need_input, out=given)
        assert A is out["seg_a"] and B is out["seg_b"] and (dx is out["d_input"] if need_input else dx is None)
        used += ["seg_a", "seg_b"] + (["d_input"] if need_input else [])
    torch.cuda.synchronize()
    got = {}
    for name in used:
        assert bool(torch.isnan(bufs[name][:, dim:]).all()), f"{name}: written beyond dim"
        got[name] = out[name].cpu().numpy()
        assert not np.isnan(got[name]).any(), f"{name}: elements the call did not write"
    return got


def _note(what, err, bound):
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"{what}: worst err / bound {ratio:.4f}")
    assert (err <= bound).all(), f"{what}: worst err / bound {ratio:.3f}"


def _check_statistics(got, x, gp, a=None, eps=EPS, what=""):
    """mean and m2 / n against the contract; the norm entry's mean is the moments entry's; rstd within what the contract allows."""
    assert np.array_equal(got["mean"].view(np.uint32), got["mean_n"].view(np.uint32))
    n, dim = x.shape
    alpha = np.ones(dim) if a is None else a.astype(np.float64)
    for g, s, e in segnorm_ref.segments_of(gp, n):
        if e <= s:
            assert (got["mean"][g] == 0).all() and (got["m2"][g] == 0).all() and (got["rstd"][g] == 0).all(), g
            continue
        mean64, var64 = segnorm_ref.moments_f64(x[s:e])
        bound_mean, bound_var = segnorm_ref.statistics_bounds(x[s:e])
        assert (got["m2"][g] >= 0).all()
        _note(what + "mean", np.abs(got["mean"][g] - mean64), bound_mean)
        _note(what + "var", np.abs(got["m2"][g].astype(np.float64) / (e - s) - var64), bound_var)
        var_t = var64 + (1 - alpha) ** 2 * mean64 ** 2
        b = bound_var + (1 - alpha) ** 2 * (2 * np.abs(mean64) * bound_mean + bound_mean ** 2) + 2.0 ** -22 * var_t
        r64 = 1 / np.sqrt(var_t + eps)
        hi = 1 / np.sqrt(np.maximum(var_t - b, 0) + eps)
        lo = 1 / np.sqrt(var_t + b + eps)
        _note(what + "rstd", np.abs(got["rstd"][g] - r64), np.maximum(hi - r64, r64 - lo) + 2.0 ** -22 * r64)


@functools.lru_cache(maxsize=None)
def _case(dim, alpha, affine):
    """The batch of SIZES at this width with its fp64 reference, computed once."""
    n, gp = _batch()
    rng = np.random.default_rng(1000 + dim)
    x = (1.5 + rng.standard_normal((n, dim))).astype(np.float32)
    dy = rng.standard_normal((n, dim)).astype(np.float32)
    w, b, a = _params(dim, alpha, affine)
    return x, dy, gp, (w, b, a), segnorm_ref.graph_norm_f64(x, gp, w, b, a, EPS, dy)


def _check_rows(got, ref, what="", names=("out", "d_input", "seg_a", "seg_b")):
    for name in names:
        if name in got:
            _note(what + name, np.abs(got[name].astype(np.float64) - ref[name]), ref["bound_" + name])


def _no_graph_rows_are_zero(got, gp):
    for name in ("out", "d_input"):
        if name in got:
            assert (got[name][:max(gp[0], 0)] == 0).all() and (got[name][gp[-1]:] == 0).all(), name


@pytest.mark.parametrize("dim", DIMS)
def test_the_three_entries_against_fp64(dim):
    x, dy, gp, (w, b, a), ref = _case(dim, "0.37", True)
    got = _run(x, gp, w, b, a, dy)
    _check_statistics(got, x, gp, a)
    _check_rows(got, ref)
    _no_graph_rows_are_zero(got, gp)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("alpha", [None, 1, 0, "0.37"])
@pytest.mark.parametrize("dim", [41, 260])
def test_parameters_given_and_null(dim, alpha, affine):
    x, dy, gp, (w, b, a), ref = _case(dim, alpha, affine)
    got = _run(x, gp, w, b, a, dy)
    _check_statistics(got, x, gp, a)
    _check_rows(got, ref)
    # NULL is the default's value: the same bits as ones / zeros / ones handed over
    if alpha is None or not affine:
        ones, zeros = np.ones(dim, np.float32), np.zeros(dim, np.float32)
        full = _run(x, gp, ones if w is None else w, zeros if b is None else b, ones if a is None else a, dy)
        for name in ("out", "rstd", "d_input", "seg_a", "seg_b"):
            assert np.array_equal(got[name].view(np.uint32), full[name].view(np.uint32)), name
    # the one-row segment: with alpha = 1 the variance is 0, rstd = 1 / sqrt(eps) and out = bias, to the bit
    if alpha in (None, 1):
        g = SIZES.index(1)
        assert (got["m2"][g] == 0).all() and np.array_equal(got["mean"][g], x[gp[g]])
        assert (got["rstd"][g] == np.float32(1) / np.sqrt(np.float32(EPS))).all()
        assert np.array_equal(got["out"][gp[g]], np.zeros(dim, np.float32) if b is None else b)


def test_constant_columns():
    n, gp = _batch()
    dim = 7
    x = (1.5 + np.random.default_rng(8).standard_normal((n, dim))).astype(np.float32)
    x[:, 2], x[:, 5] = 3.25, -1000.5
    w, b, _ = _params(dim, None, True)
    got = _run(x, gp, w, b, None)
    for g, s, e in segnorm_ref.segments_of(gp, n):
        if e > s:
            assert (got["mean"][g][[2, 5]] == [3.25, -1000.5]).all() and (got["m2"][g][[2, 5]] == 0).all(), g
            assert (got["rstd"][g][[2, 5]] == np.float32(1) / np.sqrt(np.float32(EPS))).all()
            assert (got["out"][s:e, [2, 5]] == b[[2, 5]]).all()
    _check_statistics(got, x, gp)
    _check_rows(got, segnorm_ref.graph_norm_f64(x, gp, w, b, None, EPS))


@pytest.mark.parametrize("dim", [7, 64])
@pytest.mark.parametrize("offset", [1000.0, -3e4])
def test_offset_inputs_keep_the_tight_statistics_bounds(offset, dim):
    """The input of the contract: x = offset + 0.1 randn, where E[x^2] - E[x]^2 in fp32 misses var64 by its whole value and more
    (test_segnorm_host.py); the bounds here fail such a kernel."""
    n, gp = _batch()
    rng = np.random.default_rng(11)
    x = (offset + 0.1 * rng.standard_normal((n, dim))).astype(np.float32)
    dy = rng.standard_normal((n, dim)).astype(np.float32)
    w, b, a = _params(dim, "0.37", True)
    got = _run(x, gp, w, b, a, dy)
    _check_statistics(got, x, gp, a, what=f"offset {offset:g} ")
    _check_rows(got, segnorm_ref.graph_norm_f64(x, gp, w, b, a, EPS, dy), what=f"offset {offset:g} ")
    same = sum(int(np.array_equal(got["m2"][g], segnorm_ref.moments_f32(x[s:e], s)[1])) for g, s, e in segnorm_ref.segments_of(gp, n))
    print(f"segments whose m2 has the restatement's bits: {same} of {len(gp) - 1}")


def test_a_long_segment_goes_to_the_workgroup():
    dim = 64
    rows = segnorm_ref.long_segment_rows(dim)
    assert rows == _lib.POOL_LONG_STEPS * 4 * T + 300
    gp = [0, rows]
    rng = np.random.default_rng(12)
    x = (1000.0 + 0.1 * rng.standard_normal((rows, dim))).astype(np.float32)
    dy = rng.standard_normal((rows, dim)).astype(np.float32)
    w, b, a = _params(dim, "0.37", True)
    got = _run(x, gp, w, b, a, dy)
    _check_statistics(got, x, gp, a, what="long ")
    _check_rows(got, segnorm_ref.graph_norm_f64(x, gp, w, b, a, EPS, dy), what="long ")


@pytest.mark.parametrize("dim", [3, 100])
def test_a_column_slice_of_a_wider_tensor(dim):
    x, dy, gp, (w, b, a), ref = _case(dim, "0.37", True)
    n, G = x.shape[0], len(gp) - 1
    wide_x = torch.full((n, dim + 9), NAN, device="cuda")
    wide_out = torch.full((n, 2 * dim + 6), NAN, device="cuda")
    wide_x[:, 5: 5 + dim] = _dev(x)
    stats = torch.full((G, 2 * dim + 2), NAN, device="cuda")
    res = _lib.segment_norm(wide_x[:, 5: 5 + dim], _dev(gp, torch.int32), _dev(w), _dev(b), _dev(a), EPS,
                            out=dict(out=wide_out[:, dim + 3: 2 * dim + 3], mean=stats[:, 1: dim + 1], rstd=stats[:, dim + 2:]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide_out[:, :dim + 3]).all() and torch.isnan(wide_out[:, 2 * dim + 3:]).all())
    assert bool(torch.isnan(stats[:, 0]).all() and torch.isnan(stats[:, dim + 1]).all())
    plain = _run(x, gp, w, b, a)
    for name, key in (("out", "out"), ("mean", "mean_n"), ("rstd", "rstd")):
        assert np.array_equal(res[name].cpu().numpy().view(np.uint32), plain[key].view(np.uint32)), name


def test_pointers_are_clamped_and_a_descending_pair_is_an_empty_segment():
    n, dim = 50, 5
    rng = np.random.default_rng(13)
    x = (2.0 + rng.standard_normal((n, dim))).astype(np.float32)
    dy = rng.standard_normal((n, dim)).astype(np.float32)
    w, b, a = _params(dim, "0.37", True)
    gp = [-5, 20, 10, 10, 70]                                     # -> [0, 20), empty, empty, [10, 50): the statistics are defined
    assert [(s, e) for _, s, e in segnorm_ref.segments_of(gp, n)] == [(0, 20), (20, 20), (10, 10), (10, 50)]
    _check_statistics(_run(x, gp, w, b, a), x, gp, a)
    gp = [-5, 20, 20, 70]                                         # clamped pointers that do not descend: every output
    got = _run(x, gp, w, b, a, dy)
    _check_statistics(got, x, gp, a)
    _check_rows(got, segnorm_ref.graph_norm_f64(x, gp, w, b, a, EPS, dy))


def test_a_batch_without_graphs_and_one_without_rows():
    x = (1.0 + np.random.default_rng(1).standard_normal((40, 5))).astype(np.float32)
    got = _run(x, [7], dy=x)
    assert (got["out"] == 0).all() and (got["d_input"] == 0).all() and got["mean"].shape == (0, 5)
    got = _run(np.zeros((0, 5), np.float32), [0, 0, 0], dy=np.zeros((0, 5), np.float32))
    assert all((got[name] == 0).all() and got[name].shape == (2, 5) for name in ("mean", "m2", "rstd", "seg_a", "seg_b"))


def test_the_backward_without_d_input_gives_the_same_sums():
    x, dy, gp, (w, b, a), ref = _case(64, "0.37", True)
    both, sums = _run(x, gp, w, b, a, dy), _run(x, gp, w, b, a, dy, need_input=False)
    assert "d_input" not in sums
    for name in ("seg_a", "seg_b"):
        assert np.array_equal(both[name].view(np.uint32), sums[name].view(np.uint32)), name
    _check_rows(sums, ref)


@pytest.mark.parametrize("dim", [41, 64, 300])
def test_the_same_bits_on_two_runs_and_deterministic_tuning_accepts_the_calls(dim):
    x, dy, gp, (w, b, a), _ = _case(dim, "0.37", True)
    first = _run(x, gp, w, b, a, dy)
    try:
        _lib.set_tuning(deterministic=1)
        second = _run(x, gp, w, b, a, dy)
    finally:
        _lib.reset_tuning()
    for name in first:
        assert np.array_equal(first[name].view(np.uint32), second[name].view(np.uint32)), name
    rows = segnorm_ref.long_segment_rows(64)
    xl = np.random.default_rng(4).standard_normal((rows, 64)).astype(np.float32)
    one, two = _run(xl, [0, rows], dy=xl[::-1]), _run(xl, [0, rows], dy=xl[::-1])
    for name in one:
        assert np.array_equal(one[name].view(np.uint32), two[name].view(np.uint32)), name


def test_one_captured_forward_and_backward_replayed_on_new_inputs():
    """torch.cuda.graph without stream=, as in test_capture_gpu.py: forward and backward in one graph, replayed twice on new input
    values; every output is NaN-filled before a replay and compared with the eager call's bits after it."""
    dim = 64
    n, gp = _batch()
    G = len(gp) - 1
    gpd = _dev(gp, torch.int32)
    w, b, a = (_dev(t) for t in _params(dim, "0.37", True))
    X, dY = torch.empty(n, dim, device="cuda"), torch.empty(n, dim, device="cuda")
    out = dict(out=torch.empty(n, dim, device="cuda"), mean=torch.empty(G, dim, device="cuda"), rstd=torch.empty(G, dim, device="cuda"))
    bwd = dict(d_input=torch.empty(n, dim, device="cuda"), seg_a=torch.empty(G, dim, device="cuda"), seg_b=torch.empty(G, dim, device="cuda"))

    def step():
        _lib.segment_norm(X, gpd, w, b, a, EPS, out=out)
        _lib.segment_norm_backward(dY, X, out["mean"], out["rstd"], gpd, w, a, out=bwd)

    X.normal_()
    dY.normal_()
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
        rng = np.random.default_rng(seed)
        xh, gh = (seed + rng.standard_normal((n, dim))).astype(np.float32), rng.standard_normal((n, dim)).astype(np.float32)
        X.copy_(_dev(xh))
        dY.copy_(_dev(gh))
        for t in list(out.values()) + list(bwd.values()):
            t.fill_(NAN)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        replayed = {k: v.cpu().numpy().copy() for k, v in {**out, **bwd}.items()}
        eager = _run(xh, gp, *_params(dim, "0.37", True), gh, pad=0)
        for name, key in (("out", "out"), ("mean", "mean_n"), ("rstd", "rstd"), ("d_input", "d_input"), ("seg_a", "seg_a"), ("seg_b", "seg_b")):
            assert np.array_equal(replayed[name].view(np.uint32), eager[key].view(np.uint32)), (seed, name)
        _check_rows(replayed, segnorm_ref.graph_norm_f64(xh, gp, *_params(dim, "0.37", True), EPS, gh), what="replayed ")


def test_the_worst_ratios():
    """(last in the file: prints what the tests above measured, for profiles/graph_norm/README.md)"""
    for what in sorted(WORST):
        print(f"worst {what}: {WORST[what]:.4f}")

"""gnna_gather_rows_scale_ld_f32 / gnna_gather_rows_scale_backward_ld_f32 on the GPU, through the C ABI (_lib) and through GNNA,
against tests/topk_ref.py.

The forward and d_input are one fp32 multiplication per element and are compared exactly.  d_scale is a sum of `dim` products:
it is held within the project's bound for fp32 sums, 1e-4 * max(1, sum |terms|) of fp64 (a sum of 200 terms errs by at most
200 * 2^-24 = 1.2e-5 of sum |terms| in any order).  Rows: 0, 1, one more than a wavefront's step of every lane layout, and enough
for several workgroups."""
import numpy as np
import pytest
import torch

import far_offsets as F
import topk_ref
from gnnadvisor_osdi21_amd import _lib, load_extension

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 5, 63, 64, 65, 128, 200)
NAN = float("nan")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _padded(rows, width, pad):
    """A NaN-filled buffer [rows, width + pad] and its view [rows, width]."""
    buf = torch.full((rows, width + pad), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[:, :width]


def _slice_of(a, pad):
    """`a` as a column slice of a wider NaN-filled matrix."""
    buf = torch.full((a.shape[0], a.shape[1] + 2 * pad), NAN, dtype=torch.float32, device="cuda")
    view = buf[:, pad: pad + a.shape[1]]
    view.copy_(_dev(a))
    return view


def case(n, m, dim, seed):
    """X [n, dim], scale [n], a selection of m increasing rows with its new_id, and dY [m, dim]."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    scale = rng.standard_normal(n).astype(np.float32)
    perm = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int32) if m else np.zeros(0, dtype=np.int32)
    new_id = np.full(n, -1, dtype=np.int32)
    new_id[perm] = np.arange(m, dtype=np.int32)
    dY = rng.standard_normal((m, dim)).astype(np.float32)
    return X, scale, perm, new_id, dY


def _assert_d_scale(got, ref, terms, what):
    bound = 1e-4 * np.maximum(1.0, terms)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: worst |error| / bound = {(err / bound).max() if len(err) else 0.0:.3e}")
    assert np.all(err <= bound), what


@pytest.mark.parametrize("dim", DIMS)
def test_forward_and_backward_on_strided_views(dim):
    n, m = 1500, 700
    X, scale, perm, new_id, dY = case(n, m, dim, seed=dim)
    Xv, dYv = _slice_of(X, 3), _slice_of(dY, 2)
    sd, pd, nd = _dev(scale), _dev(perm), _dev(new_id)
    for use_scale in (True, False):
        s, s_np = (sd, scale) if use_scale else (None, None)
        buf, out = _padded(m, dim, 5)
        assert _lib.gather_rows_scale(Xv, pd, s, out=out) is out
        assert np.array_equal(out.cpu().numpy(), topk_ref.gather_rows_scale(X, perm, s_np))
        assert bool(torch.isnan(buf[:, dim:]).all())                              # columns past dim are not touched
        ref_dx, ref_ds, terms = topk_ref.gather_rows_scale_backward(dY, new_id, X, s_np)
        for need_input, need_scale in ((True, True), (True, False), (False, True)):
            dbuf, dx = _padded(n, dim, 4)
            ds = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
            got_dx, got_ds = _lib.gather_rows_scale_backward(dYv, nd, Xv if need_scale else None, s, need_input, need_scale,
                                                             out={"d_input": dx, "d_scale": ds})
            assert (got_dx is dx) == need_input and (got_ds is ds) == need_scale
            if need_input:
                assert np.array_equal(dx.cpu().numpy(), ref_dx) and bool(torch.isnan(dbuf[:, dim:]).all())
            else:
                assert bool(torch.isnan(dbuf).all())
            if need_scale:
                _assert_d_scale(ds.cpu().numpy(), ref_ds, terms, f"d_scale dim={dim} scale={use_scale}")
                assert bool((ds[_dev(new_id) < 0] == 0).all())
            else:
                assert bool(torch.isnan(ds).all())


@pytest.mark.parametrize("dim", (1, 5, 64, 200))
def test_the_module_agrees_bit_for_bit_with_the_c_abi(dim):
    GNNA = load_extension()
    X, scale, perm, new_id, dY = case(600, 250, dim, seed=100 + dim)
    Xd, sd, pd, nd, dYd = _dev(X), _dev(scale), _dev(perm), _dev(new_id), _dev(dY)
    assert torch.equal(GNNA.gather_rows_scale(Xd, pd, sd), _lib.gather_rows_scale(Xd, pd, sd))
    assert torch.equal(GNNA.gather_rows_scale(Xd, pd), _lib.gather_rows_scale(Xd, pd))
    dx, ds = GNNA.gather_rows_scale_backward(dYd, nd, Xd, sd, True, True)
    dx2, ds2 = _lib.gather_rows_scale_backward(dYd, nd, Xd, sd)
    assert torch.equal(dx, dx2) and torch.equal(ds, ds2) and tuple(ds.shape) == (600,)
    dx, ds = GNNA.gather_rows_scale_backward(dYd, nd, None, None, True, False)
    assert ds is None and torch.equal(dx, _lib.gather_rows_scale_backward(dYd, nd, need_scale=False)[0])


@pytest.mark.parametrize("rows", (1, 2, 17, 65, 257, 1025))
def test_row_counts_around_a_wavefronts_step(rows):
    for dim in (1, 4, 64):
        X, scale, perm, new_id, dY = case(rows + 3, rows, dim, seed=rows)
        out = _lib.gather_rows_scale(_dev(X), _dev(perm), _dev(scale))
        assert np.array_equal(out.cpu().numpy(), topk_ref.gather_rows_scale(X, perm, scale))
        dx, ds = _lib.gather_rows_scale_backward(_dev(dY), _dev(new_id), _dev(X), _dev(scale))
        ref_dx, ref_ds, terms = topk_ref.gather_rows_scale_backward(dY, new_id, X, scale)
        assert np.array_equal(dx.cpu().numpy(), ref_dx)
        _assert_d_scale(ds.cpu().numpy(), ref_ds, terms, f"d_scale rows={rows} dim={dim}")


def test_row_ids_out_of_range():
    n, m, dim = 40, 30, 7
    X, scale, _, _, dY = case(n, m, dim, seed=5)
    perm = np.arange(m, dtype=np.int32)
    perm[[0, 7, 29]] = [-1, n, 2 ** 31 - 1]
    out = _lib.gather_rows_scale(_dev(X), _dev(perm), _dev(scale)).cpu().numpy()
    assert np.array_equal(out, topk_ref.gather_rows_scale(X, perm, scale)) and np.all(out[[0, 7, 29]] == 0)
    new_id = np.arange(n, dtype=np.int32) % m
    new_id[[1, 2, 3, 39]] = [-1, m, 2 ** 31 - 1, -(2 ** 31)]
    dx, ds = _lib.gather_rows_scale_backward(_dev(dY), _dev(new_id), _dev(X), _dev(scale))
    ref_dx, ref_ds, terms = topk_ref.gather_rows_scale_backward(dY, new_id, X, scale)
    assert np.array_equal(dx.cpu().numpy(), ref_dx) and np.all(dx.cpu().numpy()[[1, 2, 3, 39]] == 0)
    _assert_d_scale(ds.cpu().numpy(), ref_ds, terms, "d_scale")
    assert np.all(ds.cpu().numpy()[[1, 2, 3, 39]] == 0)


def test_no_rows_selected_and_no_rows_at_all():
    X, scale, perm, new_id, dY = case(33, 0, 6, seed=9)
    assert tuple(_lib.gather_rows_scale(_dev(X), _dev(perm), _dev(scale)).shape) == (0, 6)
    dx, ds = _lib.gather_rows_scale_backward(torch.zeros(0, 6, device="cuda"), _dev(new_id), _dev(X), _dev(scale))
    assert tuple(dx.shape) == (33, 6) and bool((dx == 0).all()) and bool((ds == 0).all())
    GNNA = load_extension()
    dx, ds = GNNA.gather_rows_scale_backward(torch.zeros(0, 6, device="cuda"), _dev(new_id), _dev(X), _dev(scale), True, True)
    assert bool((dx == 0).all()) and bool((ds == 0).all())
    empty = torch.zeros(0, 6, device="cuda")
    assert tuple(_lib.gather_rows_scale(empty, torch.zeros(4, dtype=torch.int32, device="cuda")).shape) == (4, 6)
    assert bool((GNNA.gather_rows_scale(empty, torch.zeros(4, dtype=torch.int32, device="cuda")) == 0).all())
    assert tuple(GNNA.gather_rows_scale_backward(empty, torch.zeros(0, dtype=torch.int32, device="cuda"), None, None, True, False)[0].shape) == (0, 6)


@pytest.mark.parametrize("dim", (3, 64, 130))
def test_unpooling_equals_index_copy(dim):
    X, _, perm, new_id, dY = case(900, 400, dim, seed=20 + dim)
    got = _lib.gather_rows_scale_backward(_dev(dY), _dev(new_id), need_scale=False)[0]
    want = torch.zeros(900, dim, device="cuda").index_copy(0, _dev(perm).long(), _dev(dY))
    assert torch.equal(got, want)


def test_a_captured_call_replays_to_the_same_bits():
    n, m, dim = 3000, 1400, 64
    X, scale, perm, new_id, dY = case(n, m, dim, seed=31)
    Xd, sd, pd, nd, dYd = _dev(X), _dev(scale), _dev(perm), _dev(new_id), _dev(dY)
    out, dx = torch.empty(m, dim, device="cuda"), torch.empty(n, dim, device="cuda")
    ds = torch.empty(n, device="cuda")

    def both():
        _lib.gather_rows_scale(Xd, pd, sd, out=out)
        _lib.gather_rows_scale_backward(dYd, nd, Xd, sd, out={"d_input": dx, "d_scale": ds})

    both()
    eager = [t.clone() for t in (out, dx, ds)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            both()
    for rep in range(3):
        for t in (out, dx, ds):
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((out, dx, ds), eager)), f"replay {rep}"
    # ... and follows its inputs
    Xd.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, 2.0 * eager[0]) and torch.equal(dx, eager[1])


def test_deterministic_tuning_accepts_both_entries():
    X, scale, perm, new_id, dY = case(500, 200, 33, seed=41)
    args = (_dev(dY), _dev(new_id), _dev(X), _dev(scale))
    first = _lib.gather_rows_scale_backward(*args)
    try:
        _lib.set_tuning(deterministic=1)
        out = _lib.gather_rows_scale(_dev(X), _dev(perm), _dev(scale))
        again = _lib.gather_rows_scale_backward(*args)
    finally:
        _lib.reset_tuning()
    assert np.array_equal(out.cpu().numpy(), topk_ref.gather_rows_scale(X, perm, scale))
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---- rows whose byte offset passes 2^32 (the arena of tests/far_offsets.py) ---------------------------------------------------

@pytest.fixture(scope="module")
def arena():
    buf = torch.empty(F.ARENA_FLOATS, dtype=torch.float32, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def _ints(rows, width, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, (rows, width), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("dim, shift", [(5, 0), (64, 1)])
def test_rows_far_apart(arena, dim, shift):
    """Every operand with rows 64 MiB apart: row 64 starts 2^32 bytes, row 256 2^32 floats past the base.  Integer-valued data, so
    every product and every sum of d_scale is exact."""
    N = F.ROWS
    X = _ints(N, dim, 70 + dim) + torch.arange(N, dtype=torch.float32).unsqueeze(1)            # rows r and r mod m differ
    dY = _ints(N, dim, 80 + dim) + torch.arange(N, dtype=torch.float32).unsqueeze(1)            # (|sums| < 64 * 275^2 < 2^24)
    scale = _ints(N, 1, 90 + dim).reshape(-1)
    perm = torch.arange(N - 1, -1, -1, dtype=torch.int32)                                       # the far rows first
    new_id = torch.arange(N, dtype=torch.int32).flip(0).clone()
    new_id[[0, 100, 271]] = -1
    W = F.Windows(arena, shift)
    Xv, dYv = W.inp(X, what="X"), W.inp(dY, what="dY")
    out, dx = W.out("node", dim, what="out"), W.out("node", dim, what="d_input")
    assert Xv.stride(0) == F.LD and out.stride(0) == F.LD
    sd, pd, nd = scale.cuda(), perm.cuda(), new_id.cuda()
    _lib.gather_rows_scale(Xv, pd, sd, out=out)
    ds = torch.full((N,), NAN, device="cuda")
    _lib.gather_rows_scale_backward(dYv, nd, Xv, sd, out={"d_input": dx, "d_scale": ds})
    torch.cuda.synchronize()
    W.check()
    assert np.array_equal(out.cpu().numpy(), topk_ref.gather_rows_scale(X.numpy(), perm.numpy(), scale.numpy()))
    ref_dx, ref_ds, _ = topk_ref.gather_rows_scale_backward(dY.numpy(), new_id.numpy(), X.numpy(), scale.numpy())
    assert np.array_equal(dx.cpu().numpy(), ref_dx) and np.array_equal(ds.cpu().numpy().astype(np.float64), ref_ds)

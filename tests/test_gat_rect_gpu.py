"""gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32 through the C ABI, against the fp64 restatement on the
[num_out_rows x num_in_rows] structure (tests/gat_rect_ref.py: reference, magnitude sums, bounds, the kink rule).

Every call pre-fills its five outputs with NaN: an element the library does not write fails the comparison.  The tests are
built around the two tables of the contract (which bound holds for rows and which for ids in every pass, which array is indexed
by which): blocks have num_in_rows > num_out_rows, the wide-and-short structure the other way round, and ids planted between the
two counts would be gathered by a pass that took the wrong bound."""
import functools
import types

import numpy as np
import pytest
import torch

import gat_rect_ref as gref
import sampling_ref as sref
from gnnadvisor_osdi21_amd import _lib, graph
from util import assert_close_f64

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -3
NAN = float("nan")


def _structure(rp, ci, n_in, partSize):
    """Device structure, its partition, and the device-built transpose with its partition at the same partSize."""
    rp, ci = torch.as_tensor(rp, dtype=torch.int32), torch.as_tensor(ci, dtype=torch.int32)
    pp, p2n = _lib.build_part(partSize, rp)
    s = types.SimpleNamespace(rp=rp.cuda(), ci=ci.cuda(), pp=pp.cuda(), p2n=p2n.cuda(), n_out=rp.numel() - 1, n_in=int(n_in),
                              ps=partSize)
    s.t_rp, s.t_ci, _ = _lib.transpose_csr(s.rp, s.ci, num_in_rows=s.n_in, want_perm=False)
    s.t_pp, s.t_p2n = _lib.build_part_device(partSize, s.t_rp)
    return s


@functools.lru_cache(maxsize=None)
def _block(seeds, fanout):
    """(rp, ci, num_src) of the block of sampling_ref.seed_sets()[seeds] on the shared graph, from the numpy restatement of the
    sampling rule (the library's sampler is compared with it element for element in test_sampling_gpu.py)."""
    rp, ci = sref.shared_graph()
    b = sref.sample_block(rp, ci, sref.seed_sets()[seeds], fanout, 77)
    return b["row_pointers"].astype(np.int32), b["column_index"].astype(np.int32), len(b["src_nodes"])


def _ptr(t):
    return None if t is None else t.data_ptr()


def raw_forward(s, H, el, er, out, lse, heads, dim, slope=0.2, flags=0, square=False, ld_h=None, ld_out=None):
    sizes = (s.n_out,) if square else (s.n_out, s.n_in)
    entry = _lib.load().gnna_gat_forward_f32 if square else _lib.load().gnna_gat_forward_rect_f32
    return entry(_ptr(H), ld_h or heads * dim, _ptr(el), _ptr(er), _ptr(s.rp), _ptr(s.ci), _ptr(s.pp), _ptr(s.p2n), slope,
                 _ptr(out), ld_out or heads * dim, _ptr(lse), *sizes, heads, dim, s.p2n.numel(), s.ps, flags,
                 _lib._stream(s.rp.device))


def raw_backward(s, H, el, er, lse, Y, dY, dH, d_el, d_er, heads, dim, slope=0.2, flags=0, square=False, null_t=False, ld_h=None,
                 ld_y=None, ld_dy=None, ld_dh=None):
    W = heads * dim
    sizes = (s.n_out,) if square else (s.n_out, s.n_in)
    entry = _lib.load().gnna_gat_backward_dir_f32 if square else _lib.load().gnna_gat_backward_rect_f32
    t = (None, None, None, None) if null_t else (_ptr(s.t_rp), _ptr(s.t_ci), _ptr(s.t_pp), _ptr(s.t_p2n))
    return entry(_ptr(H), ld_h or W, _ptr(el), _ptr(er), _ptr(lse), _ptr(Y), ld_y or W, _ptr(dY), ld_dy or W, _ptr(s.rp), _ptr(s.ci),
                 _ptr(s.pp), _ptr(s.p2n), s.p2n.numel(), *t, s.t_p2n.numel(), slope, _ptr(dH), ld_dh or W, _ptr(d_el), _ptr(d_er),
                 *sizes, heads, dim, s.ps, flags, _lib._stream(s.rp.device))


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _run(s, H, el, er, G, heads, dim, slope, square=False):
    """Forward and backward into NaN-filled outputs -> (Y, lse, dH, d_el, d_er)."""
    W = heads * dim
    Y, lse, dH, d_el, d_er = _nan(s.n_out, W), _nan(s.n_out, heads), _nan(s.n_in, W), _nan(s.n_out, heads), _nan(s.n_in, heads)
    assert raw_forward(s, H, el, er, Y, lse, heads, dim, slope, square=square) == OK, _lib.load().gnna_last_error()
    assert raw_backward(s, H, el, er, lse, Y, G, dH, d_el, d_er, heads, dim, slope, square=square) == OK, _lib.load().gnna_last_error()
    return Y, lse, dH, d_el, d_er


def _compare(got, r, what):
    """The five outputs against kernel_reference's namespace: bounds of the module docstring of gat_rect_ref."""
    Y, lse, dH, d_el, d_er = got
    for t, name in zip(got, ("Y", "lse", "dH", "d_el", "d_er")):
        assert not torch.isnan(t).any(), f"{what}: {name} has elements the call did not write"
        assert torch.isfinite(t).all(), f"{what}: {name} is not finite"
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(Y), n(r.Y), rtol=1e-5, scale=n(r.s_Y), what=f"{what} Y")
    assert_close_f64(n(lse[r.has]), n(r.lse[r.has]), rtol=1e-5, what=f"{what} lse")
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (d_el[~r.has] == 0).all(), \
        f"{what}: rows without edges must give out = lse = d_el = 0"
    assert_close_f64(n(dH), n(r.dH), rtol=1e-5, scale=n(r.s_dH), what=f"{what} dH")
    assert_close_f64(n(d_el[r.ok_el]), n(r.d_el[r.ok_el]), rtol=1e-5, scale=n(r.s_el[r.ok_el]), what=f"{what} d_el")
    assert_close_f64(n(d_er[r.ok_er]), n(r.d_er[r.ok_er]), rtol=1e-5, scale=n(r.s_er[r.ok_er]), what=f"{what} d_er")
    assert (dH[~r.reached] == 0).all() and (d_er[~r.reached] == 0).all(), f"{what}: sources no edge reaches must get exactly 0"


def _case(rp, ci, n_in, heads, dim, partSize, seed, what, slope=0.2):
    s = _structure(rp, ci, n_in, partSize)
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, seed)]
    r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, slope, what)
    _compare(_run(s, H, el, er, G, heads, dim, slope), r, what)
    return s, r


CONFIGS = [(1, 64, 32), (4, 16, 32), (2, 41, 16), (8, 3, 1)]


@pytest.mark.parametrize("heads,dim,partSize", CONFIGS)
@pytest.mark.parametrize("seeds,fanout", [(65, 5), (1000, 5), (1, -1)])
def test_forward_and_backward_on_blocks(seeds, fanout, heads, dim, partSize):
    rp, ci, n_src = _block(seeds, fanout)
    s, r = _case(rp, ci, n_src, heads, dim, partSize, seed=seeds + heads * 10 + dim, what=f"block {seeds}/{fanout} {heads}x{dim}")
    assert s.n_in > s.n_out
    if seeds == 1:      # the hub: one destination row, the long-row path of the lse pass
        assert s.n_out == 1 and r.nnz == 10000 and s.n_in > 1000
    else:
        assert (~r.has).sum() >= 10                                   # seeds 20 .. 29 have no edges


@pytest.mark.parametrize("heads,dim", [(2, 16), (1, 64)])
def test_wide_and_short_structure(heads, dim):
    rp, ci = gref.wide_short_structure()
    s, r = _case(rp, ci, 300, heads, dim, 32, seed=heads + dim, what=f"700 x 300 {heads}x{dim}")
    assert s.n_out == 700 and s.n_in == 300 and int((~r.has).sum()) == 40 and int((~r.reached).sum()) == 20


@pytest.mark.parametrize("which", ["block", "wide"])
def test_out_of_range_ids_are_skipped_in_every_pass(which):
    """Ids >= num_in_rows (among them ids below num_out_rows on the wide structure, and 2^31 - 1, and -1) in the forward
    structure; the transposed structure is the device-built one, which drops them.  The reference has those edges removed."""
    if which == "block":
        rp, ci, n_in = _block(65, 5)
    else:
        (rp, ci), n_in = gref.wide_short_structure(), 300
    bad = gref.plant_out_of_range(ci, n_in)
    assert ((bad < 0) | (bad >= n_in)).sum() >= len(ci) // 10
    s, r = _case(rp, bad, n_in, 2, 16, 32, seed=5, what=f"out-of-range ids, {which}")
    assert r.nnz < len(ci) and int(s.t_rp[-1]) == r.nnz


def test_leading_dimensions():
    """H, out (= Y), dY and dH as column blocks of wider buffers: the floats around them keep their fill value."""
    heads, dim, W = 2, 41, 82
    rp, ci, n_src = _block(65, 5)
    s = _structure(rp, ci, n_src, 32)
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 3)]
    r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, "ld")
    hbuf = torch.full((s.n_in, W + 7), 7.5, device="cuda")
    hbuf[:, 3:3 + W] = H
    obuf, gbuf, dbuf = _nan(s.n_out, 2 * W + 4), torch.full((s.n_out, W + 5), -2.0, device="cuda"), _nan(s.n_in, W + 9)
    obuf[:, :W + 4] = -3.25
    gbuf[:, 5:] = G
    dbuf[:, :5] = 1.75
    dbuf[:, 5 + W:] = 1.75
    Hv, out, dY, dH = hbuf[:, 3:3 + W], obuf[:, W + 4:], gbuf[:, 5:], dbuf[:, 5:5 + W]
    lse, d_el, d_er = _nan(s.n_out, heads), _nan(s.n_out, heads), _nan(s.n_in, heads)
    assert raw_forward(s, Hv, el, er, out, lse, heads, dim, ld_h=W + 7, ld_out=2 * W + 4) == OK
    assert raw_backward(s, Hv, el, er, lse, out, dY, dH, d_el, d_er, heads, dim, ld_h=W + 7, ld_y=2 * W + 4, ld_dy=W + 5,
                        ld_dh=W + 9) == OK
    _compare((out, lse, dH, d_el, d_er), r, "leading dimensions")
    assert (obuf[:, :W + 4] == -3.25).all() and (dbuf[:, :5] == 1.75).all() and (dbuf[:, 5 + W:] == 1.75).all()
    assert (hbuf[:, :3] == 7.5).all() and (hbuf[:, 3 + W:] == 7.5).all() and (gbuf[:, :5] == -2.0).all()
    # the same views through the wrapper, which takes the sizes and the strides from the tensors
    out2, lse2 = _lib.gat_forward(Hv, el, er, s.rp, s.ci, s.pp, s.p2n, 32, 0.2)
    assert out2.shape == (s.n_out, W) and torch.equal(lse2, lse)
    dH2, d_el2, d_er2 = _lib.gat_backward(Hv, el, er, lse2, out2, dY, s.rp, s.ci, s.pp, s.p2n, 32, 0.2,
                                          transposed=(s.t_rp, s.t_ci, s.t_pp, s.t_p2n))
    assert dH2.shape == (s.n_in, W) and d_el2.shape == (s.n_out, heads) and d_er2.shape == (s.n_in, heads)
    _compare((out2, lse2, dH2, d_el2, d_er2), r, "leading dimensions (wrapper)")
    with pytest.raises(_lib.GnnaError, match="transposed"):
        _lib.gat_backward(Hv, el, er, lse2, out2, dY, s.rp, s.ci, s.pp, s.p2n, 32, 0.2)


@pytest.mark.parametrize("heads,dim", [(4, 16), (2, 41)])
def test_square_and_rect_entries_agree(heads, dim):
    """A square (symmetric or not: the transpose is given) graph through gnna_gat_forward_f32 / gnna_gat_backward_dir_f32 and
    through the rect entries with both counts equal.  lse has one writer per row and a fixed order: the same bits.  The other
    outputs are sums of float atomics of the same kernels with the same arguments: each within the kernel bound of fp64, and of
    each other."""
    g = graph.powerlaw_graph(1500, 40000, 900, seed=heads)
    s = _structure(g.row_pointers, g.column_index, g.num_nodes, 32)
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 11)]
    r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, "square")
    sq = _run(s, H, el, er, G, heads, dim, 0.2, square=True)
    rect = _run(s, H, el, er, G, heads, dim, 0.2)
    _compare(sq, r, "square entries")
    _compare(rect, r, "rect entries, equal counts")
    assert torch.equal(sq[1], rect[1]), "lse must have the same bits from both entries"
    for a, b, scale, name in zip((sq[0], sq[2], sq[3], sq[4]), (rect[0], rect[2], rect[3], rect[4]),
                                 (r.s_Y, r.s_dH, r.s_el, r.s_er), ("Y", "dH", "d_el", "d_er")):
        assert_close_f64(a.cpu().numpy(), b.double().cpu().numpy(), rtol=1e-5, scale=scale.cpu().numpy(), what=f"square vs rect {name}")


def _bare(rp, ci, n_in, partSize=32):
    """A structure whose transpose has no edges (one of its sides has no rows): no transposed arrays, t_num_parts = 0."""
    rp, ci = torch.tensor(rp, dtype=torch.int32), torch.tensor(ci, dtype=torch.int32)
    pp, p2n = _lib.build_part(partSize, rp)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    return types.SimpleNamespace(rp=rp.cuda(), ci=ci.cuda(), pp=pp.cuda(), p2n=p2n.cuda(), n_out=rp.numel() - 1, n_in=n_in,
                                 ps=partSize, t_rp=none, t_ci=none, t_pp=none, t_p2n=none)


def test_a_side_without_rows():
    """num_in_rows = 0: out, lse, d_el are zero-filled and no input is read; num_out_rows = 0: dH and d_er are."""
    heads, dim, W = 2, 4, 8
    s = _bare([0, 2, 2, 3], [0, 1, 0], 0)
    out, lse, d_el = _nan(3, W), _nan(3, heads), _nan(3, heads)
    assert raw_forward(s, None, None, None, out, lse, heads, dim) == OK
    assert raw_backward(s, None, None, None, None, None, None, None, d_el, None, heads, dim) == OK
    assert (out == 0).all() and (lse == 0).all() and (d_el == 0).all()
    s = _bare([0], [], 5)
    dH, d_er = _nan(5, W), _nan(5, heads)
    assert raw_forward(s, None, None, None, None, None, heads, dim) == OK
    assert raw_backward(s, None, None, None, None, None, None, dH, None, d_er, heads, dim) == OK
    assert (dH == 0).all() and (d_er == 0).all()


def test_errors_are_those_of_the_square_entries():
    rp, ci, n_src = _block(65, 5)
    rect = _structure(rp, ci, n_src, 32)
    g = graph.uniform_graph(200, 1500, seed=2)
    square = _structure(g.row_pointers, g.column_index, g.num_nodes, 32)
    lib = _lib.load()

    def statuses(s, is_square, heads, dim, flags=0, null_t=False):
        W = heads * dim
        H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 1)]
        Y, lse = torch.zeros(s.n_out, W, device="cuda"), torch.zeros(s.n_out, heads, device="cuda")
        dH, d_el, d_er = _nan(s.n_in, W), _nan(s.n_out, heads), _nan(s.n_in, heads)
        f = raw_forward(s, H, el, er, Y, lse, heads, dim, flags=flags, square=is_square)
        b = raw_backward(s, H, el, er, lse, Y, G, dH, d_el, d_er, heads, dim, flags=flags, square=is_square, null_t=null_t)
        return f, b, lib.gnna_last_error().decode()

    for kw, want in ((dict(heads=2, dim=4, flags=_lib.ACCUMULATE), UNSUPPORTED), (dict(heads=65, dim=1), UNSUPPORTED),
                     (dict(heads=1, dim=257), UNSUPPORTED)):
        assert statuses(square, True, **kw)[:2] == (want, want), kw
        assert statuses(rect, False, **kw)[:2] == (want, want), kw
    before = _lib.get_tuning()
    try:
        _lib.set_tuning(deterministic=1)
        for s, is_square in ((square, True), (rect, False)):
            f, b, msg = statuses(s, is_square, 2, 4)
            assert (f, b) == (UNSUPPORTED, UNSUPPORTED) and "deterministic" in msg
    finally:
        _lib.reset_tuning()
    assert _lib.get_tuning() == before
    for s, is_square in ((square, True), (rect, False)):
        f, b, msg = statuses(s, is_square, 2, 4, null_t=True)
        assert (f, b) == (OK, INVALID) and "null index pointer" in msg
    assert "gnna_gat_backward_rect_f32" in statuses(rect, False, 2, 4, null_t=True)[2]
    assert lib.gnna_version() == 601

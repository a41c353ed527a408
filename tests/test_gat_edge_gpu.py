"""gnna_gat_edge_forward_f32 / gnna_gat_edge_backward_f32 / gnna_gat_alpha_f32 (include/gnna_gat_edge.h) through the C ABI,
against the fp64 restatement over the edge list with positions (tests/gat_edge_ref.py: reference, magnitude sums, bounds, the
kink rule).  Every call pre-fills its outputs with NaN: an element the library does not write fails the comparison.

Inputs: gat_rect_ref.wide_short_structure() (700 x 300, 8,908 edges, a 5,000-edge hub row for the long-row path of the lse
pass, 40 rows without edges, 20 unreached sources, duplicate edges), gat_rect_ref.inputs(seed=7) and ee = randn(8908, heads) of
seed 9.  Bounds: 1e-5 * max(1, sum of |terms|) per element; alpha 1e-5 absolute (alpha <= 1, and the fp32 error of the
exponent's argument at |z| < 8 is below 1e-6)."""
import functools

import pytest
import torch

import gat_edge_ref as eref
import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib, graph
from test_gat_rect_gpu import _nan, _ptr, _structure
from util import assert_close_f64

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -3
N_IN = 300


def _with_perm(s):
    """_structure's transpose is built without its permutation: the same builder once more, with it (the same bits)."""
    t_rp, t_ci, perm = _lib.transpose_csr(s.rp, s.ci, num_in_rows=s.n_in, want_perm=True)
    assert torch.equal(t_rp, s.t_rp) and torch.equal(t_ci, s.t_ci)
    s.perm = perm
    s.nnz = s.ci.numel()
    return s


def _ee(nnz, heads):
    return torch.randn(nnz, heads, generator=torch.Generator().manual_seed(9)).cuda()


def raw_forward(s, H, el, er, ee, out, lse, heads, dim, slope=0.2, p=0.0, seed=0, flags=0, ld_h=None, ld_out=None, nnz=None):
    return _lib.load().gnna_gat_edge_forward_f32(
        _ptr(H), ld_h or heads * dim, _ptr(el), _ptr(er), _ptr(ee), _ptr(s.rp), _ptr(s.ci), _ptr(s.pp), _ptr(s.p2n), slope, p, seed,
        _ptr(out), ld_out or heads * dim, _ptr(lse), s.n_out, s.n_in, s.nnz if nnz is None else nnz, heads, dim, s.p2n.numel(), s.ps,
        flags, _lib._stream(s.rp.device))


def raw_backward(s, H, el, er, ee, lse, Y, dY, dH, d_el, d_er, d_ee, heads, dim, slope=0.2, p=0.0, seed=0, flags=0, t=None,
                 t_edge_pos="perm", ld_h=None, ld_y=None, ld_dy=None, ld_dh=None, nnz=None):
    W = heads * dim
    t = (s.t_rp, s.t_ci, s.t_pp, s.t_p2n) if t is None else t
    tpos = s.perm if isinstance(t_edge_pos, str) else t_edge_pos
    return _lib.load().gnna_gat_edge_backward_f32(
        _ptr(H), ld_h or W, _ptr(el), _ptr(er), _ptr(ee), _ptr(lse), _ptr(Y), ld_y or W, _ptr(dY), ld_dy or W, _ptr(s.rp), _ptr(s.ci),
        _ptr(s.pp), _ptr(s.p2n), s.p2n.numel(), *[_ptr(x) for x in t], t[3].numel(), _ptr(tpos), slope, p, seed, _ptr(dH),
        ld_dh or W, _ptr(d_el), _ptr(d_er), _ptr(d_ee), s.n_out, s.n_in, s.nnz if nnz is None else nnz, heads, dim, s.ps, flags,
        _lib._stream(s.rp.device))


def raw_alpha(s, el, er, ee, lse, alpha, heads, slope=0.2):
    return _lib.load().gnna_gat_alpha_f32(_ptr(el), _ptr(er), _ptr(ee), _ptr(lse), _ptr(s.rp), _ptr(s.ci), slope, _ptr(alpha),
                                          s.n_out, s.n_in, s.nnz, heads, _lib._stream(s.rp.device))


def _run(s, H, el, er, ee, G, heads, dim, slope=0.2, p=0.0, seed=0, **bw):
    """Forward, alpha and backward into NaN-filled outputs -> (Y, lse, alpha, dH, d_el, d_er, d_ee)."""
    W = heads * dim
    Y, lse, alpha = _nan(s.n_out, W), _nan(s.n_out, heads), _nan(s.nnz, heads)
    dH, d_el, d_er, d_ee = _nan(s.n_in, W), _nan(s.n_out, heads), _nan(s.n_in, heads), _nan(s.nnz, heads)
    err = lambda: _lib.load().gnna_last_error()
    assert raw_forward(s, H, el, er, ee, Y, lse, heads, dim, slope, p, seed) == OK, err()
    assert raw_alpha(s, el, er, ee, lse, alpha, heads, slope) == OK, err()
    assert raw_backward(s, H, el, er, ee, lse, Y, G, dH, d_el, d_er, d_ee, heads, dim, slope, p, seed, **bw) == OK, err()
    return Y, lse, alpha, dH, d_el, d_er, d_ee


def _compare(got, r, what):
    """The seven outputs against gat_edge_ref.kernel_reference's namespace."""
    Y, lse, alpha, dH, d_el, d_er, d_ee = got
    for t, name in zip(got, ("Y", "lse", "alpha", "dH", "d_el", "d_er", "d_ee")):
        assert not torch.isnan(t).any(), f"{what}: {name} has elements the call did not write"
        assert torch.isfinite(t).all(), f"{what}: {name} is not finite"
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(Y), n(r.Y), rtol=1e-5, scale=n(r.s_Y), what=f"{what} Y")
    assert_close_f64(n(lse[r.has]), n(r.lse[r.has]), rtol=1e-5, what=f"{what} lse")
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (d_el[~r.has] == 0).all(), \
        f"{what}: rows without edges must give out = lse = d_el = 0"
    err = (alpha.double() - r.alpha).abs().max().item()
    print(f"{what}: max |alpha - ref| = {err:.3e}")
    assert err <= 1e-5, f"{what} alpha: max err {err:.3e}"
    assert_close_f64(n(dH), n(r.dH), rtol=1e-5, scale=n(r.s_dH), what=f"{what} dH")
    assert_close_f64(n(d_el[r.ok_el]), n(r.d_el[r.ok_el]), rtol=1e-5, scale=n(r.s_el[r.ok_el]), what=f"{what} d_el")
    assert_close_f64(n(d_er[r.ok_er]), n(r.d_er[r.ok_er]), rtol=1e-5, scale=n(r.s_er[r.ok_er]), what=f"{what} d_er")
    assert_close_f64(n(d_ee[r.ok_ee]), n(r.d_ee[r.ok_ee]), rtol=1e-5, scale=n(r.s_ee[r.ok_ee]), what=f"{what} d_ee")
    assert (dH[~r.reached] == 0).all() and (d_er[~r.reached] == 0).all(), f"{what}: sources no edge reaches must get exactly 0"
    skipped = torch.ones(alpha.shape[0], dtype=torch.bool, device=alpha.device)
    skipped[r.pos] = False
    assert (alpha[skipped] == 0).all() and (d_ee[skipped] == 0).all(), f"{what}: a skipped edge's alpha and d_ee rows must be 0"


@functools.lru_cache(maxsize=None)
def _wide(partSize, planted):
    rp, ci = gref.wide_short_structure()
    if planted:
        ci = gref.plant_out_of_range(ci, N_IN)
    return _with_perm(_structure(rp, ci, N_IN, partSize))


def _inputs(s, heads, dim):
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 7)]
    return H, el, er, _ee(s.nnz, heads), G


# widths, with the partSizes 1 / 3 / 32 and planted out-of-range ids spread over them
CONFIGS = [(1, 64, 32, False), (4, 16, 3, True), (3, 7, 1, False), (8, 64, 32, True), (1, 1, 3, False)]


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["plain", "drop"])
@pytest.mark.parametrize("heads,dim,partSize,planted", CONFIGS)
def test_all_outputs_against_fp64(heads, dim, partSize, planted, p):
    s = _wide(partSize, planted)
    assert s.nnz == 8908 and s.n_out == 700
    H, el, er, ee, G = _inputs(s, heads, dim)
    what = f"{heads}x{dim} ps{partSize}{' planted' if planted else ''} p={p}"
    r = eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, 0.2, p, 0xABCDEF, what=what)
    assert r.excluded == 0 and (r.nnz < s.nnz) == planted
    _compare(_run(s, H, el, er, ee, G, heads, dim, 0.2, p, 0xABCDEF), r, what)


@pytest.mark.parametrize("heads,dim,partSize", [(4, 16, 32), (1, 64, 3)])
def test_positions_line_up_in_all_three_passes(heads, dim, partSize):
    """ee = -40 on every third position of column_index, 0 elsewhere, negative_slope = 1 (the score is z itself, so -40 in the
    score is a factor exp(-40) on the edge's weight).  Within a row el is fixed and |er| < 4, so a suppressed edge weighs less
    than exp(-40 + 8) ~ 1e-14 of any other edge of its row: Y, dH, d_el and d_er equal the fp64 attention of gat_rect_ref (no
    edge term at all) over the remaining edges only.  A pass that read ee at another position than the one it gathers would
    drop a live edge and keep a suppressed one.  A row ALL of whose edges are suppressed (a row of one edge can be) keeps them:
    a shift of every score of a row leaves its softmax as it was."""
    s = _wide(partSize, False)
    H, el, er, _, G = _inputs(s, heads, dim)
    assert er.abs().max().item() < 4.0
    ee = torch.zeros(s.nnz, heads, device="cuda")
    ee[::3] = -40.0
    rows = eref.edges_with_positions(s.rp, s.ci, N_IN)[0]
    sup = torch.zeros(s.nnz, dtype=torch.bool, device="cuda")
    sup[::3] = True
    has_live = torch.zeros(s.n_out, dtype=torch.bool, device="cuda")
    has_live[rows[~sup]] = True
    gone = sup & has_live[rows]                              # the edges that leave the function
    assert int(gone.sum()) > s.nnz // 4 and int((sup & ~gone).sum()) > 0
    ci_rest = s.ci.clone()
    ci_rest[gone] = N_IN + 1                                 # out of range: gat_rect_ref leaves them out
    r = gref.kernel_reference(H, el, er, G, s.rp, ci_rest, heads, 1.0, "the remaining edges")
    Y, lse, alpha, dH, d_el, d_er, d_ee = _run(s, H, el, er, ee, G, heads, dim, slope=1.0)
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(Y), n(r.Y), rtol=1e-5, scale=n(r.s_Y), what="remaining edges: Y")
    assert_close_f64(n(dH), n(r.dH), rtol=1e-5, scale=n(r.s_dH), what="remaining edges: dH")
    assert_close_f64(n(d_el), n(r.d_el), rtol=1e-5, scale=n(r.s_el), what="remaining edges: d_el")
    assert_close_f64(n(d_er), n(r.d_er), rtol=1e-5, scale=n(r.s_er), what="remaining edges: d_er")
    # |dz| <= alpha (|dalpha| + |c|) <= alpha (absdot + crow[i]): the scale of d_ee at alpha = 1
    Gh, Hh = G.double().view(-1, heads, dim), H.double().view(-1, heads, dim)
    absdot = (Gh[rows].abs() * Hh[s.ci.long()].abs()).sum(-1)
    crow = (Gh.abs() * r.s_Y.view(-1, heads, dim)).sum(-1)
    scale = (absdot + crow[rows]).clamp(min=1.0)
    print(f"suppressed: max alpha {alpha[gone].max().item():.3e}, max |d_ee| / scale {(d_ee[gone].abs() / scale[gone]).max().item():.3e}")
    assert alpha[gone].max().item() <= 1e-12
    assert ((d_ee[gone].abs().double() / scale[gone]) <= 1e-12).all()


def test_zero_edge_term_is_the_plain_attention():
    """ee = 0: the five outputs of gat_rect_ref's reference, which has no edge term; and gnna_gat_alpha_f32 with ee = NULL gives
    the alpha of the call with ee = 0."""
    heads, dim = 4, 16
    s = _wide(32, True)
    H, el, er, _, G = _inputs(s, heads, dim)
    ee = torch.zeros(s.nnz, heads, device="cuda")
    r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, "ee = 0")
    Y, lse, alpha, dH, d_el, d_er, d_ee = _run(s, H, el, er, ee, G, heads, dim)
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(Y), n(r.Y), rtol=1e-5, scale=n(r.s_Y), what="ee = 0 Y")
    assert_close_f64(n(lse[r.has]), n(r.lse[r.has]), rtol=1e-5, what="ee = 0 lse")
    assert_close_f64(n(dH), n(r.dH), rtol=1e-5, scale=n(r.s_dH), what="ee = 0 dH")
    assert_close_f64(n(d_el[r.ok_el]), n(r.d_el[r.ok_el]), rtol=1e-5, scale=n(r.s_el[r.ok_el]), what="ee = 0 d_el")
    assert_close_f64(n(d_er[r.ok_er]), n(r.d_er[r.ok_er]), rtol=1e-5, scale=n(r.s_er[r.ok_er]), what="ee = 0 d_er")
    plain = _nan(s.nnz, heads)
    assert raw_alpha(s, el, er, None, lse, plain, heads) == OK, _lib.load().gnna_last_error()
    e = eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, 0.2, what="ee = 0")
    err = (plain.double() - e.alpha).abs().max().item()
    print(f"alpha with ee = NULL: max err {err:.3e}")
    assert err <= 1e-5 and not torch.isnan(plain).any()
    assert torch.equal(plain, alpha)
    # and through the wrappers, which take the sizes from the tensors
    Y2, lse2 = _lib.gat_edge_forward(H, el, er, ee, s.rp, s.ci, s.pp, s.p2n, s.ps, 0.2)
    assert torch.equal(lse2, lse)
    assert torch.equal(_lib.gat_alpha(el, er, None, lse2, s.rp, s.ci, 0.2), alpha)
    assert_close_f64(n(Y2), n(r.Y), rtol=1e-5, scale=n(r.s_Y), what="ee = 0 Y (wrapper)")
    # (Y is an input of the backward: the same Y, the same d_ee -- the forward's own sums are added in no fixed order)
    out = _lib.gat_edge_backward(H, el, er, ee, lse2, Y, G, s.rp, s.ci, s.pp, s.p2n, s.perm, s.ps, 0.2,
                                 transposed=(s.t_rp, s.t_ci, s.t_pp, s.t_p2n))
    assert torch.equal(out[3], d_ee) and out[3].shape == (s.nnz, heads)


@functools.lru_cache(maxsize=None)
def _symmetric():
    g = graph.powerlaw_graph(1500, 40000, 900, seed=4)
    s = _with_perm(_structure(g.row_pointers, g.column_index, g.num_nodes, 32))
    s.rev = _lib.reverse_edges(g.row_pointers, g.column_index).cuda()
    assert s.nnz <= 40000
    return s


@pytest.mark.parametrize("how", ["own structure + reverse-edge map", "transpose + perm"])
def test_symmetric_graph_both_ways(how):
    heads, dim = 4, 16
    s = _symmetric()
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 7)]
    ee = _ee(s.nnz, heads)
    r = eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, 0.2, what=how)
    bw = dict(t=(s.rp, s.ci, s.pp, s.p2n), t_edge_pos=s.rev) if how.startswith("own") else {}
    _compare(_run(s, H, el, er, ee, G, heads, dim, **bw), r, how)


def test_out_of_range_edge_positions_are_skipped_in_the_source_side_pass():
    """t_edge_pos with values outside [0, num_edges) planted: those transposed edges are missing from d_er and dH only -- d_el,
    d_ee and the forward do not read t_edge_pos."""
    heads, dim = 4, 16
    s = _wide(32, False)
    H, el, er, ee, G = _inputs(s, heads, dim)
    tpos = s.perm.clone()
    where = torch.arange(5, s.nnz, 11, device="cuda")
    lost = tpos[where].long()                               # the forward positions whose transposed edge is skipped
    tpos[where] = torch.tensor([s.nnz, -1, 2 ** 31 - 1, s.nnz + 9], dtype=torch.int32, device="cuda").repeat(len(where) // 4 + 1)[:len(where)]
    t_skip = torch.zeros(s.nnz, dtype=torch.bool, device="cuda")
    t_skip[lost] = True
    r = eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, 0.2, t_skip=t_skip, what="planted t_edge_pos")
    _compare(_run(s, H, el, er, ee, G, heads, dim, t_edge_pos=tpos), r, "planted t_edge_pos")


def test_d_ee_is_the_same_bits_on_every_run():
    heads, dim = 8, 64
    s = _wide(32, True)
    H, el, er, ee, G = _inputs(s, heads, dim)
    Y, lse, alpha, _, _, _, first = _run(s, H, el, er, ee, G, heads, dim, p=0.5, seed=3)
    # the same inputs, Y among them (the forward adds its sums in no fixed order: another forward is another Y)
    dH, d_el, d_er, second = _nan(s.n_in, heads * dim), _nan(s.n_out, heads), _nan(s.n_in, heads), _nan(s.nnz, heads)
    assert raw_backward(s, H, el, er, ee, lse, Y, G, dH, d_el, d_er, second, heads, dim, p=0.5, seed=3) == OK
    assert torch.equal(first, second) and first.abs().max().item() > 0
    # lse and alpha have one writer per element too
    lse2, alpha2 = _nan(s.n_out, heads), _nan(s.nnz, heads)
    assert raw_forward(s, H, el, er, ee, _nan(s.n_out, heads * dim), lse2, heads, dim, p=0.5, seed=3) == OK
    assert raw_alpha(s, el, er, ee, lse2, alpha2, heads) == OK
    assert torch.equal(lse, lse2) and torch.equal(alpha, alpha2)


def test_accumulate_means_for_d_ee_what_it_means_for_the_other_gradients():
    """GNNA_ACCUMULATE is refused by the backward entries of the fused attention (their gradients are zero-filled and added to
    with atomics); d_ee follows: the call is refused before any device work and d_ee keeps its fill."""
    heads, dim = 2, 8
    s = _wide(32, False)
    H, el, er, ee, G = _inputs(s, heads, dim)
    Y, lse = _nan(s.n_out, heads * dim), _nan(s.n_out, heads)
    assert raw_forward(s, H, el, er, ee, Y, lse, heads, dim) == OK
    dH, d_el, d_er, d_ee = _nan(s.n_in, heads * dim), _nan(s.n_out, heads), _nan(s.n_in, heads), torch.full((s.nnz, heads), 2.5, device="cuda")
    assert raw_backward(s, H, el, er, ee, lse, Y, G, dH, d_el, d_er, d_ee, heads, dim, flags=_lib.ACCUMULATE) == UNSUPPORTED
    assert b"GNNA_ACCUMULATE" in _lib.load().gnna_last_error()
    assert (d_ee == 2.5).all() and torch.isnan(d_el).all()
    assert raw_forward(s, H, el, er, ee, Y, lse, heads, dim, flags=_lib.ACCUMULATE) == UNSUPPORTED


def test_strided_rows():
    """H, out (= Y), dY and dH as column blocks of wider buffers: the floats around them keep their fill value."""
    heads, dim, W = 3, 7, 21
    s = _wide(3, False)
    H, el, er, ee, G = _inputs(s, heads, dim)
    r = eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, 0.2, what="ld")
    hbuf = torch.full((s.n_in, W + 7), 7.5, device="cuda")
    hbuf[:, 3:3 + W] = H
    obuf, gbuf, dbuf = _nan(s.n_out, 2 * W + 4), torch.full((s.n_out, W + 5), -2.0, device="cuda"), _nan(s.n_in, W + 9)
    obuf[:, :W + 4] = -3.25
    gbuf[:, 5:] = G
    dbuf[:, :5] = 1.75
    dbuf[:, 5 + W:] = 1.75
    Hv, out, dY, dH = hbuf[:, 3:3 + W], obuf[:, W + 4:], gbuf[:, 5:], dbuf[:, 5:5 + W]
    lse, d_el, d_er, d_ee, alpha = _nan(s.n_out, heads), _nan(s.n_out, heads), _nan(s.n_in, heads), _nan(s.nnz, heads), _nan(s.nnz, heads)
    assert raw_forward(s, Hv, el, er, ee, out, lse, heads, dim, ld_h=W + 7, ld_out=2 * W + 4) == OK
    assert raw_alpha(s, el, er, ee, lse, alpha, heads) == OK
    assert raw_backward(s, Hv, el, er, ee, lse, out, dY, dH, d_el, d_er, d_ee, heads, dim, ld_h=W + 7, ld_y=2 * W + 4, ld_dy=W + 5,
                        ld_dh=W + 9) == OK
    _compare((out, lse, alpha, dH, d_el, d_er, d_ee), r, "leading dimensions")
    assert (obuf[:, :W + 4] == -3.25).all() and (dbuf[:, :5] == 1.75).all() and (dbuf[:, 5 + W:] == 1.75).all()
    assert (hbuf[:, :3] == 7.5).all() and (hbuf[:, 3 + W:] == 7.5).all() and (gbuf[:, :5] == -2.0).all()
    # the same views through the wrappers
    out2, lse2 = _lib.gat_edge_forward(Hv, el, er, ee, s.rp, s.ci, s.pp, s.p2n, s.ps, 0.2)
    got = _lib.gat_edge_backward(Hv, el, er, ee, lse2, out2, dY, s.rp, s.ci, s.pp, s.p2n, s.perm, s.ps, 0.2,
                                 transposed=(s.t_rp, s.t_ci, s.t_pp, s.t_p2n))
    _compare((out2, lse2, _lib.gat_alpha(el, er, ee, lse2, s.rp, s.ci, 0.2), *got), r, "leading dimensions (wrappers)")

"""gnna_gatv2_forward_f32 / gnna_gatv2_backward_f32 through the C ABI (include/gnna_gatv2.h) against the fp64 restatement of
tests/gatv2_ref.py: out, lse, dHs, dHd, d_att (and Y again as the backward's input).

Structures: gat_rect_ref.wide_short_structure() -- 700 x 300 with a 5,000-edge hub row (the long-row path of the lse pass and a
run that spans several 64-id loads), duplicate edges, 40 rows without edges and 20 sources no edge reaches -- as it is and with
ids outside the source rows planted; a small symmetric square graph passed as its own transpose; a directed square graph with
the device-built transpose.  partSize 3 and 32: a row's groups straddle the wavefronts of a workgroup and workgroups.
Shapes: 8 of the 28 lane layouts -- LPH = 1 (64 x 1) to 64 (1 x 256), dim % 4 != 0, rows wider than one wave-wide load (8 x 40:
column blocks of whole heads); tests/test_attn_layouts_gpu.py runs every layout.
Bounds: 1e-5 * max(1, sum of |terms|) * max(1, S) (gatv2_ref's docstring); elements of dHs / dHd with an edge at the kink of the
leaky ReLU are excluded, nothing of d_att or the forward is.  Every call pre-fills its outputs with NaN, so an element the
library does not write fails the comparison.  The seeds: gatv2_ref.inputs under seeds 5 .. 12 was checked on the CPU in fp64
to have no element at the kink except 3 x 5 (seed 7), which has a few; kernel_reference asserts the cap either way."""
import functools

import numpy as np
import pytest
import torch

import gat_rect_ref as gref
import gatv2_ref as vref
from gnnadvisor_osdi21_amd import _lib, graph, load_extension
from test_gat_rect_gpu import _bare, _nan, _ptr, _structure
from util import assert_close_f64

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -3
SEED = 0x1234
SLOPE = 0.2
# (heads, dim): seed of the inputs
SEEDS = {(1, 64): 5, (4, 16): 6, (3, 5): 7, (8, 8): 8, (1, 256): 9, (64, 1): 10, (2, 33): 11, (8, 40): 12}


def raw_forward(s, Hs, Hd, att, out, lse, heads, dim, p=0.0, rng_seed=SEED, flags=0, ld_hs=None, ld_hd=None, ld_out=None):
    W = heads * dim
    return _lib.load().gnna_gatv2_forward_f32(
        _ptr(Hs), ld_hs or W, _ptr(Hd), ld_hd or W, _ptr(att), _ptr(s.rp), _ptr(s.ci), _ptr(s.pp), _ptr(s.p2n), SLOPE, p, rng_seed,
        _ptr(out), ld_out or W, _ptr(lse), s.n_out, s.n_in, heads, dim, s.p2n.numel(), s.ps, flags, _lib._stream(s.rp.device))


def raw_backward(s, Hs, Hd, att, lse, Y, dY, dHs, dHd, d_att, heads, dim, p=0.0, rng_seed=SEED, flags=0, own_transpose=False,
                 lds=None):
    W = heads * dim
    ld = dict(hs=W, hd=W, y=W, dy=W, dhs=W, dhd=W)
    ld.update(lds or {})
    t = (s.rp, s.ci, s.pp, s.p2n) if own_transpose else (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    return _lib.load().gnna_gatv2_backward_f32(
        _ptr(Hs), ld["hs"], _ptr(Hd), ld["hd"], _ptr(att), _ptr(lse), _ptr(Y), ld["y"], _ptr(dY), ld["dy"], _ptr(s.rp), _ptr(s.ci),
        _ptr(s.pp), _ptr(s.p2n), s.p2n.numel(), *[_ptr(x) for x in t], t[3].numel(), SLOPE, p, rng_seed, _ptr(dHs), ld["dhs"],
        _ptr(dHd), ld["dhd"], _ptr(d_att), s.n_out, s.n_in, heads, dim, s.ps, flags, _lib._stream(s.rp.device))


def _err():
    return _lib.load().gnna_last_error()


def _run(s, Hs, Hd, att, G, heads, dim, p=0.0, rng_seed=SEED, own_transpose=False):
    """Forward and backward into NaN-filled outputs -> (Y, lse, dHs, dHd, d_att)."""
    W = heads * dim
    Y, lse, dHs, dHd, d_att = _nan(s.n_out, W), _nan(s.n_out, heads), _nan(s.n_in, W), _nan(s.n_out, W), _nan(heads, dim)
    assert raw_forward(s, Hs, Hd, att, Y, lse, heads, dim, p, rng_seed) == OK, _err()
    assert raw_backward(s, Hs, Hd, att, lse, Y, G, dHs, dHd, d_att, heads, dim, p, rng_seed, own_transpose=own_transpose) == OK, _err()
    return Y, lse, dHs, dHd, d_att


def _compare(got, r, what):
    """The five outputs against kernel_reference's namespace: the bounds of gatv2_ref's docstring."""
    Y, lse, dHs, dHd, d_att = got
    for t, name in zip(got, ("Y", "lse", "dHs", "dHd", "d_att")):
        assert not torch.isnan(t).any(), f"{what}: {name} has elements the call did not write"
        assert torch.isfinite(t).all(), f"{what}: {name} is not finite"
    n = lambda t: t.cpu().numpy()
    rtol = 1e-5 * r.factor
    assert_close_f64(n(Y), n(r.Y), rtol=rtol, scale=n(r.s_Y), what=f"{what} Y")
    assert_close_f64(n(lse[r.has]), n(r.lse[r.has]), rtol=rtol, what=f"{what} lse")
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (dHd[~r.has] == 0).all(), \
        f"{what}: rows without edges must give out = lse = dHd = 0"
    assert_close_f64(n(dHs[r.ok_dHs]), n(r.dHs[r.ok_dHs]), rtol=rtol, scale=n(r.s_dHs[r.ok_dHs]), what=f"{what} dHs")
    assert_close_f64(n(dHd[r.ok_dHd]), n(r.dHd[r.ok_dHd]), rtol=rtol, scale=n(r.s_dHd[r.ok_dHd]), what=f"{what} dHd")
    assert_close_f64(n(d_att), n(r.d_att), rtol=rtol, scale=n(r.s_att), what=f"{what} d_att")
    assert (dHs[~r.reached] == 0).all(), f"{what}: sources no edge reaches must get exactly 0"


@functools.lru_cache(maxsize=None)
def _wide(partSize=32, planted=False):
    rp, ci = gref.wide_short_structure()
    return _structure(rp, gref.plant_out_of_range(ci, 300) if planted else ci, 300, partSize)


@functools.lru_cache(maxsize=None)
def _wide_case(heads, dim, planted, p):
    """Inputs on the device and their fp64 reference on the wide-short structure: computed once, shared, never written."""
    s = _wide(32, planted)
    Hs, Hd, att, G = [t.cuda() for t in vref.inputs(s.n_out, s.n_in, heads, dim, SEEDS[heads, dim])]
    r = vref.kernel_reference(Hs, Hd, att, G, s.rp, s.ci, heads, SLOPE, p, SEED, f"700 x 300 {heads}x{dim} planted={planted} p={p}")
    return Hs, Hd, att, G, r


# ---- 1. the six outputs ------------------------------------------------------------------------------------------------------

# every shape on the plain and on the planted structure; partSize 3 and 32 alternate over them
CASES = [(h, d, ps, planted) for k, (h, d) in enumerate(SEEDS) for planted, ps in ((False, (32, 3)[k % 2]), (True, (3, 32)[k % 2]))]


@pytest.mark.parametrize("heads,dim,partSize,planted", CASES)
def test_outputs_against_fp64(heads, dim, partSize, planted):
    s = _wide(partSize, planted)
    Hs, Hd, att, G, r = _wide_case(heads, dim, planted, 0.0)
    what = f"700 x 300 {heads}x{dim} partSize={partSize} planted={planted}"
    if planted:
        assert r.nnz < int(s.rp[-1]) and int(s.t_rp[-1]) == r.nnz
    assert int((~r.has).sum()) >= 40 and int((~r.reached).sum()) >= 20
    if (heads, dim) == (3, 5):
        assert 0 < r.excluded_dHs + r.excluded_dHd <= 8          # (one (i, j) pair at the kink, repeated by the hub row's duplicates)
    else:
        assert r.excluded_dHs == 0 and r.excluded_dHd == 0
    _compare(_run(s, Hs, Hd, att, G, heads, dim), r, what)


@pytest.mark.parametrize("heads,dim,partSize,planted", [(1, 64, 3, False), (4, 16, 32, True), (3, 5, 3, False), (8, 40, 32, False),
                                                        (64, 1, 3, True)])
def test_outputs_with_the_mask(heads, dim, partSize, planted):
    """attn_drop = 0.5 against the restated mask of gat_drop_ref; lse is that of the undropped scores."""
    s = _wide(partSize, planted)
    Hs, Hd, att, G, r = _wide_case(heads, dim, planted, 0.5)
    assert 0 < int((r.k > 0).sum()) < r.k.numel()
    got = _run(s, Hs, Hd, att, G, heads, dim, 0.5, SEED)
    _compare(got, r, f"700 x 300 {heads}x{dim} partSize={partSize} planted={planted} p=0.5")
    plain = _wide_case(heads, dim, planted, 0.0)[4]
    assert_close_f64(got[1][r.has].cpu().numpy(), plain.lse[r.has].cpu().numpy(), rtol=1e-5 * r.factor, what="lse with the mask")
    other = _run(s, Hs, Hd, att, G, heads, dim, 0.5, SEED + 1)
    assert not torch.equal(other[0], got[0]) and torch.equal(other[1], got[1])       # another mask, the same lse


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim,partSize", [(4, 16, 32), (3, 5, 3), (1, 256, 32)])
def test_lse_bits_and_a_backward_called_twice(heads, dim, partSize):
    s = _wide(partSize, False)
    Hs, Hd, att, G, r = _wide_case(heads, dim, False, 0.0)
    W = heads * dim
    Y, lse, dHs, dHd, d_att = _run(s, Hs, Hd, att, G, heads, dim, 0.0, SEED)
    # lse: one writer per (row, head), a fixed order: the same bits on every run, and with attn_drop = 0 whatever the seed
    Y2, lse2 = _nan(s.n_out, W), _nan(s.n_out, heads)
    assert raw_forward(s, Hs, Hd, att, Y2, lse2, heads, dim, 0.0, SEED) == OK, _err()
    assert torch.equal(lse2, lse)
    Y3, lse3 = _nan(s.n_out, W), _nan(s.n_out, heads)
    assert raw_forward(s, Hs, Hd, att, Y3, lse3, heads, dim, 0.0, SEED + 99) == OK, _err()
    assert torch.equal(lse3, lse)
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(Y3), n(r.Y), rtol=1e-5 * r.factor, scale=n(r.s_Y), what="attn_drop = 0 with another seed")
    # the backward again, into the same buffers: nothing (a partial of d_att, the scratch) is carried over from the first call
    first = d_att.clone()
    assert raw_backward(s, Hs, Hd, att, lse, Y, G, dHs, dHd, d_att, heads, dim, 0.0, SEED) == OK, _err()
    _compare((Y, lse, dHs, dHd, d_att), r, "the backward called twice")
    assert_close_f64(n(d_att), n(first.double()), rtol=2e-5 * r.factor, scale=n(r.s_att), what="d_att of the second call")


# ---- 3. row strides -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim", [(2, 33), (8, 8)])
def test_row_strides_larger_than_the_width(heads, dim):
    s = _wide(3, True)
    Hs0, Hd0, att, G0, r = _wide_case(heads, dim, True, 0.0)
    W = heads * dim

    def padded(t, pad, fill):
        buf = torch.full((t.shape[0], W + pad), fill, device="cuda")
        buf[:, 1:1 + W] = t
        return buf, buf[:, 1:1 + W]

    (hs_b, Hs), (hd_b, Hd), (g_b, G) = padded(Hs0, 3, 7.5), padded(Hd0, 6, -1.5), padded(G0, 2, 2.5)
    (y_b, Y), (dhs_b, dHs), (dhd_b, dHd) = padded(_nan(s.n_out, W), 5, 3.25), padded(_nan(s.n_in, W), 4, 3.25), padded(_nan(s.n_out, W), 7, 3.25)
    lse, d_att = _nan(s.n_out, heads), _nan(heads, dim)
    assert raw_forward(s, Hs, Hd, att, Y, lse, heads, dim, ld_hs=W + 3, ld_hd=W + 6, ld_out=W + 5) == OK, _err()
    assert raw_backward(s, Hs, Hd, att, lse, Y, G, dHs, dHd, d_att, heads, dim,
                        lds=dict(hs=W + 3, hd=W + 6, y=W + 5, dy=W + 2, dhs=W + 4, dhd=W + 7)) == OK, _err()
    _compare((Y, lse, dHs, dHd, d_att), r, f"strided rows {heads}x{dim}")
    for buf in (y_b, dhs_b, dhd_b):
        assert (buf[:, 0] == 3.25).all() and (buf[:, 1 + W:] == 3.25).all(), "written outside the rows"
    assert (hs_b[:, 0] == 7.5).all() and (hd_b[:, 1 + W:] == -1.5).all() and (g_b[:, 0] == 2.5).all()


# ---- 4. square structures -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim,p", [(4, 16, 0.0), (3, 5, 0.5)])
def test_a_symmetric_graph_as_its_own_transpose_with_hs_is_hd(heads, dim, p):
    """The source-side pass reads row j's edges as the edges j -> i; Hs and Hd are one pointer (shared weights)."""
    g = graph.powerlaw_graph(500, 8000, 300, seed=4)
    s = _structure(g.row_pointers, g.column_index, g.num_nodes, 32)
    rows, cl = gref.edges_of(g.row_pointers, g.column_index, g.num_nodes)
    assert torch.equal((rows * g.num_nodes + cl).sort().values, (cl * g.num_nodes + rows).sort().values)      # symmetric
    H, _, att, G = [t.cuda() for t in vref.inputs(s.n_out, s.n_in, heads, dim, SEEDS[heads, dim])]
    r = vref.kernel_reference(H, H, att, G, s.rp, s.ci, heads, SLOPE, p, SEED, "symmetric")
    _compare(_run(s, H, H, att, G, heads, dim, p, SEED, own_transpose=True), r, "symmetric, structure given twice, Hs is Hd")
    _compare(_run(s, H, H, att, G, heads, dim, p, SEED), r, "symmetric, device-built transpose, Hs is Hd")


@pytest.mark.parametrize("heads,dim,p", [(2, 33, 0.0), (8, 8, 0.5)])
def test_a_directed_square_graph(heads, dim, p):
    rng = np.random.default_rng(5)
    n = 600
    deg = rng.integers(0, 30, size=n)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n, size=rp[-1])
    s = _structure(rp, ci, n, 3)                                      # gnna_transpose_csr_i32 + gnna_build_part_device_i32
    assert not torch.equal(s.t_rp, s.rp)
    Hs, Hd, att, G = [t.cuda() for t in vref.inputs(n, n, heads, dim, SEEDS[heads, dim])]
    r = vref.kernel_reference(Hs, Hd, att, G, s.rp, s.ci, heads, SLOPE, p, SEED, "directed")
    _compare(_run(s, Hs, Hd, att, G, heads, dim, p, SEED), r, "directed square graph")


def test_a_side_without_rows():
    """num_in_rows = 0: out, lse, dHd and d_att are zero-filled and no input is read; num_out_rows = 0: dHs and d_att are."""
    heads, dim, W = 2, 4, 8
    s = _bare([0, 2, 2, 3], [0, 1, 0], 0)
    out, lse, dHd, d_att = _nan(3, W), _nan(3, heads), _nan(3, W), _nan(heads, dim)
    assert raw_forward(s, None, None, None, out, lse, heads, dim, 0.5) == OK, _err()
    assert raw_backward(s, None, None, None, None, None, None, None, dHd, d_att, heads, dim, 0.5) == OK, _err()
    assert (out == 0).all() and (lse == 0).all() and (dHd == 0).all() and (d_att == 0).all()
    s = _bare([0], [], 5)
    dHs, d_att = _nan(5, W), _nan(heads, dim)
    assert raw_forward(s, None, None, None, None, None, heads, dim, 0.5) == OK, _err()
    assert raw_backward(s, None, None, None, None, None, None, dHs, None, d_att, heads, dim, 0.5) == OK, _err()
    assert (dHs == 0).all() and (d_att == 0).all()


# ---- 5. flags, refusals on the device, and the two bindings ----------------------------------------------------------------------

def test_relu_epilogue_and_refusals():
    heads, dim = 4, 16
    s = _wide(32, False)
    Hs, Hd, att, G, r = _wide_case(heads, dim, False, 0.0)
    W = heads * dim
    Y, lse = _nan(s.n_out, W), _nan(s.n_out, heads)
    assert raw_forward(s, Hs, Hd, att, Y, lse, heads, dim, flags=_lib.EPILOGUE_RELU) == OK, _err()
    n = lambda t: t.cpu().numpy()
    assert (Y >= 0).all() and bool((r.Y < 0).any())
    assert_close_f64(n(Y), n(r.Y.clamp(min=0)), rtol=1e-5 * r.factor, scale=n(r.s_Y), what="ReLU epilogue")
    dHs, dHd, d_att = _nan(s.n_in, W), _nan(s.n_out, W), _nan(heads, dim)
    for bad in (-0.1, 1.0, float("nan")):
        assert raw_forward(s, Hs, Hd, att, Y, lse, heads, dim, bad) == INVALID and b"gnna_gatv2_forward_f32: attn_drop" in _err()
        assert raw_backward(s, Hs, Hd, att, lse, Y, G, dHs, dHd, d_att, heads, dim, bad) == INVALID
        assert b"gnna_gatv2_backward_f32: attn_drop" in _err()
    assert raw_backward(s, Hs, Hd, att, lse, Y, G, dHs, dHd, d_att, heads, dim, flags=_lib.ACCUMULATE) == UNSUPPORTED
    try:
        _lib.set_tuning(deterministic=1)
        assert raw_forward(s, Hs, Hd, att, Y, lse, heads, dim) == UNSUPPORTED and b"deterministic" in _err()
        assert raw_backward(s, Hs, Hd, att, lse, Y, G, dHs, dHd, d_att, heads, dim) == UNSUPPORTED
    finally:
        _lib.reset_tuning()
    for t in (dHs, dHd, d_att):
        assert torch.isnan(t).all(), "a refused call must not write"
    assert _lib.load().gnna_version() == 601


@pytest.mark.parametrize("kind", ["square", "directed", "rectangular"])
def test_both_bindings_agree(kind):
    """One small case through _lib.gatv2_* (strided inputs and outputs) and GNNAdvisor.gatv2_*: each within the kernel bound of
    fp64; lse has one writer per (row, head) and must have the same bits."""
    GNNA = load_extension()
    PS, heads, dim = 2, 2, 3
    W = heads * dim
    rp, ci = {"square": ([0, 5, 6, 7, 8, 9, 9], [0, 1, 2, 3, 4, 0, 0, 0, 0]),
              "directed": ([0, 5, 6, 8, 9, 10, 10], [0, 1, 2, 3, 4, 0, 0, 3, 0, 0]),
              "rectangular": ([0, 5, 5, 7], [0, 1, 2, 3, 5, 4, 0])}[kind]
    s = _structure(rp, ci, 6, PS)
    Hs0, Hd, att, G0 = [t.cuda() for t in vref.inputs(s.n_out, s.n_in, heads, dim, seed=11)]
    Hbuf, Gbuf = torch.full((s.n_in, W + 3), 7.5, device="cuda"), torch.full((s.n_out, W + 5), -2.0, device="cuda")
    Hbuf[:, 1:1 + W], Gbuf[:, 3:3 + W] = Hs0, G0
    Hs, G = Hbuf[:, 1:1 + W], Gbuf[:, 3:3 + W]
    p, seed = 0.5, 2 ** 64 - 3                                         # (a seed above 2^63: unsigned all the way down)
    r = vref.kernel_reference(Hs, Hd, att, G, s.rp, s.ci, heads, SLOPE, p, seed, kind)
    transposed = None if kind == "square" else (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    graph_ = (s.rp, s.ci, s.pp, s.p2n, PS, SLOPE, p, seed)
    Y, lse = _lib.gatv2_forward(Hs, Hd, att, *graph_)
    got = _lib.gatv2_backward(Hs, Hd, att, lse, Y, G, *graph_, transposed=transposed)
    _compare((Y, lse, *got), r, f"{kind} _lib")
    obuf, dbuf = torch.full((s.n_out, W + 4), 3.25, device="cuda"), torch.full((s.n_in, W + 4), 3.25, device="cuda")
    Y2, lse2 = _lib.gatv2_forward(Hs, Hd, att, *graph_, out=obuf[:, 2:2 + W])
    got2 = _lib.gatv2_backward(Hs, Hd, att, lse2, Y2, G, *graph_, transposed=transposed, dHs=dbuf[:, 2:2 + W])
    _compare((Y2, lse2, *got2), r, f"{kind} _lib, strided outputs")
    for buf in (obuf, dbuf):
        assert (buf[:, :2] == 3.25).all() and (buf[:, 2 + W:] == 3.25).all()
    Ym, lsem = GNNA.gatv2_forward(Hs, Hd, att, *graph_)
    gotm = GNNA.gatv2_backward(Hs, Hd, att, lsem, Ym, G, *graph_, None if transposed is None else list(transposed))
    _compare((Ym, lsem, *gotm), r, f"{kind} GNNAdvisor")
    assert torch.equal(lsem, lse) and torch.equal(lse2, lse)
    assert (Hbuf[:, 0] == 7.5).all() and (Hbuf[:, 1 + W:] == 7.5).all() and (Gbuf[:, :3] == -2.0).all()
    with pytest.raises(_lib.GnnaError, match="attn_drop"):
        _lib.gatv2_forward(Hs, Hd, att, s.rp, s.ci, s.pp, s.p2n, PS, SLOPE, 1.0, seed)
    with pytest.raises(RuntimeError, match="attn_drop"):
        GNNA.gatv2_forward(Hs, Hd, att, s.rp, s.ci, s.pp, s.p2n, PS, SLOPE, 1.0, seed)

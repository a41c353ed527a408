"""gnna_gat_forward_drop_f32 / gnna_gat_backward_drop_f32 through the C ABI (include/gnna_ext.h): the mask against its
restatement edge for edge, and the five outputs against the fp64 reference with the mask (tests/gat_drop_ref.py).

Inputs: gat_rect_ref.inputs(..., seed=7) on gat_rect_ref.wide_short_structure() -- 700 x 300 with a 5,000-edge hub row (the
long-row lse path), duplicate edges, 40 rows without edges and 20 sources no edge reaches.  Bounds are those of
test_gat_rect_gpu.py (its `_compare`): 1e-5 of max(1, sum of |terms|), with the kink rule of gat_rect_ref.  Every call pre-fills
its outputs with NaN, so an element the library does not write fails the comparison."""
import functools

import numpy as np
import pytest
import torch

import gat_drop_ref as dref
import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib, graph, load_extension
from test_gat_rect_gpu import _bare, _compare, _nan, _ptr, _structure

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -3
SEED = 0x1234
WIDTHS = [(1, 64), (4, 16), (3, 7), (8, 64), (1, 1)]       # (8, 64): a 512-float row, two column blocks of whole heads


def raw_forward(s, H, el, er, out, lse, heads, dim, p, rng_seed, slope=0.2, flags=0, ld_h=None, ld_out=None):
    return _lib.load().gnna_gat_forward_drop_f32(
        _ptr(H), ld_h or heads * dim, _ptr(el), _ptr(er), _ptr(s.rp), _ptr(s.ci), _ptr(s.pp), _ptr(s.p2n), slope, p, rng_seed,
        _ptr(out), ld_out or heads * dim, _ptr(lse), s.n_out, s.n_in, heads, dim, s.p2n.numel(), s.ps, flags, _lib._stream(s.rp.device))


def raw_backward(s, H, el, er, lse, Y, dY, dH, d_el, d_er, heads, dim, p, rng_seed, slope=0.2, flags=0, own_transpose=False):
    W = heads * dim
    t = (s.rp, s.ci, s.pp, s.p2n) if own_transpose else (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    return _lib.load().gnna_gat_backward_drop_f32(
        _ptr(H), W, _ptr(el), _ptr(er), _ptr(lse), _ptr(Y), W, _ptr(dY), W, _ptr(s.rp), _ptr(s.ci), _ptr(s.pp), _ptr(s.p2n),
        s.p2n.numel(), *[_ptr(x) for x in t], t[3].numel(), slope, p, rng_seed, _ptr(dH), W, _ptr(d_el), _ptr(d_er), s.n_out, s.n_in,
        heads, dim, s.ps, flags, _lib._stream(s.rp.device))


def _run(s, H, el, er, G, heads, dim, p, rng_seed, slope=0.2, own_transpose=False):
    """Forward and backward into NaN-filled outputs -> (Y, lse, dH, d_el, d_er)."""
    W = heads * dim
    Y, lse, dH, d_el, d_er = _nan(s.n_out, W), _nan(s.n_out, heads), _nan(s.n_in, W), _nan(s.n_out, heads), _nan(s.n_in, heads)
    assert raw_forward(s, H, el, er, Y, lse, heads, dim, p, rng_seed, slope) == OK, _lib.load().gnna_last_error()
    assert raw_backward(s, H, el, er, lse, Y, G, dH, d_el, d_er, heads, dim, p, rng_seed, slope, own_transpose=own_transpose) == OK, \
        _lib.load().gnna_last_error()
    return Y, lse, dH, d_el, d_er


@functools.lru_cache(maxsize=None)
def _wide(partSize=32, planted=False):
    rp, ci = gref.wide_short_structure()
    return _structure(rp, gref.plant_out_of_range(ci, 300) if planted else ci, 300, partSize)


def _compare_drop(got, r, what):
    _compare(got, r, what)
    Y, _lse, _dH, d_el, _d_er = got
    heads = r.none_kept.shape[1]
    none = r.none_kept
    assert (Y.view(Y.shape[0], heads, -1)[none] == 0).all() and (d_el[none] == 0).all(), \
        f"{what}: a (row, head) whose edges are all dropped must give out = 0 and d_el = 0"


# ---- 1. the mask, edge for edge ---------------------------------------------------------------------------------------------

def _kept_counts(s, heads, dim, rng_seed, p=0.5):
    """H = 1, el = er = 0: alpha = 1 / deg(i) on every edge, so out[i, h, f] * deg(i) / 2 is the number of kept edges of (i, h)."""
    H = torch.ones(s.n_in, heads * dim, device="cuda")
    el, er = torch.zeros(s.n_out, heads, device="cuda"), torch.zeros(s.n_in, heads, device="cuda")
    out, lse = _nan(s.n_out, heads * dim), _nan(s.n_out, heads)
    assert raw_forward(s, H, el, er, out, lse, heads, dim, p, rng_seed) == OK, _lib.load().gnna_last_error()
    deg = (s.rp[1:] - s.rp[:-1]).double()
    x = out.double().view(s.n_out, heads, dim) * deg[:, None, None] / 2
    counts = x.round()
    assert (x - counts).abs().max() < 0.1 and (counts == counts[:, :, :1]).all(), "not a count, or not the same for every feature"
    assert (lse[deg > 0].double() - torch.log(deg[deg > 0])[:, None]).abs().max() < 1e-5 and (lse[deg == 0] == 0).all(), \
        "lse is that of the undropped scores"
    return counts[:, :, 0].long().cpu()


@pytest.mark.parametrize("heads,dim", WIDTHS)
def test_the_mask_is_the_restated_one_for_every_row_and_head(heads, dim):
    s = _wide()
    rows, cl = gref.edges_of(s.rp.cpu(), s.ci.cpu(), s.n_in)
    assert rows.numel() == int(s.rp[-1])                               # (every id is in range: deg is the softmax's count)
    kept = dref.keep_mask(SEED, rows.numpy(), cl.numpy(), heads, 0.5)
    want = torch.zeros(s.n_out, heads, dtype=torch.long).index_add_(0, rows, torch.from_numpy(kept).long())
    got = _kept_counts(s, heads, dim, SEED)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} (row, head) pairs keep another number of edges"
    assert torch.equal(_kept_counts(s, heads, dim, SEED), got), "the same seed must give the same mask"
    other = _kept_counts(s, heads, dim, SEED + 1)
    assert not torch.equal(other, got)
    kept1 = dref.keep_mask(SEED + 1, rows.numpy(), cl.numpy(), heads, 0.5)
    assert torch.equal(other, torch.zeros(s.n_out, heads, dtype=torch.long).index_add_(0, rows, torch.from_numpy(kept1).long()))


# ---- 2. the five outputs with the mask --------------------------------------------------------------------------------------

# every width once per p; out-of-range ids and the part sizes 1, 3 and 32 spread over them
CASES = [(1, 64, 32, False), (4, 16, 32, False), (3, 7, 3, True), (8, 64, 1, False), (1, 1, 32, True), (4, 16, 3, True)]


@pytest.mark.parametrize("p", [0.5, 0.6])
@pytest.mark.parametrize("heads,dim,partSize,planted", CASES)
def test_five_outputs_against_fp64_with_the_mask(heads, dim, partSize, planted, p):
    s = _wide(partSize, planted)
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 7)]
    what = f"700 x 300 {heads}x{dim} partSize={partSize} planted={planted} p={p}"
    r = dref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, p, SEED, what)
    if planted:
        assert r.nnz < int(s.rp[-1]) and int(s.t_rp[-1]) == r.nnz
    assert int((~r.has).sum()) >= 40 and int((~r.reached).sum()) >= 20
    if (heads, dim, planted, p) == (4, 16, False, 0.5):
        assert r.excluded == 0 and int(r.none_kept.sum()) == 264        # (what the fp64 check of the rule found on the CPU)
    assert int(r.none_kept.sum()) > 0
    _compare_drop(_run(s, H, el, er, G, heads, dim, p, SEED), r, what)


# ---- 3. p = 0 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim", [(4, 16), (3, 7)])
def test_p_zero_is_the_plain_call(heads, dim):
    s = _wide()
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 7)]
    r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, "p = 0")
    _compare(_run(s, H, el, er, G, heads, dim, 0.0, SEED), r, f"p = 0 {heads}x{dim}")


# ---- 4. structures ----------------------------------------------------------------------------------------------------------

def test_a_symmetric_graph_passes_its_own_structure_as_the_transposed_one():
    """The source-side pass reads row j's edges as the edges j -> i and computes the key of (i, j, h) from the row and the id."""
    heads, dim = 4, 16
    g = graph.powerlaw_graph(1500, 40000, 900, seed=4)
    s = _structure(g.row_pointers, g.column_index, g.num_nodes, 32)
    rows, cl = gref.edges_of(g.row_pointers, g.column_index, g.num_nodes)
    assert torch.equal((rows * g.num_nodes + cl).sort().values, (cl * g.num_nodes + rows).sort().values)      # symmetric
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 7)]
    r = dref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, 0.6, SEED, "symmetric")
    _compare_drop(_run(s, H, el, er, G, heads, dim, 0.6, SEED, own_transpose=True), r, "symmetric, structure given twice")
    _compare_drop(_run(s, H, el, er, G, heads, dim, 0.6, SEED), r, "symmetric, device-built transpose")


def test_a_directed_square_graph():
    heads, dim = 2, 41
    rng = np.random.default_rng(5)
    n = 900
    deg = rng.integers(0, 30, size=n)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n, size=rp[-1])
    s = _structure(rp, ci, n, 16)                                     # gnna_transpose_csr_i32 + gnna_build_part_device_i32
    assert not torch.equal(s.t_rp, s.rp)
    H, el, er, G = [t.cuda() for t in gref.inputs(n, n, heads, dim, 7)]
    r = dref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, 0.5, SEED, "directed")
    _compare_drop(_run(s, H, el, er, G, heads, dim, 0.5, SEED), r, "directed square graph")


def test_a_side_without_rows():
    heads, dim, W = 2, 4, 8
    s = _bare([0, 2, 2, 3], [0, 1, 0], 0)
    out, lse, d_el = _nan(3, W), _nan(3, heads), _nan(3, heads)
    assert raw_forward(s, None, None, None, out, lse, heads, dim, 0.5, SEED) == OK
    assert raw_backward(s, None, None, None, None, None, None, None, d_el, None, heads, dim, 0.5, SEED) == OK
    assert (out == 0).all() and (lse == 0).all() and (d_el == 0).all()
    s = _bare([0], [], 5)
    dH, d_er = _nan(5, W), _nan(5, heads)
    assert raw_forward(s, None, None, None, None, None, heads, dim, 0.5, SEED) == OK
    assert raw_backward(s, None, None, None, None, None, None, dH, None, d_er, heads, dim, 0.5, SEED) == OK
    assert (dH == 0).all() and (d_er == 0).all()


# ---- 5. refusals, and the two bindings ----------------------------------------------------------------------------------------

def test_refusals():
    s = _wide()
    heads, dim = 2, 4
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, 1)]
    lib = _lib.load()

    def statuses(p, flags=0):
        Y, lse = torch.zeros(s.n_out, heads * dim, device="cuda"), torch.zeros(s.n_out, heads, device="cuda")
        dH, d_el, d_er = _nan(s.n_in, heads * dim), _nan(s.n_out, heads), _nan(s.n_in, heads)
        f = raw_forward(s, H, el, er, Y, lse, heads, dim, p, SEED, flags=flags)
        fmsg = lib.gnna_last_error().decode()
        b = raw_backward(s, H, el, er, lse, Y, G, dH, d_el, d_er, heads, dim, p, SEED, flags=flags)
        return f, b, fmsg, lib.gnna_last_error().decode(), dH

    before = _lib.get_tuning()
    try:
        _lib.set_tuning(deterministic=1)
        f, b, fmsg, bmsg, _ = statuses(0.5)
        assert (f, b) == (UNSUPPORTED, UNSUPPORTED)
        assert "gnna_gat_forward_drop_f32" in fmsg and "gnna_gat_backward_drop_f32" in bmsg and "deterministic" in bmsg
    finally:
        _lib.reset_tuning()
    assert _lib.get_tuning() == before
    for bad in (-0.1, 1.0, float("nan")):
        f, b, fmsg, bmsg, dH = statuses(bad)
        assert (f, b) == (INVALID, INVALID) and "attn_drop" in fmsg and "gnna_gat_backward_drop_f32: attn_drop" in bmsg
        assert torch.isnan(dH).all(), "a refused call must not write"
    assert statuses(0.5, flags=_lib.ACCUMULATE)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert statuses(0.5)[:2] == (OK, OK) and lib.gnna_version() == 601


@pytest.mark.parametrize("kind", ["square", "directed", "rectangular"])
def test_both_bindings_agree(kind):
    """One small case with leading dimensions through _lib.gat_*_drop and GNNAdvisor.gat_*_drop: each within the kernel bound
    of fp64; lse has one writer per row and must have the same bits."""
    GNNA = load_extension()
    PS, heads, dim = 2, 2, 2
    W = heads * dim
    rp, ci = {"square": ([0, 5, 6, 7, 8, 9, 9], [0, 1, 2, 3, 4, 0, 0, 0, 0]),
              "directed": ([0, 5, 6, 8, 9, 10, 10], [0, 1, 2, 3, 4, 0, 0, 3, 0, 0]),
              "rectangular": ([0, 5, 5, 7], [0, 1, 2, 3, 5, 4, 0])}[kind]
    s = _structure(rp, ci, 6, PS)
    H0, el, er, G0 = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, seed=11)]
    Hbuf, Gbuf = torch.full((s.n_in, W + 3), 7.5, device="cuda"), torch.full((s.n_out, W + 5), -2.0, device="cuda")
    Hbuf[:, 1:1 + W], Gbuf[:, 3:3 + W] = H0, G0
    H, G = Hbuf[:, 1:1 + W], Gbuf[:, 3:3 + W]
    p, seed = 0.5, 2 ** 64 - 3                                         # (a seed above 2^63: unsigned all the way down)
    r = dref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, 0.2, p, seed, kind)
    assert 0 < int((r.k > 0).sum()) < r.k.numel()
    transposed = None if kind == "square" else (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    graph_ = (s.rp, s.ci, s.pp, s.p2n, PS, 0.2, p, seed)
    Y, lse = _lib.gat_forward_drop(H, el, er, *graph_)
    got = _lib.gat_backward_drop(H, el, er, lse, Y, G, *graph_, transposed=transposed)
    _compare_drop((Y, lse, *got), r, f"{kind} _lib")
    obuf, dbuf = torch.full((s.n_out, W + 4), 3.25, device="cuda"), torch.full((s.n_in, W + 4), 3.25, device="cuda")
    Y2, lse2 = _lib.gat_forward_drop(H, el, er, *graph_, out=obuf[:, 2:2 + W])
    got2 = _lib.gat_backward_drop(H, el, er, lse2, Y2, G, *graph_, dH=dbuf[:, 2:2 + W], transposed=transposed)
    _compare_drop((Y2, lse2, *got2), r, f"{kind} _lib, strided outputs")
    for buf in (obuf, dbuf):
        assert (buf[:, :2] == 3.25).all() and (buf[:, 2 + W:] == 3.25).all()
    Ym, lsem = GNNA.gat_forward_drop(H, el, er, *graph_)
    gotm = GNNA.gat_backward_drop(H, el, er, lsem, Ym, G, *graph_, None if transposed is None else list(transposed))
    _compare_drop((Ym, lsem, *gotm), r, f"{kind} GNNAdvisor")
    assert torch.equal(lsem, lse) and torch.equal(lse2, lse)
    assert (Hbuf[:, 0] == 7.5).all() and (Hbuf[:, 1 + W:] == 7.5).all() and (Gbuf[:, :3] == -2.0).all()
    with pytest.raises(_lib.GnnaError, match="attn_drop"):
        _lib.gat_forward_drop(H, el, er, s.rp, s.ci, s.pp, s.p2n, PS, 0.2, 1.0, seed)
    with pytest.raises(RuntimeError, match="attn_drop"):
        GNNA.gat_forward_drop(H, el, er, s.rp, s.ci, s.pp, s.p2n, PS, 0.2, 1.0, seed)

"""gnna_dot_attn_forward_f32 / gnna_dot_attn_backward_f32 through the C ABI (include/gnna_dotattn.h) against the fp64 restatement
of tests/dotattn_ref.py: out, lse, dQ, dK, dV (and Y again as the backward's input).

Structures: gat_rect_ref.wide_short_structure() -- 700 x 300 with a 5,000-edge hub row (the long-row path of the lse pass and a
run that spans several 64-id loads), duplicate edges, 40 rows without edges and 20 sources no edge reaches -- as it is and with
ids outside the source rows planted; a small symmetric square graph passed as its own transpose with Q, K and V as column slices
of one [N, 3 W] matrix; a directed square graph with the device-built transpose.  partSize 3 and 32: a row's groups straddle the
wavefronts of a workgroup and workgroups.
Shapes: 8 of the 28 lane layouts -- LPH = 1 (64 x 1) to 64 (1 x 256), dim % 4 != 0, rows wider than one wave-wide load (8 x 40:
column blocks of whole heads); tests/test_attn_layouts_gpu.py runs every layout.  Inputs: randn Q, K, V, dY with scale = 1 / sqrt(dim).
Bounds: 1e-5 * max(1, sum of |terms|) * max(1, S) (dotattn_ref's docstring); the function is smooth, so no element is excluded.
Every call pre-fills its outputs with NaN, so an element the library does not write fails the comparison.  S is printed per
shape."""
import functools

import numpy as np
import pytest
import torch

import dotattn_ref as tref
import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib, graph, load_extension
from test_gat_rect_gpu import _bare, _nan, _ptr, _structure
from util import assert_close_f64

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -3
SEED = 0x1234
# (heads, dim): seed of the inputs
SEEDS = {(1, 64): 5, (4, 16): 6, (3, 5): 7, (8, 8): 8, (1, 256): 9, (64, 1): 10, (2, 33): 11, (8, 40): 12}


def _scale(dim):
    return 1.0 / dim ** 0.5


def raw_forward(s, Q, K, V, out, lse, heads, dim, p=0.0, rng_seed=SEED, flags=0, scale=None, ld_q=None, ld_k=None, ld_v=None,
                ld_out=None):
    W = heads * dim
    return _lib.load().gnna_dot_attn_forward_f32(
        _ptr(Q), ld_q or W, _ptr(K), ld_k or W, _ptr(V), ld_v or W, _ptr(s.rp), _ptr(s.ci), _ptr(s.pp), _ptr(s.p2n),
        _scale(dim) if scale is None else scale, p, rng_seed, _ptr(out), ld_out or W, _ptr(lse), s.n_out, s.n_in, heads, dim,
        s.p2n.numel(), s.ps, flags, _lib._stream(s.rp.device))


def raw_backward(s, Q, K, V, lse, Y, dY, dQ, dK, dV, heads, dim, p=0.0, rng_seed=SEED, flags=0, scale=None, own_transpose=False,
                 lds=None):
    W = heads * dim
    ld = dict(q=W, k=W, v=W, y=W, dy=W, dq=W, dk=W, dv=W)
    ld.update(lds or {})
    t = (s.rp, s.ci, s.pp, s.p2n) if own_transpose else (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    return _lib.load().gnna_dot_attn_backward_f32(
        _ptr(Q), ld["q"], _ptr(K), ld["k"], _ptr(V), ld["v"], _ptr(lse), _ptr(Y), ld["y"], _ptr(dY), ld["dy"], _ptr(s.rp), _ptr(s.ci),
        _ptr(s.pp), _ptr(s.p2n), s.p2n.numel(), *[_ptr(x) for x in t], t[3].numel(), _scale(dim) if scale is None else scale, p,
        rng_seed, _ptr(dQ), ld["dq"], _ptr(dK), ld["dk"], _ptr(dV), ld["dv"], s.n_out, s.n_in, heads, dim, s.ps, flags,
        _lib._stream(s.rp.device))


def _err():
    return _lib.load().gnna_last_error()


def _run(s, Q, K, V, G, heads, dim, p=0.0, rng_seed=SEED, own_transpose=False, scale=None):
    """Forward and backward into NaN-filled outputs -> (Y, lse, dQ, dK, dV)."""
    W = heads * dim
    Y, lse, dQ, dK, dV = _nan(s.n_out, W), _nan(s.n_out, heads), _nan(s.n_out, W), _nan(s.n_in, W), _nan(s.n_in, W)
    assert raw_forward(s, Q, K, V, Y, lse, heads, dim, p, rng_seed, scale=scale) == OK, _err()
    assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, p, rng_seed, scale=scale, own_transpose=own_transpose) == OK, _err()
    return Y, lse, dQ, dK, dV


def _compare(got, r, what):
    """The five outputs against kernel_reference's namespace: the bounds of dotattn_ref's docstring."""
    Y, lse, dQ, dK, dV = got
    print(f"{what}: S = {r.S:.3f}")
    for t, name in zip(got, ("Y", "lse", "dQ", "dK", "dV")):
        assert not torch.isnan(t).any(), f"{what}: {name} has elements the call did not write"
        assert torch.isfinite(t).all(), f"{what}: {name} is not finite"
    n = lambda t: t.cpu().numpy()
    rtol = 1e-5 * r.factor
    assert_close_f64(n(Y), n(r.Y), rtol=rtol, scale=n(r.s_Y), what=f"{what} Y")
    assert_close_f64(n(lse[r.has]), n(r.lse[r.has]), rtol=rtol, what=f"{what} lse")
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (dQ[~r.has] == 0).all(), \
        f"{what}: rows without edges must give out = lse = dQ = 0"
    assert_close_f64(n(dQ), n(r.dQ), rtol=rtol, scale=n(r.s_dQ), what=f"{what} dQ")
    assert_close_f64(n(dK), n(r.dK), rtol=rtol, scale=n(r.s_dK), what=f"{what} dK")
    assert_close_f64(n(dV), n(r.dV), rtol=rtol, scale=n(r.s_dV), what=f"{what} dV")
    assert (dK[~r.reached] == 0).all() and (dV[~r.reached] == 0).all(), f"{what}: sources no edge reaches must get exactly 0"


@functools.lru_cache(maxsize=None)
def _wide(partSize=32, planted=False):
    rp, ci = gref.wide_short_structure()
    return _structure(rp, gref.plant_out_of_range(ci, 300) if planted else ci, 300, partSize)


@functools.lru_cache(maxsize=None)
def _wide_case(heads, dim, planted, p):
    """Inputs on the device and their fp64 reference on the wide-short structure: computed once, shared, never written."""
    s = _wide(32, planted)
    Q, K, V, G = [t.cuda() for t in tref.inputs(s.n_out, s.n_in, heads, dim, SEEDS[heads, dim])]
    r = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, _scale(dim), p, SEED)
    return Q, K, V, G, r


# ---- 1. the five outputs -----------------------------------------------------------------------------------------------------

# every shape on the plain and on the planted structure; partSize 3 and 32 alternate over them
CASES = [(h, d, ps, planted) for k, (h, d) in enumerate(SEEDS) for planted, ps in ((False, (32, 3)[k % 2]), (True, (3, 32)[k % 2]))]


@pytest.mark.parametrize("heads,dim,partSize,planted", CASES)
def test_outputs_against_fp64(heads, dim, partSize, planted):
    s = _wide(partSize, planted)
    Q, K, V, G, r = _wide_case(heads, dim, planted, 0.0)
    what = f"700 x 300 {heads}x{dim} partSize={partSize} planted={planted}"
    if planted:
        assert r.nnz < int(s.rp[-1]) and int(s.t_rp[-1]) == r.nnz
    assert int((~r.has).sum()) >= 40 and int((~r.reached).sum()) >= 20
    _compare(_run(s, Q, K, V, G, heads, dim), r, what)


@pytest.mark.parametrize("heads,dim,partSize,planted", [(1, 64, 3, False), (4, 16, 32, True), (3, 5, 3, False), (8, 40, 32, False),
                                                        (64, 1, 3, True)])
def test_outputs_with_the_mask(heads, dim, partSize, planted):
    """attn_drop = 0.5 against the restated mask of gat_drop_ref; lse is that of the undropped scores."""
    s = _wide(partSize, planted)
    Q, K, V, G, r = _wide_case(heads, dim, planted, 0.5)
    assert 0 < int((r.k > 0).sum()) < r.k.numel()
    got = _run(s, Q, K, V, G, heads, dim, 0.5, SEED)
    _compare(got, r, f"700 x 300 {heads}x{dim} partSize={partSize} planted={planted} p=0.5")
    plain = _wide_case(heads, dim, planted, 0.0)[4]
    assert_close_f64(got[1][r.has].cpu().numpy(), plain.lse[r.has].cpu().numpy(), rtol=1e-5 * r.factor, what="lse with the mask")
    other = _run(s, Q, K, V, G, heads, dim, 0.5, SEED + 1)
    assert not torch.equal(other[0], got[0]) and torch.equal(other[1], got[1])       # another mask, the same lse


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim,partSize", [(4, 16, 32), (3, 5, 3), (1, 256, 32)])
def test_lse_bits_and_a_backward_called_twice(heads, dim, partSize):
    s = _wide(partSize, False)
    Q, K, V, G, r = _wide_case(heads, dim, False, 0.0)
    W = heads * dim
    Y, lse, dQ, dK, dV = _run(s, Q, K, V, G, heads, dim, 0.0, SEED)
    # lse: one writer per (row, head), a fixed order: the same bits on every run, and with attn_drop = 0 whatever the seed
    Y2, lse2 = _nan(s.n_out, W), _nan(s.n_out, heads)
    assert raw_forward(s, Q, K, V, Y2, lse2, heads, dim, 0.0, SEED) == OK, _err()
    assert torch.equal(lse2, lse)
    Y3, lse3 = _nan(s.n_out, W), _nan(s.n_out, heads)
    assert raw_forward(s, Q, K, V, Y3, lse3, heads, dim, 0.0, SEED + 99) == OK, _err()
    assert torch.equal(lse3, lse)
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(Y3), n(r.Y), rtol=1e-5 * r.factor, scale=n(r.s_Y), what="attn_drop = 0 with another seed")
    # the backward again, into the same buffers: nothing (a partial row, the scratch) is carried over from the first call
    assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, 0.0, SEED) == OK, _err()
    _compare((Y, lse, dQ, dK, dV), r, "the backward called twice")


# ---- 3. row strides -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim", [(2, 33), (8, 8)])
def test_row_strides_larger_than_the_width(heads, dim):
    s = _wide(3, True)
    Q0, K0, V0, G0, r = _wide_case(heads, dim, True, 0.0)
    W = heads * dim

    def padded(t, pad, fill):
        buf = torch.full((t.shape[0], W + pad), fill, device="cuda")
        buf[:, 1:1 + W] = t
        return buf, buf[:, 1:1 + W]

    (q_b, Q), (k_b, K), (v_b, V), (g_b, G) = padded(Q0, 3, 7.5), padded(K0, 6, -1.5), padded(V0, 9, 4.5), padded(G0, 2, 2.5)
    (y_b, Y), (dq_b, dQ) = padded(_nan(s.n_out, W), 5, 3.25), padded(_nan(s.n_out, W), 4, 3.25)
    (dk_b, dK), (dv_b, dV) = padded(_nan(s.n_in, W), 7, 3.25), padded(_nan(s.n_in, W), 1, 3.25)
    lse = _nan(s.n_out, heads)
    assert raw_forward(s, Q, K, V, Y, lse, heads, dim, ld_q=W + 3, ld_k=W + 6, ld_v=W + 9, ld_out=W + 5) == OK, _err()
    assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim,
                        lds=dict(q=W + 3, k=W + 6, v=W + 9, y=W + 5, dy=W + 2, dq=W + 4, dk=W + 7, dv=W + 1)) == OK, _err()
    _compare((Y, lse, dQ, dK, dV), r, f"strided rows {heads}x{dim}")
    for buf in (y_b, dq_b, dk_b, dv_b):
        assert (buf[:, 0] == 3.25).all() and (buf[:, 1 + W:] == 3.25).all(), "written outside the rows"
    assert (q_b[:, 0] == 7.5).all() and (k_b[:, 1 + W:] == -1.5).all() and (v_b[:, 1 + W:] == 4.5).all() and (g_b[:, 0] == 2.5).all()


# ---- 4. square structures -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dim,p", [(4, 16, 0.0), (3, 5, 0.5)])
def test_a_symmetric_graph_as_its_own_transpose_with_slices_of_one_matrix(heads, dim, p):
    """The source-side pass reads row j's edges as the edges j -> i; Q, K and V are column slices of one [N, 3 W] matrix."""
    g = graph.powerlaw_graph(500, 8000, 300, seed=4)
    s = _structure(g.row_pointers, g.column_index, g.num_nodes, 32)
    rows, cl = gref.edges_of(g.row_pointers, g.column_index, g.num_nodes)
    assert torch.equal((rows * g.num_nodes + cl).sort().values, (cl * g.num_nodes + rows).sort().values)      # symmetric
    W = heads * dim
    gen = torch.Generator().manual_seed(SEEDS[heads, dim])
    P = torch.randn(s.n_out, 3 * W, generator=gen).cuda()
    G = torch.randn(s.n_out, W, generator=gen).cuda()
    Q, K, V = P[:, :W], P[:, W:2 * W], P[:, 2 * W:]
    r = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, _scale(dim), p, SEED)
    for own, what in ((True, "structure given twice"), (False, "device-built transpose")):
        Y, lse, dQ, dK, dV = _nan(s.n_out, W), _nan(s.n_out, heads), _nan(s.n_out, W), _nan(s.n_in, W), _nan(s.n_in, W)
        assert raw_forward(s, Q, K, V, Y, lse, heads, dim, p, ld_q=3 * W, ld_k=3 * W, ld_v=3 * W) == OK, _err()
        assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, p, own_transpose=own,
                            lds=dict(q=3 * W, k=3 * W, v=3 * W)) == OK, _err()
        _compare((Y, lse, dQ, dK, dV), r, f"symmetric {heads}x{dim} p={p}, {what}, slices of one matrix")


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
    Q, K, V, G = [t.cuda() for t in tref.inputs(n, n, heads, dim, SEEDS[heads, dim])]
    r = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, _scale(dim), p, SEED)
    _compare(_run(s, Q, K, V, G, heads, dim, p, SEED), r, f"directed square graph {heads}x{dim} p={p}")


def test_a_side_without_rows():
    """num_in_rows = 0: out, lse and dQ are zero-filled and no input is read; num_out_rows = 0: dK and dV are."""
    heads, dim, W = 2, 4, 8
    s = _bare([0, 2, 2, 3], [0, 1, 0], 0)
    out, lse, dQ = _nan(3, W), _nan(3, heads), _nan(3, W)
    assert raw_forward(s, None, None, None, out, lse, heads, dim, 0.5) == OK, _err()
    assert raw_backward(s, None, None, None, None, None, None, dQ, None, None, heads, dim, 0.5) == OK, _err()
    assert (out == 0).all() and (lse == 0).all() and (dQ == 0).all()
    s = _bare([0], [], 5)
    dK, dV = _nan(5, W), _nan(5, W)
    assert raw_forward(s, None, None, None, None, None, heads, dim, 0.5) == OK, _err()
    assert raw_backward(s, None, None, None, None, None, None, None, dK, dV, heads, dim, 0.5) == OK, _err()
    assert (dK == 0).all() and (dV == 0).all()


# ---- 5. scale, flags, refusals on the device, and the two bindings --------------------------------------------------------------

def test_scale_zero_is_uniform_attention():
    """scale = 0: every z is 0, alpha = 1 / (edges of the row), out is the mean of V over the row's edges (duplicates counted
    twice) and lse = log(edges); dQ and dK are exactly 0."""
    heads, dim = 4, 16
    s = _wide(32, False)
    Q, K, V, G, _ = _wide_case(heads, dim, False, 0.0)
    r = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, 0.0)
    got = _run(s, Q, K, V, G, heads, dim, scale=0.0)
    _compare(got, r, "scale = 0")
    rows, cl = gref.edges_of(s.rp, s.ci, s.n_in)
    cnt = torch.bincount(rows, minlength=s.n_out).double()
    mean = torch.zeros(s.n_out, heads * dim, dtype=torch.float64, device="cuda").index_add_(0, rows, V.double()[cl]) / cnt.clamp(min=1)[:, None]
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(got[0]), n(mean), rtol=1e-5, scale=n(r.s_Y), what="scale = 0: the mean of V")
    assert_close_f64(n(got[1][r.has]), n(torch.log(cnt[r.has])[:, None].expand(-1, heads)), rtol=1e-5, what="scale = 0: lse = log(edges)")
    assert (got[2] == 0).all() and (got[3] == 0).all()


def test_relu_epilogue_and_refusals():
    heads, dim = 4, 16
    s = _wide(32, False)
    Q, K, V, G, r = _wide_case(heads, dim, False, 0.0)
    W = heads * dim
    Y, lse = _nan(s.n_out, W), _nan(s.n_out, heads)
    assert raw_forward(s, Q, K, V, Y, lse, heads, dim, flags=_lib.EPILOGUE_RELU) == OK, _err()
    n = lambda t: t.cpu().numpy()
    assert (Y >= 0).all() and bool((r.Y < 0).any())
    assert_close_f64(n(Y), n(r.Y.clamp(min=0)), rtol=1e-5 * r.factor, scale=n(r.s_Y), what="ReLU epilogue")
    dQ, dK, dV = _nan(s.n_out, W), _nan(s.n_in, W), _nan(s.n_in, W)
    for bad in (-0.1, 1.0, float("nan")):
        assert raw_forward(s, Q, K, V, Y, lse, heads, dim, bad) == INVALID and b"gnna_dot_attn_forward_f32: attn_drop" in _err()
        assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, bad) == INVALID
        assert b"gnna_dot_attn_backward_f32: attn_drop" in _err()
    for bad in (float("nan"), float("inf")):
        assert raw_forward(s, Q, K, V, Y, lse, heads, dim, scale=bad) == INVALID and b"gnna_dot_attn_forward_f32: scale" in _err()
        assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, scale=bad) == INVALID
    assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, flags=_lib.EPILOGUE_RELU) == INVALID
    assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim, flags=_lib.ACCUMULATE) == UNSUPPORTED
    try:
        _lib.set_tuning(deterministic=1)
        assert raw_forward(s, Q, K, V, Y, lse, heads, dim) == UNSUPPORTED and b"deterministic" in _err()
        assert raw_backward(s, Q, K, V, lse, Y, G, dQ, dK, dV, heads, dim) == UNSUPPORTED
    finally:
        _lib.reset_tuning()
    for t in (dQ, dK, dV):
        assert torch.isnan(t).all(), "a refused call must not write"
    assert _lib.load().gnna_version() == 601


@pytest.mark.parametrize("kind", ["square", "directed", "rectangular"])
def test_both_bindings_agree(kind):
    """One small case through _lib.dot_attn_* (strided inputs and outputs) and GNNAdvisor.dot_attn_*: each within the kernel bound
    of fp64; lse has one writer per (row, head) and must have the same bits."""
    GNNA = load_extension()
    PS, heads, dim = 2, 2, 3
    W = heads * dim
    scale = 0.7
    rp, ci = {"square": ([0, 5, 6, 7, 8, 9, 9], [0, 1, 2, 3, 4, 0, 0, 0, 0]),
              "directed": ([0, 5, 6, 8, 9, 10, 10], [0, 1, 2, 3, 4, 0, 0, 3, 0, 0]),
              "rectangular": ([0, 5, 5, 7], [0, 1, 2, 3, 5, 4, 0])}[kind]
    s = _structure(rp, ci, 6, PS)
    Q, K0, V0, G0 = [t.cuda() for t in tref.inputs(s.n_out, s.n_in, heads, dim, seed=11)]
    KV, Gbuf = torch.full((s.n_in, 2 * W + 3), 7.5, device="cuda"), torch.full((s.n_out, W + 5), -2.0, device="cuda")
    KV[:, 1:1 + W], KV[:, 1 + W:1 + 2 * W], Gbuf[:, 3:3 + W] = K0, V0, G0
    K, V, G = KV[:, 1:1 + W], KV[:, 1 + W:1 + 2 * W], Gbuf[:, 3:3 + W]
    p, seed = 0.5, 2 ** 64 - 3                                         # (a seed above 2^63: unsigned all the way down)
    r = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, scale, p, seed)
    transposed = None if kind == "square" else (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    graph_ = (s.rp, s.ci, s.pp, s.p2n, PS, scale, p, seed)
    Y, lse = _lib.dot_attn_forward(Q, K, V, heads, *graph_)
    got = _lib.dot_attn_backward(Q, K, V, heads, lse, Y, G, *graph_, transposed=transposed)
    _compare((Y, lse, *got), r, f"{kind} _lib")
    obuf, dbuf = torch.full((s.n_out, W + 4), 3.25, device="cuda"), torch.full((s.n_in, W + 4), 3.25, device="cuda")
    Y2, lse2 = _lib.dot_attn_forward(Q, K, V, heads, *graph_, out=obuf[:, 2:2 + W])
    got2 = _lib.dot_attn_backward(Q, K, V, heads, lse2, Y2, G, *graph_, transposed=transposed, dK=dbuf[:, 2:2 + W])
    _compare((Y2, lse2, *got2), r, f"{kind} _lib, strided outputs")
    for buf in (obuf, dbuf):
        assert (buf[:, :2] == 3.25).all() and (buf[:, 2 + W:] == 3.25).all()
    Ym, lsem = GNNA.dot_attn_forward(Q, K, V, heads, *graph_)
    gotm = GNNA.dot_attn_backward(Q, K, V, heads, lsem, Ym, G, *graph_, None if transposed is None else list(transposed))
    _compare((Ym, lsem, *gotm), r, f"{kind} GNNAdvisor")
    assert torch.equal(lsem, lse) and torch.equal(lse2, lse)
    assert (KV[:, 0] == 7.5).all() and (KV[:, 1 + 2 * W:] == 7.5).all() and (Gbuf[:, :3] == -2.0).all()
    # the default scale of the wrapper is 1 / sqrt(dim)
    Yd, _ = _lib.dot_attn_forward(Q, K, V, heads, s.rp, s.ci, s.pp, s.p2n, PS)
    rd = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, _scale(dim))
    assert_close_f64(Yd.cpu().numpy(), rd.Y.cpu().numpy(), rtol=1e-5 * rd.factor, scale=rd.s_Y.cpu().numpy(), what="default scale")
    with pytest.raises(_lib.GnnaError, match="attn_drop"):
        _lib.dot_attn_forward(Q, K, V, heads, s.rp, s.ci, s.pp, s.p2n, PS, scale, 1.0, seed)
    with pytest.raises(RuntimeError, match="attn_drop"):
        GNNA.dot_attn_forward(Q, K, V, heads, s.rp, s.ci, s.pp, s.p2n, PS, scale, 1.0, seed)

"""The two binding layers on the smallest graph on which a binding slip shows: every operation that both the ctypes wrappers
(``_lib``) and the ``GNNAdvisor`` module expose, run through both.

Graph: 6 nodes, symmetric; row 0 has 5 edges (partSize 2: three neighbor-groups), row 5 none.  A directed variant (one edge
without its reverse) and a block of 3 destination rows over the 6 source rows serve the entries that take them.  Features are
dim 3 (no multiple of 4; 5 for sddmm, which takes no less than 4) column blocks of wider buffers (leading dimension != dim);
`out` is given as a strided view of a sentinel-filled buffer once and left out once.  A wrong leading dimension, row count or stream, or an output the library did
not fill, shows as a wrong element, a touched sentinel or the poison value (conftest.py: GNNA_DEBUG_POISON=1).

Sums, max / min and dot products run on small integers: every intermediate is exact in fp32 (and in bf16) whatever order the
atomics land in, so the two layers and the integer reference agree bit for bit, `arg` included.  The softmax-based families are
held, per layer, to the fp64 formula at the bounds of their own tests (test_edge_attention_gpu.py, test_gat_rect_gpu.py)."""
import types

import numpy as np
import pytest
import torch

import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib, load_extension
from test_edge_attention_gpu import SOFTMAX_RTOL, _softmax64
from test_gat_rect_gpu import _compare
from util import assert_close_f64

pytestmark = pytest.mark.gpu
GNNA = load_extension()
PS, DIM, HEADS, HDIM = 2, 3, 2, 2
SENTINEL = 12288.0          # (exact in bfloat16 as well)
INT_POISON = -(2 ** 31)


def _structure(rp, ci, n_in):
    """Device CSR with its partition and, built on the device, its transpose with the partition of that."""
    rp, ci = torch.tensor(rp, dtype=torch.int32), torch.tensor(ci, dtype=torch.int32)
    pp, p2n = _lib.build_part(PS, rp)
    s = types.SimpleNamespace(rp=rp.cuda(), ci=ci.cuda(), pp=pp.cuda(), p2n=p2n.cuda(), n_out=rp.numel() - 1, n_in=n_in,
                              rows=torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long()), cols=ci.long())
    s.t_rp, s.t_ci, _ = _lib.transpose_csr(s.rp, s.ci, num_in_rows=n_in, want_perm=False)
    s.t_pp, s.t_p2n = _lib.build_part_device(PS, s.t_rp)
    s.transposed = (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    return s


@pytest.fixture(scope="module")
def g():
    d = types.SimpleNamespace()
    d.sym = _structure([0, 5, 6, 7, 8, 9, 9], [0, 1, 2, 3, 4, 0, 0, 0, 0], 6)
    d.directed = _structure([0, 5, 6, 8, 9, 10, 10], [0, 1, 2, 3, 4, 0, 0, 3, 0, 0], 6)
    d.rect = _structure([0, 5, 5, 7], [0, 1, 2, 3, 5, 4, 0], 6)
    gen = torch.Generator().manual_seed(7)
    d.buf = torch.randint(-3, 4, (6, 5), generator=gen).float().cuda()       # X = buf[:, 1:4]: dim 3, leading dimension 5
    d.X = d.buf[:, 1:4]
    d.deg = torch.tensor([1., 2., 1., 3., 2., 1.]).cuda()
    d.w = torch.randint(-2, 3, (10,), generator=gen).float().cuda()
    d.base = torch.randint(-3, 4, (6, DIM), generator=gen).float().cuda()
    return d


def _sum64(s, X, coef=None):
    """Exact reference of a weighted neighbor sum: out[i] = sum_e coef[e] X[col(e)] (float64 on the host)."""
    X = X.double().cpu()
    coef = torch.ones(s.cols.numel(), dtype=torch.float64) if coef is None else coef.double().cpu()
    return torch.zeros(s.n_out, X.shape[1], dtype=torch.float64).index_add_(0, s.rows, coef[:, None] * X[s.cols])


def _view(rows, dim, fill=None):
    """(buffer [rows, dim + 4] of SENTINEL, its column block [:, 2 : 2 + dim], optionally set to `fill`)."""
    buf = torch.full((rows, dim + 4), SENTINEL, device="cuda")
    view = buf[:, 2:2 + dim]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _untouched(buf, dim, what):
    assert (buf[:, :2] == SENTINEL).all() and (buf[:, 2 + dim:] == SENTINEL).all(), f"{what}: written outside the strided view"


def _same(a, b, ref, what):
    """Both layers' results: bitwise equal, equal to the exact reference, nothing left as the allocation was poisoned."""
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
    if a.is_floating_point():
        assert not torch.isnan(a).any() and not torch.isnan(b).any(), f"{what}: elements the call did not write"
    else:
        assert (a != INT_POISON).all() and (b != INT_POISON).all(), f"{what}: elements the call did not write"
    assert torch.equal(a, b), f"{what}: the two layers differ"
    assert torch.equal(a.cpu().double(), ref.double()), f"{what}: differs from the exact reference"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_general_aggregation_fp32(g, mode):
    s, eps = g.sym, 2.0
    coef = [None, (g.deg.cpu()[s.rows] * g.deg.cpu()[s.cols]), torch.full((9,), eps)][mode]
    ref = _sum64(s, g.X, coef)
    deg = g.deg if mode == 1 else None
    a = _lib.agg_ld(mode, g.X, s.ci, s.pp, s.p2n, 6, PS, degrees_out=deg, degrees_in=deg, epsilon=eps)
    b = GNNA.aggregate_ld(mode, g.X, s.ci, deg, eps, s.pp, s.p2n, PS)
    _same(a, b, ref, f"mode {mode}, fresh out")
    # into a strided view, added to what it holds and clamped at zero
    want = torch.clamp(g.base.cpu().double() + ref, min=0)
    buf_a, out_a = _view(6, DIM, g.base)
    buf_b, out_b = _view(6, DIM, g.base)
    assert _lib.agg_ld(mode, g.X, s.ci, s.pp, s.p2n, 6, PS, degrees_out=deg, degrees_in=deg, epsilon=eps, out=out_a,
                       accumulate=True, relu=True) is out_a
    GNNA.aggregate_ld(mode, g.X, s.ci, deg, eps, s.pp, s.p2n, PS, out=out_b, accumulate=True, relu=True)
    _same(out_a, out_b, want, f"mode {mode}, strided out")
    _untouched(buf_a, DIM, "agg_ld")
    _untouched(buf_b, DIM, "aggregate_ld")


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mode", [0, 1])
def test_general_aggregation_bf16(g, mode, out_dtype):
    s = g.sym
    Xb = g.buf.bfloat16()[:, 1:4]
    coef = [None, (g.deg.cpu()[s.rows] * g.deg.cpu()[s.cols])][mode]
    ref = _sum64(s, g.X, coef)                                    # (integers below 256: exact in bfloat16 too)
    deg = g.deg if mode == 1 else None
    a = _lib.agg_ld_x16(mode, Xb, s.ci, s.pp, s.p2n, 6, PS, degrees_out=deg, degrees_in=deg, out_dtype=out_dtype)
    b = GNNA.aggregate_ld(mode, Xb, s.ci, deg, 1.0, s.pp, s.p2n, PS, out_dtype=out_dtype)
    assert a.dtype == out_dtype
    _same(a, b, ref, f"bf16 mode {mode} -> {out_dtype}, fresh out")
    buf_a, buf_b = (torch.full((6, DIM + 4), SENTINEL, device="cuda", dtype=out_dtype) for _ in range(2))
    _lib.agg_ld_x16(mode, Xb, s.ci, s.pp, s.p2n, 6, PS, degrees_out=deg, degrees_in=deg, out=buf_a[:, 2:2 + DIM])
    GNNA.aggregate_ld(mode, Xb, s.ci, deg, 1.0, s.pp, s.p2n, PS, out=buf_b[:, 2:2 + DIM])
    _same(buf_a[:, 2:2 + DIM], buf_b[:, 2:2 + DIM], ref, f"bf16 mode {mode} -> {out_dtype}, strided out")
    _untouched(buf_a, DIM, "agg_ld_x16")
    _untouched(buf_b, DIM, "aggregate_ld (bf16)")


def test_edge_weighted_aggregation(g):
    s, w = g.sym, g.w[:9].contiguous()
    ref = _sum64(s, g.X, w)
    _same(_lib.agg_edge(g.X, s.ci, w, s.pp, s.p2n, 6, PS), GNNA.aggregate_edge(g.X, s.ci, w, s.pp, s.p2n, PS), ref, "fresh out")
    want = torch.clamp(g.base.cpu().double() + ref, min=0)
    buf_a, out_a = _view(6, DIM, g.base)
    buf_b, out_b = _view(6, DIM, g.base)
    _lib.agg_edge(g.X, s.ci, w, s.pp, s.p2n, 6, PS, out=out_a, accumulate=True, relu=True)
    GNNA.aggregate_edge(g.X, s.ci, w, s.pp, s.p2n, PS, out=out_b, accumulate=True, relu=True)
    _same(out_a, out_b, want, "strided out")
    _untouched(buf_a, DIM, "agg_edge")
    _untouched(buf_b, DIM, "aggregate_edge")


def _reduce64(s, X, op):
    """Exact max / min over every row's edges and the smallest position that supplies it (0 and -1 for a row without edges)."""
    X = X.cpu()
    out, arg = torch.zeros(s.n_out, X.shape[1]), torch.full((s.n_out, X.shape[1]), -1, dtype=torch.int32)
    for i in range(s.n_out):
        e = (s.rows == i).nonzero()[:, 0]
        if e.numel():
            vals = X[s.cols[e]]                                                   # [edges of row i, dim] in position order
            best = vals.max(0).values if op == _lib.REDUCE_MAX else vals.min(0).values
            out[i] = best
            arg[i] = e[(vals == best).int().argmax(0)].int()                      # (argmax: the first position that ties)
    return out, arg


@pytest.mark.parametrize("op", [_lib.REDUCE_MAX, _lib.REDUCE_MIN])
def test_reduce_and_scatter_arg(g, op):
    s = g.sym
    ref, ref_arg = _reduce64(s, g.X, op)
    a, a_arg = _lib.agg_reduce_ld(op, g.X, s.ci, s.pp, s.p2n, PS)
    b, b_arg = GNNA.aggregate_reduce(op, g.X, s.ci, s.pp, s.p2n, PS)
    _same(a, b, ref, "reduce, fresh out")
    _same(a_arg, b_arg, ref_arg, "arg, fresh")
    buf_a, out_a = _view(6, DIM)
    buf_b, out_b = _view(6, DIM)
    _, a_arg2 = _lib.agg_reduce_ld(op, g.X, s.ci, s.pp, s.p2n, PS, out=out_a, relu=True)
    _, b_arg2 = GNNA.aggregate_reduce(op, g.X, s.ci, s.pp, s.p2n, PS, out=out_b, relu=True)
    _same(out_a, out_b, torch.clamp(ref, min=0), "reduce, strided out")
    _same(a_arg2, b_arg2, ref_arg, "arg beside a strided out")
    _untouched(buf_a, DIM, "agg_reduce_ld")
    _untouched(buf_b, DIM, "aggregate_reduce")
    assert _lib.agg_reduce_ld(op, g.X, s.ci, s.pp, s.p2n, PS, want_arg=False)[1] is None
    assert GNNA.aggregate_reduce(op, g.X, s.ci, s.pp, s.p2n, PS, want_arg=False)[1] is None
    # the backward, on the square graph and on the block (3 rows of gradient scattered over 6 source rows)
    for t, grad, arg in ((s, g.X, a_arg), (g.rect, g.X[:3], _lib.agg_reduce_ld(op, g.X, g.rect.ci, g.rect.pp, g.rect.p2n, PS,
                                                                               num_out_rows=3)[1])):
        want = torch.zeros(6, DIM, dtype=torch.float64)
        for i, f in (arg.cpu() >= 0).nonzero().tolist():
            want[t.cols[int(arg[i, f])], f] += float(grad[i, f])
        _same(_lib.scatter_arg_ld(grad, arg, t.ci, 6), GNNA.scatter_arg(grad, arg, t.ci, 6), want, f"scatter_arg, {t.n_out} rows")


@pytest.mark.parametrize("heads", [1, 2])
def test_edge_softmax_and_backward(g, heads):
    s = g.directed
    gen = torch.Generator().manual_seed(heads)
    scores, grad = (torch.randn(heads, 10, generator=gen).cuda() for _ in range(2))
    sc, gr = (scores[0], grad[0]) if heads == 1 else (scores, grad)
    ref = _softmax64(scores, s.rp)
    dot = torch.zeros(heads, 6, dtype=torch.float64).index_add_(1, s.rows, (ref * grad.double()).cpu()).cuda()
    ref_ds = ref * (grad.double() - dot[:, s.rows.cuda()])
    adot = torch.zeros(heads, 6, dtype=torch.float64).index_add_(1, s.rows, (ref * grad.double().abs()).cpu()).cuda()
    scale = ref * (grad.double().abs() + adot[:, s.rows.cuda()])
    probs = {"_lib": _lib.edge_softmax(sc, s.rp), "GNNAdvisor": GNNA.edge_softmax(sc, s.rp)}
    for layer, p in probs.items():
        assert p.shape == sc.shape
        assert_close_f64(p.view(heads, 10).cpu().numpy(), ref.cpu().numpy(), rtol=SOFTMAX_RTOL, what=f"{layer} softmax")
    p = probs["_lib"]
    for layer, ds in (("_lib", _lib.edge_softmax_backward(p, gr, s.rp)), ("GNNAdvisor", GNNA.edge_softmax_backward(p, gr, s.rp))):
        assert ds.shape == sc.shape
        assert_close_f64(ds.view(heads, 10).cpu().numpy(), ref_ds.cpu().numpy(), rtol=SOFTMAX_RTOL, scale=scale.cpu().numpy(),
                         what=f"{layer} softmax backward")


@pytest.mark.parametrize("kind", ["square", "directed", "rectangular"])
def test_gat_forward_and_backward(g, kind):
    s = {"square": g.sym, "directed": g.directed, "rectangular": g.rect}[kind]
    W = HEADS * HDIM
    H0, el, er, G0 = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, HEADS, HDIM, seed=11)]
    Hbuf = torch.full((s.n_in, W + 2), SENTINEL, device="cuda")
    H = Hbuf[:, 1:1 + W].copy_(H0)                                              # leading dimension W + 2
    Gbuf = torch.full((s.n_out, W + 3), SENTINEL, device="cuda")
    G = Gbuf[:, 3:].copy_(G0)
    r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, HEADS, 0.2, kind)
    transposed = None if kind == "square" else s.transposed
    graph = (s.rp, s.ci, s.pp, s.p2n)
    # ctypes: fresh outputs, then Y / dH as strided views
    Y, lse = _lib.gat_forward(H, el, er, *graph, PS)
    dH, d_el, d_er = _lib.gat_backward(H, el, er, lse, Y, G, *graph, PS, transposed=transposed)
    _compare((Y, lse, dH, d_el, d_er), r, f"{kind} _lib")
    buf_y, out_y = _view(s.n_out, W)
    buf_h, out_h = _view(s.n_in, W)
    Y2, lse2 = _lib.gat_forward(H, el, er, *graph, PS, out=out_y)
    dH2, d_el2, d_er2 = _lib.gat_backward(H, el, er, lse2, Y2, G, *graph, PS, dH=out_h, transposed=transposed)
    assert Y2 is out_y and dH2 is out_h
    _compare((Y2, lse2, dH2, d_el2, d_er2), r, f"{kind} _lib, strided outputs")
    _untouched(buf_y, W, "gat_forward")
    _untouched(buf_h, W, "gat_backward")
    # the module (it allocates its outputs)
    Ym, lsem = GNNA.gat_forward(H, el, er, *graph, PS)
    got = GNNA.gat_backward(H, el, er, lsem, Ym, G, *graph, PS, 0.2, None if transposed is None else list(transposed))
    _compare((Ym, lsem, *got), r, f"{kind} GNNAdvisor")
    assert torch.equal(lsem, lse), "lse is bit-reproducible: the layers must agree on it"
    assert (Hbuf[:, 0] == SENTINEL).all() and (Hbuf[:, -1] == SENTINEL).all() and (Gbuf[:, :3] == SENTINEL).all()


@pytest.mark.parametrize("kind", ["square", "rectangular"])
def test_sddmm(g, kind):
    """(sddmm refuses dim < 4: the smallest width that is no multiple of 4 is 5 here, again as column blocks)"""
    s = g.sym if kind == "square" else g.rect
    gen = torch.Generator().manual_seed(9)
    B = torch.randint(-3, 4, (6, 7), generator=gen).float().cuda()[:, 1:6]                   # leading dimension 7
    A = torch.randint(-3, 4, (s.n_out, 8), generator=gen).float().cuda()[:, 2:7]             # leading dimension 8
    ref = (A.cpu().double()[s.rows] * B.cpu().double()[s.cols]).sum(1)
    _same(_lib.sddmm(A, B, s.ci, s.pp, s.p2n, PS), GNNA.sddmm(A, B, s.ci, s.pp, s.p2n, PS), ref, f"sddmm {kind}, strided")
    A, B = A.contiguous(), B.contiguous()                                                   # (_lib: gnna_sddmm_f32)
    _same(_lib.sddmm(A, B, s.ci, s.pp, s.p2n, PS), GNNA.sddmm(A, B, s.ci, s.pp, s.p2n, PS), ref, f"sddmm {kind}, contiguous")


def test_xtg(g):
    G = g.base[:, :2]                                                             # (both layers copy a strided operand)
    ref = g.X.cpu().double().t() @ G.cpu().double()
    _same(_lib.xtg(g.X, G), GNNA.xtg(g.X, G), ref, "xtg")


@pytest.mark.parametrize("kind", ["square", "directed", "rectangular"])
def test_transpose_csr_and_build_part_device(g, kind):
    s = {"square": g.sym, "directed": g.directed, "rectangular": g.rect}[kind]
    perm = np.argsort(s.cols.numpy(), kind="stable")
    want_rp = np.r_[0, np.cumsum(np.bincount(s.cols.numpy(), minlength=s.n_in))]
    a = _lib.transpose_csr(s.rp, s.ci, num_in_rows=s.n_in)
    b = GNNA.transpose_csr(s.rp, s.ci, s.n_in)
    for name, x, y, ref in zip(("t_row_pointers", "t_column_index", "t_perm"), a, b, (want_rp, s.rows.numpy()[perm], perm)):
        _same(x, y, torch.from_numpy(np.asarray(ref)), f"{kind} {name}")
    assert len(GNNA.transpose_csr(s.rp, s.ci, s.n_in, False)) == 2 and _lib.transpose_csr(s.rp, s.ci, s.n_in, want_perm=False)[2] is None
    host = _lib.build_part(PS, a[0].cpu())
    for name, x, y, ref in zip(("partPtr", "part2Node"), _lib.build_part_device(PS, a[0]), GNNA.build_part_device(PS, a[0]), host):
        _same(x, y, ref, f"{kind} {name}")

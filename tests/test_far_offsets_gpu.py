"""Every entry point that takes a leading dimension, with its row-strided operands 2^31 bytes, 2^32 bytes, 2^31 elements and 2^32
elements past their base pointers (tests/far_offsets.py holds the geometry and the graph).

The arena: one flat float32 buffer of 2^32 + 2^29 elements (18 GiB), allocated once per module and never filled as a whole.
Operands are torch.as_strided views of it (of its int32 / bfloat16 / float16 reinterpretation for `arg` and the 16-bit features).
Node-sized operands have 272 rows 2^24 floats (64 MiB) apart:

    row  32 starts 2^31 bytes past row 0   (the sign bit of a 32-bit byte offset)
    row  64 starts 2^32 bytes past it
    row 128 starts 2^31 float elements past it
    row 256 starts 2^32 float elements past it      (16-bit views: 2^25 elements apart; rows 64 and 128 are the element marks)

Segment-sized operands (pool outputs, their lse and gradients) have 18 rows 2^28 floats apart: the same marks at rows 2, 4, 8, 16.
Every operand of a call has its own column window at k * 4096 floats into the rows, k = 1, 2, ...; a case runs once with the windows
as they are (16 KiB aligned: the layout the gather reads in place) and once shifted by one float (no 16-byte piece is aligned).
The 4 floats on each side of an input window are NaN; those beside an output window hold a sentinel that must survive, and the
window itself starts as NaN / INT_MIN, which must not.  Before an input is written, the host asserts that its rows r and r mod 64,
r mod 128, r mod 256 differ (r mod 4, 8, 16 for the 18-row views): a kernel that dropped the high bits of an offset would read
or write such an aliased row and cannot pass.

The graph (far_offsets.graphs): 272 nodes, so that every arena row is a destination and a source.  Degrees: row 0: 0, row 1: 1,
rows 2 / 3 / 4: 63 / 64 / 65, row 5: a hub of 283 edges with 16 repeated ids, the other rows 6 to 23.  Every row of at least 5
edges has a source in each of [0, 32), [32, 64), [64, 128), [128, 256), [256, 272).  Variants: symmetric, directed (with the
device-built transpose), rectangular (270 x 272), and 63 x 63 for the narrow 32-bit-offset paths (63 * 2^26 bytes < 2^32, the top
offset bit set from row 32 on).  The pools run over 18 segments with an empty one.  partSize 32.

Sums, max / min / arg, SDDMM and the typed family run on small integers: exact in fp32 (and from bf16 / fp16) in any order, so
they are compared for equality with the integer reference.  The softmax-based families run on randn inputs against the fp64
reference of their own test files at those files' bounds.  Softmax aggregation and both pools ("the same bits on every run") are
also held to the bits of the same call on contiguous copies: none of them chooses its schedule by the leading dimension."""
import types

import numpy as np
import pytest
import torch

import attnpool_ref
import dotattn_ref as tref
import far_offsets as F
import gat_drop_ref as dref
import gat_edge_ref as eref
import gat_rect_ref as gref
import gatv2_ref as vref
import pool_ref
import softagg_ref as S
from gnnadvisor_osdi21_amd import _lib, load_extension
from test_attnpool_gpu import _worst as attnpool_worst
from test_dotattn_gpu import _compare as dot_compare
from test_gat_drop_gpu import _compare_drop as drop_compare
from test_gat_edge_gpu import _compare as edge_compare
from test_gat_rect_gpu import _compare as gat_compare
from test_gatv2_gpu import _compare as gatv2_compare
from test_softagg_gpu import _check as softagg_check

pytestmark = pytest.mark.gpu
GNNA = load_extension()
PS = 32
N = F.ROWS
ALIGN = pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
WIDTHS = pytest.mark.parametrize("dim", [64, 41])
SHAPES = pytest.mark.parametrize("heads,hdim", [(4, 16), (3, 5)])


@pytest.fixture(scope="module")
def arena():
    buf = torch.empty(F.ARENA_FLOATS, dtype=torch.float32, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def _structure(rp, ci, n_in):
    """Device CSR with its partition and, built on the device, its transpose (with the permutation) and the partition of that."""
    rp, ci = torch.from_numpy(rp), torch.from_numpy(ci)
    pp, p2n = _lib.build_part(PS, rp)
    n_out = rp.numel() - 1
    s = types.SimpleNamespace(rp=rp.cuda(), ci=ci.cuda(), pp=pp.cuda(), p2n=p2n.cuda(), n_out=n_out, n_in=n_in, nnz=ci.numel(),
                              rows=torch.repeat_interleave(torch.arange(n_out), (rp[1:] - rp[:-1]).long()), cols=ci.long())
    s.t_rp, s.t_ci, s.perm = _lib.transpose_csr(s.rp, s.ci, num_in_rows=n_in, want_perm=True)
    s.t_pp, s.t_p2n = _lib.build_part_device(PS, s.t_rp)
    s.transposed = (s.t_rp, s.t_ci, s.t_pp, s.t_p2n)
    s.graph = (s.rp, s.ci, s.pp, s.p2n)
    return s


@pytest.fixture(scope="module")
def g():
    """The structures on the device; far_offsets.graphs asserts the degree list, the symmetry and the five regions on the host."""
    made = F.graphs()
    return types.SimpleNamespace(**{k: _structure(*getattr(made, k)) for k in ("sym", "directed", "rect", "small")})


def _ints(rows, width, seed, lo=-3, hi=3, dtype=torch.float32):
    return torch.randint(lo, hi + 1, (rows, width), generator=torch.Generator().manual_seed(seed)).to(dtype)


def _randn(rows, width, seed):
    return torch.randn(rows, width, generator=torch.Generator().manual_seed(seed))


def _exact(got, ref, what):
    got = got.cpu()
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} against {tuple(ref.shape)}"
    assert torch.equal(got.double(), ref.double()), \
        f"{what}: {int((got.double() != ref.double()).sum())} of {ref.numel()} elements differ from the exact reference, first in " \
        f"row {int((got.double() != ref.double()).any(1).nonzero()[0])}"


def _sum64(s, X, coef=None):
    """Exact weighted neighbor sum in float64 on the host: out[i] = sum_e coef[e] X[col(e)]."""
    X = X.double()
    coef = torch.ones(s.nnz, dtype=torch.float64) if coef is None else coef.double()
    return torch.zeros(s.n_out, X.shape[1], dtype=torch.float64).index_add_(0, s.rows, coef[:, None] * X[s.cols])


def _reduce_ref(s, X, op):
    """Exact max / min over every row's edges and the smallest position that supplies it (0 and -1 for a row without edges)."""
    out, arg = torch.zeros(s.n_out, X.shape[1]), torch.full((s.n_out, X.shape[1]), -1, dtype=torch.int32)
    rp = s.rp.cpu()
    for i in range(s.n_out):
        a, b = int(rp[i]), int(rp[i + 1])
        if b > a:
            vals = X[s.cols[a:b]]
            best = vals.max(0).values if op == _lib.REDUCE_MAX else vals.min(0).values
            out[i] = best
            arg[i] = (a + (vals == best).int().argmax(0)).int()
    return out, arg


DEG = (1.0 + torch.arange(N) % 3)             # "degrees" 1, 2, 3: the GCN coefficients stay small integers


def _mode_coef(s, mode, eps):
    return [None, DEG[s.rows] * DEG[s.cols], torch.full((s.nnz,), eps)][mode]


# ---- base aggregation --------------------------------------------------------------------------------------------------------

TUNINGS = {"default": {}, "phases_4": dict(column_phases=4), "deterministic": dict(deterministic=1),
           "sweep_steps_aside": dict(sweep=1, column_phases=4)}


@ALIGN
@WIDTHS
@pytest.mark.parametrize("tuning", list(TUNINGS))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_agg_ld(arena, g, mode, tuning, dim, shift):
    """Plain into a poisoned far `out`, then accumulated onto what a far `out` holds and clamped at zero.  sweep_steps_aside: X spans
    more than 2^32 bytes, which the sweep kernel's 32-bit offsets do not serve: the streaming kernel must run, on the 4 phases."""
    s, eps = g.sym, 2.0
    X, base = _ints(N, dim, 10 + dim), _ints(N, dim, 20 + dim, -40, 40)
    ref = _sum64(s, X, _mode_coef(s, mode, eps))
    deg = DEG.cuda() if mode == 1 else None
    w = F.Windows(arena, shift)
    Xv = w.inp(X, what="X")
    out1, out2 = w.out("node", dim, what="out"), w.out("node", dim, fill=base, what="out (accumulate, relu)")
    try:
        _lib.set_tuning(**TUNINGS[tuning])
        before = _lib.runtime_counters()["sweep_launches"]
        assert _lib.agg_ld(mode, Xv, s.ci, s.pp, s.p2n, N, PS, degrees_out=deg, degrees_in=deg, epsilon=eps, out=out1) is out1
        phases = _lib.last_num_phases()
        _lib.agg_ld(mode, Xv, s.ci, s.pp, s.p2n, N, PS, degrees_out=deg, degrees_in=deg, epsilon=eps, out=out2, accumulate=True, relu=True)
        swept = _lib.runtime_counters()["sweep_launches"] - before
    finally:
        _lib.reset_tuning()
    _exact(out1, ref, f"agg_ld mode {mode} {tuning}")
    _exact(out2, torch.clamp(base.double() + ref, min=0), f"agg_ld mode {mode} {tuning}, accumulate and relu")
    w.check()
    assert swept == 0, "the sweep kernel ran on a source matrix of more than 2^32 bytes"
    if "column_phases" in TUNINGS[tuning]:
        assert phases == 4, f"the sliced schedule was asked for 4 phases and ran {phases}"


@ALIGN
@WIDTHS
def test_agg_ld_on_a_prepared_graph_with_packed_ids(arena, g, dim, shift):
    s = g.sym
    ci = s.ci.clone()                                     # (the plan is pinned to this copy of the ids, and leaves with it)
    X = _ints(N, dim, 30 + dim)
    w = F.Windows(arena, shift)
    Xv, out = w.inp(X, what="X"), w.out("node", dim, what="out")
    try:
        _lib.set_tuning(column_phases=4)
        _lib.prepare_graph(ci, s.pp, s.p2n, N, N, PS, dims=(dim,))
        before = _lib.runtime_counters()["packed_launches"]
        _lib.agg_ld(0, Xv, ci, s.pp, s.p2n, N, PS, out=out)
        packed = _lib.runtime_counters()["packed_launches"] - before
    finally:
        _lib.reset_tuning()
        _lib.release_graph(ci)
    _exact(out, _sum64(s, X), "agg_ld, prepared")
    w.check()
    assert packed == 1, "the prepared graph's packed ids were not used"


@ALIGN
@WIDTHS
@pytest.mark.parametrize("tuning", ["default", "phases_4", "sweep"])
def test_agg_ld_narrow_offsets_with_the_top_bit_set(arena, g, tuning, dim, shift):
    """63 rows: X spans 63 * 2^26 bytes < 2^32, so the 32-bit-offset instantiations run, and from row 32 on the top bit of the
    offset is set.  The sweep kernel serves this size: it must run when forced."""
    s = g.small
    X = _ints(63, dim, 40 + dim)
    w = F.Windows(arena, shift)
    Xv, out = w.inp(X, what="X"), w.out("node", dim, rows=63, what="out")
    try:
        _lib.set_tuning(**{"default": {}, "phases_4": dict(column_phases=4), "sweep": dict(sweep=1, column_phases=4, deterministic=0)}[tuning])
        before = _lib.runtime_counters()["sweep_launches"]
        _lib.agg_ld(0, Xv, s.ci, s.pp, s.p2n, 63, PS, out=out)
        swept = _lib.runtime_counters()["sweep_launches"] - before
    finally:
        _lib.reset_tuning()
    _exact(out, _sum64(s, X), f"agg_ld, 63 rows, {tuning}")
    w.check()
    assert swept == (1 if tuning == "sweep" else 0), f"{tuning}: {swept} sweep launches"


@ALIGN
@WIDTHS
def test_agg_rect_with_windows(arena, g, dim, shift):
    """agg_rect takes a contiguous X: the arena itself as a [rows, dim] matrix of 75 M (dim 64) or 117 M (dim 41) rows, the graph's
    272 sources every ceil(2^24 / dim) rows of it (2^24 floats apart or a little more: the marks fall at the same sources), the
    row before and the row after each of them NaN.  Four source windows, taken two at a time."""
    s = g.sym
    M = (F.ARENA_FLOATS - 8) // dim
    big = arena[shift: shift + M * dim].view(M, dim)
    every, first = -(-F.LD // dim), 4
    at = torch.arange(N, dtype=torch.int64) * every + first                               # increasing: the ids stay sorted
    assert int(at[-1]) + 2 <= M and int(at[64]) * dim * 4 >= 1 << 32 and int(at[256]) * dim >= 1 << 32
    X = _ints(N, dim, 50 + dim)
    F.distinct_rows(X, (64, 128, 256), "X")
    three = torch.as_strided(arena, (N, 3 * dim), (every * dim, 1), (first - 1) * dim + shift)
    three.fill_(float("nan"))
    three[:, dim: 2 * dim].copy_(X.cuda())
    assert three[:, dim: 2 * dim].data_ptr() == big[first].data_ptr() and torch.equal(big[int(at[-1])].cpu(), X[-1])
    ci = at[s.cols].int().cuda()
    out = _lib.agg_rect(0, big, ci, s.pp, s.p2n, N, PS, windows=(4, 0, 2))
    _lib.agg_rect(0, big, ci, s.pp, s.p2n, N, PS, out=out, accumulate=True, windows=(4, 2, 4))
    _exact(out, _sum64(s, X), "agg_rect over 4 windows")


@ALIGN
@WIDTHS
@pytest.mark.parametrize("out_dtype", ["same", "float32"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_agg_ld_x16(arena, g, dtype, out_dtype, dim, shift):
    s = g.sym
    out_dtype = dtype if out_dtype == "same" else torch.float32
    X = _ints(N, dim, 60 + dim)
    w = F.Windows(arena, shift)
    Xv = w.inp(X.to(dtype), what="X")
    assert Xv.stride(0) == 1 << 25
    for mode, eps in ((0, 1.0), (2, 2.0)):
        ref = _sum64(s, X, _mode_coef(s, mode, eps))
        out = w.out("node", dim, dtype=out_dtype, what=f"out, mode {mode}")
        assert _lib.agg_ld_x16(mode, Xv, s.ci, s.pp, s.p2n, N, PS, epsilon=eps, out=out) is out
        # (the fp32 sum is exact; a 16-bit result is that sum rounded once)
        _exact(out.float(), ref.float().to(out_dtype).float(), f"agg_ld_x16 {dtype} -> {out_dtype}, mode {mode}")
    base = _ints(N, dim, 70 + dim, -40, 40)
    acc = w.out("node", dim, fill=base, what="out (accumulate, relu)")
    _lib.agg_ld_x16(0, Xv, s.ci, s.pp, s.p2n, N, PS, out=acc, accumulate=True, relu=True)
    _exact(acc, torch.clamp(base.double() + _sum64(s, X), min=0), f"agg_ld_x16 {dtype}, accumulate and relu")
    w.check()


@ALIGN
@WIDTHS
def test_agg_edge(arena, g, dim, shift):
    s = g.directed
    X, base = _ints(N, dim, 270 + dim), _ints(N, dim, 280 + dim, -40, 40)
    wgt = _ints(s.nnz, 1, 290 + dim, -2, 2)[:, 0].contiguous()
    ref = _sum64(s, X, wgt)
    w = F.Windows(arena, shift)
    Xv = w.inp(X, what="X")
    out, acc = w.out("node", dim, what="out"), w.out("node", dim, fill=base, what="out (accumulate, relu)")
    assert _lib.agg_edge(Xv, s.ci, wgt.cuda(), s.pp, s.p2n, N, PS, out=out) is out
    _lib.agg_edge(Xv, s.ci, wgt.cuda(), s.pp, s.p2n, N, PS, out=acc, accumulate=True, relu=True)
    _exact(out, ref, "agg_edge")
    _exact(acc, torch.clamp(base.double() + ref, min=0), "agg_edge, accumulate and relu")
    w.check()


@ALIGN
@WIDTHS
@pytest.mark.parametrize("kind", ["sym", "rect"])
def test_sddmm(arena, g, kind, dim, shift):
    s = getattr(g, kind)
    A, B = _ints(s.n_out, dim, 80 + dim), _ints(s.n_in, dim, 90 + dim)
    w = F.Windows(arena, shift)
    Av, Bv = w.inp(A, what="dst_feat"), w.inp(B, what="src_feat")
    got = _lib.sddmm(Av, Bv, s.ci, s.pp, s.p2n, PS)
    ref = (A.double()[s.rows] * B.double()[s.cols]).sum(1)
    _exact(got[:, None], ref[:, None], f"sddmm {kind}")
    _exact(GNNA.sddmm(Av, Bv, s.ci, s.pp, s.p2n, PS)[:, None], ref[:, None], f"GNNAdvisor sddmm {kind}")


# ---- max / min, scatter_arg, statistics --------------------------------------------------------------------------------------

@ALIGN
@WIDTHS
@pytest.mark.parametrize("op", [_lib.REDUCE_MAX, _lib.REDUCE_MIN], ids=["max", "min"])
def test_agg_reduce_and_scatter_arg(arena, g, op, dim, shift):
    s = g.directed
    X, grad = _ints(N, dim, 100 + dim, -8, 8), _ints(N, dim, 110 + dim)
    ref, ref_arg = _reduce_ref(s, X, op)
    w = F.Windows(arena, shift)
    Xv = w.inp(X, what="X")
    out, arg = w.out("node", dim, what="out"), w.out("node", dim, dtype=torch.int32, what="arg")
    got = _lib.agg_reduce_ld(op, Xv, s.ci, s.pp, s.p2n, PS, out=out, arg=arg)
    assert got[0] is out and got[1] is arg
    _exact(out, ref, "agg_reduce_ld")
    _exact(arg, ref_arg, "agg_reduce_ld arg")
    out_r = w.out("node", dim, what="out (relu)")
    _lib.agg_reduce_ld(op, Xv, s.ci, s.pp, s.p2n, PS, out=out_r, want_arg=False, relu=True)
    _exact(out_r, torch.clamp(ref, min=0), "agg_reduce_ld, relu")
    # the backward: gradient and arg far, and the atomics land in far rows
    want = torch.zeros(N, dim, dtype=torch.float64)
    rows, cols = (ref_arg >= 0).nonzero(as_tuple=True)
    want.index_put_((s.cols[ref_arg[rows, cols].long()], cols), grad.double()[rows, cols], accumulate=True)
    gv, av = w.inp(grad, what="grad_out"), w.inp(ref_arg, what="arg")
    d1 = w.out("node", dim, what="scatter_arg out")
    base = _ints(N, dim, 120 + dim, -40, 40)
    d2 = w.out("node", dim, fill=base, what="scatter_arg out (accumulate)")
    assert _lib.scatter_arg_ld(gv, av, s.ci, N, out=d1) is d1
    _lib.scatter_arg_ld(gv, av, s.ci, N, out=d2, accumulate=True)
    _exact(d1, want, "scatter_arg_ld")
    _exact(d2, base.double() + want, "scatter_arg_ld, accumulate")
    w.check()


@ALIGN
@WIDTHS
def test_agg_reduce_through_the_extension_module(arena, g, dim, shift):
    s = g.directed
    X = _ints(N, dim, 130 + dim, -8, 8)
    w = F.Windows(arena, shift)
    Xv, out = w.inp(X, what="X"), w.out("node", dim, what="out")
    for op in (_lib.REDUCE_MAX, _lib.REDUCE_MIN):
        ref, ref_arg = _reduce_ref(s, X, op)
        got, arg = GNNA.aggregate_reduce(op, Xv, s.ci, s.pp, s.p2n, PS, out=out)
        _exact(out, ref, "aggregate_reduce")
        _exact(arg, ref_arg, "aggregate_reduce arg")
        w.check()
        out.fill_(float("nan"))
        grad = _ints(N, dim, 140 + dim)
        gv = w.inp(grad, what="grad_out")                                  # (the module takes a contiguous arg and allocates the result)
        want = torch.zeros(N, dim, dtype=torch.float64)
        rows, cols = (ref_arg >= 0).nonzero(as_tuple=True)
        want.index_put_((s.cols[ref_arg[rows, cols].long()], cols), grad.double()[rows, cols], accumulate=True)
        _exact(GNNA.scatter_arg(gv, ref_arg.cuda(), s.ci, N), want, "scatter_arg")


@ALIGN
@WIDTHS
def test_agg_stats_with_every_output_far(arena, g, dim, shift):
    s = g.directed
    X = _ints(N, dim, 150 + dim, -8, 8)
    w = F.Windows(arena, shift)
    Xv = w.inp(X, what="X")
    out = {name: w.out("node", dim, what=name) for name in _lib.STATS}
    out.update({name: w.out("node", dim, dtype=torch.int32, what=name) for name in ("argmax", "argmin")})
    res = _lib.agg_stats_ld(Xv, s.ci, s.pp, s.p2n, out=out)
    assert all(res[k] is out[k] for k in out)
    _exact(out["sum"], _sum64(s, X), "sum")
    _exact(out["sumsq"], _sum64(s, X * X), "sumsq")
    for name, op in (("max", _lib.REDUCE_MAX), ("min", _lib.REDUCE_MIN)):
        ref, ref_arg = _reduce_ref(s, X, op)
        _exact(out[name], ref, name)
        _exact(out["arg" + name], ref_arg, "arg" + name)
    w.check()


# ---- the typed family --------------------------------------------------------------------------------------------------------

@ALIGN
@WIDTHS
def test_typed_expand_contract_and_coef_grad(arena, g, dim, shift):
    s, R, B = g.directed, 5, 3
    gen = torch.Generator().manual_seed(160 + dim)
    ety = torch.randint(0, R, (s.nnz,), generator=gen).int()
    nrm = torch.randint(1, 3, (s.nnz,), generator=gen).float()
    coef = torch.randint(-2, 3, (R, B), generator=gen).float()
    X, G = _ints(N, dim, 170 + dim), _ints(N, B * dim, 180 + dim)
    c = (nrm[:, None] * coef[ety.long()]).double()                                    # [nnz, B]
    w = F.Windows(arena, shift)
    Xv, Gv = w.inp(X, what="X"), w.inp(G, what="G")
    dev = (s.ci, ety.cuda(), nrm.cuda(), s.pp, s.p2n)
    # expand: out[i, b * dim + f] = sum_e c[e, b] X[col(e), f]
    want = torch.zeros(N, B, dim, dtype=torch.float64).index_add_(0, s.rows, c[:, :, None] * X.double()[s.cols][:, None, :])
    out = w.out("node", B * dim, what="expand out")
    assert _lib.agg_typed_expand(Xv, coef.cuda(), *dev, N, PS, out=out) is out
    _exact(out, want.view(N, B * dim), "agg_typed_expand")
    # contract: out[i, f] = sum_e sum_b c[e, b] G[col(e), b * dim + f]
    want = torch.zeros(N, dim, dtype=torch.float64).index_add_(0, s.rows, (c[:, :, None] * G.double().view(N, B, dim)[s.cols]).sum(1))
    out = w.out("node", dim, what="contract out")
    assert _lib.agg_typed_contract(Gv, coef.cuda(), *dev, N, PS, out=out) is out
    _exact(out, want, "agg_typed_contract")
    # coef_grad: out[r, b] = sum_{e of type r} n[e] <X[col(e)], G[row(e), b]>
    dots = (X.double()[s.cols][:, None, :] * G.double().view(N, B, dim)[s.rows]).sum(-1) * nrm.double()[:, None]
    want = torch.zeros(R, B, dtype=torch.float64).index_add_(0, ety.long(), dots)
    _exact(_lib.typed_coef_grad(Xv, Gv, *dev, R, PS), want, "typed_coef_grad")
    w.check()


# ---- softmax aggregation -----------------------------------------------------------------------------------------------------

@ALIGN
@WIDTHS
def test_agg_softmax_and_backward(arena, g, dim, shift):
    s = g.directed
    X, dY = _randn(N, dim, 190 + dim), _randn(N, dim, 200 + dim)
    t = 3.0 * torch.randn(dim, generator=torch.Generator().manual_seed(210 + dim))
    ref = S.reference(X, t, s.rp.cpu(), s.ci.cpu(), dY)
    w = F.Windows(arena, shift)
    Xv, dYv, tv = w.inp(X, what="X"), w.inp(dY, what="dY"), t.cuda()
    out, lse, sq, dX = (w.out("node", dim, what=name) for name in ("out", "lse", "sq", "dX"))
    got = _lib.agg_softmax(Xv, tv, s.rp, s.ci, out=out, lse=lse, sq=sq)
    assert got[0] is out and got[1] is lse and got[2] is sq
    assert _lib.agg_softmax_backward(Xv, tv, lse, out, dYv, s.t_rp, s.t_ci, out=dX) is dX
    softagg_check((out, lse, sq, dX), ref, f"agg_softmax D={dim}")
    w.check()
    # the same bits as on contiguous copies (one schedule whatever the leading dimension)
    c = _lib.agg_softmax(X.cuda(), tv, s.rp, s.ci, want_sq=True)
    cdX = _lib.agg_softmax_backward(X.cuda(), tv, c[1], c[0], dY.cuda(), s.t_rp, s.t_ci)
    for name, a, b in zip(("out", "lse", "sq", "dX"), (out, lse, sq, dX), (*c, cdX)):
        assert torch.equal(a, b), f"agg_softmax {name}: other bits than on contiguous operands"


# ---- fused attention ---------------------------------------------------------------------------------------------------------

@ALIGN
@SHAPES
@pytest.mark.parametrize("kind", ["sym", "directed", "rect"])
def test_gat_forward_and_backward(arena, g, kind, heads, hdim, shift):
    s, W = getattr(g, kind), heads * hdim
    H, el, er, G = gref.inputs(s.n_out, s.n_in, heads, hdim, seed=11 + heads)
    r = gref.kernel_reference(H.cuda(), el.cuda(), er.cuda(), G.cuda(), s.rp, s.ci, heads, 0.2, kind)
    w = F.Windows(arena, shift)
    Hv, Gv, el, er = w.inp(H, what="H"), w.inp(G, what="dY"), el.cuda(), er.cuda()
    Y, dH = w.out("node", W, rows=s.n_out, what="out"), w.out("node", W, rows=s.n_in, what="dH")
    transposed = None if kind == "sym" else s.transposed
    got = _lib.gat_forward(Hv, el, er, *s.graph, PS, out=Y)
    assert got[0] is Y
    lse = got[1]
    got = _lib.gat_backward(Hv, el, er, lse, Y, Gv, *s.graph, PS, dH=dH, transposed=transposed)
    assert got[0] is dH
    gat_compare((Y, lse, dH, got[1], got[2]), r, f"gat {kind} {heads}x{hdim}")
    w.check()
    # the extension module: its own outputs, the far inputs
    Ym, lsem = GNNA.gat_forward(Hv, el, er, *s.graph, PS)
    gm = GNNA.gat_backward(Hv, el, er, lsem, Y, Gv, *s.graph, PS, 0.2, None if transposed is None else list(transposed))
    gat_compare((Ym, lsem, *gm), r, f"GNNAdvisor gat {kind} {heads}x{hdim}")
    assert torch.equal(lsem, lse)


@ALIGN
@SHAPES
def test_gat_drop_forward_and_backward(arena, g, heads, hdim, shift):
    s, W, p, seed = g.directed, heads * hdim, 0.5, 0x1234
    H, el, er, G = gref.inputs(s.n_out, s.n_in, heads, hdim, seed=21 + heads)
    r = dref.kernel_reference(H.cuda(), el.cuda(), er.cuda(), G.cuda(), s.rp, s.ci, heads, 0.2, p, seed, "drop")
    w = F.Windows(arena, shift)
    Hv, Gv, el, er = w.inp(H, what="H"), w.inp(G, what="dY"), el.cuda(), er.cuda()
    Y, dH = w.out("node", W, what="out"), w.out("node", W, what="dH")
    _, lse = _lib.gat_forward_drop(Hv, el, er, *s.graph, PS, 0.2, p, seed, out=Y)
    got = _lib.gat_backward_drop(Hv, el, er, lse, Y, Gv, *s.graph, PS, 0.2, p, seed, dH=dH, transposed=s.transposed)
    drop_compare((Y, lse, dH, got[1], got[2]), r, f"gat_drop {heads}x{hdim}")
    w.check()


@ALIGN
@SHAPES
def test_gat_edge_forward_and_backward(arena, g, heads, hdim, shift):
    s, W = g.directed, heads * hdim
    H, el, er, G = gref.inputs(s.n_out, s.n_in, heads, hdim, seed=31 + heads)
    ee = torch.randn(s.nnz, heads, generator=torch.Generator().manual_seed(9)).cuda()
    r = eref.kernel_reference(H.cuda(), el.cuda(), er.cuda(), ee, G.cuda(), s.rp, s.ci, heads, 0.2, 0.5, 0xABCDEF, what="edge")
    w = F.Windows(arena, shift)
    Hv, Gv, el, er = w.inp(H, what="H"), w.inp(G, what="dY"), el.cuda(), er.cuda()
    Y, dH = w.out("node", W, what="out"), w.out("node", W, what="dH")
    _, lse = _lib.gat_edge_forward(Hv, el, er, ee, *s.graph, PS, 0.2, 0.5, 0xABCDEF, out=Y)
    alpha = _lib.gat_alpha(el, er, ee, lse, s.rp, s.ci, 0.2)
    got = _lib.gat_edge_backward(Hv, el, er, ee, lse, Y, Gv, *s.graph, s.perm, PS, 0.2, 0.5, 0xABCDEF, transposed=s.transposed, dH=dH)
    edge_compare((Y, lse, alpha, dH, got[1], got[2], got[3]), r, f"gat_edge {heads}x{hdim}")
    w.check()


@ALIGN
@SHAPES
@pytest.mark.parametrize("kind", ["sym", "rect"])
def test_gatv2_forward_and_backward(arena, g, kind, heads, hdim, shift):
    s, W = getattr(g, kind), heads * hdim
    Hs, Hd, att, G = vref.inputs(s.n_out, s.n_in, heads, hdim, 41 + heads)
    r = vref.kernel_reference(Hs.cuda(), Hd.cuda(), att.cuda(), G.cuda(), s.rp, s.ci, heads, 0.2, 0.0, 0, f"gatv2 {kind}")
    w = F.Windows(arena, shift)
    Hsv, Hdv, Gv, att = w.inp(Hs, what="Hs"), w.inp(Hd, what="Hd"), w.inp(G, what="dY"), att.cuda()
    Y, dHs, dHd = w.out("node", W, rows=s.n_out, what="out"), w.out("node", W, rows=s.n_in, what="dHs"), w.out("node", W, rows=s.n_out, what="dHd")
    _, lse = _lib.gatv2_forward(Hsv, Hdv, att, *s.graph, PS, out=Y)
    got = _lib.gatv2_backward(Hsv, Hdv, att, lse, Y, Gv, *s.graph, PS, transposed=None if kind == "sym" else s.transposed, dHs=dHs, dHd=dHd)
    assert got[0] is dHs and got[1] is dHd
    gatv2_compare((Y, lse, dHs, dHd, got[2]), r, f"gatv2 {kind} {heads}x{hdim}")
    w.check()


@ALIGN
@SHAPES
@pytest.mark.parametrize("kind", ["sym", "directed"])
def test_dot_attn_forward_and_backward(arena, g, kind, heads, hdim, shift):
    """Q, K and V are three windows of the same arena rows, as the ops layer passes three column blocks of one projection."""
    s, W = getattr(g, kind), heads * hdim
    Q, K, V, G = tref.inputs(s.n_out, s.n_in, heads, hdim, 51 + heads)
    scale = 1.0 / hdim ** 0.5
    r = tref.kernel_reference(Q.cuda(), K.cuda(), V.cuda(), G.cuda(), s.rp, s.ci, heads, scale)
    w = F.Windows(arena, shift)
    Qv, Kv, Vv, Gv = w.inp(Q, what="Q"), w.inp(K, what="K"), w.inp(V, what="V"), w.inp(G, what="dY")
    Y, dQ, dK, dV = (w.out("node", W, what=name) for name in ("out", "dQ", "dK", "dV"))
    _, lse = _lib.dot_attn_forward(Qv, Kv, Vv, heads, *s.graph, PS, out=Y)
    got = _lib.dot_attn_backward(Qv, Kv, Vv, heads, lse, Y, Gv, *s.graph, PS, transposed=None if kind == "sym" else s.transposed,
                                 dQ=dQ, dK=dK, dV=dV)
    assert got[0] is dQ and got[1] is dK and got[2] is dV
    dot_compare((Y, lse, dQ, dK, dV), r, f"dot_attn {kind} {heads}x{hdim}")
    w.check()


# ---- the pools ---------------------------------------------------------------------------------------------------------------

LAYOUTS = pytest.mark.parametrize("layout", list(F.SEGMENTS))


@ALIGN
@WIDTHS
@LAYOUTS
def test_segment_pool_and_backward(arena, layout, dim, shift):
    gp = F.SEGMENTS[layout]
    gpd = torch.from_numpy(gp).cuda()
    X = _ints(N, dim, 220 + dim, -8, 8)
    ref = pool_ref.forward(X.numpy(), gp)
    assert (ref["count"] == 0).any()
    w = F.Windows(arena, shift)
    Xv = w.inp(X, what="X")
    out = {name: w.out("seg", dim, what=name) for name in _lib.POOL_STATS}
    out.update({name: w.out("seg", dim, dtype=torch.int32, what=name) for name in ("argmax", "argmin")})
    res = _lib.segment_pool(Xv, gpd, want=_lib.POOL_STATS, out=out)
    assert all(res[k] is out[k] for k in out)
    for name in ("sum", "max", "min", "argmax", "argmin"):
        _exact(out[name], torch.from_numpy(np.ascontiguousarray(ref[name])), f"segment_pool {name}")
    mean = w.out("seg", dim, what="mean")
    _lib.segment_pool(Xv, gpd, want=("sum",), mean=True, out={"sum": mean})
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), pool_ref.mean_f32(X.numpy(), gp).view(np.uint32)), "mean"
    same = _lib.segment_pool(X.cuda(), gpd, want=_lib.POOL_STATS)
    assert all(torch.equal(same[k], out[k]) for k in out), "other bits than on a contiguous X"
    # the module, on the far X
    for name, t in zip(("sum", "max", "argmax", "min", "argmin"), GNNA.segment_pool(Xv, gpd, True, True, True, False)):
        assert torch.equal(t, out[name]), f"GNNAdvisor segment_pool {name}"
    # backward: every gradient and both position arrays far and segment-sized, dX node-sized
    grads = {name: _ints(F.SEG_ROWS, dim, 230 + dim + k, -4, 4) for k, name in enumerate(("d_sum", "d_max", "d_min"))}
    gv = {name: w.inp(t, kind="seg", what=name) for name, t in grads.items()}
    for is_mean in (False, True):
        dX = w.out("node", dim, what=f"dX mean={is_mean}")
        assert _lib.segment_pool_backward(gpd, N, d_sum=gv["d_sum"], d_max=gv["d_max"], argmax=out["argmax"], d_min=gv["d_min"],
                                          argmin=out["argmin"], mean=is_mean, out=dX) is dX
        want = pool_ref.backward(gp, N, dim, mean=is_mean, argmax=ref["argmax"], argmin=ref["argmin"],
                                 **{k: v.numpy() for k, v in grads.items()})
        assert np.array_equal(dX.cpu().numpy(), want), f"segment_pool_backward mean={is_mean}"
    w.check()


@ALIGN
@WIDTHS
@LAYOUTS
@pytest.mark.parametrize("per", ["row", "element"])
def test_segment_attn_pool_and_backward(arena, per, layout, dim, shift):
    gp = F.SEGMENTS[layout]
    gpd = torch.from_numpy(gp).cuda()
    gd = 1 if per == "row" else dim
    rng = np.random.default_rng(240 + dim)
    X, gate = rng.standard_normal((N, dim)).astype(np.float32), (2.0 * rng.standard_normal((N, gd))).astype(np.float32)
    dY = rng.standard_normal((F.SEG_ROWS, dim)).astype(np.float32)
    ref = attnpool_ref.reference(X, gate, gp, dY)
    w = F.Windows(arena, shift)
    Xv, gv = w.inp(torch.from_numpy(X), what="X"), w.inp(torch.from_numpy(gate), what="gate")
    dYv = w.inp(torch.from_numpy(dY), kind="seg", what="dY")
    out = {"out": w.out("seg", dim, what="out"), "lse": w.out("seg", gd, what="lse")}
    res = _lib.segment_attn_pool(Xv, gv, gpd, out=out)
    assert res["out"] is out["out"] and res["lse"] is out["lse"]
    given = {"d_input": w.out("node", dim, what="d_input"), "d_gate": w.out("node", gd, what="d_gate")}
    d_input, d_gate = _lib.segment_attn_pool_backward(Xv, gv, out["lse"], out["out"], dYv, gpd, out=given)
    assert d_input is given["d_input"] and d_gate is given["d_gate"]
    got = {k: v.cpu().numpy() for k, v in {**out, **given}.items()}
    print("worst ratio to the bound:", attnpool_worst(got, ref, ("out", "lse", "d_input", "d_gate")))
    w.check()
    Xc, gc = torch.from_numpy(X).cuda(), torch.from_numpy(gate).cuda()
    same = _lib.segment_attn_pool(Xc, gc, gpd)
    sd = _lib.segment_attn_pool_backward(Xc, gc, same["lse"], same["out"], torch.from_numpy(dY).cuda(), gpd)
    for name, a, b in (("out", out["out"], same["out"]), ("lse", out["lse"], same["lse"]), ("d_input", d_input, sd[0]), ("d_gate", d_gate, sd[1])):
        assert torch.equal(a, b), f"segment_attn_pool {name}: other bits than on contiguous operands"


# ---- the general aggregation through the extension module ---------------------------------------------------------------------

@ALIGN
@WIDTHS
def test_aggregate_ld_through_the_extension_module(arena, g, dim, shift):
    s = g.sym
    X, base = _ints(N, dim, 250 + dim), _ints(N, dim, 260 + dim, -40, 40)
    w = F.Windows(arena, shift)
    Xv = w.inp(X, what="X")
    Xb = w.inp(X.bfloat16(), what="X bf16")
    for mode in (0, 1, 2):
        ref = _sum64(s, X, _mode_coef(s, mode, 2.0))
        deg = DEG.cuda() if mode == 1 else None
        out, acc = w.out("node", dim, what=f"out mode {mode}"), w.out("node", dim, fill=base, what=f"out mode {mode} (accumulate, relu)")
        GNNA.aggregate_ld(mode, Xv, s.ci, deg, 2.0, s.pp, s.p2n, PS, out=out)
        GNNA.aggregate_ld(mode, Xv, s.ci, deg, 2.0, s.pp, s.p2n, PS, out=acc, accumulate=True, relu=True)
        _exact(out, ref, f"aggregate_ld mode {mode}")
        _exact(acc, torch.clamp(base.double() + ref, min=0), f"aggregate_ld mode {mode}, accumulate and relu")
    outb = w.out("node", dim, what="out from bf16")
    GNNA.aggregate_ld(0, Xb, s.ci, None, 1.0, s.pp, s.p2n, PS, out=outb)
    _exact(outb, _sum64(s, X), "aggregate_ld bf16 -> float32")
    w.check()

"""The gather kernels with more than one neighbor-group per wavefront and a partial last chunk, on the GPU.

The parity tests use graphs too small to leave G = 1 groups per wavefront on a 256-CU device (G is halved while there are fewer
than T = 16 * compute units chunks), so the chunk geometry the four kernel families share (csrc/gnna_launch.h) is exercised here:
N rows with exactly one edge each, row i reading column (i * 7919) % N, so that num_parts = N at any partSize, with N just
above and just below the sizes at which G changes -- (64 T + 1, 32) -> G = 64 and one group in the last chunk, (64 T - 64, 32) ->
G = 32, (20 T + 3, 100) -> G = 20 (not a power of two) and 3 groups in the last chunk, (20 T - 20, 100) -> G = 10.

With one edge per row the sum, the max and the softmax-weighted row are a single term, so the 16-bit, reduce and GAT results
must EQUAL the gathered row (computed here on the CPU), and the typed one is a product of three factors (fp64 reference, 1e-4).

With one edge per row every group is a run of its own.  The multi-edge variants at the end run the same four families on
gat_rect_ref.multi_run_structure -- (64 T + 1, 1) -> G = 64, rows of 0 .. 12 groups, and (7 T, 100) -> G = 5, every 50th row three
groups -- where a wavefront merges the groups of a row into a run, walks several runs, and rows are cut by chunk and workgroup
boundaries (tests/test_attn_cases_host.py asserts that of the structures; tests/test_attn_chunks_gpu.py runs the attention
kernels on them).  Ids are folded onto 251 source rows.  References: the CSR oracle (x16), reduce_ref (max / min; the position is
the smallest winning one), pna_ref's centred moments turned back into sum and sum of squares (stats), rgcn_ref's dense relations
(typed); the sums within the project's bound 1e-4 * max(1, sum of |terms|), the extrema and their positions exactly."""
import functools

import numpy as np
import pytest
import torch

import attn_cases
import gat_rect_ref as gref
import oracle
import pna_ref
import reduce_ref
import rgcn_ref
from gnnadvisor_osdi21_amd import _lib
from util import assert_close_f64

pytestmark = pytest.mark.gpu

SLOPE = 0.2
# (id, N from T, partSize)
SHAPES = [("64T+1_ps32", lambda T: 64 * T + 1, 32), ("64T-64_ps32", lambda T: 64 * T - 64, 32),
          ("20T+3_ps100", lambda T: 20 * T + 3, 100), ("20T-20_ps100", lambda T: 20 * T - 20, 100)]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])


@functools.lru_cache(maxsize=None)
def _case(n):
    """The graph and every input and expected value for N = n rows, on the CPU; made once, never written to."""
    gen = torch.Generator().manual_seed(n)
    col = (torch.arange(n, dtype=torch.int64) * 7919) % n
    c = dict(n=n, col=col)
    c["rp"] = torch.arange(n + 1, dtype=torch.int32)          # one edge per row: row pointers = group pointers
    c["p2n"] = torch.arange(n, dtype=torch.int32)
    c["X"] = torch.randn(n, 4, generator=gen)
    c["X16"] = torch.randn(n, 8, generator=gen).bfloat16()
    c["el"], c["er"] = torch.randn(n, 1, generator=gen), torch.randn(n, 1, generator=gen)
    c["ety"] = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int32)
    c["enorm"] = torch.rand(n, generator=gen) + 0.5
    c["coef"] = torch.randn(2, 2, generator=gen)
    # the single term of every row, in fp64
    c["gathered"] = c["X"].double()[col]
    c["gathered16"] = c["X16"].double()[col]
    z = (c["el"].double() + c["er"].double()[col]).float()                 # (an fp32 sum is the rounded exact sum)
    c["score"] = torch.where(z > 0, z, (z.double() * float(np.float32(SLOPE))).float())
    w = c["enorm"].double()[:, None] * c["coef"].double()[c["ety"].long()]                    # [n, bases]
    c["typed"] = (w[:, :, None] * c["gathered"][:, None, :]).reshape(n, 8)
    return c


def _graph(shape):
    c = _case(shape[1](16 * _lib.device_cus()))
    return c, c["col"].int().cuda(), c["rp"].cuda(), c["p2n"].cuda(), shape[2]


def _equal(got, want64, what):
    """Every element of `got` equals the fp64 value (which is an fp32 / bf16 number here)."""
    got, want64 = got.double().cpu(), want64.double()
    assert got.shape == want64.shape
    off = ~(got == want64)                  # (a NaN compares false: it counts as off)
    assert not off.any(), f"{what}: {int(off.sum())} of {off.numel()} elements differ"


def _x16(shape, relu):
    c, col, pp, p2n, ps = _graph(shape)
    out = _lib.agg_ld_x16(_lib.MODE_SAG, c["X16"].cuda(), col, pp, p2n, c["n"], ps, out_dtype=torch.float32, relu=relu)
    assert out.dtype == torch.float32
    _equal(out, c["gathered16"].clamp(min=0) if relu else c["gathered16"], "agg_ld_x16")


def _gat(shape, relu):
    c, col, pp, p2n, ps = _graph(shape)
    out, lse = _lib.gat_forward(c["X"].cuda(), c["el"].cuda(), c["er"].cuda(), pp, col, pp, p2n, ps, SLOPE, relu=relu)
    _equal(lse, c["score"], "gat_forward lse")
    _equal(out, c["gathered"].clamp(min=0) if relu else c["gathered"], "gat_forward out")


@shapes
def test_x16_sum_of_one_term(shape):
    _x16(shape, relu=False)


@shapes
def test_reduce_max_of_one_term_and_its_position(shape):
    c, col, pp, p2n, ps = _graph(shape)
    out, arg = _lib.agg_reduce_ld(_lib.REDUCE_MAX, c["X"].cuda(), col, pp, p2n, ps)
    _equal(out, c["gathered"], "agg_reduce_ld values")
    assert torch.equal(arg.cpu(), torch.arange(c["n"], dtype=torch.int32)[:, None].expand(-1, 4)), "agg_reduce_ld positions"


@shapes
def test_gat_forward_of_one_edge_per_row(shape):
    _gat(shape, relu=False)


@shapes
def test_typed_expand_of_one_edge_per_row(shape):
    c, col, pp, p2n, ps = _graph(shape)
    out = _lib.agg_typed_expand(c["X"].cuda(), c["coef"].cuda(), col, c["ety"].cuda(), c["enorm"].cuda(), pp, p2n, c["n"], ps)
    assert_close_f64(out.cpu().numpy(), c["typed"].numpy(), what="agg_typed_expand")


def test_relu_epilogue_x16():
    _x16(SHAPES[0], relu=True)


def test_relu_epilogue_gat():
    _gat(SHAPES[0], relu=True)


# ---- several edges per row: runs of several groups, several runs per wavefront -----------------------------------------------------

MULTI = [0, 2]                            # of attn_cases.GEOMETRIES: (64 T + 1, 1) and (7 T, 100)
multi = pytest.mark.parametrize("k", MULTI, ids=[attn_cases.GEOMETRIES[k][0] for k in MULTI])
N_SRC = 251


@functools.lru_cache(maxsize=None)
def _multi_case(k):
    """The structure, every input and the fp64 references on the CPU; made once, never written to."""
    _, parts_of, ps, want_G = attn_cases.GEOMETRIES[k]
    P = parts_of(16 * _lib.device_cus())
    rp, ci, _ = gref.multi_run_structure(P, ps)
    rp, ci = torch.from_numpy(rp), torch.from_numpy(ci % N_SRC)
    pp, p2n = _lib.build_part(ps, rp)
    assert p2n.numel() == P and attn_cases.chunk_grid(P, ps, _lib.device_cus())[0] == want_G
    n = rp.numel() - 1
    gen = torch.Generator().manual_seed(900 + k)
    c = dict(n=n, ps=ps, rp=rp, ci=ci, pp=pp, p2n=p2n)
    c["X"] = torch.randn(N_SRC, 4, generator=gen)
    c["X16"] = torch.randn(N_SRC, 8, generator=gen).bfloat16()
    c["ety"] = torch.randint(0, 2, (ci.numel(),), generator=gen, dtype=torch.int32)
    c["enorm"] = torch.rand(ci.numel(), generator=gen) + 0.5
    c["coef"] = torch.randn(2, 2, generator=gen)
    rows, src = reduce_ref._rows_of(rp), ci.long()
    c["has"] = torch.bincount(rows, minlength=n) > 0
    X64 = c["X"].double()
    # x16: the CSR oracle over the bf16 values (exact in fp32), and over their magnitudes for the scale
    x16 = c["X16"].float().numpy()
    c["sum16"] = oracle.csr_f64(0, x16, rp.numpy(), ci.numpy())
    c["abs16"] = oracle.csr_f64(0, np.abs(x16), rp.numpy(), ci.numpy())
    # max / min and the smallest winning position (reduce_ref: the library's tie rule)
    S = X64[src]
    idx = rows[:, None].expand_as(S)
    pos = torch.arange(src.numel())[:, None].expand_as(S)
    for how in ("amax", "amin"):
        ext = reduce_ref._agg64(X64, rp, ci, how)
        cand = torch.where(S == ext[rows], pos, torch.full_like(pos, src.numel()))
        first = torch.full((n, 4), src.numel(), dtype=torch.int64).scatter_reduce(0, idx, cand, reduce="amin", include_self=True)
        c[how] = ext
        c["arg" + how] = torch.where(c["has"][:, None], first, torch.full_like(first, -1)).int()
    # sum and sum of squares from pna_ref's centred moments: sum = c mean, sumsq = c (var + mean^2)
    mean, std, mx, mn = pna_ref._stats64(X64, rows, src, n)
    cnt = torch.bincount(rows, minlength=n).double()[:, None]
    c["sum"], c["sumsq"] = cnt * mean, cnt * (std ** 2 - pna_ref.EPS + mean ** 2)
    assert torch.equal(mx, c["amax"]) and torch.equal(mn, c["amin"])
    c["abs"] = torch.zeros(n, 4, dtype=torch.float64).index_add_(0, rows, S.abs())
    return c


def _typed_reference(c):
    """rgcn_ref's dense relations (on the GPU), and the same on the magnitudes for the scale."""
    A = rgcn_ref.dense_relations(c["rp"], c["ci"], c["ety"], c["enorm"], 2, c["n"], N_SRC)
    X, coef = c["X"].double().cuda(), c["coef"].double().cuda()
    return rgcn_ref.dense_expand(A, X, coef).cpu().numpy(), rgcn_ref.dense_expand(A, X.abs(), coef.abs()).cpu().numpy()


@multi
def test_x16_sum_of_runs(k):
    c = _multi_case(k)
    out = _lib.agg_ld_x16(_lib.MODE_SAG, c["X16"].cuda(), c["ci"].cuda(), c["pp"].cuda(), c["p2n"].cuda(), c["n"], c["ps"],
                          out_dtype=torch.float32)
    assert_close_f64(out.cpu().numpy(), c["sum16"], scale=c["abs16"], what="agg_ld_x16")
    assert (out[~c["has"].cuda()] == 0).all()


@multi
@pytest.mark.parametrize("how", ["amax", "amin"])
def test_reduce_of_runs_and_its_positions(k, how):
    c = _multi_case(k)
    op = _lib.REDUCE_MAX if how == "amax" else _lib.REDUCE_MIN
    out, arg = _lib.agg_reduce_ld(op, c["X"].cuda(), c["ci"].cuda(), c["pp"].cuda(), c["p2n"].cuda(), c["ps"], num_out_rows=c["n"])
    _equal(out, c[how], f"agg_reduce_ld {how} values")
    assert torch.equal(arg.cpu(), c["arg" + how]), f"agg_reduce_ld {how} positions"


@multi
def test_stats_of_runs(k):
    c = _multi_case(k)
    res = _lib.agg_stats_ld(c["X"].cuda(), c["ci"].cuda(), c["pp"].cuda(), c["p2n"].cuda(), c["n"], c["ps"])
    assert_close_f64(res["sum"].cpu().numpy(), c["sum"].numpy(), scale=c["abs"].numpy(), what="agg_stats sum")
    assert_close_f64(res["sumsq"].cpu().numpy(), c["sumsq"].numpy(), scale=c["sumsq"].numpy(), what="agg_stats sumsq")
    for name, how in (("max", "amax"), ("min", "amin")):
        _equal(res[name], c[how], f"agg_stats {name}")
        assert torch.equal(res["arg" + name].cpu(), c["arg" + how]), f"agg_stats arg{name}"


@multi
def test_typed_expand_of_runs(k):
    c = _multi_case(k)
    out = _lib.agg_typed_expand(c["X"].cuda(), c["coef"].cuda(), c["ci"].cuda(), c["ety"].cuda(), c["enorm"].cuda(), c["pp"].cuda(),
                                c["p2n"].cuda(), c["n"], c["ps"])
    T, Ts = _typed_reference(c)
    assert_close_f64(out.cpu().numpy(), T, scale=Ts, what="agg_typed_expand")

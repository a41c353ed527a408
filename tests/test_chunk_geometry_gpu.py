"""The gather kernels with more than one neighbor-group per wavefront and a partial last chunk, on the GPU.

The parity tests use graphs too small to leave G = 1 groups per wavefront on a 256-CU device (G is halved while there are fewer
than T = 16 * compute units chunks), so the chunk geometry the four kernel families share (csrc/gnna_launch.h) is exercised here:
N rows with exactly one edge each, row i reading column (i * 7919) % N, so that num_parts = N at any partSize, with N just
above and just below the sizes at which G changes -- (64 T + 1, 32) -> G = 64 and one group in the last chunk, (64 T - 64, 32) ->
G = 32, (20 T + 3, 100) -> G = 20 (not a power of two) and 3 groups in the last chunk, (20 T - 20, 100) -> G = 10.

With one edge per row the sum, the max and the softmax-weighted row are a single term, so the 16-bit, reduce and GAT results
must EQUAL the gathered row (computed here on the CPU), and the typed one is a product of three factors (fp64 reference, 1e-4)."""
import functools

import numpy as np
import pytest
import torch

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

"""The three entries of include/gnna_segnorm.h with their row-strided operands 2^31 bytes, 2^32 bytes, 2^31 elements and 2^32
elements past their base pointers, built from tests/far_offsets.py as test_far_offsets_gpu.py builds its cases: node-sized operands
(X, dY, out, d_input) are 272 rows 64 MiB apart, segment-sized ones (mean, m2, rstd, seg_a, seg_b) 18 rows 1 GiB apart, each in its
own column window of an 18 GiB arena of this module, aligned and shifted by one float; NaN beside every input, a sentinel that must
survive beside every output, NaN inside it that must not.  The entries do not choose their schedule by a leading dimension ("the
same bits on every run"), so every output is held to the bits of the same call on contiguous copies -- which test_segnorm_gpu.py
holds to fp64."""
import numpy as np
import pytest
import torch

import far_offsets as F
from gnnadvisor_osdi21_amd import _lib

pytestmark = pytest.mark.gpu
N, DIM, EPS = F.ROWS, 41, 1e-5


@pytest.fixture(scope="module")
def arena():
    buf = torch.empty(F.ARENA_FLOATS, dtype=torch.float32, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def _randn(rows, width, seed):
    return torch.randn(rows, width, generator=torch.Generator().manual_seed(seed))


def _same(far, near, what):
    assert np.array_equal(far.cpu().numpy().view(np.uint32), near.cpu().numpy().view(np.uint32)), f"{what}: other bits than on contiguous operands"


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("layout", list(F.SEGMENTS))
def test_moments_norm_and_backward(arena, layout, shift):
    gp = F.SEGMENTS[layout]
    gpd = torch.from_numpy(gp).cuda()
    assert (np.diff(gp) == 0).any()                               # an empty segment among the 18
    X, dY = 1.5 + _randn(N, DIM, 31), _randn(N, DIM, 32)
    wgt, bias, alpha = (t.cuda() for t in (1.0 + 0.3 * _randn(1, DIM, 33)[0], _randn(1, DIM, 34)[0], 0.4 + 0.1 * _randn(1, DIM, 35)[0]))
    # on contiguous operands
    near_m = _lib.segment_moments(X.cuda(), gpd)
    near = _lib.segment_norm(X.cuda(), gpd, wgt, bias, alpha, EPS)
    near_dx, near_a, near_b = _lib.segment_norm_backward(dY.cuda(), X.cuda(), near["mean"], near["rstd"], gpd, wgt, alpha)
    # every operand far
    w = F.Windows(arena, shift)
    Xv, dYv = w.inp(X, what="X"), w.inp(dY, what="dY")
    mean, m2 = w.out("seg", DIM, what="mean"), w.out("seg", DIM, what="m2")
    res = _lib.segment_moments(Xv, gpd, out=dict(mean=mean, m2=m2))
    assert res["mean"] is mean and res["m2"] is m2
    _same(mean, near_m["mean"], "moments mean")
    _same(m2, near_m["m2"], "moments m2")
    out = dict(out=w.out("node", DIM, what="out"), mean=w.out("seg", DIM, what="norm mean"), rstd=w.out("seg", DIM, what="rstd"))
    res = _lib.segment_norm(Xv, gpd, wgt, bias, alpha, EPS, out=out)
    assert all(res[k] is out[k] for k in out)
    for name in out:
        _same(out[name], near[name], "norm " + name)
    # the backward reads the statistics from far, segment-sized inputs of their own
    mean_in = w.inp(near["mean"].cpu(), kind="seg", what="mean (input)")
    rstd_in = w.inp(near["rstd"].cpu(), kind="seg", what="rstd (input)")
    bwd = dict(d_input=w.out("node", DIM, what="d_input"), seg_a=w.out("seg", DIM, what="seg_a"), seg_b=w.out("seg", DIM, what="seg_b"))
    dx, A, B = _lib.segment_norm_backward(dYv, Xv, mean_in, rstd_in, gpd, wgt, alpha, out=bwd)
    assert dx is bwd["d_input"] and A is bwd["seg_a"] and B is bwd["seg_b"]
    _same(dx, near_dx, "d_input")
    _same(A, near_a, "seg_a")
    _same(B, near_b, "seg_b")
    # without d_input: the sums alone, far
    A2, B2 = w.out("seg", DIM, what="seg_a alone"), w.out("seg", DIM, what="seg_b alone")
    none, _, _ = _lib.segment_norm_backward(dYv, Xv, mean_in, rstd_in, gpd, wgt, alpha, need_input=False, out=dict(seg_a=A2, seg_b=B2))
    assert none is None
    _same(A2, near_a, "seg_a alone")
    _same(B2, near_b, "seg_b alone")
    w.check()

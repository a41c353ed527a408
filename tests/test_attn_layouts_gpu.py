"""Every lane layout of the fused attention kernels, in every family and on every side, and every rung of GAT's own lse pass.

Part 1.  The 34 shapes of tests/attn_cases.py -- one (heads, dim) per (log_lph, log_lpr) of attn_layout and one column-block shape
per log_lph = 1 .. 6 (tests/test_launch_geometry.py proves the table against the header) -- through the forward and backward
entries of GAT (rect, drop, edge), GATv2 and dot-product attention at the C ABI, on gat_rect_ref.threshold_structure(): rows of
t - 1, t, t + 1 edges around every t at which an lse pass sends a row to the whole block ((64 / LPR) * 32 edges in the shared
pass of GATv2 and dot) and around the 64 ids of one load of the pull kernels, a row without edges, 10 sources no edge reaches.
Plain and planted (ids outside the source rows) structures alternate over the shapes, and so do partSize 1, 3 and 32.
The calls, the NaN pre-fill of every output and the comparisons are those of the families' own kernel tests (imported, not
copied), against their fp64 restatements under the bounds those state: 1e-5 * max(1, sum of |terms|), times max(1, S) for
GATv2 and dot (S is printed); the exact zeros of rows without edges and of unreached sources; the kink rule of the GAT
references with its cap.

Part 2.  launch_lse of csrc/gnna_gat.hip picks seg, the lanes per row, as
    seg = 4; while (seg < 64 && seg * 4 < avg) seg <<= 1;
with avg = the avg_degree of gnna_tuning when it is set, so avg_degree = 1, 17, 33, 65, 129 give seg = 4, 8, 16, 32, 64 (17 > 16,
33 > 32, 65 > 64 and 129 > 128 each take one more doubling than the value before), and a row is `long` above seg * 32 edges --
127 / 128 / 129 up to 2047 / 2048 / 2049 edges are rows of the structure.  HB, the heads per block, is the power of two >= heads,
8 at most: heads = 1, 2, 3, 5, 9 give HB = 1, 2, 4 (one slot idle), 8 (three idle) and 8 with a second block in grid.y (seven
idle).  seg cannot be observed from outside; the five values are what the loop gives as read.  Each (heads, avg_degree) runs
the plain and the edge-term instance of the pass; lse and Y are compared with fp64 and lse must have the same bits on a second
call."""
import functools

import pytest
import torch

import attn_cases
import dotattn_ref as tref
import gat_drop_ref as dref
import gat_edge_ref as eref
import gat_rect_ref as gref
import gatv2_ref as vref
import test_dotattn_gpu as dot
import test_gat_drop_gpu as drop
import test_gat_edge_gpu as edge
import test_gat_rect_gpu as rect
import test_gatv2_gpu as v2
from gnnadvisor_osdi21_amd import _lib
from util import assert_close_f64

pytestmark = pytest.mark.gpu
OK = 0
SLOPE = 0.2
SEED = 0x1234
N_IN = gref.THRESHOLD_N_IN
# (family, attn_drop): the entries and modes every shape runs
MODES = [("rect", 0.0), ("drop", 0.5), ("edge", 0.0), ("edge", 0.5), ("gatv2", 0.0), ("gatv2", 0.5), ("dot", 0.0), ("dot", 0.5)]
# (heads, dim, partSize, planted, seed of the inputs)
SHAPES = [(h, d, (1, 3, 32)[k % 3], k % 2 == 1, 100 + k) for k, (h, d) in enumerate(attn_cases.ALL_SHAPES)]


@functools.lru_cache(maxsize=None)
def _threshold(partSize, planted):
    rp, ci = gref.threshold_structure()
    s = rect._structure(rp, gref.plant_out_of_range(ci, N_IN) if planted else ci, N_IN, partSize)
    return edge._with_perm(s)


def run_family(family, p, s, heads, dim, seed, what):
    """One forward and backward of `family` on the structure s into NaN-filled outputs, compared with the family's fp64 reference
    by the family's own _compare.  -> the reference's namespace."""
    if family in ("rect", "drop", "edge"):
        H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, seed)]
        if family == "rect":
            r = gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, SLOPE, what)
            rect._compare(rect._run(s, H, el, er, G, heads, dim, SLOPE), r, what)
        elif family == "drop":
            r = dref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, SLOPE, p, SEED, what)
            drop._compare_drop(drop._run(s, H, el, er, G, heads, dim, p, SEED, SLOPE), r, what)
        else:
            ee = edge._ee(s.nnz, heads)
            r = eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, SLOPE, p, SEED, what=what)
            edge._compare(edge._run(s, H, el, er, ee, G, heads, dim, SLOPE, p, SEED), r, what)
    elif family == "gatv2":
        Hs, Hd, att, G = [t.cuda() for t in vref.inputs(s.n_out, s.n_in, heads, dim, seed)]
        r = vref.kernel_reference(Hs, Hd, att, G, s.rp, s.ci, heads, SLOPE, p, SEED, what)
        print(f"{what}: S = {r.S:.3f}")
        v2._compare(v2._run(s, Hs, Hd, att, G, heads, dim, p, SEED), r, what)
    else:
        Q, K, V, G = [t.cuda() for t in tref.inputs(s.n_out, s.n_in, heads, dim, seed)]
        r = tref.kernel_reference(Q, K, V, G, s.rp, s.ci, heads, dot._scale(dim), p, SEED)
        dot._compare(dot._run(s, Q, K, V, G, heads, dim, p, SEED), r, what)            # (prints S)
    if p > 0:
        assert 0 < int((r.k > 0).sum()) < r.k.numel(), f"{what}: the mask must keep some but not all edges"
    return r


# ---- 1. every layout, every family, every side -----------------------------------------------------------------------------------

@pytest.mark.parametrize("family,p", MODES, ids=[f"{f}-p{p}" for f, p in MODES])
@pytest.mark.parametrize("heads,dim,partSize,planted,seed", SHAPES, ids=[f"{h}x{d}-ps{ps}{'-planted' if pl else ''}" for h, d, ps, pl, _ in SHAPES])
def test_every_layout(heads, dim, partSize, planted, seed, family, p):
    s = _threshold(partSize, planted)
    r = run_family(family, p, s, heads, dim, seed, f"{family} p={p} {heads}x{dim} partSize={partSize} planted={planted}")
    # (planted: a short row may lose all its edges and join the row without any)
    assert (r.nnz < s.nnz) == planted and int((~r.has).sum()) == (3 if planted else 1) and int((~r.reached).sum()) >= 10


def test_the_structure_is_the_one_described():
    s = _threshold(32, False)
    lengths = (s.rp[1:] - s.rp[:-1]).cpu().tolist()
    assert set(gref.threshold_lengths()) <= set(lengths) and s.n_out == 62 and s.n_in == N_IN and 12000 < s.nnz < 13000


# ---- 2. the rungs of GAT's lse pass ----------------------------------------------------------------------------------------------

LSE_HEADS = [1, 2, 3, 5, 9]
AVG_DEGREES = [1, 17, 33, 65, 129]           # seg = 4, 8, 16, 32, 64 (the module docstring)
LSE_DIM = 4


@functools.lru_cache(maxsize=None)
def _lse_case(heads, with_edge_term):
    """Inputs on the device and the fp64 reference of the forward: computed once per head count, shared, never written."""
    s = _threshold(3, False)
    H, el, er, G = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, LSE_DIM, 300 + heads)]
    if with_edge_term:
        ee = edge._ee(s.nnz, heads)
        return H, el, er, ee, eref.kernel_reference(H, el, er, ee, G, s.rp, s.ci, heads, SLOPE, what=f"lse rungs, edge term, {heads} heads")
    return H, el, er, None, gref.kernel_reference(H, el, er, G, s.rp, s.ci, heads, SLOPE, f"lse rungs, {heads} heads")


@pytest.mark.parametrize("with_edge_term", [False, True], ids=["rect", "edge"])
@pytest.mark.parametrize("avg_degree", AVG_DEGREES)
@pytest.mark.parametrize("heads", LSE_HEADS)
def test_every_rung_of_the_gat_lse_pass(heads, avg_degree, with_edge_term):
    s = _threshold(3, False)
    H, el, er, ee, r = _lse_case(heads, with_edge_term)
    what = f"{'edge' if with_edge_term else 'rect'} {heads} heads avg_degree={avg_degree}"

    def forward():
        Y, lse = rect._nan(s.n_out, heads * LSE_DIM), rect._nan(s.n_out, heads)
        if with_edge_term:
            rc = edge.raw_forward(s, H, el, er, ee, Y, lse, heads, LSE_DIM, SLOPE)
        else:
            rc = rect.raw_forward(s, H, el, er, Y, lse, heads, LSE_DIM, SLOPE)
        assert rc == OK, _lib.load().gnna_last_error()
        return Y, lse

    before = _lib.get_tuning()
    try:
        _lib.set_tuning(avg_degree=avg_degree)
        assert _lib.get_tuning()["avg_degree"] == avg_degree
        Y, lse = forward()
        _, lse2 = forward()
    finally:
        _lib.reset_tuning()
    assert _lib.get_tuning() == before
    for t, name in ((Y, "Y"), (lse, "lse")):
        assert not torch.isnan(t).any(), f"{what}: {name} has elements the call did not write"
        assert torch.isfinite(t).all(), f"{what}: {name} is not finite"
    n = lambda t: t.cpu().numpy()
    assert_close_f64(n(lse[r.has]), n(r.lse[r.has]), rtol=1e-5, what=f"{what} lse")
    assert_close_f64(n(Y), n(r.Y), rtol=1e-5, scale=n(r.s_Y), what=f"{what} Y")
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all(), f"{what}: rows without edges must give out = lse = 0"
    assert torch.equal(lse2, lse), f"{what}: lse must have the same bits on every call"

"""What the structures and cases of the attention tests claim, checked without a GPU: the row lengths of
gat_rect_ref.threshold_structure(), what the launch makes of gat_rect_ref.multi_run_structure() on a 256-CU device (the
project's own build_part and the restated chunk_grid of tests/attn_cases.py), and that the kink cap of the GAT references (fewer
than 1e-3 of the edges within 1e-6 of the kink of the leaky ReLU -- asserted inside kernel_reference) holds for the inputs of
every GAT case of tests/test_attn_layouts_gpu.py and tests/test_attn_chunks_gpu.py, from the fp64 reference alone."""
import functools

import numpy as np
import pytest
import torch

import attn_cases
import gat_drop_ref as dref
import gat_edge_ref as eref
import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib

CUS = 256
T = 16 * CUS
SLOPE = 0.2
SEED = 0x1234
GAT_MODES = [("rect", 0.0), ("drop", 0.5), ("edge", 0.0), ("edge", 0.5)]


def test_threshold_structure_has_the_listed_rows():
    rp, ci = gref.threshold_structure()
    deg = np.diff(rp)
    want = gref.threshold_lengths()
    assert len(want) == 26 and sum(want) == 12203
    counts = {int(d): int((deg == d).sum()) for d in want}
    assert all(counts[d] >= 1 for d in want) and counts[0] == 1 and all(counts[d] == 1 for d in want if d > 11)
    assert len(deg) == 62 and (np.sort(deg)[:-21] <= 11).all() and 12203 + 36 <= rp[-1] <= 12203 + 36 * 11
    assert ci.min() == 0 and ci.max() == gref.THRESHOLD_N_IN - 11 and len(np.unique(ci)) == gref.THRESHOLD_N_IN - 10
    assert (np.diff(ci) < 0).any()                                                           # unsorted
    assert all(len(np.unique(ci[rp[i]:rp[i + 1]])) < deg[i] for i in np.nonzero(deg > 140)[0])   # duplicates
    # every switch sits between two rows: t edges are short for the pass that switches above t, t + 1 are long
    for t in gref.THRESHOLDS:
        assert counts[t] == 1 and counts[t + 1] == 1
    bad = gref.plant_out_of_range(ci, gref.THRESHOLD_N_IN)
    assert ((bad < 0) | (bad >= gref.THRESHOLD_N_IN)).sum() >= len(ci) // 10


@functools.lru_cache(maxsize=None)
def _geometry(k):
    name, parts_of, ps, want_G = attn_cases.GEOMETRIES[k]
    rp, ci, n_in = gref.multi_run_structure(parts_of(T), ps)
    pp, p2n = _lib.build_part(ps, torch.from_numpy(rp))
    return rp, ci, n_in, pp.numpy(), p2n.numpy(), ps, want_G, parts_of(T)


@pytest.mark.parametrize("k", range(3), ids=[g[0] for g in attn_cases.GEOMETRIES])
def test_multi_run_structure_and_what_the_launch_makes_of_it(k):
    rp, ci, n_in, pp, p2n, ps, want_G, P = _geometry(k)
    deg = np.diff(rp)
    assert len(p2n) == P and pp[-1] == rp[-1]
    G, blocks = attn_cases.chunk_grid(P, ps, CUS)
    assert G == want_G and blocks == -(-(-(-P // G)) // 4)
    assert ci.min() == 0 and ci.max() == n_in - 11 and n_in < len(deg)
    runs = attn_cases.runs_of(p2n, G)
    assert runs["rows_cut_by_chunk"] >= 1 and runs["rows_cut_by_block"] >= 1
    if ps == 1:
        assert deg.min() == 0 and deg.max() == 12 and (np.diff(pp) == 1).all()
        assert np.array_equal(np.bincount(p2n, minlength=len(deg)), deg)                     # a row of k edges: k groups
    else:
        hubs = deg == 250
        assert hubs.sum() >= len(deg) // 50 - 1 and hubs[26::50][:-1].all() and deg[~hubs].max() <= 8 and deg.min() == 1
        assert (np.bincount(p2n, minlength=len(deg))[hubs] == 3).all()
    if k == 0:
        assert P % G == 1                                                                    # one group in the last chunk
    if G >= 3:
        assert runs["runs_per_chunk"].max() >= 3 and runs["groups_per_run"].max() >= 3
    else:
        assert runs["runs_per_chunk"].max() == 2 and runs["groups_per_run"].max() == 2


def test_runs_of_on_a_hand_made_partition():
    # rows 0 0 0 1 | 1 2 2 2 | 2 3 4 4 | 4 4 4 4 | 5 at G = 4
    p2n = [0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 4, 4, 4, 4, 4, 4, 5]
    runs = attn_cases.runs_of(p2n, 4)
    assert runs["runs_per_chunk"].tolist() == [2, 2, 3, 1, 1] and runs["groups_per_run"].tolist() == [3, 1, 1, 3, 1, 1, 2, 4, 1]
    assert runs["rows_cut_by_chunk"] == 3 and runs["rows_cut_by_block"] == 0
    assert attn_cases.runs_of(p2n, 1)["rows_cut_by_block"] == 3               # blocks of 4 groups: the same cuts, rows 1, 2 and 4


def _kink_cap(family, p, H, el, er, G, rp, ci, heads, what):
    rp, ci = torch.from_numpy(rp), torch.from_numpy(ci)
    if family == "rect":
        r = gref.kernel_reference(H, el, er, G, rp, ci, heads, SLOPE, what)
    elif family == "drop":
        r = dref.kernel_reference(H, el, er, G, rp, ci, heads, SLOPE, p, SEED, what)
    else:
        ee = torch.randn(ci.numel(), heads, generator=torch.Generator().manual_seed(9))       # (test_gat_edge_gpu._ee)
        r = eref.kernel_reference(H, el, er, ee, G, rp, ci, heads, SLOPE, p, SEED, what=what)
    assert r.excluded < 1e-3 * max(1, r.nnz)
    return r


@pytest.mark.parametrize("family,p", GAT_MODES, ids=[f"{f}-p{p}" for f, p in GAT_MODES])
def test_the_kink_cap_holds_for_every_gat_case_of_the_layout_tests(family, p):
    """The inputs of tests/test_attn_layouts_gpu.py: gat_rect_ref.inputs(seed = 100 + k) for the k-th shape, plain and planted
    structures alternating, and those of the lse rungs (dim 4, seed 300 + heads)."""
    rp, ci = gref.threshold_structure()
    planted = gref.plant_out_of_range(ci, gref.THRESHOLD_N_IN)
    for k, (heads, dim) in enumerate(attn_cases.ALL_SHAPES):
        H, el, er, G = gref.inputs(len(rp) - 1, gref.THRESHOLD_N_IN, heads, dim, 100 + k)
        _kink_cap(family, p, H, el, er, G, rp, planted if k % 2 else ci, heads, f"{family} {heads}x{dim}")
    if p == 0.0:
        for heads in (1, 2, 3, 5, 9):
            H, el, er, G = gref.inputs(len(rp) - 1, gref.THRESHOLD_N_IN, heads, 4, 300 + heads)
            _kink_cap(family, p, H, el, er, G, rp, ci, heads, f"{family} lse rungs {heads} heads")


@pytest.mark.parametrize("heads,dim", attn_cases.CHUNK_SHAPES, ids=["%dx%d" % s for s in attn_cases.CHUNK_SHAPES])
@pytest.mark.parametrize("k", range(3), ids=[g[0] for g in attn_cases.GEOMETRIES])
def test_the_kink_cap_holds_for_every_gat_case_of_the_chunk_tests(k, heads, dim):
    """The inputs of tests/test_attn_chunks_gpu.py on a 256-CU device: gat_rect_ref.inputs(seed = 500 + 10 k + heads)."""
    rp, ci, n_in = _geometry(k)[:3]
    H, el, er, G = gref.inputs(len(rp) - 1, n_in, heads, dim, 500 + 10 * k + heads)
    for family, p in GAT_MODES:
        _kink_cap(family, p, H, el, er, G, rp, ci, heads, f"{family} p={p} {attn_cases.GEOMETRIES[k][0]} {heads}x{dim}")

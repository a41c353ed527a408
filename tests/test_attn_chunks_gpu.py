"""The fused attention kernels with several neighbor-groups per wavefront and real runs, on the GPU.

chunk_grid (csrc/gnna_launch.h) halves G, the groups a wavefront takes, while there are fewer than T = 16 * compute units chunks,
so the structures of the families' kernel tests all run at G = 1: every group is then a run of its own and no wavefront meets a
second row.  Here gat_rect_ref.multi_run_structure has exactly the number of groups that gives (tests/attn_cases.py::GEOMETRIES)

    64 T + 1 groups at partSize 1    G = 64, one group in the last chunk     rows of 0 .. 12 edges: runs of up to 12 groups
    2 T + 5  groups at partSize 1    G = 2
    7 T      groups at partSize 100  G = 5 (no power of two)                 every 50th row has three groups

so that a wavefront merges the groups of a row into a run, walks several runs, and rows are cut by chunk and by workgroup
boundaries (two wavefronts, or two workgroups, add to one row); tests/test_attn_cases_host.py asserts those properties for a
256-CU device without a GPU.  The transposed structure (the source-side passes) has a third of the rows, so its rows are runs of
up to dozens of groups at partSize 1 and it runs at G >= 2 as well.  GATv2's destination-side pass keeps a lane's share of d_att in registers across every run of its
wavefront: d_att is compared at gatv2_ref's own bound like every other output.

Shapes (1, 64), (4, 16), (3, 5), (2, 33); the eight entry / mode pairs of tests/test_attn_layouts_gpu.py, whose run_family makes
the calls (NaN pre-fill, the families' own _compare, their fp64 references and bounds).  S of GATv2 and dot is printed."""
import functools

import pytest

import attn_cases
import gat_rect_ref as gref
import test_gat_edge_gpu as edge
import test_gat_rect_gpu as rect
from gnnadvisor_osdi21_amd import _lib
from test_attn_layouts_gpu import MODES, run_family

pytestmark = pytest.mark.gpu
mode_ids = [f"{f}-p{p}" for f, p in MODES]


@functools.lru_cache(maxsize=None)
def _geometry(k):
    """The device structure of GEOMETRIES[k] for this device's compute units, with its transpose; made once, never written."""
    name, parts_of, ps, want_G = attn_cases.GEOMETRIES[k]
    P = parts_of(16 * _lib.device_cus())
    rp, ci, n_in = gref.multi_run_structure(P, ps)
    s = edge._with_perm(rect._structure(rp, ci, n_in, ps))
    assert s.p2n.numel() == P
    G, blocks = attn_cases.chunk_grid(P, ps, _lib.device_cus())
    assert G == want_G, (name, G)
    if k == 0:
        assert P % G == 1 and blocks * 4 * G >= P                     # one group in the last chunk
    runs = attn_cases.runs_of(s.p2n.cpu().numpy(), G)
    assert runs["rows_cut_by_chunk"] >= 1 and runs["rows_cut_by_block"] >= 1 and runs["runs_per_chunk"].max() >= min(G, 3)
    assert runs["groups_per_run"].max() >= min(G, 3)
    # the source side: several groups per wavefront as well
    assert attn_cases.chunk_grid(s.t_p2n.numel(), ps, _lib.device_cus())[0] >= 2
    return s


def _case(k, heads, dim, family, p, tuning=None):
    s = _geometry(k)
    what = f"{attn_cases.GEOMETRIES[k][0]} {family} p={p} {heads}x{dim}" + (f" {tuning}" if tuning else "")
    r = run_family(family, p, s, heads, dim, 500 + 10 * k + heads, what)
    assert r.nnz == s.nnz and int((~r.reached).sum()) >= 10 and (k == 2 or int((~r.has).sum()) >= 1)


@pytest.mark.parametrize("family,p", MODES, ids=mode_ids)
@pytest.mark.parametrize("heads,dim", attn_cases.CHUNK_SHAPES, ids=["%dx%d" % s for s in attn_cases.CHUNK_SHAPES])
@pytest.mark.parametrize("k", range(3), ids=[g[0] for g in attn_cases.GEOMETRIES])
def test_several_groups_per_wavefront(k, heads, dim, family, p):
    _case(k, heads, dim, family, p)


@pytest.mark.parametrize("xcd_remap", [0, 1], ids=["off", "on"])
@pytest.mark.parametrize("family,p", MODES, ids=mode_ids)
def test_chunks_with_the_xcd_remap_forced(family, p, xcd_remap):
    """G = 64 with the chunk of a wavefront taken from the remapped workgroup number, and from the plain one: the partial last
    workgroup and the chunk without groups behind the last one are then other wavefronts' business."""
    before = _lib.get_tuning()
    try:
        _lib.set_tuning(xcd_remap=xcd_remap)
        assert _lib.get_tuning()["xcd_remap"] == xcd_remap
        _case(0, 4, 16, family, p, tuning=f"xcd_remap={xcd_remap}")
    finally:
        _lib.reset_tuning()
    assert _lib.get_tuning() == before

"""The host side of test_far_offsets_gpu.py: the graph has the degrees, the symmetry and the sources on each side of every mark
that the GPU tests rely on (far_offsets.graphs asserts them), and the geometry puts the marks where the docstrings say."""
import numpy as np

import far_offsets as F


def test_the_graph_has_the_degree_list_and_a_source_in_every_region():
    made = F.graphs()
    rp, ci, n_in = made.sym
    assert len(rp) == F.ROWS + 1 and n_in == F.ROWS
    assert [int(d) for d in np.diff(rp)[:6]] == [0, 1, 63, 64, 65, 283]
    assert len(made.rect[0]) == 271 and made.rect[2] == F.ROWS and made.small[2] == 63
    for rp, ci, n_in in (made.sym, made.directed, made.rect, made.small):
        assert ci.min() >= 0 and ci.max() < n_in and rp[-1] == len(ci)
        assert all((np.diff(ci[rp[i]:rp[i + 1]]) >= 0).all() for i in range(len(rp) - 1)), "the ids of a row are sorted"


def test_the_marks_fall_at_the_rows_named():
    for name, bound in (("2^31 bytes", (1 << 31) // 4), ("2^32 bytes", (1 << 32) // 4), ("2^31 floats", 1 << 31), ("2^32 floats", 1 << 32)):
        assert F.MARKS[name] * F.LD == bound and F.SEG_MARKS[name] * F.SEG_LD == bound
    assert F.ROWS * F.LD + (1 << 28) == F.ARENA_FLOATS == F.SEG_ROWS * F.SEG_LD
    assert max(F.MARKS.values()) < F.ROWS and max(F.SEG_MARKS.values()) < F.SEG_ROWS
    for gp in F.SEGMENTS.values():
        assert (np.diff(gp) == 0).any() and (np.diff(gp) >= 0).all() and gp[-1] <= F.ROWS

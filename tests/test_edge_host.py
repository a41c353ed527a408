"""gnna_reverse_edges_i32 (host): the reverse-edge map the backward of the edge-weighted aggregation reads its weights
through, and the C ABI names of the edge-attention additions (0.6.1)."""
import os

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph


def _rows(rp):
    rp = np.asarray(rp, dtype=np.int64)
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def _check_rev(rp, ci, rev):
    """rev is an involution that maps (i, j) to (j, i), and the k-th (i, j) of a row to the k-th (j, i)."""
    rp, ci, rev = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(rev, dtype=np.int64)
    row = _rows(rp)
    e = np.arange(ci.size)
    assert ((rev >= 0) & (rev < ci.size)).all()
    assert (rev[rev] == e).all(), "rev[rev[e]] != e"
    assert (ci[rev] == row).all(), "column_index[rev[e]] != row(e)"
    assert (row[rev] == ci).all(), "row(rev[e]) != column_index[e]"
    # the k-th (i, j) in position order pairs with the k-th (j, i)
    key = row * (ci.max() + 1 if ci.size else 1) + ci
    order = np.lexsort((e, key))                 # by (pair, position)
    rank = np.empty_like(e)
    ks = key[order]
    starts = np.r_[0, np.flatnonzero(np.diff(ks)) + 1]
    run = np.repeat(starts, np.diff(np.r_[starts, ks.size]))
    rank[order] = np.arange(ks.size) - run
    assert (rank[rev] == rank).all(), "duplicate pairs must pair in order"


@pytest.mark.parametrize("kind,seed", [("powerlaw", 1), ("powerlaw", 2), ("rmat", 3), ("rmat", 4)])
def test_reverse_edges_on_generated_graphs(kind, seed):
    if kind == "powerlaw":
        g = graph.powerlaw_graph(3000, 60000, 800, seed=seed)
    else:
        g = graph.rmat_graph(4096, 80000, seed=seed)
    rev = _lib.reverse_edges(g.row_pointers, g.column_index)
    assert rev.dtype == torch.int32 and rev.numel() == g.column_index.numel()
    _check_rev(g.row_pointers.numpy(), g.column_index.numpy(), rev.numpy())


def _hand_built():
    """Rows unsorted, duplicate pairs (0, 1) x 2 / (1, 0) x 2, self loops (2, 2) x 2 and (3, 3), an empty row 4."""
    rows = [
        [1, 2, 1, 3],        # 0
        [0, 3, 0],           # 1
        [2, 0, 2],           # 2
        [3, 1, 0],           # 3
        [],                  # 4
    ]
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ci = np.array([c for r in rows for c in r], dtype=np.int32)
    return torch.from_numpy(rp), torch.from_numpy(ci)


def test_reverse_edges_duplicates_self_loops_unsorted():
    rp, ci = _hand_built()
    rev = _lib.reverse_edges(rp, ci).numpy()
    _check_rev(rp.numpy(), ci.numpy(), rev)
    # explicit: row 0 = positions 0..3, row 1 = 4..6; the first (0, 1) (pos 0) pairs with the first (1, 0) (pos 4)
    assert rev[0] == 4 and rev[2] == 6 and rev[4] == 0 and rev[6] == 2
    # self loops: (2, 2) at positions 7 and 9 pair with themselves in order
    assert rev[7] == 7 and rev[9] == 9


@pytest.mark.parametrize("threads", ["1", "3", "8"])
def test_reverse_edges_independent_of_thread_count(threads, monkeypatch):
    g = graph.powerlaw_graph(20000, 400000, 3000, seed=9)
    monkeypatch.setenv("GNNA_HOST_THREADS", "1")
    want = _lib.reverse_edges(g.row_pointers, g.column_index)
    monkeypatch.setenv("GNNA_HOST_THREADS", threads)
    got = _lib.reverse_edges(g.row_pointers, g.column_index)
    assert torch.equal(got, want)


def test_reverse_edges_refuses_asymmetric_structure():
    rp, ci = _hand_built()
    ci = ci.clone()
    ci[5] = 1                    # row 1: (1, 3) becomes a self loop (1, 1); (3, 1) at position 11 loses its partner
    with pytest.raises(_lib.GnnaError) as exc:
        _lib.reverse_edges(rp, ci)
    msg = str(exc.value)
    assert "libgnna error -1" in msg and "not symmetric" in msg
    assert "edge 11 (3 -> 1)" in msg, msg


def test_reverse_edges_refuses_bad_ids():
    rp, ci = _hand_built()
    ci = ci.clone()
    ci[3] = 7
    with pytest.raises(_lib.GnnaError, match=r"column_index\[3\] = 7 is not a node id"):
        _lib.reverse_edges(rp, ci)


def test_exports_carry_the_edge_attention_entry_points():
    for name in ("gnna_agg_edge_ld_f32", "gnna_edge_softmax_f32", "gnna_edge_softmax_backward_f32", "gnna_reverse_edges_i32"):
        assert name in _lib.EXPORTS
        getattr(_lib.load(), name)


def test_expected_aggregations_count_gat_heads():
    from gnnadvisor_osdi21_amd.decider import expected_aggregations
    assert expected_aggregations("gat", 602, 64, 41, epochs=10, heads=4) == [(64, 80), (41, 20)]
    assert expected_aggregations("gat", 602, 64, 41, epochs=10) == [(64, 20), (41, 20)]

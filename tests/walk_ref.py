"""numpy restatements of the two rules of include/gnna_walk.h -- the walk rule of gnna_random_walk_i32 and the subgraph rule of
gnna_induced_subgraph_i32 -- and the inputs their tests share (checker side only).  Nothing here reads the library."""
import functools

import numpy as np

from sampling_ref import host_build_part, keys_of, shared_graph     # noqa: F401  (re-exported for the tests)


def row_extent(rp, v, nnz):
    """(lo, d): the candidate positions [lo, lo + d) of row v; d = 0 for a row whose pointers decrease or leave [0, nnz]."""
    lo, hi = int(rp[v]), int(rp[v + 1])
    return lo, (hi - lo if 0 <= lo and hi <= nnz and hi > lo else 0)


def step_index(key, d):
    """j = floor(key * d / 2^64), in Python integers."""
    return (int(key) * int(d)) >> 64


def random_walks(rp, ci, roots, walk_length, rng_seed):
    """-> (walks [R, L + 1], edge_ids [R, L]) int64, as the walk rule states them."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n, nnz, L = len(rp) - 1, len(ci), int(walk_length)
    walks = np.full((len(roots), L + 1), -1, dtype=np.int64)
    eids = np.full((len(roots), L), -1, dtype=np.int64)
    for w, root in enumerate(np.asarray(roots, np.int64)):
        if not 0 <= root < n:
            continue
        v = walks[w, 0] = int(root)
        if L == 0:
            continue
        keys = keys_of(rng_seed, np.arange(w * L, w * L + L, dtype=np.uint64))
        for t in range(L):
            lo, d = row_extent(rp, v, nnz)
            if d > 0:
                e = lo + step_index(keys[t], d)
                c = int(ci[e])
                if 0 <= c < n:
                    v, eids[w, t] = c, e
            walks[w, t + 1] = v
    return walks, eids


def induced_subgraph(rp, ci, nodes, partSize=None):
    """-> dict(nodes = S, new_id, row_pointers, column_index, edge_ids[, partPtr, part2Node]) int64, as the subgraph rule states
    them; raises ValueError naming the first index of `nodes` that is neither in the graph nor -1."""
    rp, ci, nodes = np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(nodes, np.int64)
    n, nnz = len(rp) - 1, len(ci)
    bad = np.flatnonzero(((nodes < 0) | (nodes >= n)) & (nodes != -1))
    if len(bad):
        raise ValueError("nodes[%d]" % bad[0])
    S = np.unique(nodes[nodes >= 0])                              # distinct, increasing
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[S] = np.arange(len(S))
    sub_rp, cols, eids = [0], [], []
    for v in S:
        lo, d = row_extent(rp, v, nnz)
        e = np.arange(lo, lo + d, dtype=np.int64)
        c = ci[e]
        inside = (c >= 0) & (c < n)
        keep = np.zeros(d, dtype=bool)
        keep[inside] = new_id[c[inside]] >= 0
        cols.append(new_id[c[keep]])
        eids.append(e[keep])
        sub_rp.append(sub_rp[-1] + int(keep.sum()))
    out = {"nodes": S, "new_id": new_id, "row_pointers": np.array(sub_rp, dtype=np.int64),
           "column_index": np.concatenate(cols) if cols else np.zeros(0, np.int64),
           "edge_ids": np.concatenate(eids) if eids else np.zeros(0, np.int64)}
    if partSize is not None:
        out["partPtr"], out["part2Node"] = host_build_part(partSize, out["row_pointers"])
    return out


def dense_adjacency(sub):
    """A[a, b] = the number of edges a <- b of a restated subgraph (float64 [n, n]): duplicate edges add."""
    n = len(sub["nodes"])
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(sub["row_pointers"]))
    np.add.at(A, (rows, sub["column_index"]), 1.0)
    return A


N = 3000        # nodes of shared_graph()


@functools.lru_cache(maxsize=None)
def root_sets():
    """Roots of 1, 64, 65 and 1,000 walks: the special rows 0 .. 10, the edgeless rows 20 .. 29, -1 and N among them (from 64 on),
    with repeats."""
    rng = np.random.default_rng(21)
    sets = {1: np.array([10])}
    for size in (64, 65, 1000):
        head = np.concatenate([np.arange(11), np.arange(20, 30), [-1, N]])
        sets[size] = rng.permutation(np.concatenate([head, rng.integers(0, N, size=size - len(head))]))
    return {k: v.astype(np.int32) for k, v in sets.items()}


@functools.lru_cache(maxsize=None)
def dead_end_graph():
    """shared_graph() with every 5th column id set to -1 and every 7th to N: edges that are never followed and never kept."""
    rp, ci = shared_graph()
    ci = ci.copy()
    ci[::5] = -1
    ci[3::7] = N
    return rp, ci


@functools.lru_cache(maxsize=None)
def id_lists():
    """The node lists of the subgraph tests: empty; the hub alone; 64, 65 and 1,000 ids in non-monotone order with duplicates and
    -1 entries (the special rows among them); all 3,000 ids shuffled and doubled."""
    rng = np.random.default_rng(22)
    lists = {"empty": np.zeros(0, np.int64), "hub": np.array([10])}
    for size in (64, 65, 1000):
        distinct = np.concatenate([np.arange(11), np.arange(20, 24), rng.permutation(np.arange(30, N))[: size * 3 // 4 - 15]])
        pool = np.concatenate([distinct, [-1] * 5])
        extra = rng.choice(pool, size=size - len(pool))            # duplicates (and more -1)
        lists[str(size)] = rng.permutation(np.concatenate([pool, extra]))
        assert len(lists[str(size)]) == size
    both = np.concatenate([np.arange(N), np.arange(N)])
    lists["all"] = rng.permutation(both)
    return {k: v.astype(np.int32) for k, v in lists.items()}

"""numpy restatement of the sampling rule of gnna_sample_neighbors_i32 (include/gnna.h) and the graphs the sampling tests
share (checker side only).  Nothing here reads the library."""
import functools

import numpy as np

M64 = (1 << 64) - 1


def keys_of(rng_seed, positions):
    """The splitmix64 key of every position e (uint64 arithmetic wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        e = np.asarray(positions, dtype=np.uint64)
        z = np.uint64(rng_seed & M64) + np.uint64(0x9E3779B97F4A7C15) * (e + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def pick_row(lo, hi, fanout, rng_seed):
    """The positions taken from the candidate positions [lo, hi), in increasing order."""
    e = np.arange(lo, hi, dtype=np.int64)
    if fanout <= 0 or len(e) <= fanout:
        return e
    order = np.lexsort((e, keys_of(rng_seed, e)))         # smallest key first, a tie goes to the smaller position
    return np.sort(e[order[:fanout]])


def sample_block(rp, ci, seeds, fanout, rng_seed):
    """-> dict(row_pointers, edge_ids, column_index (local), src_nodes) as the contract states them."""
    rp, ci, seeds = np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(seeds, np.int64)
    picks = [pick_row(rp[r], rp[r + 1], fanout, rng_seed) for r in seeds]
    blk_rp = np.zeros(len(seeds) + 1, dtype=np.int64)
    blk_rp[1:] = np.cumsum([len(p) for p in picks])
    eid = np.concatenate(picks) if picks else np.zeros(0, np.int64)
    eid = eid.astype(np.int64)
    cols = ci[eid]
    others = np.setdiff1d(np.unique(cols), seeds)             # sorted: increasing global id
    src = np.concatenate([seeds, others])
    local = {int(v): i for i, v in enumerate(src)}
    blk_ci = np.array([local[int(c)] for c in cols], dtype=np.int64)
    return {"row_pointers": blk_rp, "edge_ids": eid, "column_index": blk_ci, "src_nodes": src}


def host_build_part(partSize, rp):
    pp, p2n = [], []
    for i in range(len(rp) - 1):
        for beg in range(int(rp[i]), int(rp[i + 1]), partSize):
            pp.append(beg)
            p2n.append(i)
    pp.append(int(rp[-1]) if len(rp) > 1 else 0)
    return np.array(pp, dtype=np.int64), np.array(p2n, dtype=np.int64)


SPECIAL_DEGREES = (0, 1, 4, 5, 6, 63, 64, 65, 257, 4097, 10000)


@functools.lru_cache(maxsize=None)
def shared_graph():
    """3,000 nodes: rows of 0, 1, 4, 5, 6, 63, 64, 65, 257, 4,097 and 10,000 edges (nodes 0 .. 10; node 10 is the hub of the
    long-row path), every other row 0 .. 39 edges; unsorted rows, duplicate column ids, self loops.  -> (rp, ci) int32."""
    rng = np.random.default_rng(11)
    n = 3000
    deg = rng.integers(0, 40, size=n)
    deg[:len(SPECIAL_DEGREES)] = SPECIAL_DEGREES
    deg[20:30] = 0
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n, size=rp[-1])                      # unsorted, with duplicates within the long rows
    for r in range(0, n, 7):                                  # self loops, and a duplicated neighbour
        if deg[r] >= 2:
            ci[rp[r]] = r
            ci[rp[r] + 1] = ci[rp[r + 1] - 1]
    return rp.astype(np.int32), ci.astype(np.int32)


@functools.lru_cache(maxsize=None)
def seed_sets():
    """Seed sets of 1, 64, 65 and 1,000 distinct nodes in non-monotone order, with the special rows among them."""
    rng = np.random.default_rng(12)
    sets = {1: np.array([10])}                                # the hub alone
    for size in (64, 65, 1000):
        rest = rng.permutation(np.arange(30, 3000))[: size - 30]
        s = np.concatenate([np.arange(30), rest])             # rows 0 .. 10 (special), 20 .. 29 (no edges)
        sets[size] = rng.permutation(s)
    return {k: v.astype(np.int32) for k, v in sets.items()}

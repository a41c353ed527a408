"""numpy restatement of the rule of include/gnna_spatial.h -- the radius / k-nearest-neighbour graph of gnna_radius_graph_f32 -- and
the inputs its tests share (checker side only).  Nothing here reads the library: the partition comes from the oracle."""
import functools

import numpy as np


def clamped_pointers(graph_pointers, n):
    """The pointers clamped to [0, n]; raises ValueError naming the first segment whose clamped pointers decrease."""
    p = np.clip(np.asarray(graph_pointers, np.int64), 0, n)
    bad = np.flatnonzero(np.diff(p) < 0)
    if len(bad):
        raise ValueError("segment %d" % bad[0])
    return p


def dist2(pos, i, lo, hi):
    """d2(i, j) for j in [lo, hi): fp32, column by column, a subtraction, a multiplication and an addition each."""
    pos = np.asarray(pos, np.float32)
    with np.errstate(all="ignore"):
        acc = None
        for c in range(pos.shape[1]):
            diff = (pos[lo:hi, c] - pos[i, c]).astype(np.float32)
            sq = (diff * diff).astype(np.float32)
            acc = sq if acc is None else (acc + sq).astype(np.float32)
    return acc


def radius_graph(pos, graph_pointers, radius, max_neighbors=None, loop=False, partSize=None):
    """-> dict(row_pointers [N + 1] int64, column_index [nnz'] int64, dist2 [nnz'] float32[, partPtr, part2Node]), as the rule
    states them."""
    pos = np.asarray(pos, np.float32)
    n = pos.shape[0]
    p = clamped_pointers(graph_pointers, n)
    with np.errstate(all="ignore"):
        r2 = np.float32(radius) * np.float32(radius)
    rp, cols, d2s = np.zeros(n + 1, np.int64), [], []
    kept = [(np.zeros(0, np.int64), np.zeros(0, np.float32))] * n
    for g in range(len(p) - 1):
        lo, hi = int(p[g]), int(p[g + 1])
        ids = np.arange(lo, hi, dtype=np.int64)
        for i in range(lo, hi):
            d2 = dist2(pos, i, lo, hi)
            with np.errstate(all="ignore"):
                cand = d2 <= r2                                      # (NaN compares false)
            if not loop:
                cand[i - lo] = False
            j, d = ids[cand], d2[cand]
            if max_neighbors is not None and len(j) > max_neighbors:
                key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
                keep = np.sort(np.argsort(key, kind="stable")[:max_neighbors])     # the smallest keys, back in increasing j
                j, d = j[keep], d[keep]
            kept[i] = (j, d)
    for i in range(n):
        rp[i + 1] = rp[i] + len(kept[i][0])
    out = {"row_pointers": rp,
           "column_index": np.concatenate([k[0] for k in kept]) if n else np.zeros(0, np.int64),
           "dist2": np.concatenate([k[1] for k in kept]) if n else np.zeros(0, np.float32)}
    if partSize is not None:
        import oracle
        out["partPtr"], out["part2Node"] = oracle.build_part(partSize, rp.astype(np.int32))
    return out


def edge_set(res):
    rows = np.repeat(np.arange(len(res["row_pointers"]) - 1), np.diff(res["row_pointers"]))
    return set(zip(rows.tolist(), np.asarray(res["column_index"]).tolist()))


def pointers_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def lattice():
    """(pos, graph_pointers): two sets of points of the integer lattice {0..3}^3.  Every squared distance is a small integer and
    exact in fp32, so the cutoff is hand-worked (LATTICE_RADII): no fp32 radius squares to 2 -- fp32(sqrt 2)^2 rounds to
    2 - 2^-23, which leaves the pairs at d2 = 2 OUT, the next fp32 up squares to 2 + 2^-22, which takes them IN -- while at radius
    1 and 2 the pairs at d2 = 1 and d2 = 4 sit exactly on r2 and are neighbours.  Duplicates are coincident points (d2 = 0), and
    the many equal distances leave the cap to the tie-by-id rule.  Set 0: the 64 lattice points and 16 repeats; set 1: 9 points,
    4 of them one point."""
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    first = rng.permutation(np.concatenate([grid, grid[rng.integers(0, 64, size=16)]]))
    second = np.array([[1, 1, 1]] * 4 + [[1, 1, 2], [1, 2, 2], [0, 1, 1], [3, 3, 3], [2, 1, 1]])
    pos = np.concatenate([first, second]).astype(np.float32)
    return pos, pointers_of([len(first), len(second)])


SQRT2_BELOW = float(np.float32(np.sqrt(2.0)))                                  # r2 = 1.9999999: d2 = 2 is outside
SQRT2_ABOVE = float(np.nextafter(np.float32(np.sqrt(2.0)), np.float32(2)))     # r2 = 2.0000005: d2 = 2 is inside, d2 = 3 is not
# radius: the largest d2 that is a neighbour
LATTICE_RADII = {1.0: 1, SQRT2_BELOW: 1, SQRT2_ABOVE: 2, 2.0: 4}


def random_batch(sizes, dim, seed, specials=True):
    """(pos, graph_pointers): uniform points in [0, 1)^dim scaled so that a radius of 1 gives a handful of neighbours; with
    `specials` one row each holding NaN, +inf and 1e30 (where the batch is big enough) and a pair of coincident rows."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    pos = (rng.random((n, dim), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    if specials and n >= 12:
        pos[3, 0] = np.nan
        pos[5, dim - 1] = np.inf
        pos[7, :] = 1e30
        pos[9, :] = pos[8, :]
    return pos, pointers_of(sizes)

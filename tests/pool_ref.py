"""numpy restatement of include/gnna_pool.h: the sums in fp64, the extrema by the total order on the bit patterns that
gnna_agg_reduce_ld_f32 uses (-0 below +0, a NaN with a clear sign bit above +inf, one with the sign bit set below -inf), ties to
the smallest row, an empty segment gives the value 0 and the row -1."""
import numpy as np


def order_key(x):
    """uint32 keys that order like the floats of `x` (float32) in the library's total order."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    neg = (b >> np.uint32(31)).astype(bool)
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def segments(graph_pointers, num_rows):
    """[(first row, end row)] of every segment: pointers clamped to [0, num_rows], a descending pair is an empty segment."""
    p = np.clip(np.asarray(graph_pointers, dtype=np.int64), 0, num_rows)
    return [(int(p[g]), int(max(p[g], p[g + 1]))) if p[g + 1] >= p[g] else (int(p[g]), int(p[g])) for g in range(len(p) - 1)]


def forward(X, graph_pointers):
    """-> dict: sum (fp64), abs (fp64: the sum of |x|), count, max / min (float32 bits), argmax / argmin (int32 rows)."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    segs = segments(graph_pointers, n)
    G = len(segs)
    out = dict(sum=np.zeros((G, d)), abs=np.zeros((G, d)), count=np.zeros(G, dtype=np.int64),
               max=np.zeros((G, d), dtype=np.float32), min=np.zeros((G, d), dtype=np.float32),
               argmax=np.full((G, d), -1, dtype=np.int32), argmin=np.full((G, d), -1, dtype=np.int32))
    keys = order_key(X).astype(np.int64)
    cols = np.arange(d)
    for g, (a, b) in enumerate(segs):
        out["count"][g] = b - a
        if b <= a:
            continue
        seg = X[a:b].astype(np.float64)
        out["sum"][g] = seg.sum(0)
        out["abs"][g] = np.abs(seg).sum(0)
        k = keys[a:b]
        hi, lo = k.argmax(0), k.argmin(0)              # (argmax / argmin return the first of equal keys: the smallest row)
        out["argmax"][g], out["argmin"][g] = a + hi, a + lo
        out["max"][g], out["min"][g] = X[a + hi, cols], X[a + lo, cols]
    return out


def mean_f32(X, graph_pointers):
    """What GNNA_POOL_MEAN gives when the fp32 sum is exact: float32(sum) / float32(count), one IEEE division; 0 when empty."""
    ref = forward(X, graph_pointers)
    s, c = ref["sum"].astype(np.float32), ref["count"].astype(np.float32)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0, s / np.where(c > 0, c, np.float32(1)), np.float32(0)).astype(np.float32)


def backward(graph_pointers, num_rows, dim, d_sum=None, d_max=None, argmax=None, d_min=None, argmin=None, mean=False):
    """d_input [num_rows, dim] in float32, the terms added in the order of the header: s * d_sum, then the max term, then the min
    term; a row of no graph gets 0."""
    out = np.zeros((num_rows, dim), dtype=np.float32)
    for g, (a, b) in enumerate(segments(graph_pointers, num_rows)):
        if b <= a:
            continue
        rows = np.arange(a, b)[:, None]
        acc = np.zeros((b - a, dim), dtype=np.float32)
        if d_sum is not None:
            t = np.asarray(d_sum[g], dtype=np.float32)
            if mean:
                t = (np.float32(1) / np.float32(b - a)) * t
            acc = acc + t[None, :]
        if d_max is not None:
            acc = acc + np.where(np.asarray(argmax[g])[None, :] == rows, np.asarray(d_max[g], dtype=np.float32)[None, :], np.float32(0))
        if d_min is not None:
            acc = acc + np.where(np.asarray(argmin[g])[None, :] == rows, np.asarray(d_min[g], dtype=np.float32)[None, :], np.float32(0))
        out[a:b] = acc
    return out

"""numpy restatement of include/gnna_topk.h: per segment ``sorted(rows, key=(-order(score), row))[:k]``, then the mask, the
relabelling, the CSR filter and the partition; and the two row gathers.  `brute_force_keep` is a second statement of the selection
(pairwise comparisons, no sort) that the host test holds this one against on tiny inputs."""
import numpy as np

from pool_ref import order_key, segments


def keep_count(n, ratio=None, k=None):
    """min(n, ceil(ratio * n)) in double, or min(n, k)."""
    if k is not None:
        return int(min(n, k))
    return int(min(n, int(np.ceil(np.float64(ratio) * np.float64(n)))))


def keep_mask(score, graph_pointers, ratio=None, k=None):
    """bool [N]: the rows that are kept.  A row that several segments hold (pointers that descend and rise again) is kept when
    any of them selects it."""
    score = np.asarray(score, dtype=np.float32)
    n = score.shape[0]
    key = order_key(score).astype(np.int64)
    mask = np.zeros(n, dtype=bool)
    for a, b in segments(graph_pointers, n):
        if b <= a:
            continue
        rows = sorted(range(a, b), key=lambda r: (-key[r], r))[:keep_count(b - a, ratio, k)]
        mask[rows] = True
    return mask


def brute_force_keep(score, graph_pointers, ratio=None, k=None):
    """The same mask without a sort: row r of a segment is kept when fewer than k rows of the segment beat it, where r' beats r
    when its key is larger, or equal with r' < r."""
    score = np.asarray(score, dtype=np.float32)
    n = score.shape[0]
    key = order_key(score).astype(np.int64)
    mask = np.zeros(n, dtype=bool)
    for a, b in segments(graph_pointers, n):
        kk = keep_count(max(b - a, 0), ratio, k)
        for r in range(a, b):
            beaten_by = sum(1 for q in range(a, b) if key[q] > key[r] or (key[q] == key[r] and q < r))
            if beaten_by < kk:
                mask[r] = True
    return mask


def build_part(row_pointers, partSize):
    """(partPtr [P + 1], part2Node [P]) as gnna_build_part_i32 gives them: every row's edges in groups of partSize."""
    pp, p2n = [], []
    for i in range(len(row_pointers) - 1):
        for s in range(int(row_pointers[i]), int(row_pointers[i + 1]), partSize):
            pp.append(s)
            p2n.append(i)
    pp.append(int(row_pointers[-1]) if len(row_pointers) > 1 else 0)
    return np.asarray(pp, dtype=np.int32), np.asarray(p2n, dtype=np.int32)


def segment_topk(score, graph_pointers, ratio=None, k=None, row_pointers=None, column_index=None, partSize=None):
    """-> dict of int32 arrays: new_id [N], perm [N'], graph_pointers [G + 1]; with a CSR row_pointers [N' + 1], column_index
    [nnz'], edge_ids [nnz']; with partSize partPtr / part2Node."""
    score = np.asarray(score, dtype=np.float32)
    n = score.shape[0]
    mask = keep_mask(score, graph_pointers, ratio, k)
    perm = np.flatnonzero(mask).astype(np.int32)
    new_id = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32)
    below = np.concatenate(([0], np.cumsum(mask)))                        # kept rows below every row
    p = np.clip(np.asarray(graph_pointers, dtype=np.int64), 0, n)
    out = dict(new_id=new_id, perm=perm, graph_pointers=below[p].astype(np.int32))
    if row_pointers is None:
        return out
    rp, ci = np.asarray(row_pointers, dtype=np.int64), np.asarray(column_index, dtype=np.int64)
    new_rp, new_ci, eid = [0], [], []
    for r in perm:
        for e in range(rp[r], rp[r + 1]):
            c = ci[e]
            if 0 <= c < n and mask[c]:
                new_ci.append(new_id[c])
                eid.append(e)
        new_rp.append(len(new_ci))
    out.update(row_pointers=np.asarray(new_rp, dtype=np.int32), column_index=np.asarray(new_ci, dtype=np.int32),
               edge_ids=np.asarray(eid, dtype=np.int32))
    if partSize is not None:
        out["partPtr"], out["part2Node"] = build_part(out["row_pointers"], partSize)
    return out


def gather_rows_scale(X, perm, scale=None):
    """float32 [M, dim]: scale[perm[i]] * X[perm[i]], one fp32 multiplication; zeros for a perm[i] outside the rows of X."""
    X = np.asarray(X, dtype=np.float32)
    out = np.zeros((len(perm), X.shape[1]), dtype=np.float32)
    for i, r in enumerate(perm):
        if 0 <= r < X.shape[0]:
            out[i] = X[r] if scale is None else np.float32(scale[r]) * X[r]
    return out


def gather_rows_scale_backward(dY, new_id, X=None, scale=None):
    """(d_input float32 [N, dim], d_scale fp64 [N], the sum of |terms| of d_scale fp64 [N]); d_scale and its terms are None
    without X."""
    dY = np.asarray(dY, dtype=np.float32)
    n, m, dim = len(new_id), dY.shape[0], dY.shape[1]
    d_input = np.zeros((n, dim), dtype=np.float32)
    d_scale = None if X is None else np.zeros(n)
    terms = None if X is None else np.zeros(n)
    for r, j in enumerate(new_id):
        if not 0 <= j < m:
            continue
        d_input[r] = dY[j] if scale is None else np.float32(scale[r]) * dY[j]
        if X is not None:
            prod = dY[j].astype(np.float64) * np.asarray(X[r], dtype=np.float64)
            d_scale[r], terms[r] = prod.sum(), np.abs(prod).sum()
    return d_input, d_scale, terms

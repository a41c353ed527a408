"""fp64 numpy restatement of include/gnna_edgefeat.h (forward, d_input, d_edge, each with its sum-of-|terms| scale) and the case
builders of the edge-feature tests.  The relu mask is taken from the fp32 `pre`, as the header states."""
import numpy as np
import torch

COMBINES = {"add": 0, "mul": 1}
ACTS = {"none": 0, "relu": 1}
MODES = [(c, a) for c in ("add", "mul") for a in ("none", "relu")]


def _edges(rp, ci, num_in_rows, num_edges):
    """(destination row, source id, position) of every edge that counts: the id inside [0, num_in_rows), the position < num_edges."""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n = len(rp) - 1
    lo, hi = np.minimum(rp[:-1], num_edges), np.minimum(rp[1:], num_edges)
    lo = np.minimum(lo, hi)
    counts = hi - lo
    rows = np.repeat(np.arange(n), counts)
    first = np.cumsum(counts) - counts                                    # where a row's edges begin in the list
    pos = np.arange(int(counts.sum()), dtype=np.int64) + np.repeat(lo - first, counts)
    src = ci[pos] if len(pos) else pos
    ok = (src >= 0) & (src < num_in_rows)
    return rows, src, pos, ok


def _sum_by(keys, vals, n):
    """out[k] = the sum of the rows of `vals` whose key is k (one sort, one reduceat)."""
    out = np.zeros((n, vals.shape[1]))
    if len(keys):
        order = np.argsort(keys, kind="stable")
        k, v = keys[order], vals[order]
        starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
        out[k[starts]] = np.add.reduceat(v, starts, axis=0)
    return out


def _pre_and_mask(X, E, src, pos, combine, act):
    x32, e32 = np.asarray(X, dtype=np.float32)[src], np.asarray(E, dtype=np.float32)[pos]
    pre32 = x32 + e32 if combine == "add" else x32 * e32                  # fp32: what decides the mask
    x, e = x32.astype(np.float64), e32.astype(np.float64)
    pre = x + e if combine == "add" else x * e
    mask = (pre32 > 0) if act == "relu" else np.ones_like(pre32, dtype=bool)
    return x, e, pre, mask


def forward(rp, ci, X, E, combine, act, num_edges=None):
    """-> (out [num_out_rows, dim], scale): the sum of the messages and of their magnitudes."""
    X, E = np.asarray(X), np.asarray(E)
    num_edges = len(E) if num_edges is None else num_edges
    rows, src, pos, ok = _edges(rp, ci, len(X), num_edges)
    rows, src, pos = rows[ok], src[ok], pos[ok]
    _, _, pre, mask = _pre_and_mask(X, E, src, pos, combine, act)
    msg = np.where(mask, pre, 0.0)
    n = len(rp) - 1
    return _sum_by(rows, msg, n), _sum_by(rows, np.abs(msg), n)


def backward(rp, ci, X, E, dY, combine, act, num_edges=None):
    """-> (d_input, its scale, d_edge, its scale); d_edge has num_edges rows, a skipped edge's is 0."""
    X, E, dY = np.asarray(X), np.asarray(E), np.asarray(dY, dtype=np.float32).astype(np.float64)
    num_edges = len(E) if num_edges is None else num_edges
    rows, src, pos, ok = _edges(rp, ci, len(X), num_edges)
    rows, src, pos = rows[ok], src[ok], pos[ok]
    x, e, _, mask = _pre_and_mask(X, E, src, pos, combine, act)
    g = np.where(mask, dY[rows], 0.0)
    to_x = g * e if combine == "mul" else g
    to_e = g * x if combine == "mul" else g
    d_in, s_in = _sum_by(src, to_x, len(X)), _sum_by(src, np.abs(to_x), len(X))
    d_e = np.zeros((num_edges, X.shape[1]))
    d_e[pos] = to_e
    return d_in, s_in, d_e, np.abs(d_e)


# ---- case builders ----

def small_rows_graph(num_rows, num_in_rows, seed, lo=2, hi=4):
    """A CSR whose every row has lo .. hi edges to random sources (the rows of a batch of molecules)."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(lo, hi + 1, size=num_rows)
    rp = np.zeros(num_rows + 1, dtype=np.int32)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, num_in_rows, size=int(rp[-1])).astype(np.int32)
    return rp, ci


def operands(num_in_rows, num_out_rows, nnz, dim, seed, integer=False):
    """(X, E, dY) float32: standard normal, or small integers (every sum is then exact in fp32)."""
    rng = np.random.default_rng(seed)
    if integer:
        draw = lambda *shape: rng.integers(-4, 5, size=shape).astype(np.float32)          # noqa: E731
    else:
        draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)               # noqa: E731
    return draw(num_in_rows, dim), draw(nnz, dim), draw(num_out_rows, dim)


def symmetric_graph(num_nodes, num_pairs, seed):
    """A symmetric structure without self loops or duplicates as a sorted CSR."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, num_nodes, size=num_pairs), rng.integers(0, num_nodes, size=num_pairs)
    keep = a != b
    pairs = np.unique(np.concatenate([np.stack([a[keep], b[keep]], 1), np.stack([b[keep], a[keep]], 1)]), axis=0)
    rp = np.zeros(num_nodes + 1, dtype=np.int32)
    np.add.at(rp, pairs[:, 0] + 1, 1)
    return np.cumsum(rp).astype(np.int32), pairs[:, 1].astype(np.int32)


def composed_torch(X, E, rp, ci, combine, act):
    """The composed formula in torch (any dtype, differentiable): X[ci] (+ | *) E, relu, index_add_ by destination row."""
    n = rp.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    xj = X[ci.long()]
    msg = xj + E if combine == "add" else xj * E
    if act == "relu":
        msg = torch.relu(msg)
    return torch.zeros(n, X.shape[1], dtype=X.dtype).index_add_(0, dst, msg)

"""fp64 numpy restatement of include/gnna_attnpool.h: attention pooling over the contiguous row segments of graph_pointers and its
backward pass, with the scale of every result -- the sum of the |terms| that an fp32 evaluation's error is proportional to:
sum alpha |x| for out, |lse| for lse, alpha |dY| for dX, alpha * sum |dY| (|x| + |Y|) for dGate (without the sum over the columns
for a gate per element)."""
import numpy as np

from pool_ref import segments


def gate_2d(gate):
    gate = np.asarray(gate)
    return gate[:, None] if gate.ndim == 1 else gate


def reference(X, gate, graph_pointers, dY=None):
    """-> dict: out, lse (fp64) and out_scale, lse_scale; with dY also dX, dGate [n, gate_dim], dX_scale, dGate_scale."""
    X = np.asarray(X, dtype=np.float64)
    S = gate_2d(gate).astype(np.float64)
    n, d = X.shape
    gd = S.shape[1]
    assert S.shape[0] == n and gd in (1, d)
    segs = segments(graph_pointers, n)
    G = len(segs)
    r = dict(out=np.zeros((G, d)), lse=np.zeros((G, gd)), out_scale=np.zeros((G, d)))
    if dY is not None:
        dY = np.asarray(dY, dtype=np.float64)
        r.update(dX=np.zeros((n, d)), dGate=np.zeros((n, gd)), dX_scale=np.zeros((n, d)), dGate_scale=np.zeros((n, gd)))
    for g, (a, b) in enumerate(segs):
        if b <= a:
            continue
        s, x = S[a:b], X[a:b]
        m = s.max(0)
        lse = m + np.log(np.exp(s - m).sum(0))
        alpha = np.exp(s - lse)                              # [rows, gd]; broadcasts over the columns when gd == 1
        r["lse"][g] = lse
        r["out"][g] = (alpha * x).sum(0)
        r["out_scale"][g] = (alpha * np.abs(x)).sum(0)
        if dY is not None:
            y, dy = r["out"][g], dY[g]
            r["dX"][a:b] = alpha * dy
            r["dX_scale"][a:b] = alpha * np.abs(dy)
            t, ts = alpha * dy * (x - y), alpha * np.abs(dy) * (np.abs(x) + np.abs(y))
            if gd == 1:
                t, ts = t.sum(1, keepdims=True), ts.sum(1, keepdims=True)
            r["dGate"][a:b], r["dGate_scale"][a:b] = t, ts
    r["lse_scale"] = np.abs(r["lse"])
    return r

"""fp64 reference of the softmax neighbor aggregation (include/gnna_softagg.h) on the CPU, in index form (no dense matrix), with
the sum-of-|terms| scale of every result, and the dense formula in torch for fp64 autograd on small graphs.

Per destination row i and channel f, over the edges i <- j (a duplicate edge counts twice; an id outside the source rows is left
out), with s = t[f] * x[j, f]:

    lse = logsumexp_j s (0 for a row without edges), alpha = exp(s - lse), out = sum_j alpha x, sq = sum_j alpha x^2
    dX[j, f] = sum over the edges i <- j of alpha * dY[i, f] * (1 + t[f] * (x[j, f] - out[i, f]))
    dt[f]    = sum_i dY[i, f] * (sq[i, f] - out[i, f]^2)        (summed over f as well for a scalar t)

Scales (what fp32 rounding errors are proportional to): sum alpha |x| for out, sum alpha x^2 for sq, |lse| for lse,
sum alpha |dY| (1 + |t| (|x_j| + |out_i|)) for dX, sum |dY| (sq + out^2) for dt."""
import numpy as np
import torch


def edges_of(rp, ci, n_in):
    """(destination row, source row) of every edge of the CSR whose id lies in [0, n_in), int64."""
    rp, ci = torch.as_tensor(rp).cpu().long(), torch.as_tensor(ci).cpu().long()
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])
    ok = (ci >= 0) & (ci < n_in)
    return rows[ok], ci[ok]


def transpose_csr(rp, ci, n_in):
    """(t_rp, t_ci) int32: A^T of the valid edges, n_in rows whose ids are destination rows (a stable sort by source row)."""
    rows, src = edges_of(rp, ci, n_in)
    order = torch.argsort(src, stable=True)
    t_rp = torch.zeros(n_in + 1, dtype=torch.int64)
    t_rp[1:] = torch.cumsum(torch.bincount(src, minlength=n_in), 0)
    return t_rp.int(), rows[order].int()


def reference(X, t, rp, ci, dY=None):
    """-> dict of fp64 tensors: out, lse, sq and their scales out_scale, sq_scale, lse_scale; with dY also dX, dt, dX_scale,
    dt_scale (dt has t's number of elements)."""
    X = torch.as_tensor(X).cpu().double()
    t = torch.as_tensor(t).cpu().double().reshape(-1)
    n_in, F = X.shape
    n_out = len(rp) - 1
    rows, src = edges_of(rp, ci, n_in)
    G = X[src]
    s = G * t
    z = lambda n=n_out: torch.zeros(n, F, dtype=torch.float64)
    idx = rows.unsqueeze(1).expand_as(s)
    m = torch.full((n_out, F), -np.inf, dtype=torch.float64).scatter_reduce_(0, idx, s, "amax", include_self=True)
    has = ~torch.isinf(m)
    m = torch.where(has, m, z())
    e = torch.exp(s - m[rows])
    l = z().index_add_(0, rows, e)
    one = torch.ones_like(l)
    alpha = e / torch.where(has, l, one)[rows]
    ref = {"lse": torch.where(has, m + torch.log(torch.where(has, l, one)), z())}
    ref["out"] = z().index_add_(0, rows, alpha * G)
    ref["sq"] = z().index_add_(0, rows, alpha * G * G)
    ref["out_scale"] = z().index_add_(0, rows, alpha * G.abs())
    ref["sq_scale"] = ref["sq"]
    ref["lse_scale"] = ref["lse"].abs()
    if dY is not None:
        dY = torch.as_tensor(dY).cpu().double()
        g, Yr = dY[rows], ref["out"][rows]
        ref["dX"] = z(n_in).index_add_(0, src, alpha * g * (1.0 + t * (G - Yr)))
        ref["dX_scale"] = z(n_in).index_add_(0, src, alpha * g.abs() * (1.0 + t.abs() * (G.abs() + Yr.abs())))
        dt = (dY * (ref["sq"] - ref["out"] ** 2)).sum(0)
        dt_scale = (dY.abs() * (ref["sq"] + ref["out"] ** 2)).sum(0)
        ref["dt"] = dt if t.numel() > 1 else dt.sum().reshape(1)
        ref["dt_scale"] = dt_scale if t.numel() > 1 else dt_scale.sum().reshape(1)
    return ref


def worst_ratio(got, ref, scale, rtol=1e-4):
    """max over the elements of |got - ref| / (rtol * max(1, scale)): <= 1 is assert_close_f64's bound."""
    got, ref, scale = (np.asarray(torch.as_tensor(a).detach().cpu().double()) for a in (got, ref, scale))
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - ref) / (rtol * np.maximum(1.0, scale))
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def counts_matrix(rp, ci, n_in):
    """Dense fp64 [n_out, n_in]: how often the edge i <- j occurs."""
    rows, src = edges_of(rp, ci, n_in)
    A = torch.zeros(len(rp) - 1, n_in, dtype=torch.float64)
    A.index_put_((rows, src), torch.ones(rows.numel(), dtype=torch.float64), accumulate=True)
    return A


def dense_forward(X, t, A):
    """The dense formula in torch (differentiable in X and t): Y[i, f] = sum_j alpha[i, j, f] X[j, f] with
    alpha = A[i, j] exp(t[f] X[j, f]) / sum_j' A[i, j'] exp(t[f] X[j', f]); rows of A without an entry give 0."""
    S = (X * t.reshape(1, -1)).unsqueeze(0) + torch.log(A).unsqueeze(2)          # [n_out, n_in, F]; log 0 = -inf: no edge
    has = (A.sum(1) > 0).reshape(-1, 1, 1)
    S = torch.where(has, S, torch.zeros_like(S))
    alpha = torch.where(has, torch.softmax(S, dim=1), torch.zeros_like(S))
    return (alpha * X.unsqueeze(0)).sum(1)

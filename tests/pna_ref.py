"""fp64 torch restatement of the one-gather neighbour statistics (checker side only; on the CPU) from the CENTRED definition:
mean = sum x / c, var = sum (x - mean)^2 / c (never negative, so no clamp), std = sqrt(var + eps), c = max(count, 1); max / min as
in reduce_ref.py.  ``_bounds`` gives the scales of test_pna_ops_gpu.py's docstring.  Shared by test_pna_ops_gpu.py and
test_ops_layouts_gpu.py."""
import torch

EPS = 1e-5


def _zeros(n, like):
    return torch.zeros(n, like.shape[1], dtype=torch.float64)


def _stats64(X, rows, src, n_out, eps=EPS):
    """(mean, std, max, min) in fp64 from the centred definition; differentiable in X."""
    G = X[src]
    c = torch.bincount(rows, minlength=n_out).clamp(min=1).double().unsqueeze(1)
    mean = _zeros(n_out, X).index_add(0, rows, G) / c
    var = _zeros(n_out, X).index_add(0, rows, (G - mean[rows]) ** 2) / c
    idx = rows[:, None].expand_as(G)
    mx = _zeros(n_out, X).scatter_reduce(0, idx, G, reduce="amax", include_self=False)
    mn = _zeros(n_out, X).scatter_reduce(0, idx, G, reduce="amin", include_self=False)
    return mean, torch.sqrt(var + eps), mx, mn


def _no_ties(X, rows, src, n_out):
    _, _, mx, mn = _stats64(X, rows, src, n_out)
    for ext in (mx, mn):
        hits = torch.zeros_like(ext).index_add_(0, rows, (X[src] == ext[rows]).double())
        if not bool((hits <= 1).all()):
            return False
    return True


def _bounds(X, rows, src, n_out, grads, std64):
    """(mean scale, std tolerance, dX scale) as the module docstring states them; grads: the four output gradients or None."""
    Xa = X.abs()
    c = torch.bincount(rows, minlength=n_out).clamp(min=1).double().unsqueeze(1)
    mabs = _zeros(n_out, X).index_add(0, rows, Xa[src]) / c
    m2 = _zeros(n_out, X).index_add(0, rows, X[src] ** 2) / c
    std_tol = 1e-4 * torch.clamp(3 * m2 / (std64 + EPS ** 0.5), min=1.0)
    g_mean, g_std, g_max, g_min = [None if g is None else g.abs() for g in grads]
    per_edge = torch.zeros(rows.numel(), X.shape[1], dtype=torch.float64)
    if g_mean is not None:
        per_edge += (g_mean / c)[rows]
    if g_std is not None:
        per_edge += (g_std / (c * std64))[rows] * (Xa[src] + mabs[rows])
    dx_scale = _zeros(X.shape[0], X).index_add(0, src, per_edge)
    Xr = X.clone().requires_grad_(True)                      # the same routing of the extremes' gradients, on |g|
    _, _, mx, mn = _stats64(Xr, rows, src, n_out)
    routed = sum((y * g).sum() for y, g in ((mx, g_max), (mn, g_min)) if g is not None)
    if torch.is_tensor(routed):
        routed.backward()
        dx_scale += Xr.grad
    return mabs, std_tol, dx_scale

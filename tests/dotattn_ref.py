"""fp64 restatement of the fused dot-product graph attention (include/gnna_dotattn.h) on a rectangular structure ([num_out_rows x
num_in_rows], duplicate edges count twice), with the dropout mask of tests/gat_drop_ref.py, and of a TransformerConv layer; with
the magnitude sums the tolerances are scaled by (checker side only; runs on whatever device its inputs are on).  Nothing here
reads the library.

    z = scale * <Q[i], K[j]>,  alpha = softmax_j z,  Y[i] = sum_j alpha k V[j]

Bounds (tests/util.py::assert_close_f64): kernel outputs 1e-5 * max(1, sum of |terms|); layer outputs and input gradients 1e-4 of
max|ref|; weight gradients 1e-4 of the sum-of-|terms| scale -- each times max(1, S), S = the maximum over the edges and heads of
|scale| sum_d |Q| |K|: the fp32 error of z (a sum of dim products) and of the argument of the exponential grows with that sum, and
every output is a sum of terms that carry alpha = exp(z - lse) as a factor.  The function is smooth: no element is excluded.
The terms.  With absdot = sum_f |G[i]| |V[j]| and crow[i] = sum_e alpha k absdot (the magnitude of c = <dY, Y>), an edge's |dz| is
bounded by adz = alpha (k absdot + crow); then
    Y: sum alpha k |V|      dQ[i]: |scale| sum_j adz |K[j]|      dK[j]: |scale| sum_i adz |Q[i]|      dV[j]: sum_i alpha k |G[i]|"""
import types

import torch

import gat_drop_ref as dref
import gat_rect_ref as gref


def attention64(Q, K, V, rows, cl, n_out, heads, scale, k=None):
    """fp64 attention from plain torch ops over the edge list (rows, cl): Q [n_out, heads * dim], K and V [n_in, heads * dim],
    k [nnz, heads] or None -> (Y [n_out, heads * dim], lse [n_out, heads], has_edges [n_out]).  Differentiable."""
    n_in = K.shape[0]
    dim = K.shape[1] // heads
    Qh, Kh, Vh = Q.reshape(Q.shape[0], heads, dim), K.reshape(n_in, heads, dim), V.reshape(n_in, heads, dim)
    kw = dict(dtype=Q.dtype, device=Q.device)
    z = scale * (Qh[rows] * Kh[cl]).sum(-1)                                  # [nnz, heads]
    m = torch.full((n_out, heads), -float("inf"), **kw)
    m = m.scatter_reduce(0, rows[:, None].expand_as(z), z.detach(), reduce="amax")
    ex = torch.exp(z - m[rows])
    den = torch.zeros(n_out, heads, **kw).index_add(0, rows, ex)
    alpha = ex / den[rows]
    if k is not None:
        alpha = alpha * k
    Y = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, alpha[:, :, None] * Vh[cl])
    has = torch.bincount(rows, minlength=n_out) > 0
    lse = torch.where(has[:, None], m + torch.log(den.detach().clamp(min=1e-300)), torch.zeros_like(m))
    return Y.reshape(n_out, heads * dim), lse, has


def magnitudes(Q, K, V, G, lse, rows, cl, heads, scale, k=None):
    """The sums of |terms| of the module docstring, from fp64 values (no gradient).  -> namespace(s_Y, s_dQ, s_dK, s_dV, S)."""
    with torch.no_grad():
        n_in, n_out = K.shape[0], Q.shape[0]
        dim = K.shape[1] // heads
        kw = dict(dtype=torch.float64, device=Q.device)
        Qh, Kh, Vh, Gh = Q.reshape(n_out, heads, dim), K.reshape(n_in, heads, dim), V.reshape(n_in, heads, dim), G.reshape(n_out, heads, dim)
        kk = torch.ones(cl.numel(), heads, **kw) if k is None else k
        alpha = torch.exp(scale * (Qh[rows] * Kh[cl]).sum(-1) - lse[rows])
        S = float(abs(scale) * (Qh[rows].abs() * Kh[cl].abs()).sum(-1).max()) if cl.numel() else 0.0
        absdot = (Gh[rows].abs() * Vh[cl].abs()).sum(-1)
        crow = torch.zeros(n_out, heads, **kw).index_add_(0, rows, alpha * kk * absdot)
        adz = alpha * (kk * absdot + crow[rows])                                # [nnz, heads]
        ak = (alpha * kk)[:, :, None]
        s_Y = torch.zeros(n_out, heads, dim, **kw).index_add_(0, rows, ak * Vh[cl].abs())
        s_dQ = abs(scale) * torch.zeros(n_out, heads, dim, **kw).index_add_(0, rows, adz[:, :, None] * Kh[cl].abs())
        s_dK = abs(scale) * torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl, adz[:, :, None] * Qh[rows].abs())
        s_dV = torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl, ak * Gh[rows].abs())
        W = heads * dim
        return types.SimpleNamespace(s_Y=s_Y.view(n_out, W), s_dQ=s_dQ.view(n_out, W), s_dK=s_dK.view(n_in, W), s_dV=s_dV.view(n_in, W), S=S)


def kernel_reference(Q, K, V, G, rp, ci, heads, scale, p=0.0, rng_seed=0):
    """Everything the five outputs are compared with: Q [n_out, W], K and V [n_in, W], G = dY [n_out, W] (any float dtype, any
    strides; computed in fp64 on their device), the mask of (p, rng_seed) when p > 0.  Q, K and V are separate leaves even when the
    caller passes views of one tensor: the entry returns dQ, dK and dV apart.  -> namespace(Y, lse, has, dQ, dK, dV, the fields of
    `magnitudes`, factor = max(1, S), reached, nnz, rows, cl, k)."""
    n_in, n_out = K.shape[0], Q.shape[0]
    rows, cl = gref.edges_of(rp, ci, n_in)
    k = dref.factors(rng_seed, rows, cl, heads, p, Q.device) if p > 0 else None
    Q64, K64, V64 = [t.detach().double().contiguous().clone().requires_grad_() for t in (Q, K, V)]
    G64 = G.detach().double()
    Y, lse, has = attention64(Q64, K64, V64, rows, cl, n_out, heads, scale, k)
    (Y * G64).sum().backward()
    m = magnitudes(Q64.detach(), K64.detach(), V64.detach(), G64, lse, rows, cl, heads, scale, k)
    reached = torch.bincount(cl, minlength=n_in) > 0
    zero = lambda t, ref: torch.zeros_like(ref) if t is None else t          # (a structure without edges: no gradient flows)
    return types.SimpleNamespace(Y=Y.detach(), lse=lse, has=has, dQ=zero(Q64.grad, Q64), dK=zero(K64.grad, K64), dV=zero(V64.grad, V64),
                                 reached=reached, nnz=int(cl.numel()), rows=rows, cl=cl, k=k, factor=max(1.0, m.S), **vars(m))


def transformer_layer64(X, W, W_skip, rp, ci, n_dst, heads, out_dim, concat, p=0.0, rng_seed=0, keep=None):
    """fp64 TransformerConv from the edge list: X [num_src, in] -> [num_dst, heads * out] (or [num_dst, out]); [Q | K | V] = X W with
    W [in, 3 * heads * out], Q the first num_dst rows, scale = 1 / sqrt(out); W_skip (or None) adds X[:num_dst] W_skip.  A square
    graph: num_dst = num_src.  Differentiable in X, W, W_skip.  keep: a dict that receives the projection and the attention's
    output with their gradients retained, and what `param_scales` reads after the backward."""
    n_src = X.shape[0]
    Wd = heads * out_dim
    scale = 1.0 / out_dim ** 0.5
    rows, cl = gref.edges_of(rp, ci, n_src)
    k = dref.factors(rng_seed, rows, cl, heads, p, X.device) if p > 0 else None
    P = X @ W
    Q, K, V = P[:n_dst, :Wd], P[:, Wd:2 * Wd], P[:, 2 * Wd:]
    Y, lse, _ = attention64(Q, K, V, rows, cl, n_dst, heads, scale, k)
    out = Y if concat or heads == 1 else Y.view(n_dst, heads, out_dim).mean(1)
    if W_skip is not None:
        out = out + X[:n_dst] @ W_skip
    if keep is not None:
        for t in (P, Y, out):
            if t.requires_grad:
                t.retain_grad()
        keep.update(P=P, Y=Y, out=out, lse=lse, rows=rows, cl=cl, k=k, heads=heads, scale=scale, n_dst=n_dst, Wd=Wd)
    return out


def param_scales(X, keep):
    """(sum of |terms| of dW, of dW_skip, S) after the backward of a transformer_layer64(keep=...): dW = X^T dP and dW_skip =
    X[:num_dst]^T d_out are sums over the rows."""
    P, n, Wd = keep["P"].detach(), keep["n_dst"], keep["Wd"]
    m = magnitudes(P[:n, :Wd], P[:, Wd:2 * Wd], P[:, 2 * Wd:], keep["Y"].grad, keep["lse"], keep["rows"], keep["cl"], keep["heads"],
                   keep["scale"], keep["k"])
    Xa = X.detach().abs()
    return Xa.t() @ keep["P"].grad.abs(), Xa[:n].t() @ keep["out"].grad.abs(), m.S


def inputs(n_out, n_in, heads, dim, seed):
    """Q [n_out, W], K and V [n_in, W], G [n_out, W] from torch.randn under manual_seed(seed); float32 on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    Q = torch.randn(n_out, heads * dim, generator=gen)
    K = torch.randn(n_in, heads * dim, generator=gen)
    V = torch.randn(n_in, heads * dim, generator=gen)
    G = torch.randn(n_out, heads * dim, generator=torch.Generator().manual_seed(seed + 1))
    return Q, K, V, G

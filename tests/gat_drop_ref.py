"""Restatement of the attention-dropout mask of gnna_gat_forward_drop_f32 / gnna_gat_backward_drop_f32 (include/gnna_ext.h) and
the fp64 reference of the five outputs with the mask (checker side only; nothing here reads the library).

The mask: for an edge i <- j and head h, u = (i << 35) | (j << 6) | h, key = sampling_ref.keys_of(rng_seed, u) (the sampler's
key function, imported unchanged), kept = (key >> 32) >= floor(float32(p) * 2^32), k = kept ? float32(1) / (float32(1) - p) : 0.
The reference applies k after the softmax, Y = sum alpha k H, and takes dH, d_el, d_er from fp64 autograd.  The magnitude sums
are those of gat_rect_ref.kernel_reference with k inside the terms: Y: sum alpha k |H|; dH: sum alpha k |G|; d_el / d_er: an edge
contributes alpha (k sum_f |G| |H| + sum_e alpha k sum_f |G| |H|) to the rows it feeds (dz = alpha (k dalpha - c), c = sum_e alpha
k dalpha).  Bounds and the kink rule are gat_rect_ref's."""
import types

import numpy as np
import torch

import gat_rect_ref as gref
from sampling_ref import keys_of


def threshold(p):
    """thr of the rule: computed from the float32 value of p, in double."""
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def keep_scale(p):
    """k of a kept edge: 1.0f / (1.0f - p) in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(rng_seed, rows, ids, heads, p):
    """bool [len(rows), heads]: which (edge, head) pairs are kept.  rows: destination rows i, ids: source rows j."""
    i = np.asarray(rows, dtype=np.uint64)[:, None]
    j = np.asarray(ids, dtype=np.uint64)[:, None]
    h = np.arange(heads, dtype=np.uint64)[None, :]
    u = (i << np.uint64(35)) | (j << np.uint64(6)) | h
    return (keys_of(rng_seed, u) >> np.uint64(32)) >= np.uint64(threshold(p))


def factors(rng_seed, rows, ids, heads, p, device="cpu"):
    """float64 tensor [nnz, heads] of k."""
    kept = keep_mask(rng_seed, rows.cpu().numpy(), ids.cpu().numpy(), heads, p)
    return torch.from_numpy(kept.astype(np.float64) * keep_scale(p)).to(device)


def attention64(H, el, er, rows, cl, n_out, heads, slope, k):
    """gat_rect_ref.attention64 with alpha scaled by k [nnz, heads] after the softmax -> (Y, lse, has, sum of |terms| of Y).
    lse is that of the undropped scores."""
    n_in = H.shape[0]
    dim = H.shape[1] // heads
    Hh = H.view(n_in, heads, dim)
    kw = dict(dtype=H.dtype, device=H.device)
    s = torch.nn.functional.leaky_relu(el[rows] + er[cl], slope)
    m = torch.full((n_out, heads), -float("inf"), **kw)
    m = m.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax")
    ex = torch.exp(s - m[rows])
    den = torch.zeros(n_out, heads, **kw).index_add(0, rows, ex)
    alpha = ex / den[rows] * k
    Y = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, alpha[:, :, None] * Hh[cl])
    scale = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, (alpha[:, :, None] * Hh[cl].abs()).detach())
    has = torch.bincount(rows, minlength=n_out) > 0
    lse = torch.where(has[:, None], m + torch.log(den.detach().clamp(min=1e-300)), torch.zeros_like(m))
    return Y.reshape(n_out, heads * dim), lse, has, scale.reshape(n_out, heads * dim)


def kernel_reference(H, el, er, G, rp, ci, heads, slope, p, rng_seed, what=""):
    """gat_rect_ref.kernel_reference with the mask: the same namespace, plus k [nnz, heads], rows, cl and `none_kept`
    (bool [n_out, heads]: pairs that have edges and keep none of them)."""
    n_in, n_out = H.shape[0], el.shape[0]
    dim = H.shape[1] // heads
    rows, cl = gref.edges_of(rp, ci, n_in)
    k = factors(rng_seed, rows, cl, heads, p, H.device)
    H64, el64, er64 = [t.detach().double().contiguous().requires_grad_() for t in (H, el, er)]
    G64 = G.detach().double()
    Y, lse, has, s_Y = attention64(H64, el64, er64, rows, cl, n_out, heads, slope, k)
    (Y * G64).sum().backward()
    kw = dict(dtype=torch.float64, device=H.device)
    with torch.no_grad():
        Hh, Gh = H64.view(n_in, heads, dim), G64.view(n_out, heads, dim)
        z = el64[rows] + er64[cl]
        alpha = torch.exp(torch.nn.functional.leaky_relu(z, slope) - lse[rows])
        absdot = (Gh[rows].abs() * Hh[cl].abs()).sum(-1)
        crow = torch.zeros(n_out, heads, **kw).index_add_(0, rows, alpha * k * absdot)
        term = alpha * (k * absdot + crow[rows])
        s_el = torch.zeros(n_out, heads, **kw).index_add_(0, rows, term)
        s_er = torch.zeros(n_in, heads, **kw).index_add_(0, cl, term)
        s_dH = torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl, (alpha * k)[:, :, None] * Gh[rows].abs()).view(n_in, heads * dim)
        kink = (z.abs() <= 1e-6) if slope != 1.0 else torch.zeros_like(z, dtype=torch.bool)
        excluded = int(kink.any(1).sum())
        assert excluded < 1e-3 * max(1, cl.numel()), f"{what}: {excluded} of {cl.numel()} edges at the kink"
        ok_el = torch.ones(n_out, heads, dtype=torch.bool, device=H.device)
        ok_er = torch.ones(n_in, heads, dtype=torch.bool, device=H.device)
        if excluded:
            e, h = kink.nonzero(as_tuple=True)
            ok_el[rows[e], h] = False
            ok_er[cl[e], h] = False
        reached = torch.bincount(cl, minlength=n_in) > 0
        kept_count = torch.zeros(n_out, heads, **kw).index_add_(0, rows, (k > 0).double())
        none_kept = has[:, None] & (kept_count == 0)
    return types.SimpleNamespace(Y=Y.detach(), lse=lse, has=has, s_Y=s_Y, dH=H64.grad, d_el=el64.grad, d_er=er64.grad, s_dH=s_dH,
                                 s_el=s_el, s_er=s_er, ok_el=ok_el, ok_er=ok_er, reached=reached, excluded=excluded,
                                 nnz=int(cl.numel()), k=k, rows=rows, cl=cl, none_kept=none_kept, kept_count=kept_count)


def gat_layer64(X, W, a_l, a_r, rp, ci, n_dst, heads, out_dim, concat, p, rng_seed, slope=0.2, keep=None):
    """gat_rect_ref.gat_layer64 with the mask of (p, rng_seed) on the attention coefficients."""
    n_src = X.shape[0]
    rows, cl = gref.edges_of(rp, ci, n_src)
    k = factors(rng_seed, rows, cl, heads, p, X.device)
    H = X @ W
    Hh = H.view(n_src, heads, out_dim)
    el = (Hh[:n_dst] * a_l).sum(-1)
    er = (Hh * a_r).sum(-1)
    if keep is not None:
        for t in (H, el, er):
            t.retain_grad()
        keep.update(H=H, el=el, er=er)
    Y = attention64(H, el, er, rows, cl, n_dst, heads, slope, k)[0]
    return Y if concat or heads == 1 else Y.view(n_dst, heads, out_dim).mean(1)

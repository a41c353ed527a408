"""fp64 restatement of the fused GAT attention with a per-edge score term (include/gnna_gat_edge.h) over the edge list with
positions, and of a GAT layer with edge features (checker side only; runs on whatever device its inputs are on).  Nothing here
reads the library.

    z[e,h] = el[i,h] + er[j,h] + ee[e,h],  alpha = softmax over the row of leaky_relu(z),  Y[i,h,:] = sum_e alpha k H[j,h,:]

with k the dropout factor of gat_drop_ref.factors (1 without dropout).  ee, alpha and d_ee are [nnz, heads] over ALL positions of
column_index; an edge whose id lies outside the source rows is skipped (alpha = d_ee = 0 there).  The gradients come from fp64
autograd; the formulas of the header (dz = alpha (k dalpha - c) (z > 0 ? 1 : slope), d_ee = dz, ...) are evaluated beside it and
must agree with it, and serve the case autograd cannot state: transposed edges that the source-side pass skips (`t_skip`), which
are missing from d_er and dH only.

Bounds and magnitude sums are gat_rect_ref's (kernel outputs 1e-5 of max(1, sum of |terms|)): Y: sum alpha k |H|; dH: sum alpha k
|G|; an edge contributes term[e,h] = alpha (k absdot + crow[i]) to d_el[i], d_er[j], and term[e,h] is the scale of d_ee[e,h]
itself (absdot = sum_f |G| |H|, crow = sum_e alpha k absdot).  alpha: 1e-5 absolute (alpha <= 1).  The kink rule: with slope != 1
an edge with |z| <= 1e-6 is excluded from the d_el / d_er elements it feeds and from its own d_ee element; fewer than 1e-3 of
the edges may be."""
import types

import torch

import gat_drop_ref as dref
import gat_rect_ref as gref


def edges_with_positions(rp, ci, n_in):
    """(rows, ids, pos) as int64 of the edges whose id is inside [0, n_in); pos: their positions in column_index."""
    rp, ci = rp.long(), ci.long()
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])
    keep = (ci >= 0) & (ci < n_in)
    return rows[keep], ci[keep], keep.nonzero(as_tuple=True)[0]


def attention64(H, el, er, ee_kept, rows, cl, n_out, heads, slope, k=None):
    """gat_rect_ref.attention64 with the edge term ee_kept [kept edges, heads] in the score and alpha scaled by k after the
    softmax -> (Y, lse, has, sum of |terms| of Y, alpha undropped).  Differentiable in H, el, er, ee_kept."""
    n_in = H.shape[0]
    dim = H.shape[1] // heads
    Hh = H.view(n_in, heads, dim)
    kw = dict(dtype=H.dtype, device=H.device)
    s = torch.nn.functional.leaky_relu(el[rows] + er[cl] + ee_kept, slope)
    m = torch.full((n_out, heads), -float("inf"), **kw)
    m = m.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax")
    ex = torch.exp(s - m[rows])
    den = torch.zeros(n_out, heads, **kw).index_add(0, rows, ex)
    alpha = ex / den[rows]
    ak = alpha if k is None else alpha * k
    Y = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, ak[:, :, None] * Hh[cl])
    scale = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, (ak[:, :, None] * Hh[cl].abs()).detach())
    has = torch.bincount(rows, minlength=n_out) > 0
    lse = torch.where(has[:, None], m + torch.log(den.detach().clamp(min=1e-300)), torch.zeros_like(m))
    return Y.reshape(n_out, heads * dim), lse, has, scale.reshape(n_out, heads * dim), alpha


def kernel_reference(H, el, er, ee, G, rp, ci, heads, slope, p=0.0, rng_seed=0, t_skip=None, what=""):
    """Everything the seven outputs are compared with.  ee [nnz, heads] over all positions; t_skip: bool [nnz] over forward
    positions, the edges whose transposed edge the source-side pass skips (missing from d_er and dH only).
    -> namespace(Y, lse, has, s_Y, alpha, dH, d_el, d_er, d_ee, s_dH, s_el, s_er, s_ee, ok_el, ok_er, ok_ee, reached, excluded,
    nnz, rows, cl, pos, z)."""
    n_in, n_out, nnz_all = H.shape[0], el.shape[0], ci.numel()
    dim = H.shape[1] // heads
    dev = H.device
    rows, cl, pos = edges_with_positions(rp, ci, n_in)
    kw = dict(dtype=torch.float64, device=dev)
    k = dref.factors(rng_seed, rows, cl, heads, p, dev) if p > 0.0 else torch.ones(cl.numel(), heads, **kw)
    H64, el64, er64 = [t.detach().double().contiguous().requires_grad_() for t in (H, el, er)]
    ee64 = ee.detach().double()[pos].contiguous().requires_grad_()
    G64 = G.detach().double()
    Y, lse, has, s_Y, alpha_kept = attention64(H64, el64, er64, ee64, rows, cl, n_out, heads, slope, k)
    (Y * G64).sum().backward()
    with torch.no_grad():
        Hh, Gh = H64.view(n_in, heads, dim), G64.view(n_out, heads, dim)
        z = el64[rows] + er64[cl] + ee64
        alpha = torch.exp(torch.nn.functional.leaky_relu(z, slope) - lse[rows])
        dalpha = (Gh[rows] * Hh[cl]).sum(-1)
        c = (Gh * Y.view(n_out, heads, dim)).sum(-1)
        dz = alpha * (k * dalpha - c[rows]) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
        src = torch.ones(cl.numel(), dtype=torch.bool, device=dev) if t_skip is None else ~t_skip.to(dev)[pos]
        d_el = torch.zeros(n_out, heads, **kw).index_add_(0, rows, dz)
        d_er = torch.zeros(n_in, heads, **kw).index_add_(0, cl[src], dz[src])
        dH = torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl[src], (alpha * k)[src][:, :, None] * Gh[rows[src]])
        dH = dH.view(n_in, heads * dim)
        # the formulas of the header against autograd (all of them when no transposed edge is skipped)
        tol = lambda a, b: (a - b).abs().max().item() <= 1e-9 * max(1.0, b.abs().max().item())
        assert tol(d_el, el64.grad) and tol(dz, ee64.grad) and tol(alpha, alpha_kept.detach()), f"{what}: formulas vs autograd"
        if t_skip is None:
            assert tol(d_er, er64.grad) and tol(dH, H64.grad), f"{what}: formulas vs autograd (source side)"
        absdot = (Gh[rows].abs() * Hh[cl].abs()).sum(-1)
        crow = torch.zeros(n_out, heads, **kw).index_add_(0, rows, alpha * k * absdot)
        term = alpha * (k * absdot + crow[rows])
        s_el = torch.zeros(n_out, heads, **kw).index_add_(0, rows, term)
        s_er = torch.zeros(n_in, heads, **kw).index_add_(0, cl[src], term[src])
        s_dH = torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl[src], (alpha * k)[src][:, :, None] * Gh[rows[src]].abs())
        s_dH = s_dH.view(n_in, heads * dim)
        kink = (z.abs() <= 1e-6) if slope != 1.0 else torch.zeros_like(z, dtype=torch.bool)
        excluded = int(kink.any(1).sum())
        assert excluded < 1e-3 * max(1, cl.numel()), f"{what}: {excluded} of {cl.numel()} edges at the kink"
        ok_el = torch.ones(n_out, heads, dtype=torch.bool, device=dev)
        ok_er = torch.ones(n_in, heads, dtype=torch.bool, device=dev)
        ok_ee = torch.ones(nnz_all, heads, dtype=torch.bool, device=dev)
        if excluded:
            e, h = kink.nonzero(as_tuple=True)
            ok_el[rows[e], h] = False
            ok_er[cl[e], h] = False
            ok_ee[pos[e], h] = False
        full = lambda v: torch.zeros(nnz_all, heads, **kw).index_copy_(0, pos, v)
        reached = torch.bincount(cl[src], minlength=n_in) > 0
    return types.SimpleNamespace(Y=Y.detach(), lse=lse, has=has, s_Y=s_Y, alpha=full(alpha), dH=dH, d_el=d_el, d_er=d_er,
                                 d_ee=full(dz), s_dH=s_dH, s_el=s_el, s_er=s_er, s_ee=full(term), ok_el=ok_el, ok_er=ok_er,
                                 ok_ee=ok_ee, reached=reached, excluded=excluded, nnz=int(cl.numel()), rows=rows, cl=cl, pos=pos,
                                 z=z, k=k)


def edge_matrix(W_e, a_e, heads, out_dim):
    """M [edge_dim, heads] with M[d, h] = sum_c W_e[d, h * out + c] a_e[h, c]: ee = edge_attr @ M is PyG's
    (lin_edge(edge_attr).view(-1, heads, out) * att_edge).sum(-1) without the [nnz, heads * out] intermediate."""
    return (W_e.view(W_e.shape[0], heads, out_dim) * a_e).sum(-1)


def gat_layer64(X, W, a_l, a_r, W_e, a_e, edge_attr, rp, ci, n_dst, heads, out_dim, concat, slope=0.2, p=0.0, rng_seed=0, keep=None):
    """fp64 GATConv(edge_dim=...) from the edge list: X [num_src, in] -> [num_dst, heads * out] (or [num_dst, out]); a square
    graph has n_dst = num_src.  Differentiable in X, W, a_l, a_r, W_e, a_e, edge_attr.  keep: a dict that receives H, el, er,
    ee (all positions) and alpha (all positions) with their gradients retained."""
    n_src = X.shape[0]
    rows, cl, pos = edges_with_positions(rp, ci, n_src)
    H = X @ W
    Hh = H.view(n_src, heads, out_dim)
    el = (Hh[:n_dst] * a_l).sum(-1)
    er = (Hh * a_r).sum(-1)
    ee = edge_attr @ edge_matrix(W_e, a_e, heads, out_dim)
    if keep is not None:
        for t in (H, el, er, ee):
            t.retain_grad()
        keep.update(H=H, el=el, er=er, ee=ee)
    k = dref.factors(rng_seed, rows, cl, heads, p, X.device) if p > 0.0 else None
    Y, _, _, _, alpha = attention64(H, el, er, ee[pos], rows, cl, n_dst, heads, slope, k)
    if keep is not None:
        keep["alpha"] = torch.zeros(ci.numel(), heads, dtype=alpha.dtype, device=alpha.device).index_copy_(0, pos, alpha.detach())
    return Y if concat or heads == 1 else Y.view(n_dst, heads, out_dim).mean(1)


def param_scales(X, edge_attr, W_e, a_e, keep, heads, out_dim):
    """Sum of |terms| of (dW, da_l, da_r, dW_e, da_e, d edge_attr) after the backward of a gat_layer64(keep=...): those of
    gat_rect_ref.param_scales, and through ee = edge_attr @ M with M = edge_matrix(W_e, a_e): dM = edge_attr^T d_ee,
    dW_e[d, h out + c] = dM[d, h] a_e[h, c], da_e[h, c] = sum_d dM[d, h] W_e[d, h out + c], d edge_attr = d_ee M^T."""
    s_W, s_l, s_r = gref.param_scales(X, keep, heads, out_dim)
    d_ee = keep["ee"].grad.abs()
    s_M = edge_attr.detach().abs().t() @ d_ee                                         # [edge_dim, heads]
    We = W_e.detach().abs().view(W_e.shape[0], heads, out_dim)
    s_We = (s_M[:, :, None] * a_e.detach().abs()[None]).reshape(W_e.shape)
    s_ae = (s_M[:, :, None] * We).sum(0)
    s_ea = d_ee @ edge_matrix(W_e.detach().abs(), a_e.detach().abs(), heads, out_dim).t()
    return s_W, s_l, s_r, s_We, s_ae, s_ea

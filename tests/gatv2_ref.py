"""fp64 restatement of the fused GATv2 attention (include/gnna_gatv2.h) on a rectangular structure ([num_out_rows x num_in_rows],
duplicate edges count twice), with the dropout mask of tests/gat_drop_ref.py, and of a GATv2 layer; with the magnitude sums the
tolerances are scaled by (checker side only; runs on whatever device its inputs are on, so the kink cap can be checked without a
GPU).  Nothing here reads the library.

    t = Hs[j] + Hd[i],  z = sum_d att * lrelu(t),  alpha = softmax_j z,  Y[i] = sum_j alpha k Hs[j]

Bounds (tests/util.py::assert_close_f64): kernel outputs 1e-5 * max(1, sum of |terms|); layer outputs and input gradients 1e-4 of
max|ref|; parameter gradients 1e-4 of the sum-of-|terms| scale -- each times max(1, S), S = the maximum over the edges and heads of
sum_d |att| |lrelu(t)|: the fp32 error of z (a sum of dim products) and of the argument of the exponential grows with that sum,
and every output is a sum of terms that carry alpha = exp(z - lse) as a factor.
The terms.  With absdot = sum_f |G[i]| |Hs[j]| and crow[i] = sum_e alpha k absdot (the magnitude of c = <dY, Y>), an edge's
|dz| is bounded by adz = alpha (k absdot + crow); then
    Y: sum alpha k |Hs|      dHd[i]: sum_j adz |att| lr'      dHs[j]: sum_i (alpha k |G| + adz |att| lr')      d_att: sum adz |lrelu(t)|
with lr' = (t > 0 ? 1 : |slope|).
The kink.  z is continuous in t, so only dHs and dHd see on which side of 0 a t[d] falls: with slope != 1 an element (j, h, d) of
dHs or (i, h, d) of dHd is excluded when one of its edges has |t[d]| <= 1e-6; fewer than 1e-3 of the elements of either output may
be (asserted here).  d_att and the forward exclude nothing."""
import types

import torch

import gat_drop_ref as dref
import gat_rect_ref as gref

lrelu = torch.nn.functional.leaky_relu


def attention64(Hs, Hd, att, rows, cl, n_out, heads, slope, k=None):
    """fp64 attention from plain torch ops over the edge list (rows, cl): Hs [n_in, heads * dim], Hd [n_out, heads * dim], att
    [heads, dim], k [nnz, heads] or None -> (Y [n_out, heads * dim], lse [n_out, heads], has_edges [n_out]).  Differentiable."""
    n_in = Hs.shape[0]
    dim = Hs.shape[1] // heads
    Hsh, Hdh, a = Hs.view(n_in, heads, dim), Hd.view(Hd.shape[0], heads, dim), att.view(heads, dim)
    kw = dict(dtype=Hs.dtype, device=Hs.device)
    z = (lrelu(Hsh[cl] + Hdh[rows], slope) * a).sum(-1)                      # [nnz, heads]
    m = torch.full((n_out, heads), -float("inf"), **kw)
    m = m.scatter_reduce(0, rows[:, None].expand_as(z), z.detach(), reduce="amax")
    ex = torch.exp(z - m[rows])
    den = torch.zeros(n_out, heads, **kw).index_add(0, rows, ex)
    alpha = ex / den[rows]
    if k is not None:
        alpha = alpha * k
    Y = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, alpha[:, :, None] * Hsh[cl])
    has = torch.bincount(rows, minlength=n_out) > 0
    lse = torch.where(has[:, None], m + torch.log(den.detach().clamp(min=1e-300)), torch.zeros_like(m))
    return Y.reshape(n_out, heads * dim), lse, has


def magnitudes(Hs, Hd, att, G, lse, rows, cl, heads, slope, k=None):
    """The sums of |terms| of the module docstring and the kink masks, from fp64 values (no gradient).  -> namespace(s_Y, s_dHs,
    s_dHd, s_att, S, ok_dHs, ok_dHd, excluded_dHs, excluded_dHd)."""
    with torch.no_grad():
        n_in, n_out = Hs.shape[0], Hd.shape[0]
        dim = Hs.shape[1] // heads
        kw = dict(dtype=torch.float64, device=Hs.device)
        Hsh, Hdh, Gh, a = Hs.view(n_in, heads, dim), Hd.view(n_out, heads, dim), G.view(n_out, heads, dim), att.view(heads, dim)
        kk = torch.ones(cl.numel(), heads, **kw) if k is None else k
        t = Hsh[cl] + Hdh[rows]
        lt = lrelu(t, slope)
        alpha = torch.exp((lt * a).sum(-1) - lse[rows])
        S = float((lt.abs() * a.abs()).sum(-1).max()) if cl.numel() else 0.0
        absdot = (Gh[rows].abs() * Hsh[cl].abs()).sum(-1)
        crow = torch.zeros(n_out, heads, **kw).index_add_(0, rows, alpha * kk * absdot)
        adz = alpha * (kk * absdot + crow[rows])                                # [nnz, heads]
        dlr = torch.where(t > 0, torch.ones_like(t), torch.full_like(t, abs(slope)))
        g = adz[:, :, None] * a.abs() * dlr
        s_Y = torch.zeros(n_out, heads, dim, **kw).index_add_(0, rows, (alpha * kk)[:, :, None] * Hsh[cl].abs())
        s_dHd = torch.zeros(n_out, heads, dim, **kw).index_add_(0, rows, g)
        s_dHs = torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl, (alpha * kk)[:, :, None] * Gh[rows].abs() + g)
        s_att = (adz[:, :, None] * lt.abs()).sum(0)
        kink = (t.abs() <= 1e-6) if slope != 1.0 else torch.zeros_like(t, dtype=torch.bool)
        ok_dHs = torch.ones(n_in, heads, dim, dtype=torch.bool, device=Hs.device)
        ok_dHd = torch.ones(n_out, heads, dim, dtype=torch.bool, device=Hs.device)
        if bool(kink.any()):
            e, h, d = kink.nonzero(as_tuple=True)
            ok_dHs[cl[e], h, d] = False
            ok_dHd[rows[e], h, d] = False
        W = heads * dim
        return types.SimpleNamespace(s_Y=s_Y.view(n_out, W), s_dHs=s_dHs.view(n_in, W), s_dHd=s_dHd.view(n_out, W), s_att=s_att, S=S,
                                     ok_dHs=ok_dHs.view(n_in, W), ok_dHd=ok_dHd.view(n_out, W),
                                     excluded_dHs=int((~ok_dHs).sum()), excluded_dHd=int((~ok_dHd).sum()))


def kernel_reference(Hs, Hd, att, G, rp, ci, heads, slope, p=0.0, rng_seed=0, what=""):
    """Everything the six outputs are compared with: Hs [n_in, W], Hd [n_out, W], att [heads, dim], G = dY [n_out, W] (any float
    dtype; computed in fp64 on their device), the mask of (p, rng_seed) when p > 0.  Hs and Hd are separate leaves even when
    the caller passes one tensor twice: the entry returns dHs and dHd apart.  -> namespace(Y, lse, has, dHs, dHd, d_att, the fields
    of `magnitudes`, factor = max(1, S), reached, nnz, rows, cl, k)."""
    n_in, n_out = Hs.shape[0], Hd.shape[0]
    rows, cl = gref.edges_of(rp, ci, n_in)
    k = dref.factors(rng_seed, rows, cl, heads, p, Hs.device) if p > 0 else None
    Hs64, Hd64, att64 = [t.detach().double().contiguous().clone().requires_grad_() for t in (Hs, Hd, att)]
    G64 = G.detach().double()
    Y, lse, has = attention64(Hs64, Hd64, att64, rows, cl, n_out, heads, slope, k)
    (Y * G64).sum().backward()
    m = magnitudes(Hs64.detach(), Hd64.detach(), att64.detach(), G64, lse, rows, cl, heads, slope, k)
    for name, excluded, total in (("dHs", m.excluded_dHs, Hs.numel()), ("dHd", m.excluded_dHd, Hd.numel())):
        assert excluded < 1e-3 * max(1, total), f"{what}: {excluded} of {total} elements of {name} at the kink"
    reached = torch.bincount(cl, minlength=n_in) > 0
    return types.SimpleNamespace(Y=Y.detach(), lse=lse, has=has, dHs=Hs64.grad, dHd=Hd64.grad, d_att=att64.grad, reached=reached,
                                 nnz=int(cl.numel()), rows=rows, cl=cl, k=k, factor=max(1.0, m.S), **vars(m))


def gatv2_layer64(X, W_l, W_r, att, rp, ci, n_dst, heads, out_dim, concat, slope=0.2, p=0.0, rng_seed=0, keep=None):
    """fp64 GATv2Conv from the edge list: X [num_src, in] -> [num_dst, heads * out] (or [num_dst, out]); Hs = X W_l, Hd =
    X[:num_dst] W_r, or the first num_dst rows of Hs with W_r None (shared weights).  A square graph: num_dst = num_src.
    Differentiable in X, W_l, W_r, att.  keep: a dict that receives Hs, Hd and the attention's output with their gradients
    retained, and what `param_scales` reads after the backward."""
    n_src = X.shape[0]
    rows, cl = gref.edges_of(rp, ci, n_src)
    k = dref.factors(rng_seed, rows, cl, heads, p, X.device) if p > 0 else None
    Hs = X @ W_l
    Hd = Hs[:n_dst] if W_r is None else X[:n_dst] @ W_r
    Y, lse, _ = attention64(Hs, Hd, att, rows, cl, n_dst, heads, slope, k)
    if keep is not None:
        for t in (Hs, Hd, Y):
            if t.requires_grad:
                t.retain_grad()
        keep.update(Hs=Hs, Hd=Hd, Y=Y, lse=lse, rows=rows, cl=cl, k=k, att=att, heads=heads, slope=slope, n_dst=n_dst,
                    shared=W_r is None)
    return Y if concat or heads == 1 else Y.view(n_dst, heads, out_dim).mean(1)


def param_scales(X, keep):
    """(sum of |terms| of dW_l, of dW_r (None with shared weights), of d_att, S) after the backward of a gatv2_layer64(keep=...):
    dW = X^T dH is a sum over the rows, d_att the kernel's sum over the edges for the dY the layer's backward handed it."""
    m = magnitudes(keep["Hs"].detach(), keep["Hd"].detach(), keep["att"].detach(), keep["Y"].grad, keep["lse"], keep["rows"],
                   keep["cl"], keep["heads"], keep["slope"], keep["k"])
    Xa, n = X.detach().abs(), keep["n_dst"]
    s_Wl = Xa.t() @ keep["Hs"].grad.abs()            # (shared weights: the gradient of Hs[:n] as Hd has been added to it)
    s_Wr = None if keep["shared"] else Xa[:n].t() @ keep["Hd"].grad.abs()
    return s_Wl, s_Wr, m.s_att, m.S


def inputs(n_out, n_in, heads, dim, seed):
    """Hs [n_in, W], Hd [n_out, W] from torch.randn under manual_seed(seed), att [heads, dim] uniform in +-1/sqrt(dim) (the layer's
    init, so that S stays of order sqrt(dim) / 2), G [n_out, W]; float32 on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    Hs = torch.randn(n_in, heads * dim, generator=gen)
    Hd = torch.randn(n_out, heads * dim, generator=gen)
    att = (torch.rand(heads, dim, generator=gen) * 2 - 1) / dim ** 0.5
    G = torch.randn(n_out, heads * dim, generator=torch.Generator().manual_seed(seed + 1))
    return Hs, Hd, att, G

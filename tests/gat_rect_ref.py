"""fp64 restatement of the fused GAT attention on a rectangular structure ([num_out_rows x num_in_rows], duplicate edges count
twice) and of a GAT layer on a block, with the magnitude sums the tolerances are scaled by (checker side only; runs on whatever
device its inputs are on, so the kink cap can be checked without a GPU).  Nothing here reads the library.

Bounds (tests/util.py::assert_close_f64, as tests/test_gat_fused_gpu.py): kernel outputs rtol 1e-5 of max(1, sum of |terms|);
layer outputs and input gradients 1e-4 of max|ref|; parameter gradients 1e-4 of the sum-of-|terms| scale.  The terms of
d_el / d_er: dz = alpha (dalpha - c) with dalpha = sum_f G H and c = sum_e alpha dalpha, so an edge contributes
alpha (sum_f |G| |H| + sum_e alpha sum_f |G| |H|) to the magnitude sum of the row it feeds.  With slope != 1 the edges with
|z| <= 1e-6 (the kink of leaky_relu may fall on either side in fp32) are excluded: the (row, head) and (source, head) they feed
are left out of d_el / d_er; fewer than 1e-3 of the edges may be."""
import types

import numpy as np
import torch


def edges_of(rp, ci, n_in):
    """(rows, ids) as int64 of the edges whose id is inside [0, n_in): the others are skipped by every pass."""
    rp, ci = rp.long(), ci.long()
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])
    keep = (ci >= 0) & (ci < n_in)
    return rows[keep], ci[keep]


def attention64(H, el, er, rows, cl, n_out, heads, slope):
    """fp64 attention from plain torch ops: H [n_in, heads * dim], el [n_out, heads], er [n_in, heads] over the edge list
    (rows, cl) -> (Y [n_out, heads * dim], lse [n_out, heads], has_edges [n_out], sum of |terms| of Y).  Differentiable."""
    n_in = H.shape[0]
    dim = H.shape[1] // heads
    Hh = H.view(n_in, heads, dim)
    kw = dict(dtype=H.dtype, device=H.device)
    s = torch.nn.functional.leaky_relu(el[rows] + er[cl], slope)                  # [nnz, heads]
    m = torch.full((n_out, heads), -float("inf"), **kw)
    m = m.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax")
    ex = torch.exp(s - m[rows])
    den = torch.zeros(n_out, heads, **kw).index_add(0, rows, ex)
    alpha = ex / den[rows]
    Y = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, alpha[:, :, None] * Hh[cl])
    scale = torch.zeros(n_out, heads, dim, **kw).index_add(0, rows, (alpha[:, :, None] * Hh[cl].abs()).detach())
    has = torch.bincount(rows, minlength=n_out) > 0
    lse = torch.where(has[:, None], m + torch.log(den.detach().clamp(min=1e-300)), torch.zeros_like(m))
    return Y.reshape(n_out, heads * dim), lse, has, scale.reshape(n_out, heads * dim)


def kernel_reference(H, el, er, G, rp, ci, heads, slope, what=""):
    """Everything the five outputs are compared with: H [n_in, W], el [n_out, heads], er [n_in, heads], G = dY [n_out, W] (any
    float dtype; computed in fp64 on their device).  -> namespace(Y, lse, has, s_Y, dH, d_el, d_er, s_dH, s_el, s_er, ok_el,
    ok_er, reached, excluded, nnz)."""
    n_in, n_out = H.shape[0], el.shape[0]
    dim = H.shape[1] // heads
    rows, cl = edges_of(rp, ci, n_in)
    H64, el64, er64 = [t.detach().double().contiguous().requires_grad_() for t in (H, el, er)]
    G64 = G.detach().double()
    Y, lse, has, s_Y = attention64(H64, el64, er64, rows, cl, n_out, heads, slope)
    (Y * G64).sum().backward()
    kw = dict(dtype=torch.float64, device=H.device)
    with torch.no_grad():
        Hh, Gh = H64.view(n_in, heads, dim), G64.view(n_out, heads, dim)
        z = el64[rows] + er64[cl]
        alpha = torch.exp(torch.nn.functional.leaky_relu(z, slope) - lse[rows])
        absdot = (Gh[rows].abs() * Hh[cl].abs()).sum(-1)                             # [nnz, heads]
        crow = torch.zeros(n_out, heads, **kw).index_add_(0, rows, alpha * absdot)
        term = alpha * (absdot + crow[rows])
        s_el = torch.zeros(n_out, heads, **kw).index_add_(0, rows, term)
        s_er = torch.zeros(n_in, heads, **kw).index_add_(0, cl, term)
        s_dH = torch.zeros(n_in, heads, dim, **kw).index_add_(0, cl, alpha[:, :, None] * Gh[rows].abs()).view(n_in, heads * dim)
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
    return types.SimpleNamespace(Y=Y.detach(), lse=lse, has=has, s_Y=s_Y, dH=H64.grad, d_el=el64.grad, d_er=er64.grad, s_dH=s_dH,
                                 s_el=s_el, s_er=s_er, ok_el=ok_el, ok_er=ok_er, reached=reached, excluded=excluded,
                                 nnz=int(cl.numel()))


def gat_layer64(X, W, a_l, a_r, rp, ci, n_dst, heads, out_dim, concat, slope=0.2, keep=None):
    """fp64 GATConv on a block from the edge list: X [num_src, in] -> [num_dst, heads * out] (or [num_dst, out]); el from the
    first num_dst rows of H = X W, er from all of them.  Differentiable in X, W, a_l, a_r.  keep: a dict that receives H, el
    and er with their gradients retained (what param_scales reads after the backward)."""
    n_src = X.shape[0]
    rows, cl = edges_of(rp, ci, n_src)
    H = X @ W
    Hh = H.view(n_src, heads, out_dim)
    el = (Hh[:n_dst] * a_l).sum(-1)
    er = (Hh * a_r).sum(-1)
    if keep is not None:
        for t in (H, el, er):
            t.retain_grad()
        keep.update(H=H, el=el, er=er)
    Y = attention64(H, el, er, rows, cl, n_dst, heads, slope)[0]
    return Y if concat or heads == 1 else Y.view(n_dst, heads, out_dim).mean(1)


def param_scales(X, keep, heads, out_dim):
    """Sum of |terms| of (dW, da_l, da_r) after the backward of a gat_layer64(keep=...): the parameter gradients are sums over
    all rows, dW = X^T dH, da_l[h] = sum_i d_el[i, h] H[i, h, :], da_r[h] = sum_j d_er[j, h] H[j, h, :]."""
    H, el, er = keep["H"], keep["el"], keep["er"]
    Hh = H.detach().abs().view(H.shape[0], heads, out_dim)
    s_W = X.detach().abs().t() @ H.grad.abs()
    s_l = (Hh[:el.shape[0]] * el.grad.abs()[:, :, None]).sum(0)
    s_r = (Hh * er.grad.abs()[:, :, None]).sum(0)
    return s_W, s_l, s_r


def inputs(n_out, n_in, heads, dim, seed):
    """Seeded H [n_in, heads * dim], el [n_out, heads], er [n_in, heads], G [n_out, heads * dim] on the CPU (float32)."""
    gen = torch.Generator().manual_seed(seed)
    H = torch.randn(n_in, heads * dim, generator=gen)
    el = torch.randn(n_out, heads, generator=gen)
    er = torch.randn(n_in, heads, generator=gen)
    G = torch.randn(n_out, heads * dim, generator=torch.Generator().manual_seed(seed + 1))
    return H, el, er, G


def wide_short_structure(n_out=700, n_in=300, hub_row=17, hub_edges=5000, empty=40, unreached=20, seed=23):
    """More destination rows than source rows: random unsorted ids with duplicates, `empty` rows without edges, one row of
    `hub_edges` edges (the long-row path of the lse pass: > 2,048), and the last `unreached` source rows named by no edge.
    -> (rp, ci) int32 numpy."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 12, size=n_out)
    deg[rng.permutation(np.setdiff1d(np.arange(n_out), [hub_row]))[:empty]] = 0
    deg[hub_row] = hub_edges
    rp = np.zeros(n_out + 1, dtype=np.int64)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n_in - unreached, size=rp[-1])
    assert (deg == 0).sum() == empty and len(np.unique(ci[rp[hub_row]:rp[hub_row + 1]])) < hub_edges
    return rp.astype(np.int32), ci.astype(np.int32)


THRESHOLDS = (32, 64, 128, 256, 512, 1024, 2048)
THRESHOLD_N_IN = 150


def threshold_lengths():
    """The row lengths threshold_structure() must contain: the shortest rows and t - 1, t, t + 1 around every power of two t at
    which a pass changes its path (sorted)."""
    return sorted({0, 1, 2, 3, 5} | {t + d for t in THRESHOLDS for d in (-1, 0, 1)})


def threshold_structure(extra=36, unreached=10, seed=31):
    """A [62 x 150] structure whose destination rows have every length of threshold_lengths() once -- a row is `long` for GAT's lse
    pass above seg * 32 edges (seg = 4 .. 64 lanes) and for the shared lse pass of GATv2 / dot above (64 / LPR) * 32, and a pull
    kernel loads 64 ids per step, so each of those switches sits between two rows -- and `extra` rows of 1 .. 11 edges, in a seeded
    random order.  Random unsorted ids with duplicates (the long rows have far more edges than there are sources); the last
    `unreached` source rows are named by no edge.  About 12,400 edges.  -> (rp, ci) int32 numpy; THRESHOLD_N_IN source rows."""
    rng = np.random.default_rng(seed)
    deg = np.concatenate([np.array(threshold_lengths()), rng.integers(1, 12, size=extra)])
    deg = deg[rng.permutation(len(deg))]
    rp = np.zeros(len(deg) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, THRESHOLD_N_IN - unreached, size=rp[-1])
    return rp.astype(np.int32), ci.astype(np.int32)


def multi_run_structure(num_groups, partSize, unreached=10, seed=41):
    """A structure with exactly `num_groups` neighbor-groups at `partSize` (1 or 100) whose rows are runs of several groups, for the
    launches that give a wavefront more than one group.  partSize 1: rows of 0 .. 12 edges, so a row of k edges is a run of k
    groups.  partSize 100: rows of 1 .. 8 edges (one group) and every 50th row 250 edges (three groups).  The source side has a
    third of the rows (the transposed structure has longer rows, and enough groups for G >= 2 there too), random unsorted ids
    with duplicates, the last `unreached` sources named by no edge.  -> (rp, ci, num_in_rows), int32 numpy."""
    assert partSize in (1, 100) and num_groups >= 64
    rng = np.random.default_rng(seed + partSize)
    if partSize == 1:
        deg = rng.integers(0, 13, size=num_groups // 5)                 # mean 6: more rows than needed
        cut = int(np.searchsorted(np.cumsum(deg), num_groups, side="left"))
        deg = deg[:cut + 1]
        deg[-1] -= deg.sum() - num_groups                               # (the last row is shortened to the count; never below 1)
    else:
        n = num_groups                                                  # an upper bound of the rows
        deg = rng.integers(1, 9, size=n)
        deg[26::50] = 250
        groups = np.cumsum(-(-deg // partSize))
        cut = int(np.searchsorted(groups, num_groups, side="left"))
        deg = deg[:cut + 1]
        if groups[cut] != num_groups:                                   # a three-group row overshoots: one group in its place
            deg[-1] = 7
            deg = np.concatenate([deg, np.full(num_groups - int(groups[cut - 1]) - 1, 3)])
    assert int((-(-deg // partSize)).sum()) == num_groups
    rp = np.zeros(len(deg) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(deg)
    n_in = max(64, len(deg) // 3) + unreached
    ci = rng.integers(0, n_in - unreached, size=rp[-1])
    return rp.astype(np.int32), ci.astype(np.int32), n_in


def plant_out_of_range(ci, n_in, every=9):
    """A copy of ci with every `every`-th id replaced by one outside [0, n_in): n_in itself, n_in + 7, 2^31 - 1 and -1 in turn."""
    out = np.array(ci, dtype=np.int64)
    bad = np.array([n_in, n_in + 7, 2 ** 31 - 1, -1])
    pos = np.arange(3, len(out), every)
    out[pos] = bad[np.arange(len(pos)) % 4]
    return out.astype(np.int32)

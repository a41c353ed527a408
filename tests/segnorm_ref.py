"""An fp32 numpy restatement of how ``csrc/gnna_segnorm.hip`` gathers the centred moments of a segment, and the fp64 reference of
the whole function: what the accuracy contract of ``include/gnna_segnorm.h`` is checked against on a machine without a GPU
(test_segnorm_host.py), and what the GPU tests compare the kernels with (test_segnorm_gpu.py).

The restatement follows the kernels' order of operations, every one rounded to fp32: a slot of a wavefront takes the rows
``base + k * slots + slot`` of a piece, ``ROWS_IN_FLIGHT`` per step; the rows of a step enter as their own (count, mean, centred
sum); slots meet by a butterfly of the pairwise merge in which the lower slot is the left operand; a segment that crosses tile
boundaries is joined from one piece per tile -- slot t takes the tiles t, t + slots, ... in order, then the butterfly -- and a segment
of more than ``LONG_STEPS`` join steps by the four wavefronts of a workgroup, merged in wavefront order.  Columns are independent,
so a row of columns is carried as one array."""
import numpy as np

TILE = 256              # GNNA_POOL_TILE_ROWS
LONG_STEPS = 16         # GNNA_POOL_LONG_STEPS
ROWS_IN_FLIGHT = 4
WAVES = 4
f32 = np.float32


def lanes_per_row(dim):
    lpr = 1
    while lpr < 64 and 4 * lpr < dim:
        lpr *= 2
    return lpr


def long_segment_rows(dim):
    """The rows of the shortest segment that starts on a tile boundary and goes to the whole workgroup, plus 300."""
    return LONG_STEPS * (64 // lanes_per_row(dim)) * TILE + 300


def _zero(width):
    return f32(0), np.zeros(width, f32), np.zeros(width, f32)


def merge(x, y):
    """The pairwise merge of two (n, mean, m2) in fp32, x on the left."""
    (na, ma, qa), (nb, mb, qb) = x, y
    n = f32(na + nb)
    w = f32(nb / n) if n > 0 else f32(0)
    d = mb - ma
    return n, ma + d * w, (qa + qb) + (d * d) * f32(na * w)


def _butterfly(states):
    """The slots of a wavefront -> one: strides slots / 2 .. 1, the lower slot on the left."""
    states = list(states)
    d = len(states) // 2
    while d >= 1:
        states = [merge(states[s & ~d], states[s | d]) for s in range(len(states))]
        d //= 2
    return states[0]


def _piece(x, slots):
    """(n, mean, m2) of the rows x [rows, width] (fp32) as one wavefront gathers them."""
    rows, width = x.shape
    out = []
    for slot in range(slots):
        acc = _zero(width)
        for base in range(0, rows, slots * ROWS_IN_FLIGHT):
            mine = [base + k * slots + slot for k in range(ROWS_IN_FLIGHT) if base + k * slots + slot < rows]
            n = f32(len(mine))
            s = np.zeros(width, f32)
            for r in mine:
                s = s + x[r]
            mean = s * (f32(1) / n if n > 0 else f32(0))
            q = np.zeros(width, f32)
            for r in mine:
                d = x[r] - mean
                q = q + d * d
            acc = merge(acc, (n, mean, q))
        out.append(acc)
    return _butterfly(out)


def moments_f32(x, start=0):
    """(mean, m2) [width] in fp32 of the segment whose rows are x [rows, width], the first of them row `start` of the matrix (which
    fixes the tile boundaries), in the kernels' order of operations."""
    x = np.ascontiguousarray(x, dtype=f32)
    rows, width = x.shape
    if rows == 0:
        return np.zeros(width, f32), np.zeros(width, f32)
    slots = 64 // lanes_per_row(width)
    end = start + rows
    tf, tl = start // TILE, (end - 1) // TILE
    if tf == tl:
        _, mean, m2 = _piece(x, slots)
        return mean, m2
    pieces = []
    for t in range(tf, tl + 1):
        lo, hi = max(start, t * TILE), min(end, (t + 1) * TILE)
        pieces.append(_piece(x[lo - start: hi - start], slots))
    nt = len(pieces)
    waves = WAVES if nt > slots * LONG_STEPS else 1
    per_wave = []
    for w in range(waves):
        states = []
        for slot in range(slots):
            acc = _zero(width)
            for i in range(w * slots + slot, nt, waves * slots):
                acc = merge(acc, pieces[i])
            states.append(acc)
        per_wave.append(_butterfly(states))
    acc = per_wave[0]
    if waves > 1:
        acc = _zero(width)
        for state in per_wave:
            acc = merge(acc, state)
    return acc[1], acc[2]


def naive_var_f32(x):
    """E[x^2] - E[x]^2 with fp32 sums: what the contract excludes."""
    x = np.ascontiguousarray(x, dtype=f32)
    n = f32(x.shape[0])
    s, q = np.zeros(x.shape[1], f32), np.zeros(x.shape[1], f32)
    for row in x:
        s = s + row
        q = q + row * row
    return q / n - (s / n) * (s / n)


def moments_f64(x):
    """(mean, var = m2 / n) of the fp32 values of x in fp64."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1]), np.zeros(x.shape[1])
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def statistics_bounds(x):
    """(bound on |mean - mean64|, bound on |var - var64|) [width] of the contract for the rows x of one segment."""
    x = np.asarray(x, dtype=np.float64)
    u = 2.0 ** -24 * np.abs(x).max(0)
    _, var = moments_f64(x)
    return 4.0 * u, 1e-5 * var + 4.0 * u * np.sqrt(var)


def segments_of(pointers, num_rows):
    """[(g, start, end)] with the pointers clamped to [0, num_rows]; a descending pair is empty."""
    p = np.clip(np.asarray(pointers, dtype=np.int64), 0, num_rows)
    return [(g, int(p[g]), int(max(p[g], p[g + 1]))) for g in range(len(p) - 1)]


def graph_norm_f64(x, pointers, weight=None, bias=None, alpha=None, eps=1e-5, d_out=None):
    """The whole function in fp64 from the plain formula.  -> dict(out, mean, m2, rstd, bound_out) and, with d_out, also d_input,
    seg_a, seg_b, d_weight, d_bias, d_alpha with a bound_* for each: 1e-4 * max(1, sum of the absolute values of the terms of the
    output's formula).  The gradients come from fp64 autograd of the plain formula."""
    import torch
    x64 = torch.as_tensor(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    n_rows, width = x64.shape
    one = lambda t, v: torch.full((width,), v, dtype=torch.float64) if t is None else torch.as_tensor(np.asarray(t, dtype=np.float64))
    w, b, a = (one(t, v).requires_grad_(True) for t, v in ((weight, 1.0), (bias, 0.0), (alpha, 1.0)))
    segs = segments_of(pointers, n_rows)
    G = len(segs)
    mean, m2, rstd = (torch.zeros(G, width, dtype=torch.float64) for _ in range(3))
    out = torch.zeros(n_rows, width, dtype=torch.float64)
    bound_out = torch.zeros(n_rows, width, dtype=torch.float64)
    used = False
    for g, s, e in segs:
        if e <= s:
            continue
        xs = x64[s:e]
        m = xs.mean(0)
        xc = xs - a * m
        var = (xc * xc).mean(0)
        r = 1.0 / torch.sqrt(var + eps)
        y = w * (xc * r) + b
        out[s:e] = y                                # (segments that overlap, after a descending pair: only the statistics are defined)
        used = True
        with torch.no_grad():
            mean[g], m2[g], rstd[g] = m, ((xs - m) ** 2).sum(0), r
            bound_out[s:e] = ((xs.abs() + (a * m).abs()) * r * w.abs() + b.abs())
    res = {"mean": mean.numpy(), "m2": m2.numpy(), "rstd": rstd.numpy()}
    res["out"] = out.detach().numpy()
    res["bound_out"] = 1e-4 * np.maximum(1.0, bound_out.numpy())
    if d_out is None:
        return res
    dy = torch.as_tensor(np.asarray(d_out, dtype=np.float64))
    if used:
        (out * dy).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res["d_input"], res["d_weight"], res["d_bias"], res["d_alpha"] = (zero(t).numpy() for t in (x64, w, b, a))
    # A, B and the sums of the absolute values of the terms of every backward formula
    with torch.no_grad():
        xd, wd, ad = x64.detach(), w.detach(), a.detach()
        A, B, absA, absB = (torch.zeros(G, width, dtype=torch.float64) for _ in range(4))
        bound_dx = torch.zeros(n_rows, width, dtype=torch.float64)
        for g, s, e in segs:
            if e <= s:
                continue
            n = e - s
            xhat = (xd[s:e] - ad * mean[g]) * rstd[g]
            A[g], B[g] = dy[s:e].sum(0), (dy[s:e] * xhat).sum(0)
            absA[g], absB[g] = dy[s:e].abs().sum(0), (dy[s:e] * xhat).abs().sum(0)
            mr = (mean[g] * rstd[g]).abs()
            bound_dx[s:e] = wd.abs() * rstd[g] * (dy[s:e].abs() + xhat.abs() * absB[g] / n +
                                                  ad.abs() * (absA[g] / n + (1 - ad).abs() * mr * absB[g] / n))
        mr = (mean * rstd).abs()
        res["seg_a"], res["seg_b"] = A.numpy(), B.numpy()
        res["bound_seg_a"], res["bound_seg_b"] = 1e-4 * np.maximum(1.0, absA.numpy()), 1e-4 * np.maximum(1.0, absB.numpy())
        res["bound_d_input"] = 1e-4 * np.maximum(1.0, bound_dx.numpy())
        res["bound_d_bias"] = 1e-4 * np.maximum(1.0, absA.sum(0).numpy())
        res["bound_d_weight"] = 1e-4 * np.maximum(1.0, absB.sum(0).numpy())
        res["bound_d_alpha"] = 1e-4 * np.maximum(1.0, (mr * wd.abs() * (absA + (1 - ad).abs() * mr * absB)).sum(0).numpy())
    return res

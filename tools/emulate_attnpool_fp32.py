"""fp32 numpy emulation of the arithmetic of csrc/gnna_attnpool.hip -- the slots of a wavefront, the steps of four rows, the
butterfly of state merges, the two pieces per tile, their join in tile order by a wavefront or the workgroup, exp as exp2 of the
product with log2(e), the backward's alpha = exp(s - lse) -- on the inputs of tests/test_attnpool_gpu.py, compared with the fp64
reference tests/attnpool_ref.py.  Prints the worst |error| / (1e-4 * max(1, scale)) of every output: the figure that the docstring
of that test file records.  Needs no GPU.

    python tools/emulate_attnpool_fp32.py [dims ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import attnpool_ref  # noqa: E402
import pool_ref  # noqa: E402
import test_attnpool_gpu as cases  # noqa: E402

f32 = np.float32
LOG2E = f32(1.44269504088896340736)
T, LONG_STEPS, U, WAVES = 256, 16, 4, 4


def exp_nonpos(d):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp2((d.astype(f32) * LOG2E).astype(f32)).astype(f32)


def merge(a, b):
    """state_merge on (m [.., gd], l [.., gd], acc [.., D])"""
    m = np.maximum(a[0], b[0])
    with np.errstate(invalid="ignore"):
        fa = np.where(np.isneginf(a[0]), f32(0), exp_nonpos(a[0] - m))
        fb = np.where(np.isneginf(b[0]), f32(0), exp_nonpos(b[0] - m))
    return m, (a[1] * fa + b[1] * fb).astype(f32), (a[2] * fa + b[2] * fb).astype(f32)


def empty(shape, gd, D):
    return (np.full(shape + (gd,), -np.inf, f32), np.zeros(shape + (gd,), f32), np.zeros(shape + (D,), f32))


def fold(st, R):
    """the butterfly over the R slots (axis -2): after it every slot holds the whole"""
    d = R // 2
    while d >= 1:
        idx = np.arange(R) ^ d
        st = merge(st, tuple(v[..., idx, :] for v in st))
        d //= 2
    return st


def piece(X, S, a, b, R):
    """attnpool_tile_kernel's walk over the rows [a, b): R slots, U rows per slot and step"""
    D, gd = X.shape[1], S.shape[1]
    m, l, acc = empty((R,), gd, D)
    for base in range(a, b, R * U):
        rows = base + np.arange(U)[:, None] * R + np.arange(R)[None, :]          # [U, R]
        live = rows < b
        safe = np.where(live, rows, a)
        z = np.where(live[..., None], S[safe], f32(-np.inf))                       # [U, R, gd]
        v = np.where(live[..., None], X[safe], f32(0))
        mx = np.maximum(m, z.max(0))
        with np.errstate(invalid="ignore"):
            r = np.where(np.isneginf(m), f32(0), exp_nonpos(m - mx))
        l, acc = (l * r).astype(f32), (acc * r).astype(f32)
        for k in range(U):
            with np.errstate(invalid="ignore"):
                e = np.where(np.isneginf(z[k]), f32(0), exp_nonpos(z[k] - mx))
            l = (l + e).astype(f32)
            acc = (acc + (e * v[k]).astype(f32)).astype(f32)
        m = mx
    st = fold((m, l, acc), R)
    return tuple(v[0] for v in st)


def join(pieces, R):
    """attnpool_finish_kernel: slot t takes the pieces t, t + slots, ...; a wavefront, or the workgroup for a long segment"""
    D, gd = pieces[0][2].shape[0], pieces[0][0].shape[0]
    whole = len(pieces) > R * LONG_STEPS
    nl = WAVES * R if whole else R
    slots = []
    for t in range(nl):
        st = tuple(v[0] for v in empty((1,), gd, D))
        for i in range(t, len(pieces), nl):
            st = merge(st, pieces[i])
        slots.append(st)
    waves = []
    for w in range(nl // R):
        st = tuple(np.stack([s[j] for s in slots[w * R:(w + 1) * R]]) for j in range(3))
        waves.append(tuple(v[0] for v in fold(st, R)))
    if not whole:
        return waves[0]
    st = tuple(v[0] for v in empty((1,), gd, D))
    for w in waves:
        st = merge(st, w)
    return st


def forward(X, S, gp):
    n, D = X.shape
    gd = S.shape[1]
    lanes = 1
    while lanes < 64 and 4 * lanes < D:
        lanes *= 2
    R = 64 // lanes
    segs = pool_ref.segments(gp, n)
    out, lse = np.zeros((len(segs), D), f32), np.zeros((len(segs), gd), f32)
    for g, (a, b) in enumerate(segs):
        if b <= a:
            continue
        cuts = [a] + [t for t in range((a // T + 1) * T, b, T)] + [b]
        ps = [piece(X, S, lo, hi, R) for lo, hi in zip(cuts[:-1], cuts[1:])]
        m, l, acc = ps[0] if len(ps) == 1 else join(ps, R)
        out[g] = (acc / l).astype(f32)
        lse[g] = (m + np.log(l).astype(f32)).astype(f32)
    return out, lse


def backward(X, S, gp, lse, Y, dY):
    n, D = X.shape
    gd = S.shape[1]
    dX, dG = np.zeros((n, D), f32), np.zeros((n, gd), f32)
    for g, (a, b) in enumerate(pool_ref.segments(gp, n)):
        if b <= a:
            continue
        al = exp_nonpos(S[a:b] - lse[g])
        dX[a:b] = (al * dY[g]).astype(f32)
        t = (dY[g] * (X[a:b] - Y[g]).astype(f32)).astype(f32)
        if gd == 1:
            dot = np.zeros(b - a, f32)
            for c in range(D):                                # (the kernel adds in another fixed order; the bound is the same)
                dot = (dot + t[:, c]).astype(f32)
            dG[a:b, 0] = (al[:, 0] * dot).astype(f32)
        else:
            dG[a:b] = (al * t).astype(f32)
    return dX, dG


def main(dims):
    worst = dict(out=0.0, lse=0.0, dX=0.0, dGate=0.0)
    for dim in dims:
        for name, (n, gp) in cases.layouts(dim).items():
            for gd in sorted({1, dim}):
                for family in ("normal", "shifted", "dominant"):
                    X, S, dY = cases.inputs(n, dim, gd, gp, 1000 + dim, family)
                    ref = attnpool_ref.reference(X, S, gp, dY)
                    out, lse = forward(X, S, gp)
                    dX, dG = backward(X, S, gp, lse, out, dY)
                    for key, got in (("out", out), ("lse", lse), ("dX", dX), ("dGate", dG)):
                        ratio = float((np.abs(got - ref[key]) / (1e-4 * np.maximum(1.0, ref[key + "_scale"]))).max())
                        worst[key] = max(worst[key], ratio)
                        assert np.isfinite(got).all(), (dim, name, gd, family, key)
        print("dim", dim, {k: "%.2e" % v for k, v in worst.items()}, flush=True)
    print("worst |error| / bound:", {k: "%.2e" % v for k, v in worst.items()})


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 3, 33, 64, 257])

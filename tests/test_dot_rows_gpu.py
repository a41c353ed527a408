"""gnna_dot_attn_forward_rows_f32 / gnna_dot_attn_backward_rows_f32 through the C ABI against the fp64 restatement of
tests/dotattn_ref.py (the mask of tests/gat_drop_ref.py), under the bound of the function: 1e-5 * max(1, sum of |terms|) * max(1, S)
per element, no element excluded.  Every call pre-fills its outputs with NaN; out-of-range ids are planted in both structures; the
transposed structure is the device-built one.  The ownership limits are those of the GAT rows kernels (8 edges for a slot,
(64 / LPR) * 128 for a wavefront), so the "limits" structure is theirs."""
import functools
import types

import pytest
import torch

import dotattn_ref as tref
import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib
from test_gat_rows_gpu import LENGTHS, LIMITS_N_IN, limits_structure

pytestmark = pytest.mark.gpu
CONFIGS = [(1, 64), (4, 16), (3, 5), (1, 1), (8, 40)]      # R = 4, 4, 8, 64, 1 (two column blocks of four heads)
NAMES = ("Y", "lse", "dQ", "dK", "dV")


@functools.lru_cache(maxsize=None)
def _structure(which):
    """The planted device structure and its device-built transpose."""
    (rp, ci), n_in = (gref.wide_short_structure(), 300) if which == "hub" else (limits_structure(), LIMITS_N_IN)
    ci = gref.plant_out_of_range(ci, n_in)
    s = types.SimpleNamespace(rp=torch.as_tensor(rp).cuda(), ci=torch.as_tensor(ci).cuda(), n_out=len(rp) - 1, n_in=n_in)
    s.t_rp, s.t_ci, _ = _lib.transpose_csr(s.rp, s.ci, num_in_rows=n_in, want_perm=False)
    if which == "limits":
        assert set(LENGTHS) <= set(torch.diff(s.rp).tolist()) and set(LENGTHS) <= set(torch.diff(s.t_rp).tolist())
    return s


@functools.lru_cache(maxsize=None)
def _case(which, heads, dim, p=0.0, seed=0):
    """(structure, inputs on the device, the fp64 reference): made once, shared and left unchanged."""
    s = _structure(which)
    ins = [t.cuda() for t in tref.inputs(s.n_out, s.n_in, heads, dim, heads + dim)]
    return s, ins, tref.kernel_reference(*ins, s.rp, s.ci, heads, 1 / dim ** 0.5, p, seed)


def _run(s, Q, K, V, G, heads, dim, p=0.0, seed=0, t=None, ld_out=None, flags=0):
    """Forward and backward through the C ABI into NaN-filled outputs with rows of ld_out floats -> (Y, lse, dQ, dK, dV) as
    allocated.  t: the transposed structure (default: the device-built one of s)."""
    W, lib, stream = heads * dim, _lib.load(), _lib._stream(Q.device)
    ld_out = ld_out or W
    t_rp, t_ci = t or (s.t_rp, s.t_ci)
    Y, lse, dQ, dK, dV = [torch.full(shape, float("nan"), device="cuda") for shape in
                          ((s.n_out, ld_out), (s.n_out, heads), (s.n_out, ld_out), (s.n_in, ld_out), (s.n_in, ld_out))]
    a = lambda x: x.data_ptr()
    qkv = (a(Q), Q.stride(0), a(K), K.stride(0), a(V), V.stride(0), s.n_in)
    scale = 1 / dim ** 0.5
    assert lib.gnna_dot_attn_forward_rows_f32(*qkv, a(s.rp), a(s.ci), scale, p, seed, a(Y), ld_out, a(lse), s.n_out, heads, dim, flags,
                                              stream) == 0, lib.gnna_last_error()
    assert lib.gnna_dot_attn_backward_rows_f32(*qkv, a(lse), a(Y), ld_out, a(G), G.stride(0), a(s.rp), a(s.ci), a(t_rp), a(t_ci), scale,
                                               p, seed, a(dQ), ld_out, a(dK), ld_out, a(dV), ld_out, s.n_out, heads, dim, 0,
                                               stream) == 0, lib.gnna_last_error()
    return Y, lse, dQ, dK, dV


def _within_the_bound(what, got, r):
    worst = {}
    for name, t, ref, scale, ok in zip(NAMES, got, (r.Y, r.lse, r.dQ, r.dK, r.dV), (r.s_Y, r.lse.abs(), r.s_dQ, r.s_dK, r.s_dV),
                                       (None, r.has, None, None, None)):
        assert torch.isfinite(t).all(), f"{name} has elements the call did not write, or that are not finite"
        ratio = (t.double() - ref).abs() / (1e-5 * r.factor * scale.clamp(min=1.0))
        worst[name] = float(ratio.max() if ok is None else ratio[ok].max())
    print(f"{what}: worst error / bound", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("heads,dim", CONFIGS)
@pytest.mark.parametrize("which", ["hub", "limits"])
def test_the_five_outputs_against_fp64(which, heads, dim):
    s, ins, r = _case(which, heads, dim)
    Y, lse, dQ, dK, dV = got = _run(s, *ins, heads, dim)
    assert r.nnz < s.ci.numel() and int(s.t_rp[-1]) == r.nnz and bool((~r.has).any()) and bool((~r.reached).any())
    _within_the_bound(f"{which} {heads}x{dim}", got, r)
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (dQ[~r.has] == 0).all(), "rows without edges give 0"
    assert (dK[~r.reached] == 0).all() and (dV[~r.reached] == 0).all(), "sources no edge reaches get exactly 0"


@pytest.mark.parametrize("heads,dim", [(4, 16), (3, 5)])
@pytest.mark.parametrize("which", ["hub", "limits"])          # limits: the key's row on slot-owned and workgroup-owned rows of A^T
def test_the_mask_is_the_fused_paths_and_leaves_lse_alone(which, heads, dim):
    seed = 2 ** 63 + 11
    s, ins, r = _case(which, heads, dim, 0.5, seed)
    got = _run(s, *ins, heads, dim, 0.5, seed)
    assert r.k is not None and bool((r.k == 0).any()) and bool((r.k == 2).any())
    _within_the_bound(f"{which} {heads}x{dim} attn_drop=0.5", got, r)
    assert torch.equal(got[1], _run(s, *ins, heads, dim)[1]), "lse is that of the un-dropped scores"


def test_two_runs_give_the_same_bits_and_deterministic_tuning_accepts_them():
    s, ins, _ = _case("hub", 4, 16)
    first, second = _run(s, *ins, 4, 16, 0.5, 7), _run(s, *ins, 4, 16, 0.5, 7)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    try:
        _lib.set_tuning(deterministic=1)
        third = _run(s, *ins, 4, 16, 0.5, 7)                  # (_run asserts that both entries answer success)
    finally:
        _lib.reset_tuning()
    assert all(torch.equal(a, b) for a, b in zip(first, third))


def test_slices_of_one_matrix_a_symmetric_structure_and_the_relu_epilogue():
    """Q | K | V are column slices of one [N, 3 W + 5] matrix, the structure is passed as its own transpose, the forward clamps."""
    heads, dim, n = 3, 5, 120
    W = heads * dim
    gen = torch.Generator().manual_seed(3)
    pairs = torch.randint(0, n, (2, 900), generator=gen)
    dense = torch.zeros(n, n, dtype=torch.bool)
    dense[pairs[0], pairs[1]] = dense[pairs[1], pairs[0]] = True
    dense[5] = dense[:, 5] = False                            # a row and a source without edges
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), dense.sum(1).cumsum(0)]).int().cuda()
    ci = dense.nonzero()[:, 1].int().cuda()
    s = types.SimpleNamespace(rp=rp, ci=ci, n_out=n, n_in=n)
    P = torch.randn(n, 3 * W + 5, generator=gen).cuda()
    G = torch.randn(n, W + 3, generator=gen).cuda()[:, :W]
    Q, K, V = P[:, :W], P[:, W:2 * W], P[:, 2 * W:3 * W]
    plain = _run(s, Q, K, V, G, heads, dim, t=(rp, ci), ld_out=W + 3)
    clamped = _run(s, Q, K, V, G, heads, dim, t=(rp, ci), ld_out=W + 3, flags=2)      # (its backward reads the clamped Y: not compared)
    for got in (plain, clamped):
        assert all(torch.isnan(t[:, W:]).all() for t in (got[0], *got[2:])), "the padding columns are never touched"
    assert torch.equal(clamped[0][:, :W], plain[0][:, :W].clamp(min=0)) and bool((plain[0][:, :W] < 0).any())
    assert torch.equal(clamped[1], plain[1])
    r = tref.kernel_reference(Q, K, V, G, rp, ci, heads, 1 / dim ** 0.5)
    _within_the_bound("slices", [t if t is plain[1] else t[:, :W] for t in plain], r)
    assert (plain[0][5, :W] == 0).all() and (plain[3][5, :W] == 0).all()

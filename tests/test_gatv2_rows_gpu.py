"""gnna_gatv2_forward_rows_f32 / gnna_gatv2_backward_rows_f32 through the C ABI against the fp64 restatement of tests/gatv2_ref.py
(the mask of tests/gat_drop_ref.py), under the bound of the atomic kernels' own test: 1e-5 * max(1, sum of |terms|) * max(1, S) per
element, the kink elements of dHs / dHd excluded (none is, in these cases).  Every call pre-fills its outputs with NaN;
out-of-range ids are planted in both structures; the transposed structure is the device-built one.  The ownership limits are those
of the GAT rows kernels (8 edges for a slot, (64 / LPR) * 128 for a wavefront), so the "limits" structure is theirs."""
import functools
import types

import pytest
import torch

import gat_rect_ref as gref
import gatv2_ref as vref
from gnnadvisor_osdi21_amd import _lib
from test_gat_rows_gpu import LENGTHS, LIMITS_N_IN, limits_structure

pytestmark = pytest.mark.gpu
CONFIGS = [(1, 64), (4, 16), (3, 5), (1, 1), (8, 40)]      # R = 4, 4, 8, 64, 1 (two column blocks of four heads)
NAMES = ("Y", "lse", "dHs", "dHd", "d_att")
SLOPE = 0.2


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
    ins = [t.cuda() for t in vref.inputs(s.n_out, s.n_in, heads, dim, heads + dim)]
    return s, ins, vref.kernel_reference(*ins, s.rp, s.ci, heads, SLOPE, p, seed, f"{which} {heads}x{dim}")


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _run(s, Hs, Hd, att, G, heads, dim, p=0.0, seed=0, t=None, ld_out=None, flags=0, want=(True, True, True), forward=None):
    """Forward and backward through the C ABI into NaN-filled outputs with rows of ld_out floats -> (Y, lse, dHs, dHd, d_att) as
    allocated (None for a gradient that is not wanted).  t: the transposed structure (default: the device-built one of s);
    forward: (Y, lse) of an earlier call, to run the backward alone."""
    W, lib, stream = heads * dim, _lib.load(), _lib._stream(Hs.device)
    ld_out = ld_out or W
    t_rp, t_ci = t or (s.t_rp, s.t_ci)
    a = lambda x: None if x is None else x.data_ptr()
    ins = (a(Hs), Hs.stride(0), a(Hd), Hd.stride(0), a(att), s.n_in)
    if forward is None:
        Y, lse = _nan(s.n_out, ld_out), _nan(s.n_out, heads)
        assert lib.gnna_gatv2_forward_rows_f32(*ins, a(s.rp), a(s.ci), SLOPE, p, seed, a(Y), ld_out, a(lse), s.n_out, heads, dim, flags,
                                               stream) == 0, lib.gnna_last_error()
    else:
        Y, lse = forward
    dHs, dHd, d_att = [_nan(*shape) if w else None for w, shape in zip(want, ((s.n_in, ld_out), (s.n_out, ld_out), (heads, dim)))]
    assert lib.gnna_gatv2_backward_rows_f32(*ins, a(lse), a(Y), ld_out, a(G), G.stride(0), a(s.rp), a(s.ci), a(t_rp), a(t_ci), SLOPE, p,
                                            seed, a(dHs), ld_out, a(dHd), ld_out, a(d_att), s.n_out, heads, dim, 0,
                                            stream) == 0, lib.gnna_last_error()
    return Y, lse, dHs, dHd, d_att


def _within_the_bound(what, got, r):
    worst = {}
    for name, t, ref, scale, ok in zip(NAMES, got, (r.Y, r.lse, r.dHs, r.dHd, r.d_att), (r.s_Y, r.lse.abs(), r.s_dHs, r.s_dHd, r.s_att),
                                       (None, r.has, r.ok_dHs, r.ok_dHd, None)):
        assert torch.isfinite(t).all(), f"{name} has elements the call did not write, or that are not finite"
        ratio = (t.double() - ref).abs() / (1e-5 * r.factor * scale.clamp(min=1.0))
        worst[name] = float(ratio.max() if ok is None else ratio[ok].max())
    print(f"{what}: worst error / bound", {k: round(v, 4) for k, v in worst.items()}, "S", round(r.S, 2),
          "excluded", r.excluded_dHs, r.excluded_dHd)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("heads,dim", CONFIGS)
@pytest.mark.parametrize("which", ["hub", "limits"])
def test_the_outputs_against_fp64(which, heads, dim):
    s, ins, r = _case(which, heads, dim)
    Y, lse, dHs, dHd, d_att = got = _run(s, *ins, heads, dim)
    assert r.nnz < s.ci.numel() and int(s.t_rp[-1]) == r.nnz and bool((~r.has).any()) and bool((~r.reached).any())
    _within_the_bound(f"{which} {heads}x{dim}", got, r)
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (dHd[~r.has] == 0).all(), "rows without edges give 0"
    assert (dHs[~r.reached] == 0).all(), "sources no edge reaches get exactly 0"


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


def test_one_matrix_for_both_sides_a_symmetric_structure_and_the_relu_epilogue():
    """Hs and Hd are the SAME column slice of a wider matrix, the structure is passed as its own transpose, the forward clamps."""
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
    H = torch.randn(n, W + 7, generator=gen).cuda()[:, 2:2 + W]
    G = torch.randn(n, W + 3, generator=gen).cuda()[:, :W]
    att = ((torch.rand(heads, dim, generator=gen) * 2 - 1) / dim ** 0.5).cuda()
    plain = _run(s, H, H, att, G, heads, dim, t=(rp, ci), ld_out=W + 3)
    clamped = _run(s, H, H, att, G, heads, dim, t=(rp, ci), ld_out=W + 3, flags=2)      # (its backward reads the clamped Y: not compared)
    for got in (plain, clamped):
        assert all(torch.isnan(t[:, W:]).all() for t in (got[0], got[2], got[3])), "the padding columns are never touched"
    assert torch.equal(clamped[0][:, :W], plain[0][:, :W].clamp(min=0)) and bool((plain[0][:, :W] < 0).any())
    assert torch.equal(clamped[1], plain[1])
    r = vref.kernel_reference(H, H, att, G, rp, ci, heads, SLOPE, what="one matrix")       # (Hs and Hd as separate leaves)
    _within_the_bound("one matrix", [plain[0][:, :W], plain[1], plain[2][:, :W], plain[3][:, :W], plain[4]], r)
    assert (plain[0][5, :W] == 0).all() and (plain[2][5, :W] == 0).all()


def test_null_outputs_give_the_bits_of_the_full_call():
    s, ins, _ = _case("limits", 3, 5)
    full = _run(s, *ins, 3, 5, 0.5, 7)
    for want in ((True, False, False), (False, True, True), (False, False, True)):
        part = _run(s, *ins, 3, 5, 0.5, 7, want=want, forward=full[:2])
        for name, w, a, b in zip(NAMES[2:], want, part[2:], full[2:]):
            assert (a is None) if not w else torch.equal(a, b), (want, name)


def test_the_empty_call_writes_zeros_to_d_att():
    heads, dim = 4, 16
    s = types.SimpleNamespace(rp=torch.zeros(1, dtype=torch.int32).cuda(), ci=torch.zeros(1, dtype=torch.int32).cuda(), n_out=0, n_in=7,
                              t_rp=torch.zeros(8, dtype=torch.int32).cuda(), t_ci=torch.zeros(1, dtype=torch.int32).cuda())
    Hs, Hd, att, G = [t.cuda() for t in vref.inputs(1, 7, heads, dim, 1)]
    got = _run(s, Hs, Hd[:0], att, G[:0], heads, dim, forward=(_nan(0, heads * dim), _nan(0, heads)))
    assert (got[4] == 0).all() and (got[2] == 0).all(), "d_att (and dHs) of a call without destination rows"

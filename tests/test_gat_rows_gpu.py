"""gnna_gat_forward_rows_f32 / gnna_gat_backward_rows_f32 through the C ABI against the fp64 restatement of tests/gat_rect_ref.py,
under the bound tests/test_gat_rect_gpu.py applies to the same five outputs (rtol 1e-5 of max(1, sum of |terms|), the kink rule),
and their reproducibility.  Every call pre-fills its outputs with NaN; out-of-range ids are planted in both structures; the
transposed structure is the device-built one."""
import functools
import types

import numpy as np
import pytest
import torch

import gat_rect_ref as gref
from gnnadvisor_osdi21_amd import _lib

pytestmark = pytest.mark.gpu
# (heads, dim): LPR lanes per row -> rows per wavefront R = 64 / LPR; a row is `long` above R * 128 edges
CONFIGS = [(1, 64), (4, 16), (3, 5), (1, 1), (8, 40)]      # R = 4, 4, 8, 64, 1 (two column blocks of four heads)
# every ownership limit of the kernels: a slot's own row up to 8 edges; the whole workgroup above 128 * R for R = 1, 4, 8, 64
LIMITS = (8, 128, 512, 1024, 8192)
LENGTHS = sorted({0, 1} | {t + d for t in LIMITS for d in (-1, 0, 1)})
LIMITS_N_IN = 200 + len(LENGTHS)


def limits_structure(seed=53):
    """A [(17 + 40) x 217] structure whose destination rows have every length of LENGTHS once (ids in the first 200 sources), then
    40 rows that give source 200 + k exactly LENGTHS[k] edges: every position plant_out_of_range will overwrite (position % 9 == 3)
    holds a filler id, so the in-degrees survive the planting.  -> (rp, ci) int32 numpy."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, 200, size=sum(LENGTHS))
    want = rng.permutation(np.repeat(200 + np.arange(len(LENGTHS)), LENGTHS))
    free = np.flatnonzero((len(top) + np.arange(len(want) * 9 // 8 + 9)) % 9 != 3)[:len(want)]
    low = np.zeros(free[-1] + 1, dtype=np.int64)
    low[free] = want
    cuts = np.linspace(0, len(low), 41).astype(np.int64)
    rp = np.concatenate([np.cumsum([0] + LENGTHS), len(top) + cuts[1:]])
    return rp.astype(np.int32), np.concatenate([top, low]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _structure(which):
    """The planted device structure and its device-built transpose."""
    (rp, ci), n_in = (gref.wide_short_structure(), 300) if which == "hub" else (limits_structure(), LIMITS_N_IN)
    ci = gref.plant_out_of_range(ci, n_in)
    s = types.SimpleNamespace(rp=torch.as_tensor(rp).cuda(), ci=torch.as_tensor(ci).cuda(), n_out=len(rp) - 1, n_in=n_in)
    s.t_rp, s.t_ci, _ = _lib.transpose_csr(s.rp, s.ci, num_in_rows=n_in, want_perm=False)
    if which == "limits":
        assert set(LENGTHS) <= set(np.diff(rp).tolist()) and set(LENGTHS) <= set(torch.diff(s.t_rp).tolist())
    return s


@functools.lru_cache(maxsize=None)
def _case(which, heads, dim):
    """(structure, inputs on the device, the fp64 reference): made once, shared and left unchanged."""
    s = _structure(which)
    ins = [t.cuda() for t in gref.inputs(s.n_out, s.n_in, heads, dim, heads + dim)]
    return s, ins, gref.kernel_reference(*ins, s.rp, s.ci, heads, 0.2, f"{which} {heads}x{dim}")


def _run(s, H, el, er, G, heads, dim):
    """Forward and backward through the C ABI into NaN-filled outputs -> (Y, lse, dH, d_el, d_er)."""
    W, lib, stream = heads * dim, _lib.load(), _lib._stream(H.device)
    Y, lse, dH, d_el, d_er = [torch.full(shape, float("nan"), device="cuda") for shape in
                              ((s.n_out, W), (s.n_out, heads), (s.n_in, W), (s.n_out, heads), (s.n_in, heads))]
    p = lambda t: t.data_ptr()
    assert lib.gnna_gat_forward_rows_f32(p(H), W, s.n_in, p(el), p(er), p(s.rp), p(s.ci), 0.2, p(Y), W, p(lse), s.n_out, heads, dim, 0,
                                         stream) == 0, lib.gnna_last_error()
    assert lib.gnna_gat_backward_rows_f32(p(H), W, s.n_in, p(el), p(er), p(lse), p(Y), W, p(G), W, p(s.rp), p(s.ci), p(s.t_rp),
                                          p(s.t_ci), 0.2, p(dH), W, p(d_el), p(d_er), s.n_out, heads, dim, 0, stream) == 0, lib.gnna_last_error()
    return Y, lse, dH, d_el, d_er


@pytest.mark.parametrize("heads,dim", CONFIGS)
@pytest.mark.parametrize("which", ["hub", "limits"])
def test_the_five_outputs_against_fp64(which, heads, dim):
    s, ins, r = _case(which, heads, dim)
    Y, lse, dH, d_el, d_er = got = _run(s, *ins, heads, dim)
    assert r.nnz < s.ci.numel() and int(s.t_rp[-1]) == r.nnz and bool((~r.has).any()) and bool((~r.reached).any())
    worst = {}
    for name, t, ref, scale, ok in (("Y", Y, r.Y, r.s_Y, None), ("lse", lse, r.lse, r.lse.abs(), r.has), ("dH", dH, r.dH, r.s_dH, None),
                                    ("d_el", d_el, r.d_el, r.s_el, r.ok_el), ("d_er", d_er, r.d_er, r.s_er, r.ok_er)):
        assert torch.isfinite(t).all(), f"{name} has elements the call did not write, or that are not finite"
        ratio = (t.double() - ref).abs() / (1e-5 * scale.clamp(min=1.0))
        worst[name] = float(ratio.max() if ok is None else ratio[ok].max())
    print(f"{which} {heads}x{dim}: worst error / bound", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (d_el[~r.has] == 0).all(), "rows without edges give 0"
    assert (dH[~r.reached] == 0).all() and (d_er[~r.reached] == 0).all(), "sources no edge reaches get exactly 0"


def test_two_runs_give_the_same_bits_and_deterministic_tuning_accepts_them():
    s, ins, _ = _case("hub", 4, 16)
    first, second = _run(s, *ins, 4, 16), _run(s, *ins, 4, 16)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    try:
        _lib.set_tuning(deterministic=1)
        third = _run(s, *ins, 4, 16)                          # (_run asserts that both entries answer success)
    finally:
        _lib.reset_tuning()
    assert all(torch.equal(a, b) for a, b in zip(first, third))

"""gnna_dot_attn_forward_rows_x16 / gnna_dot_attn_backward_rows_x16 (include/gnna_dot_rows_x16.h) through the C ABI against the fp64
restatement of tests/dotattn_ref.py on the 16-bit-ROUNDED inputs.  With B = 1e-5 * max(1, S) * max(1, sum of |terms|), the bound of
the fp32 kernels (tests/test_dot_rows_gpu.py), a 16-bit output is one rounding of an fp32 value within B of the reference: its bound
is B + u * (|ref| + B), u = 2^-8 (bf16) or 2^-11 (fp16); dQ and dK get u * sum of |terms| on top (c is made from the rounded Y:
|dc| <= u * crow, hence |d dz| <= u * adz); lse is fp32 and held to B alone.  No element is excluded.  Outputs are pre-filled with
NaN, out-of-range ids are planted in both structures, the transposed structure is the device-built one.  With 8 elements per lane
the configurations give R = 8, 4, 8, 64 and 1 rows per wavefront, so every limit of the "limits" structure (row lengths in {0, 1} u
{8, 128, 512, 1024, 8192} +- {0, 1}) is the wavefront limit of one of them; (8, 5) and (1, 1) move element by element, (12, 40) walks
two column blocks (8 + 4 heads)."""
import functools
import types

import pytest
import torch

import dotattn_ref as tref
from gnnadvisor_osdi21_amd import _lib
from test_dot_rows_gpu import NAMES, _structure

pytestmark = pytest.mark.gpu
CONFIGS = [(1, 64), (2, 64), (8, 5), (1, 1), (12, 40)]
TYPES = {torch.bfloat16: (_lib.BF16, 2.0 ** -8), torch.float16: (_lib.F16, 2.0 ** -11)}
both_types = pytest.mark.parametrize("dtype", list(TYPES), ids=["bf16", "fp16"])


@functools.lru_cache(maxsize=None)
def _case(which, heads, dim, dtype, p=0.0, seed=0):
    """(structure, 16-bit inputs on the device, the fp64 reference of those inputs): made once, shared and left unchanged."""
    s = _structure(which)
    ins = [t.cuda().to(dtype) for t in tref.inputs(s.n_out, s.n_in, heads, dim, heads + dim)]
    return s, ins, tref.kernel_reference(*ins, s.rp, s.ci, heads, 1 / dim ** 0.5, p, seed)


def _shifted(t, ld):
    """A copy of t as a view with row stride ld whose base is one element past an aligned address."""
    buf = torch.zeros(t.shape[0] * ld + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape[0], ld)[:, :t.shape[1]]
    view.copy_(t)
    return view


def _run(s, Q, K, V, G, heads, dim, p=0.0, seed=0, t=None, ld_out=None, flags=0, shift=False):
    """Forward and backward through the C ABI into NaN-filled outputs with rows of ld_out elements -> (Y, lse, dQ, dK, dV) as
    allocated.  t: the transposed structure (default: the device-built one of s); shift: the outputs start one element in."""
    W, lib, stream = heads * dim, _lib.load(), _lib._stream(Q.device)
    ld_out = ld_out or W
    t_rp, t_ci = t or (s.t_rp, s.t_ci)
    nan = lambda rows, ld, dtype: torch.full((rows * ld + 1,), float("nan"), dtype=dtype, device="cuda")[int(shift):][:rows * ld].view(rows, ld)
    Y, dQ, dK, dV = [nan(rows, ld_out, Q.dtype) for rows in (s.n_out, s.n_out, s.n_in, s.n_in)]
    lse = nan(s.n_out, heads, torch.float32)
    a = lambda x: x.data_ptr()
    qkv = (TYPES[Q.dtype][0], a(Q), Q.stride(0), a(K), K.stride(0), a(V), V.stride(0), s.n_in)
    scale = 1 / dim ** 0.5
    assert lib.gnna_dot_attn_forward_rows_x16(*qkv, a(s.rp), a(s.ci), scale, p, seed, a(Y), ld_out, a(lse), s.n_out, heads, dim, flags,
                                              stream) == 0, lib.gnna_last_error()
    assert lib.gnna_dot_attn_backward_rows_x16(*qkv, a(lse), a(Y), ld_out, a(G), G.stride(0), a(s.rp), a(s.ci), a(t_rp), a(t_ci), scale,
                                               p, seed, a(dQ), ld_out, a(dK), ld_out, a(dV), ld_out, s.n_out, heads, dim, 0,
                                               stream) == 0, lib.gnna_last_error()
    return Y, lse, dQ, dK, dV


def within_the_bound(what, got, r, dtype):
    u, worst = TYPES[dtype][1], {}
    for name, t, ref, scale in zip(NAMES, got, (r.Y, r.lse, r.dQ, r.dK, r.dV), (r.s_Y, r.lse.abs(), r.s_dQ, r.s_dK, r.s_dV)):
        assert torch.isfinite(t).all(), f"{name} has elements the call did not write, or that are not finite"
        bound = 1e-5 * r.factor * scale.clamp(min=1.0)
        if name != "lse":
            bound = bound + u * (ref.abs() + bound) + (u * scale if name in ("dQ", "dK") else 0.0)
        ratio = (t.double() - ref).abs() / bound
        worst[name] = float(ratio[r.has].max() if name == "lse" else ratio.max())
    print(f"{what}: worst error / bound", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@both_types
@pytest.mark.parametrize("heads,dim", CONFIGS)
@pytest.mark.parametrize("which", ["hub", "limits"])
def test_the_five_outputs_against_fp64(which, heads, dim, dtype):
    s, ins, r = _case(which, heads, dim, dtype)
    Y, lse, dQ, dK, dV = got = _run(s, *ins, heads, dim)
    assert r.nnz < s.ci.numel() and int(s.t_rp[-1]) == r.nnz and bool((~r.has).any()) and bool((~r.reached).any())
    within_the_bound(f"{which} {heads}x{dim} {dtype}", got, r, dtype)
    assert (Y[~r.has] == 0).all() and (lse[~r.has] == 0).all() and (dQ[~r.has] == 0).all(), "rows without edges give 0"
    assert (dK[~r.reached] == 0).all() and (dV[~r.reached] == 0).all(), "sources no edge reaches get exactly 0"


@pytest.mark.parametrize("heads,dim", [(2, 64), (8, 5)])
@pytest.mark.parametrize("which", ["hub", "limits"])
def test_the_mask_is_the_fused_paths_and_leaves_lse_alone(which, heads, dim):
    seed = 2 ** 63 + 11
    s, ins, r = _case(which, heads, dim, torch.bfloat16, 0.5, seed)
    got = _run(s, *ins, heads, dim, 0.5, seed)
    assert r.k is not None and bool((r.k == 0).any()) and bool((r.k == 2).any())
    within_the_bound(f"{which} {heads}x{dim} attn_drop=0.5", got, r, torch.bfloat16)
    assert torch.equal(got[1], _run(s, *ins, heads, dim)[1]), "lse is that of the un-dropped scores"


@both_types
def test_two_runs_give_the_same_bits_and_deterministic_tuning_accepts_them(dtype):
    s, ins, _ = _case("hub", 2, 64, dtype)
    first, second = _run(s, *ins, 2, 64, 0.5, 7), _run(s, *ins, 2, 64, 0.5, 7)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    try:
        _lib.set_tuning(deterministic=1)
        third = _run(s, *ins, 2, 64, 0.5, 7)                  # (_run asserts that both entries answer success)
    finally:
        _lib.reset_tuning()
    assert all(torch.equal(a, b) for a, b in zip(first, third))


@both_types
@pytest.mark.parametrize("which", ["hub", "limits"])
def test_the_vector_path_and_the_element_path_give_the_same_bits(which, dtype):
    """The same (2, 64) inputs aligned (16-byte pieces) and as views one element past alignment with an odd row stride."""
    s, ins, _ = _case(which, 2, 64, dtype)
    assert all(t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 for t in ins)
    aligned = _run(s, *ins, 2, 64)
    moved = [_shifted(t, 129) for t in ins]
    assert all(t.data_ptr() % 4 == 2 and torch.equal(t, u) for t, u in zip(moved, ins))
    shifted = _run(s, *moved, 2, 64, ld_out=129, shift=True)
    for name, a, b in zip(NAMES, aligned, shifted):
        assert torch.equal(a, b if name == "lse" else b[:, :128]), name


@pytest.mark.parametrize("heads,dim,pad", [(3, 5, 5), (4, 16, 0)])
def test_slices_of_one_matrix_a_symmetric_structure_and_the_relu_epilogue(heads, dim, pad):
    """Q | K | V are column slices of one 16-bit [N, 3 W + pad] matrix (W = 15: unaligned slices; W = 64: aligned ones), the
    structure is passed as its own transpose, the forward clamps."""
    n, W, dtype = 120, heads * dim, torch.bfloat16
    gen = torch.Generator().manual_seed(3)
    pairs = torch.randint(0, n, (2, 900), generator=gen)
    dense = torch.zeros(n, n, dtype=torch.bool)
    dense[pairs[0], pairs[1]] = dense[pairs[1], pairs[0]] = True
    dense[5] = dense[:, 5] = False                            # a row and a source without edges
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), dense.sum(1).cumsum(0)]).int().cuda()
    ci = dense.nonzero()[:, 1].int().cuda()
    s = types.SimpleNamespace(rp=rp, ci=ci, n_out=n, n_in=n)
    P = torch.randn(n, 3 * W + pad, generator=gen).cuda().to(dtype)
    G = torch.randn(n, W + 3, generator=gen).cuda().to(dtype)[:, :W]
    Q, K, V = P[:, :W], P[:, W:2 * W], P[:, 2 * W:3 * W]
    plain = _run(s, Q, K, V, G, heads, dim, t=(rp, ci), ld_out=W + 3)
    clamped = _run(s, Q, K, V, G, heads, dim, t=(rp, ci), ld_out=W + 3, flags=2)      # (its backward reads the clamped Y: not compared)
    for got in (plain, clamped):
        assert all(torch.isnan(t[:, W:]).all() for t in (got[0], *got[2:])), "the padding columns are never touched"
    assert torch.equal(clamped[0][:, :W], plain[0][:, :W].clamp(min=0)) and bool((plain[0][:, :W] < 0).any())
    assert torch.equal(clamped[1], plain[1])
    r = tref.kernel_reference(Q, K, V, G, rp, ci, heads, 1 / dim ** 0.5)
    within_the_bound(f"slices W={W}", [t if t is plain[1] else t[:, :W] for t in plain], r, dtype)
    assert (plain[0][5, :W] == 0).all() and (plain[3][5, :W] == 0).all()

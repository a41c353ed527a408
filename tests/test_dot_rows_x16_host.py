"""The 16-bit rows form of the fused dot-product attention (include/gnna_dot_rows_x16.h), the parts that need no GPU: the refusals
both entries make before any device work -- those of gnna_dot_rows.h under the new names, and a bad `type` -- and that
gnna_tuning.deterministic = 1 is not one of them.  (The binding surface and the build lists are pinned by
test_binding_table_host.py.)"""
import ctypes

import pytest

from gnnadvisor_osdi21_amd import _lib

_B = [(ctypes.c_uint16 * 64)() for _ in range(10)]
_I = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]      # Q, K, V, out | Y, lse, dY, dQ, dK, dV
I = ctypes.cast(_I, ctypes.c_void_p).value
FWD, BWD = "gnna_dot_attn_forward_rows_x16", "gnna_dot_attn_backward_rows_x16"


def _forward(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(type=_lib.BF16, q=F[0], k=F[1], v=F[2], out=F[3], lse=F[4], rp=I, ld_q=8, ld_k=8, ld_v=8, ld_out=8, n_out=2, n_in=2, heads=2,
             dim=4, flags=0, scale=0.5, attn_drop=0.0)
    a.update(kw)
    return getattr(_lib.load(), FWD)(a["type"], a["q"], a["ld_q"], a["k"], a["ld_k"], a["v"], a["ld_v"], a["n_in"], a["rp"], I, a["scale"],
                                     a["attn_drop"], 0, a["out"], a["ld_out"], a["lse"], a["n_out"], a["heads"], a["dim"], a["flags"], None)


def _backward(**kw):
    a = dict(type=_lib.F16, q=F[0], k=F[1], v=F[2], y=F[3], lse=F[4], dy=F[5], dq=F[6], dk=F[7], dv=F[8], rp=I, t_rp=I, ld_q=8, ld_k=8,
             ld_v=8, ld_y=8, ld_dy=8, ld_dq=8, ld_dk=8, ld_dv=8, n_out=2, n_in=2, heads=2, dim=4, flags=0, scale=0.5, attn_drop=0.0)
    a.update(kw)
    return getattr(_lib.load(), BWD)(a["type"], a["q"], a["ld_q"], a["k"], a["ld_k"], a["v"], a["ld_v"], a["n_in"], a["lse"], a["y"],
                                     a["ld_y"], a["dy"], a["ld_dy"], a["rp"], I, a["t_rp"], I, a["scale"], a["attn_drop"], 0, a["dq"],
                                     a["ld_dq"], a["dk"], a["ld_dk"], a["dv"], a["ld_dv"], a["n_out"], a["heads"], a["dim"], a["flags"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


@pytest.mark.parametrize("call, name", [(_forward, FWD), (_backward, BWD)])
def test_refusals_both_entries_make_before_any_device_work(call, name):
    for bad in (_lib.F32, 3, -1):
        assert call(type=bad) == -1 and _last() == f"{name}: type must be GNNA_BF16 or GNNA_F16 (got {bad})"
    assert call(heads=65) == -3 and _last() == f"{name}: at most 64 heads (got 65)"
    assert call(dim=257) == -3 and _last() == f"{name}: at most 256 floats per head (got 257)"
    assert call(flags=1) == -3 and _last() == f"{name}: GNNA_ACCUMULATE is not supported"
    assert call(flags=8) == -1 and _last() == f"{name}: unknown flag bits 0x8"
    assert call(heads=0) == -1 and _last() == f"{name}: bad size (num_out_rows=2 num_in_rows=2 heads=0 dim=4)"
    assert call(n_out=1 << 29) == -3 and _last() == f"{name}: 536870912 rows in one call (at most 536870911): shard the rows"
    for attn_drop, shown in ((1.0, "1"), (-0.5, "-0.5"), (float("nan"), "nan")):
        assert call(attn_drop=attn_drop) == -1 and _last() == f"{name}: attn_drop must be in [0, 1) (got {shown})"
    for scale, shown in ((float("inf"), "inf"), (float("nan"), "nan")):
        assert call(scale=scale) == -1 and _last() == f"{name}: scale must be finite (got {shown})"
    for ld in ("ld_q", "ld_k", "ld_v"):
        assert call(**{ld: 7}) == -1 and f"{ld}=7" in _last(), ld
        assert call(**{ld: 1 << 29}) == -1 and "row strides must be >= heads * dim and < 2^29" in _last(), ld
    for kw in (dict(q=None), dict(k=None), dict(v=None)):
        assert call(**kw) == -1 and _last() == f"{name}: null pointer", kw


def test_refusals_of_the_forward():
    assert _forward(flags=4) == -1 and _last() == f"{FWD}: unknown flag bits 0x4"
    assert _forward(ld_out=7) == -1 and "ld_out=7" in _last()
    for kw in (dict(out=None), dict(lse=None), dict(rp=None)):
        assert _forward(**kw) == -1 and _last() == f"{FWD}: null pointer", kw
    for kw in (dict(out=F[0]), dict(out=F[1]), dict(out=F[2]), dict(out=F[4]), dict(lse=F[0]), dict(lse=F[1]), dict(lse=F[2])):
        assert _forward(**kw) == -1 and _last() == f"{FWD}: an output must not alias an input or the other output", kw


def test_refusals_of_the_backward():
    assert _backward(flags=2) == -1 and _last() == f"{BWD}: unknown flag bits 0x2"              # the ReLU epilogue: forward only
    for ld in ("ld_y", "ld_dy", "ld_dq", "ld_dk", "ld_dv"):
        assert _backward(**{ld: 7}) == -1 and f"{ld}=7" in _last(), ld
    for kw in (dict(lse=None), dict(y=None), dict(dy=None)):
        assert _backward(**kw) == -1 and _last() == f"{BWD}: null pointer", kw
    for kw in (dict(rp=None), dict(t_rp=None)):
        assert _backward(**kw) == -1 and _last().startswith(f"{BWD}: null index pointer"), kw
    for out in ("dq", "dk", "dv"):
        for inp in range(6):                                                                   # Q, K, V, Y, lse, dY
            assert _backward(**{out: F[inp]}) == -1 and _last() == f"{BWD}: an output must not alias an input", (out, inp)
    for kw in (dict(dq=F[7]), dict(dq=F[8]), dict(dk=F[8])):
        assert _backward(**kw) == -1 and _last() == f"{BWD}: the outputs must not alias each other", kw


def test_deterministic_tuning_does_not_refuse():
    """Calls with nothing to write return before any device work, and answer success under deterministic = 1 (gnna_agg_ld_x16, the
    other 16-bit kernel, refuses there: it adds with float atomics)."""
    try:
        _lib.set_tuning(deterministic=1)
        assert _forward(n_out=0, out=None, lse=None) == 0
        assert _backward(dq=None, dk=None, dv=None) == 0
        assert _forward(heads=65) == -3 and "deterministic" not in _last()                     # (the other checks still run)
    finally:
        _lib.reset_tuning()

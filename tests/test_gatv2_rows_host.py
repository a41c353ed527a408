"""The rows form of the fused GATv2 attention (include/gnna_gatv2_rows.h), the part that needs no GPU: the refusals both entries make
before any device work, each with the entry's name in gnna_last_error.  (The binding surface and the build lists are pinned by
test_binding_table_host.py.)"""
import ctypes

import pytest

from gnnadvisor_osdi21_amd import _lib

_B = [(ctypes.c_float * 64)() for _ in range(10)]
_I = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]      # Hs, Hd, att, out | Y, lse, dY, dHs, dHd, d_att
I = ctypes.cast(_I, ctypes.c_void_p).value
DEFAULTS = dict(hs=F[0], hd=F[1], att=F[2], out=F[3], y=F[3], lse=F[4], dy=F[5], dhs=F[6], dhd=F[7], datt=F[8], rp=I, t_rp=I, ld_hs=8,
                ld_hd=8, ld_out=8, ld_y=8, ld_dy=8, ld_dhs=8, ld_dhd=8, n_out=2, n_in=2, heads=2, dim=4, flags=0, slope=0.2,
                attn_drop=0.0)


def _forward(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(DEFAULTS, **kw)
    return _lib.load().gnna_gatv2_forward_rows_f32(a["hs"], a["ld_hs"], a["hd"], a["ld_hd"], a["att"], a["n_in"], a["rp"], I, a["slope"],
                                                   a["attn_drop"], 0, a["out"], a["ld_out"], a["lse"], a["n_out"], a["heads"], a["dim"],
                                                   a["flags"], None)


def _backward(**kw):
    a = dict(DEFAULTS, **kw)
    return _lib.load().gnna_gatv2_backward_rows_f32(a["hs"], a["ld_hs"], a["hd"], a["ld_hd"], a["att"], a["n_in"], a["lse"], a["y"],
                                                    a["ld_y"], a["dy"], a["ld_dy"], a["rp"], I, a["t_rp"], I, a["slope"], a["attn_drop"],
                                                    0, a["dhs"], a["ld_dhs"], a["dhd"], a["ld_dhd"], a["datt"], a["n_out"], a["heads"],
                                                    a["dim"], a["flags"], None)


BOTH = [(_forward, "gnna_gatv2_forward_rows_f32"), (_backward, "gnna_gatv2_backward_rows_f32")]
FWD, BWD = BOTH[:1], BOTH[1:]
REFUSALS = [   # (entries, arguments, status, what gnna_last_error says after the entry's name)
    (BOTH, dict(flags=1), -3, "GNNA_ACCUMULATE is not supported"),
    (BOTH, dict(flags=8), -1, "unknown flag bits 0x8"),
    (BWD, dict(flags=2), -1, "unknown flag bits 0x2"),                                  # the ReLU epilogue: forward only
    (BOTH, dict(heads=0), -1, "bad size (num_out_rows=2 num_in_rows=2 heads=0 dim=4)"),
    (BOTH, dict(heads=65), -3, "at most 64 heads (got 65)"),
    (BOTH, dict(dim=257), -3, "at most 256 floats per head (got 257)"),
    (BOTH, dict(n_out=1 << 29), -3, "536870912 rows in one call (at most 536870911): shard the rows"),
    (BOTH, dict(attn_drop=1.0), -1, "attn_drop must be in [0, 1) (got 1)"),
    (BOTH, dict(attn_drop=-0.5), -1, "attn_drop must be in [0, 1) (got -0.5)"),
    (BOTH, dict(attn_drop=float("nan")), -1, "attn_drop must be in [0, 1) (got nan)"),
    (BOTH, dict(slope=float("inf")), -1, "negative_slope must be finite (got inf)"),
    (BOTH, dict(slope=float("nan")), -1, "negative_slope must be finite (got nan)"),
    (BOTH, dict(ld_hs=7), -1, "ld_hs=7"),
    (BOTH, dict(ld_hd=7), -1, "ld_hd=7"),
    (FWD, dict(ld_out=7), -1, "ld_out=7"),
    (BWD, dict(ld_dy=7), -1, "ld_dy=7"),
    (BWD, dict(ld_dhs=7), -1, "ld_dhs=7"),
    (BOTH, dict(hs=None), -1, "null pointer"),
    (BOTH, dict(att=None), -1, "null pointer"),
    (FWD, dict(lse=None), -1, "null pointer"),
    (FWD, dict(rp=None), -1, "null pointer"),
    (BWD, dict(dy=None), -1, "null pointer"),
    (BWD, dict(rp=None), -1, "null index pointer"),
    (BWD, dict(t_rp=None), -1, "null index pointer"),
    (FWD, dict(out=F[2]), -1, "an output must not alias an input or the other output"),
    (FWD, dict(lse=F[0]), -1, "an output must not alias an input or the other output"),
    (BWD, dict(datt=F[2]), -1, "an output must not alias an input"),
    (BWD, dict(dhs=F[0]), -1, "an output must not alias an input"),
    (BWD, dict(dhd=F[6]), -1, "the outputs must not alias each other"),
]


@pytest.mark.parametrize("entries, kw, status, says", REFUSALS, ids=[f"{'+'.join(n[11:14] for _, n in e)}-{k}" for e, k, _, _ in REFUSALS])
def test_refusals_before_any_device_work(entries, kw, status, says):
    for call, name in entries:
        assert call(**kw) == status
        last = _lib.load().gnna_last_error().decode()
        assert last.startswith(f"{name}: ") and says in last, last

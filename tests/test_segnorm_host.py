"""Per-graph normalisation (include/gnna_segnorm.h), the part that needs no GPU: every argument check answers through
gnna_last_error before any device work; the fp32 restatement of the moments pass (segnorm_ref.py) stays inside the accuracy contract
of the header, which a sum of x^2 does not; and the driver's flags.  The header's entries, table and signatures are checked with
every other header's in test_binding_table_host.py."""
import ctypes
import os

import numpy as np
import pytest

import segnorm_ref
from gnnadvisor_osdi21_amd import _lib, graph_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")
HEADER = "gnna_segnorm.h"


def test_the_header_is_extern_c_and_the_module_includes_it():
    assert 'extern "C"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "gnna_segnorm.h"' in open(os.path.join(CSRC, "gnna_torch.cpp")).read()


# ---- the argument checks: host buffers stand in for device memory, every call returns before it touches the device ----

_B = [(ctypes.c_float * 64)() for _ in range(10)]
_I = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = ctypes.cast(_I, ctypes.c_void_p).value
INVALID, UNSUPPORTED = -1, -3


def _moments(**kw):
    a = dict(x=F[0], ld_in=4, n=8, gp=I, G=2, mean=F[1], ld_mean=4, m2=F[2], ld_m2=4, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_moments_ld_f32(a["x"], a["ld_in"], a["n"], a["gp"], a["G"], a["mean"], a["ld_mean"], a["m2"],
                                                   a["ld_m2"], a["dim"], a["flags"], None)


def _norm(**kw):
    a = dict(x=F[0], ld_in=4, n=8, gp=I, G=2, w=F[3], b=F[4], al=F[5], eps=1e-5, out=F[6], ld_out=4, mean=F[1], ld_mean=4, rstd=F[2],
             ld_rstd=4, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_norm_ld_f32(a["x"], a["ld_in"], a["n"], a["gp"], a["G"], a["w"], a["b"], a["al"], a["eps"], a["out"],
                                                a["ld_out"], a["mean"], a["ld_mean"], a["rstd"], a["ld_rstd"], a["dim"], a["flags"], None)


def _backward(**kw):
    a = dict(dy=F[7], ld_do=4, x=F[0], ld_in=4, mean=F[1], ld_mean=4, rstd=F[2], ld_rstd=4, w=F[3], al=F[5], gp=I, G=2, dx=F[6], ld_din=4,
             A=F[8], ld_a=4, B=F[9], ld_b=4, n=8, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_norm_backward_ld_f32(a["dy"], a["ld_do"], a["x"], a["ld_in"], a["mean"], a["ld_mean"], a["rstd"],
                                                         a["ld_rstd"], a["w"], a["al"], a["gp"], a["G"], a["dx"], a["ld_din"], a["A"],
                                                         a["ld_a"], a["B"], a["ld_b"], a["n"], a["dim"], a["flags"], None)


ENTRIES = {"gnna_segment_moments_ld_f32": _moments, "gnna_segment_norm_ld_f32": _norm, "gnna_segment_norm_backward_ld_f32": _backward}
COMMON = [
    (dict(flags=1), INVALID, "{e}: unknown flag bits 0x1 (the entry has no flags)"),
    (dict(dim=0), INVALID, "{e}: dim must be >= 1 (got 0)"),
    (dict(n=-1), INVALID, "{e}: negative size (num_rows=-1 num_segments=2)"),
    (dict(G=-3), INVALID, "{e}: negative size (num_rows=8 num_segments=-3)"),
    (dict(G=1 << 29), UNSUPPORTED, "{e}: 536870912 segments in one call (at most 536870911): shard the batch"),
    (dict(n=1 << 31), UNSUPPORTED, "{e}: 2147483648 rows in one call (at most 2147483647: graph_pointers is int32)"),
    (dict(gp=None), INVALID, "{e}: null graph_pointers"),
]
SPECIFIC = [
    (_moments, dict(ld_in=3), INVALID,
     "gnna_segment_moments_ld_f32: row strides must be >= dim and < 2^29 elements (ld_in=3 ld_mean=4 ld_m2=4 dim=4)"),
    (_moments, dict(ld_m2=1 << 29), INVALID,
     "gnna_segment_moments_ld_f32: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_mean=4 ld_m2=536870912 dim=4)"),
    (_moments, dict(x=F[0] + 2), INVALID, "gnna_segment_moments_ld_f32: feature, pointer and statistic pointers must be 4-byte aligned"),
    (_moments, dict(mean=F[0]), INVALID, "gnna_segment_moments_ld_f32: an output must not alias an input"),
    (_moments, dict(m2=F[1]), INVALID, "gnna_segment_moments_ld_f32: the outputs must not alias each other"),
    (_moments, dict(m2=None), INVALID, "gnna_segment_moments_ld_f32: null output pointer (mean and m2 are both written)"),
    (_moments, dict(x=None), INVALID, "gnna_segment_moments_ld_f32: null feature pointer"),
    (_norm, dict(eps=0.0), INVALID, "gnna_segment_norm_ld_f32: eps must be finite and > 0 (got 0)"),
    (_norm, dict(eps=-1e-5), INVALID, "gnna_segment_norm_ld_f32: eps must be finite and > 0 (got -1e-05)"),
    (_norm, dict(eps=float("inf")), INVALID, "gnna_segment_norm_ld_f32: eps must be finite and > 0 (got inf)"),
    (_norm, dict(eps=float("nan")), INVALID, "gnna_segment_norm_ld_f32: eps must be finite and > 0 (got nan)"),
    (_norm, dict(ld_out=2), INVALID,
     "gnna_segment_norm_ld_f32: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_out=2 ld_mean=4 ld_rstd=4 dim=4)"),
    (_norm, dict(out=F[6] + 1), INVALID, "gnna_segment_norm_ld_f32: feature, pointer, parameter and output pointers must be 4-byte aligned"),
    (_norm, dict(out=F[0]), INVALID, "gnna_segment_norm_ld_f32: an output must not alias an input"),
    (_norm, dict(rstd=F[3]), INVALID, "gnna_segment_norm_ld_f32: an output must not alias an input"),
    (_norm, dict(rstd=F[1]), INVALID, "gnna_segment_norm_ld_f32: the outputs must not alias each other"),
    (_norm, dict(rstd=None), INVALID, "gnna_segment_norm_ld_f32: null statistic pointer (mean and rstd are both written)"),
    (_norm, dict(x=None), INVALID, "gnna_segment_norm_ld_f32: null feature pointer"),
    (_norm, dict(out=None), INVALID, "gnna_segment_norm_ld_f32: null output pointer"),
    (_backward, dict(ld_b=3), INVALID,
     "gnna_segment_norm_backward_ld_f32: row strides must be >= dim and < 2^29 elements (ld_do=4 ld_in=4 ld_mean=4 ld_rstd=4 ld_din=4 "
     "ld_a=4 ld_b=3 dim=4)"),
    (_backward, dict(ld_din=3), INVALID,
     "gnna_segment_norm_backward_ld_f32: row strides must be >= dim and < 2^29 elements (ld_do=4 ld_in=4 ld_mean=4 ld_rstd=4 ld_din=3 "
     "ld_a=4 ld_b=4 dim=4)"),
    (_backward, dict(dy=F[7] + 2), INVALID,
     "gnna_segment_norm_backward_ld_f32: gradient, feature, statistic, parameter and pointer pointers must be 4-byte aligned"),
    (_backward, dict(dx=F[7]), INVALID, "gnna_segment_norm_backward_ld_f32: an output must not alias an input"),
    (_backward, dict(B=F[8]), INVALID, "gnna_segment_norm_backward_ld_f32: the outputs must not alias each other"),
    (_backward, dict(A=None), INVALID, "gnna_segment_norm_backward_ld_f32: null output pointer (seg_a and seg_b are always written)"),
    (_backward, dict(mean=None), INVALID, "gnna_segment_norm_backward_ld_f32: null statistic pointer"),
    (_backward, dict(dy=None), INVALID, "gnna_segment_norm_backward_ld_f32: null feature or gradient pointer"),
]


def _last_error():
    return _lib.load().gnna_last_error().decode()


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("change, code, message", COMMON, ids=[",".join(c) for c, _, _ in COMMON])
def test_what_the_three_entries_refuse_alike(entry, change, code, message):
    assert ENTRIES[entry](**change) == code
    assert _last_error() == message.format(e=entry)


@pytest.mark.parametrize("call, change, code, message", SPECIFIC, ids=[f"{c.__name__}-{','.join(ch)}-{k}" for k, (c, ch, _, _) in enumerate(SPECIFIC)])
def test_what_each_entry_refuses(call, change, code, message):
    assert call(**change) == code
    assert _last_error() == message


def test_a_null_d_input_leaves_its_stride_with_the_upper_bound_only():
    assert _backward(dx=None, ld_din=0, gp=None) == INVALID and "null graph_pointers" in _last_error()     # (the stride check passed)
    assert _backward(dx=None, ld_din=1 << 29) == INVALID and "row strides" in _last_error()


def test_calls_without_work_return_at_once():
    assert _moments(G=0, gp=None) == 0
    assert _norm(G=0, n=0, gp=None, x=None, out=None) == 0
    assert _backward(G=0, n=0, gp=None) == 0 and _backward(G=0, gp=None, dx=None) == 0


# ---- the accuracy contract, on the restatement ----

SHAPES = [(1, 0, 4), (2, 255, 7), (3, 0, 1), (63, 10, 64), (64, 200, 64), (65, 0, 3), (255, 1, 41), (256, 0, 64), (257, 255, 100),
          (600, 100, 64), (5000, 17, 8)]
OFFSETS = [(0.0, 1.0), (1000.0, 0.1), (-3e4, 0.1)]


def offset_rows(rows, width, offset, spread, seed):
    g = np.random.default_rng(seed)
    return (offset + spread * g.standard_normal((rows, width))).astype(np.float32)


@pytest.mark.parametrize("offset, spread", OFFSETS)
def test_the_restatement_stays_inside_the_contract(offset, spread):
    worst_mean = worst_var = 0.0
    for seed, (rows, start, width) in enumerate(SHAPES):
        x = offset_rows(rows, width, offset, spread, seed)
        mean, m2 = segnorm_ref.moments_f32(x, start)
        assert mean.dtype == m2.dtype == np.float32 and (m2 >= 0).all()
        mean64, var64 = segnorm_ref.moments_f64(x)
        bound_mean, bound_var = segnorm_ref.statistics_bounds(x)
        err_mean, err_var = np.abs(mean - mean64), np.abs(m2.astype(np.float64) / rows - var64)
        assert (err_mean <= bound_mean).all() and (err_var <= bound_var).all(), (rows, start, width)
        if rows > 1:
            worst_mean, worst_var = max(worst_mean, (err_mean / bound_mean).max()), max(worst_var, (err_var / bound_var).max())
        else:
            assert (m2 == 0).all() and (mean == x[0]).all()
    print(f"offset {offset}: worst |mean - mean64| / bound {worst_mean:.3f}, worst |var - var64| / bound {worst_var:.3f}")


def test_the_restatement_takes_the_workgroup_join_for_a_long_segment():
    rows = segnorm_ref.long_segment_rows(64)
    assert rows == 16 * 4 * 256 + 300 and (rows + 255) // 256 > 4 * segnorm_ref.LONG_STEPS
    x = offset_rows(rows, 8, 1000.0, 0.1, 5)[:, :8]
    # (at width 8 the same rows are 66 tiles over 32 slots: the wavefront's join; at width 64 the workgroup's -- both inside)
    for cols in (x, np.tile(x, (1, 8))):
        mean, m2 = segnorm_ref.moments_f32(cols, 0)
        mean64, var64 = segnorm_ref.moments_f64(cols)
        bound_mean, bound_var = segnorm_ref.statistics_bounds(cols)
        assert (np.abs(mean - mean64) <= bound_mean).all() and (np.abs(m2.astype(np.float64) / rows - var64) <= bound_var).all()


@pytest.mark.parametrize("offset", [1000.0, -3e4])
def test_a_sum_of_squares_misses_the_contract_on_offset_data(offset):
    x = offset_rows(600, 64, offset, 0.1, 9)
    _, var64 = segnorm_ref.moments_f64(x)
    _, bound_var = segnorm_ref.statistics_bounds(x)
    naive = np.abs(segnorm_ref.naive_var_f32(x).astype(np.float64) - var64)
    assert (naive > bound_var).mean() > 0.9 and np.median(naive / var64) > 0.5


def test_the_fp64_reference_is_the_plain_formula():
    g = np.random.default_rng(2)
    x, gp = g.standard_normal((12, 3)) + 2.0, [2, 7, 7, 8, 11]
    w, b, a = g.standard_normal(3), g.standard_normal(3), np.array([1.0, 0.0, 0.37])
    ref = segnorm_ref.graph_norm_f64(x, gp, w, b, a, 1e-5, g.standard_normal((12, 3)))
    assert (ref["out"][:2] == 0).all() and (ref["out"][11:] == 0).all() and (ref["d_input"][:2] == 0).all()
    assert (ref["mean"][1] == 0).all() and (ref["rstd"][1] == 0).all()                           # the empty segment
    seg = x[2:7]
    xc = seg - a * seg.mean(0)
    assert np.allclose(ref["out"][2:7], w * xc / np.sqrt((xc * xc).mean(0) + 1e-5) + b, rtol=1e-12)
    # the one-row segment: with alpha = 1 the variance is 0, rstd = 1 / sqrt(eps) and out = bias
    assert np.isclose(ref["rstd"][2][0], 1 / np.sqrt(1e-5)) and np.isclose(ref["out"][7][0], b[0])
    assert np.allclose(ref["seg_a"].sum(0), ref["d_bias"]) and np.allclose(ref["seg_b"].sum(0), ref["d_weight"])
    m, r = ref["mean"], ref["rstd"]
    assert np.allclose(-(m * w * r * (ref["seg_a"] - (1 - a) * m * r * ref["seg_b"])).sum(0), ref["d_alpha"])


# ---- the driver ----

def test_the_driver_takes_norm_and_fused_norm():
    args = graph_main.build_parser().parse_args([])
    assert args.norm == "none" and args.fused_norm is True
    args = graph_main.build_parser().parse_args(["--norm", "graph", "--fused_norm", "False"])
    assert args.norm == "graph" and args.fused_norm is False
    graph_main._parse(args)


def test_the_driver_refuses_an_unknown_norm_and_keeps_the_dtype_message():
    with pytest.raises(SystemExit, match=r"--norm takes none or graph \(got 'batch'\)"):
        graph_main._parse(graph_main.build_parser().parse_args(["--norm", "batch"]))
    with pytest.raises(SystemExit):
        graph_main.build_parser().parse_args(["--fused_norm", "yes"])
    with pytest.raises(SystemExit, match=r"--dtype float16: the readout \(sum / mean / max / min over the rows of a graph\) is float32 only; "
                                         r"run graph_main with --dtype float32"):
        graph_main._parse(graph_main.build_parser().parse_args(["--norm", "graph", "--dtype", "float16"]))

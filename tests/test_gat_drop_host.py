"""Attention dropout of the fused GAT attention, the parts that need no GPU (the binding surface of include/gnna_ext.h is pinned
by test_binding_table_host.py): the drop entries are the rect ones with two more arguments, the text of the mask rule, the
restated mask (tests/gat_drop_ref.py), the refusals the entries make before any device work, the driver's flag and the layer's
argument."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gat_drop_ref as dref
from gnnadvisor_osdi21_amd import _lib
from test_binding_table_host import _codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gnna_ext.h")).read()


def test_the_drop_entries_are_the_rect_entries_with_two_more_arguments():
    for drop, rect in (("gnna_gat_forward_drop_f32", "gnna_gat_forward_rect_f32"), ("gnna_gat_backward_drop_f32", "gnna_gat_backward_rect_f32")):
        assert _codes(*_lib.HEADERS["gnna_ext.h"][drop])[1].replace("ffQ", "f", 1) == _codes(*_lib.HEADERS["gnna.h"][rect])[1]


def test_the_header_states_the_rule():
    flat = re.sub(r"[\s*]+", " ", _header())
    for piece in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "u = (i << 35) | (j << 6) | h",
                  "thr = (uint32) floor((double)attn_drop 2^32)", "kept(i, j, h) = (key >> 32) >= thr",
                  "k = kept ? 1.0f / (1.0f - attn_drop) : 0", "dz = alpha (k dalpha - c) (z > 0 ? 1 : slope)",
                  "duplicate edges (i, j) are kept or dropped together", "GNNA_ERR_INVALID_ARGUMENT before any device work"):
        assert piece in flat, piece


def test_one_key_function_in_the_shared_device_header():
    csrc = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")
    defs = {f: len(re.findall(r"uint64_t\s+key_of_position\s*\(", open(os.path.join(csrc, f)).read())) for f in os.listdir(csrc)
            if f.endswith((".hip", ".h", ".cpp"))}
    assert {f: n for f, n in defs.items() if n} == {"gnna_device.h": 1}
    for f in ("gnna_sample.hip", "gnna_gat.hip"):
        assert "key_of_position(" in open(os.path.join(csrc, f)).read()


def test_the_restated_mask():
    rng = np.random.default_rng(3)
    rows, ids = rng.integers(0, 1 << 29, 4000), rng.integers(0, 1 << 29, 4000)
    assert dref.keep_mask(0x1234, rows, ids, 64, 0.0).all() and dref.threshold(0.0) == 0 and dref.keep_scale(0.0) == 1.0
    # thr comes from the float32 value of p: 0.6f = 0.60000002384185791015625
    assert dref.threshold(0.6) == int(np.floor(0.60000002384185791015625 * 2 ** 32)) == 2576980480
    assert dref.threshold(0.6) != int(np.floor(0.6 * 2 ** 32))
    assert dref.threshold(0.5) == 1 << 31 and dref.keep_scale(0.5) == 2.0
    assert dref.threshold(np.nextafter(np.float32(1), np.float32(0))) == 2 ** 32 - 256
    # a function of (seed, i, j, h): one known key by hand (u = (1 << 35) | (2 << 6) | 3, seed 5), duplicates agree, heads differ
    z = (5 + 0x9E3779B97F4A7C15 * (((1 << 35) | (2 << 6) | 3) + 1)) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    key = z ^ (z >> 31)
    for p in (0.1, 0.5, 0.9):
        assert bool(dref.keep_mask(5, [1], [2], 4, p)[0, 3]) == ((key >> 32) >= dref.threshold(p))
    m = dref.keep_mask(9, [7, 7, 8], [3, 3, 3], 8, 0.5)
    assert (m[0] == m[1]).all() and (m[0] != m[2]).any()
    share = dref.keep_mask(1, rows, ids, 8, 0.6).mean()
    assert abs(share - 0.4) < 5 * np.sqrt(0.24 / 32000)         # 5 sigma of 32,000 draws


_B = [(ctypes.c_float * 64)() for _ in range(9)]
_I = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = ctypes.cast(_I, ctypes.c_void_p).value


def _forward(attn_drop, **kw):
    a = dict(heads=2, flags=0)
    a.update(kw)
    return _lib.load().gnna_gat_forward_drop_f32(F[0], 8, F[1], F[2], I, I, I, I, 0.2, attn_drop, 7, F[3], 8, F[4], 2, 2, a["heads"], 4, 1,
                                                 32, a["flags"], None)


def _backward(attn_drop, **kw):
    a = dict(heads=2, flags=0)
    a.update(kw)
    return _lib.load().gnna_gat_backward_drop_f32(F[0], 8, F[1], F[2], F[3], F[4], 8, F[5], 8, I, I, I, I, 1, I, I, I, I, 1, 0.2, attn_drop,
                                                  7, F[6], 8, F[7], F[8], 2, 2, a["heads"], 4, 32, a["flags"], None)


@pytest.mark.parametrize("call, name", [(_forward, "gnna_gat_forward_drop_f32"), (_backward, "gnna_gat_backward_drop_f32")])
def test_refusals_before_any_device_work(call, name):
    """Host buffers stand in for device memory: every call returns before it touches the device."""
    last = lambda: _lib.load().gnna_last_error().decode()
    for bad, shown in ((-0.1, "-0.1"), (1.0, "1"), (float("nan"), "nan"), (1.5, "1.5"), (float("inf"), "inf")):
        assert call(bad) == -1
        assert last().startswith(f"{name}: attn_drop must be in [0, 1) (got ") and shown in last().lower()
    # the rect entries' refusals under the entry's own name, before attn_drop is looked at
    assert call(0.5, heads=65) == -3 and last() == f"{name}: at most 64 heads (got 65)"
    assert call(0.5, heads=0) == -1 and last() == f"{name}: bad size (num_out_rows=2 num_in_rows=2 heads=0 dim=4 num_parts=1)"
    assert call(0.5, flags=1) == -3 and last() == f"{name}: GNNA_ACCUMULATE is not supported"
    try:
        _lib.set_tuning(deterministic=1)
        assert call(0.5) == -3
        assert last() == f"{name} has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"
    finally:
        _lib.reset_tuning()


def test_the_wrappers_take_the_mask_after_the_slope():
    fwd = list(inspect.signature(_lib.gat_forward_drop).parameters)
    bwd = list(inspect.signature(_lib.gat_backward_drop).parameters)
    assert fwd[:11] == ["H", "el", "er", "row_pointers", "column_index", "part_pointers", "part2Node", "partSize", "negative_slope",
                        "attn_drop", "rng_seed"]
    assert bwd[:14] == ["H", "el", "er", "lse", "Y", "dY", "row_pointers", "column_index", "part_pointers", "part2Node", "partSize",
                        "negative_slope", "attn_drop", "rng_seed"] and inspect.signature(_lib.gat_backward_drop).parameters["transposed"].default is None


def test_driver_flag():
    from gnnadvisor_osdi21_amd import main as driver
    p = driver.build_parser()
    assert p.parse_args([]).attn_drop == 0.0
    args = p.parse_args(["--model", "gat", "--fused_attention", "True", "--attn_drop", "0.6"])
    assert (args.model, args.attn_drop) == ("gat", 0.6)
    assert "one mask" in re.sub(r"\s+", " ", p.format_help())


@pytest.mark.parametrize("extra, message", [
    (["--model", "gcn", "--attn_drop", "0.6"], "--attn_drop.*--model gat"),
    (["--model", "sage", "--attn_drop", "0.1"], "--attn_drop.*--model gat"),
    (["--model", "gat", "--attn_drop", "1.0"], "--attn_drop must be in \\[0, 1\\)"),
    (["--model", "gat", "--attn_drop", "-0.5"], "--attn_drop must be in \\[0, 1\\)"),
    (["--model", "gat", "--attn_drop", "nan"], "--attn_drop"),
    (["--model", "gat", "--attn_drop", "0.6", "--hip_graph", "True"], "--hip_graph"),
    (["--model", "gat", "--attn_drop", "0.6", "--dtype", "bfloat16"], "float32"),
    (["--model", "gat", "--attn_drop", "0.6", "--fanout", "5,5"], "--fused_attention True"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    with pytest.raises(SystemExit, match=message):
        driver.main(["--synthetic", "no-such-config"] + extra)


def test_the_layer_has_the_argument():
    from gnnadvisor_osdi21_amd import ops
    sig = inspect.signature(ops.GATConv.__init__)
    assert sig.parameters["attn_drop"].default == 0.0
    assert list(sig.parameters)[:7] == ["self", "input_dim", "output_dim", "heads", "concat", "negative_slope", "fused"]
    assert inspect.signature(ops.GATConv.forward).parameters["rng_seed"].default is None
    conv = ops.GATConv(4, 4, attn_drop=0.25)
    assert conv.attn_drop == 0.25 and conv.last_rng_seed is None and ops.GATConv(4, 4).attn_drop == 0.0
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="attn_drop"):
            ops.GATConv(4, 4, attn_drop=bad)

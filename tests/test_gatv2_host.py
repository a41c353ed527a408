"""Fused GATv2 attention, the parts that need no GPU (the binding surface of include/gnna_gatv2.h and the build lists are pinned
by test_binding_table_host.py): what the header states, the refusals the two entries make before any device work, the driver's flags
and the layer's arguments."""
import ctypes
import inspect
import os
import re

import pytest

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gnna_gatv2.h")).read()


def test_the_header_states_the_function():
    flat = re.sub(r"[\s*]+", " ", _header())
    for piece in ("t[d] = Hs[j,h,d] + Hd[i,h,d]", "z = sum_d att[h,d] lrelu(t[d])", "alpha = exp(z - lse[i,h])",
                  "dz = alpha (k dalpha - c)", "g[d] = dz att[h,d] (t[d] > 0 ? 1 : s)", "dHd[i,h,:] = sum_j g",
                  "dHs[j,h,:] = sum_i (alpha k dY[i,h,:] + g)", "d_att[h,d] = sum_edges dz lrelu(t[d])",
                  "MAY be the same pointer", "heads <= 64, dim <= 256", "GNNA_ERR_INVALID_ARGUMENT before any device work"):
        assert piece in flat, piece


_B = [(ctypes.c_float * 64)() for _ in range(10)]
_I = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = ctypes.cast(_I, ctypes.c_void_p).value


def _forward(attn_drop=0.5, **kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(hs=F[0], hd=F[1], att=F[2], out=F[3], lse=F[4], ld_hs=8, ld_hd=8, ld_out=8, n_out=2, n_in=2, heads=2, dim=4, P=1, ps=32,
             flags=0, rp=I)
    a.update(kw)
    return _lib.load().gnna_gatv2_forward_f32(a["hs"], a["ld_hs"], a["hd"], a["ld_hd"], a["att"], a["rp"], I, I, I, 0.2, attn_drop, 7,
                                              a["out"], a["ld_out"], a["lse"], a["n_out"], a["n_in"], a["heads"], a["dim"], a["P"],
                                              a["ps"], a["flags"], None)


def _backward(attn_drop=0.5, **kw):
    a = dict(hs=F[0], hd=F[1], att=F[2], lse=F[4], y=F[3], dy=F[5], dhs=F[6], dhd=F[7], datt=F[8], ld_hs=8, ld_hd=8, ld_y=8, ld_dy=8,
             ld_dhs=8, ld_dhd=8, n_out=2, n_in=2, heads=2, dim=4, P=1, tP=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_gatv2_backward_f32(a["hs"], a["ld_hs"], a["hd"], a["ld_hd"], a["att"], a["lse"], a["y"], a["ld_y"], a["dy"],
                                               a["ld_dy"], I, I, I, I, a["P"], I, I, I, I, a["tP"], 0.2, attn_drop, 7, a["dhs"],
                                               a["ld_dhs"], a["dhd"], a["ld_dhd"], a["datt"], a["n_out"], a["n_in"], a["heads"],
                                               a["dim"], a["ps"], a["flags"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


@pytest.mark.parametrize("call, name", [(_forward, "gnna_gatv2_forward_f32"), (_backward, "gnna_gatv2_backward_f32")])
def test_refusals_both_entries_make_before_any_device_work(call, name):
    for bad, shown in ((-0.1, "-0.1"), (1.0, "1"), (float("nan"), "nan"), (1.5, "1.5"), (float("inf"), "inf")):
        assert call(bad) == -1
        assert _last().startswith(f"{name}: attn_drop must be in [0, 1) (got ") and shown in _last().lower()
    # the rect entries' refusals under the entry's own name, before attn_drop is looked at
    assert call(2.0, heads=65) == -3 and _last() == f"{name}: at most 64 heads (got 65)"
    assert call(heads=0) == -1 and _last() == f"{name}: bad size (num_out_rows=2 num_in_rows=2 heads=0 dim=4 num_parts=1)"
    assert call(dim=0) == -1 and _last() == f"{name}: bad size (num_out_rows=2 num_in_rows=2 heads=2 dim=0 num_parts=1)"
    assert call(n_in=-1) == -1 and _last().startswith(f"{name}: bad size (num_out_rows=2 num_in_rows=-1 ")
    assert call(P=-1) == -1 and _last().startswith(f"{name}: bad size (")
    assert call(dim=257) == -3 and _last() == f"{name}: at most 256 floats per head (got 257)"
    assert call(ps=0) == -1 and _last() == f"{name}: partSize must be positive (got 0)"
    assert call(n_out=1 << 29) == -3 and _last() == f"{name}: 536870912 rows in one call (at most 536870911): shard the rows"
    assert call(n_in=1 << 29) == -3 and "shard the rows" in _last()
    assert call(flags=1) == -3 and _last() == f"{name}: GNNA_ACCUMULATE is not supported"
    assert call(flags=8) == -1 and _last() == f"{name}: unknown flag bits 0x8"
    assert call(ld_hs=7) == -1 and _last().startswith(f"{name}: row strides must be >= heads * dim and < 2^29 floats (ld_hs=7 ld_hd=8 ")
    assert call(ld_hd=1 << 29) == -1 and "ld_hd=536870912" in _last()
    assert call(hs=None) == -1 and _last() == f"{name}: null pointer"
    assert call(hd=None) == -1 and _last() == f"{name}: null pointer"
    assert call(att=None) == -1 and _last() == f"{name}: null pointer"
    try:
        _lib.set_tuning(deterministic=1)
        assert call() == -3
        assert _last() == f"{name} has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"
    finally:
        _lib.reset_tuning()


def test_refusals_of_the_forward():
    name = "gnna_gatv2_forward_f32"
    assert _forward(flags=2 | 4) == -1 and _last() == f"{name}: unknown flag bits 0x6"
    assert _forward(ld_out=7) == -1 and "ld_out=7" in _last()
    assert _forward(out=None) == -1 and _last() == f"{name}: null pointer"
    assert _forward(lse=None) == -1 and _last() == f"{name}: null pointer"
    assert _forward(rp=None) == -1 and _last() == f"{name}: null pointer"
    alias = f"{name}: an output must not alias an input or the other output"
    for kw in (dict(out=F[0]), dict(out=F[1]), dict(out=F[2]), dict(out=F[4]), dict(lse=F[0]), dict(lse=F[1]), dict(lse=F[2])):
        assert _forward(**kw) == -1 and _last() == alias, kw
    # no destination row: nothing to write, nothing to check beyond the sizes; Hs is Hd passes the alias check (it then needs a device)
    assert _forward(n_out=0, out=None, lse=None) == 0


def test_refusals_of_the_backward():
    name = "gnna_gatv2_backward_f32"
    assert _backward(flags=2) == -1 and _last() == f"{name}: unknown flag bits 0x2"          # (the ReLU epilogue is the forward's)
    assert _backward(tP=-1) == -1 and _last() == f"{name}: bad size (t_num_parts=-1)"
    assert _backward(datt=None) == -1 and _last() == f"{name}: null pointer"
    assert _backward(datt=None, n_out=0, n_in=0) == -1 and _last() == f"{name}: null pointer"     # d_att is written on every call
    for kw in (dict(ld_y=7), dict(ld_dy=7), dict(ld_dhs=7), dict(ld_dhd=7)):
        assert _backward(**kw) == -1 and f"{list(kw)[0]}=7" in _last(), kw
    for kw in (dict(lse=None), dict(y=None), dict(dy=None), dict(dhs=None), dict(dhd=None)):
        assert _backward(**kw) == -1 and _last() == f"{name}: null pointer", kw
    assert _backward(n_out=0, dhs=None) == -1 and _last() == f"{name}: dHs: null pointer or a row stride outside [heads * dim, 2^29)"
    assert _backward(n_in=0, ld_dhd=3) == -1 and _last() == f"{name}: dHd: null pointer or a row stride outside [heads * dim, 2^29)"
    for out in ("dhs", "dhd", "datt"):
        for inp in (0, 1, 2, 3, 4, 5):
            assert _backward(**{out: F[inp]}) == -1 and _last() == f"{name}: an output must not alias an input", (out, inp)
    for kw in (dict(dhs=F[7]), dict(dhs=F[8]), dict(dhd=F[8])):
        assert _backward(**kw) == -1 and _last() == f"{name}: the outputs must not alias each other", kw


def test_the_wrappers():
    fwd = list(inspect.signature(_lib.gatv2_forward).parameters)
    bwd = inspect.signature(_lib.gatv2_backward).parameters
    assert fwd[:11] == ["Hs", "Hd", "att", "row_pointers", "column_index", "part_pointers", "part2Node", "partSize", "negative_slope",
                        "attn_drop", "rng_seed"]
    assert list(bwd)[:14] == ["Hs", "Hd", "att", "lse", "Y", "dY", "row_pointers", "column_index", "part_pointers", "part2Node",
                              "partSize", "negative_slope", "attn_drop", "rng_seed"] and bwd["transposed"].default is None
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    assert "gnna_gatv2.h" in GNNA.gatv2_forward.__doc__ and "(dHs, dHd, d_att)" in GNNA.gatv2_backward.__doc__


def test_driver_flags():
    from gnnadvisor_osdi21_amd import main as driver
    p = driver.build_parser()
    args = p.parse_args(["--model", "gatv2", "--fused_attention", "True", "--attn_drop", "0.6", "--heads", "4", "--fanout", "5,5"])
    assert (args.model, args.attn_drop, args.heads, args.fanout) == ("gatv2", 0.6, 4, "5,5")
    assert "GATv2" in p.format_help()


@pytest.mark.parametrize("extra, message", [
    (["--model", "gatv2", "--hip_graph", "True"], "--model gatv2 does not support --hip_graph True: run it with --hip_graph False"),
    (["--model", "gatv2", "--dtype", "bfloat16"], "--dtype bfloat16: the attention layers .* are float32 only; run --model gatv2 with "
                                                  "--dtype float32"),
    (["--model", "gatv2", "--dtype", "float16"], "run --model gatv2 with --dtype float32"),
    (["--model", "gatv2", "--attn_drop", "1.0"], "--attn_drop must be in \\[0, 1\\)"),
    (["--model", "gatv2", "--heads", "0"], "--heads must be >= 1"),
    (["--model", "gatv2", "--fanout", "5,5"], "--model gatv2 --fanout runs on the fused attention kernels only .*add --fused_attention True"),
    (["--model", "gatv2", "--fused_attention", "True", "--fanout", "5"], "--model gatv2 has 2 layers \\(got 1\\)"),
    (["--model", "gatv2", "--fused_attention", "True", "--fanout", "5,5", "--batch_size", "0"], "--batch_size must be >= 1"),
    # the gat checks keep their text for gat, and the other models are still sent to --model gat
    (["--model", "gat", "--hip_graph", "True"], "--model gat does not support --hip_graph True: run it with --hip_graph False"),
    (["--model", "gat", "--dtype", "bfloat16"], "run --model gat with --dtype float32"),
    (["--model", "gat", "--fanout", "5,5"], "--model gat --fanout runs on the fused attention kernels only"),
    (["--model", "gcn", "--fused_attention", "True"], "run it with --model gat \\(got --model gcn\\)"),
    (["--model", "gcn", "--attn_drop", "0.5"], "--attn_drop drops attention coefficients: run it with --model gat \\(got --model gcn\\)"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    with pytest.raises(SystemExit, match=message):
        driver.main(["--synthetic", "no-such-config"] + extra)


def test_the_layer_and_its_argument_errors():
    import torch
    from gnnadvisor_osdi21_amd import ops
    sig = inspect.signature(ops.GATv2Conv.__init__)
    assert list(sig.parameters) == ["self", "input_dim", "output_dim", "heads", "concat", "negative_slope", "share_weights", "attn_drop",
                                    "fused"]
    assert [sig.parameters[n].default for n in ("heads", "concat", "negative_slope", "share_weights", "attn_drop", "fused")] == \
        [1, True, 0.2, False, 0.0, True]
    assert inspect.signature(ops.GATv2Conv.forward).parameters["rng_seed"].default is None
    conv = ops.GATv2Conv(6, 5, heads=3, attn_drop=0.25)
    assert {n: tuple(q.shape) for n, q in conv.named_parameters()} == {"W_l": (6, 15), "W_r": (6, 15), "att": (3, 5)}
    assert conv.attn_drop == 0.25 and conv.last_rng_seed is None and conv.fused
    bound = 1 / 5 ** 0.5
    assert all(float(q.detach().abs().max()) <= bound for q in conv.parameters())
    shared = ops.GATv2Conv(6, 5, heads=3, share_weights=True)
    assert sorted(n for n, _ in shared.named_parameters()) == ["W_l", "att"] and shared.W_r is None
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="attn_drop"):
            ops.GATv2Conv(4, 4, attn_drop=bad)
    with pytest.raises(ValueError, match="heads"):
        ops.GATv2Conv(4, 4, heads=0)
    # fp32 only, as GATConv raises it; raised before the graph is looked at
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 only"):
            ops.GATv2Conv(4, 4)(torch.zeros(3, 4, dtype=dtype), None)
    fwd = list(inspect.signature(ops.GATv2Attention.forward).parameters)
    assert fwd == ["ctx", "Hs", "Hd", "att", "inputInfo", "negative_slope", "attn_drop", "rng_seed"]
    H, att = torch.zeros(3, 8), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="attn_drop must be in \\[0, 1\\)"):
        ops.GATv2Attention.apply(H, H, att, None, 0.2, 1.0, 0)
    with pytest.raises(TypeError, match="float32 only"):
        ops.GATv2Attention.apply(H.double(), H.double(), att, None, 0.2)
    with pytest.raises(ValueError, match="att \\[heads, F\\] expected"):
        ops.GATv2Attention.apply(H, H, torch.zeros(3, 4), None, 0.2)

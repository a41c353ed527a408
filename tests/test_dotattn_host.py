"""Fused dot-product graph attention, the parts that need no GPU (the binding surface of include/gnna_dotattn.h and the build lists
are pinned by test_binding_table_host.py): what the header states, the refusals the two entries make before any device work, the
driver's flags and the layer's arguments."""
import ctypes
import inspect
import os
import re

import pytest

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gnna_dotattn.h")).read()


def test_the_header_states_the_function():
    flat = re.sub(r"[\s*]+", " ", _header())
    for piece in ("z = scale sum_d Q[i,h,d] K[j,h,d]", "lse[i,h] = logsumexp_j z (0 for a row without edges)",
                  "alpha = exp(z - lse[i,h])", "out[i,h,:] = sum_j alpha k V[j,h,:]", "c[i,h] = <dY[i,h,:], Y[i,h,:]>",
                  "dalpha = <dY[i,h,:], V[j,h,:]>", "dz = alpha (k dalpha - c)", "dQ[i,h,:] = scale sum_j dz K[j,h,:]",
                  "dK[j,h,:] = scale sum_i dz Q[i,h,:]", "dV[j,h,:] = sum_i alpha k dY[i,h,:]", "MAY overlap",
                  "heads <= 64, dim <= 256", "GNNA_ERR_INVALID_ARGUMENT before any device work", "a scale that is NaN or infinite"):
        assert piece in flat, piece


_B = [(ctypes.c_float * 64)() for _ in range(10)]
_I = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = ctypes.cast(_I, ctypes.c_void_p).value


def _forward(attn_drop=0.5, **kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(q=F[0], k=F[1], v=F[2], out=F[3], lse=F[4], ld_q=8, ld_k=8, ld_v=8, ld_out=8, n_out=2, n_in=2, heads=2, dim=4, P=1, ps=32,
             flags=0, rp=I, scale=0.5)
    a.update(kw)
    return _lib.load().gnna_dot_attn_forward_f32(a["q"], a["ld_q"], a["k"], a["ld_k"], a["v"], a["ld_v"], a["rp"], I, I, I, a["scale"],
                                                 attn_drop, 7, a["out"], a["ld_out"], a["lse"], a["n_out"], a["n_in"], a["heads"],
                                                 a["dim"], a["P"], a["ps"], a["flags"], None)


def _backward(attn_drop=0.5, **kw):
    a = dict(q=F[0], k=F[1], v=F[2], lse=F[4], y=F[3], dy=F[5], dq=F[6], dk=F[7], dv=F[8], ld_q=8, ld_k=8, ld_v=8, ld_y=8, ld_dy=8,
             ld_dq=8, ld_dk=8, ld_dv=8, n_out=2, n_in=2, heads=2, dim=4, P=1, tP=1, ps=32, flags=0, scale=0.5)
    a.update(kw)
    return _lib.load().gnna_dot_attn_backward_f32(a["q"], a["ld_q"], a["k"], a["ld_k"], a["v"], a["ld_v"], a["lse"], a["y"], a["ld_y"],
                                                  a["dy"], a["ld_dy"], I, I, I, I, a["P"], I, I, I, I, a["tP"], a["scale"], attn_drop, 7,
                                                  a["dq"], a["ld_dq"], a["dk"], a["ld_dk"], a["dv"], a["ld_dv"], a["n_out"], a["n_in"],
                                                  a["heads"], a["dim"], a["ps"], a["flags"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


@pytest.mark.parametrize("call, name", [(_forward, "gnna_dot_attn_forward_f32"), (_backward, "gnna_dot_attn_backward_f32")])
def test_refusals_both_entries_make_before_any_device_work(call, name):
    for bad, shown in ((-0.1, "-0.1"), (1.0, "1"), (float("nan"), "nan"), (1.5, "1.5"), (float("inf"), "inf")):
        assert call(bad) == -1
        assert _last().startswith(f"{name}: attn_drop must be in [0, 1) (got ") and shown in _last().lower()
    # new with these entries: the scale
    for bad, shown in ((float("nan"), "nan"), (float("inf"), "inf"), (-float("inf"), "-inf")):
        assert call(scale=bad) == -1
        assert _last().startswith(f"{name}: scale must be finite (got ") and shown in _last().lower()
    # the rect entries' refusals under the entry's own name, before attn_drop and scale are looked at
    assert call(2.0, heads=65) == -3 and _last() == f"{name}: at most 64 heads (got 65)"
    assert call(scale=float("nan"), heads=65) == -3 and _last() == f"{name}: at most 64 heads (got 65)"
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
    assert call(ld_q=7) == -1 and _last().startswith(f"{name}: row strides must be >= heads * dim and < 2^29 floats (ld_q=7 ld_k=8 ld_v=8 ")
    assert call(ld_k=1 << 29) == -1 and "ld_k=536870912" in _last()
    assert call(ld_v=7) == -1 and "ld_v=7" in _last()
    for kw in (dict(q=None), dict(k=None), dict(v=None)):
        assert call(**kw) == -1 and _last() == f"{name}: null pointer", kw
    try:
        _lib.set_tuning(deterministic=1)
        assert call() == -3
        assert _last() == f"{name} has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"
    finally:
        _lib.reset_tuning()


def test_refusals_of_the_forward():
    name = "gnna_dot_attn_forward_f32"
    assert _forward(flags=2 | 4) == -1 and _last() == f"{name}: unknown flag bits 0x6"
    assert _forward(ld_out=7) == -1 and "ld_out=7" in _last()
    assert _forward(out=None) == -1 and _last() == f"{name}: null pointer"
    assert _forward(lse=None) == -1 and _last() == f"{name}: null pointer"
    assert _forward(rp=None) == -1 and _last() == f"{name}: null pointer"
    alias = f"{name}: an output must not alias an input or the other output"
    for kw in (dict(out=F[0]), dict(out=F[1]), dict(out=F[2]), dict(out=F[4]), dict(lse=F[0]), dict(lse=F[1]), dict(lse=F[2])):
        assert _forward(**kw) == -1 and _last() == alias, kw
    # no destination row: nothing to write, nothing to check beyond the sizes (Q, K and V as one pointer pass the alias check; that
    # call then needs a device)
    assert _forward(n_out=0, out=None, lse=None) == 0
    assert _forward(n_out=0, out=None, lse=None, scale=float("nan")) == -1


def test_refusals_of_the_backward():
    name = "gnna_dot_attn_backward_f32"
    assert _backward(flags=2) == -1 and _last() == f"{name}: unknown flag bits 0x2"          # (the ReLU epilogue is the forward's)
    assert _backward(tP=-1) == -1 and _last() == f"{name}: bad size (t_num_parts=-1)"
    for kw in (dict(ld_y=7), dict(ld_dy=7), dict(ld_dq=7), dict(ld_dk=7), dict(ld_dv=7)):
        assert _backward(**kw) == -1 and f"{list(kw)[0]}=7" in _last(), kw
    for kw in (dict(lse=None), dict(y=None), dict(dy=None), dict(dq=None), dict(dk=None), dict(dv=None)):
        assert _backward(**kw) == -1 and _last() == f"{name}: null pointer", kw
    assert _backward(n_out=0, dk=None) == -1 and _last() == f"{name}: dK / dV: null pointer or a row stride outside [heads * dim, 2^29)"
    assert _backward(n_out=0, ld_dv=3) == -1 and _last() == f"{name}: dK / dV: null pointer or a row stride outside [heads * dim, 2^29)"
    assert _backward(n_in=0, ld_dq=3) == -1 and _last() == f"{name}: dQ: null pointer or a row stride outside [heads * dim, 2^29)"
    for out in ("dq", "dk", "dv"):
        for inp in (0, 1, 2, 3, 4, 5):
            assert _backward(**{out: F[inp]}) == -1 and _last() == f"{name}: an output must not alias an input", (out, inp)
    for kw in (dict(dq=F[7]), dict(dq=F[8]), dict(dk=F[8])):
        assert _backward(**kw) == -1 and _last() == f"{name}: the outputs must not alias each other", kw


def test_the_wrappers():
    fwd = list(inspect.signature(_lib.dot_attn_forward).parameters)
    bwd = inspect.signature(_lib.dot_attn_backward).parameters
    assert fwd[:12] == ["Q", "K", "V", "heads", "row_pointers", "column_index", "part_pointers", "part2Node", "partSize", "scale",
                        "attn_drop", "rng_seed"]
    assert list(bwd)[:15] == ["Q", "K", "V", "heads", "lse", "Y", "dY", "row_pointers", "column_index", "part_pointers", "part2Node",
                              "partSize", "scale", "attn_drop", "rng_seed"] and bwd["transposed"].default is None
    assert inspect.signature(_lib.dot_attn_forward).parameters["scale"].default is None and bwd["scale"].default is None
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    assert "gnna_dotattn.h" in GNNA.dot_attn_forward.__doc__ and "(dQ, dK, dV)" in GNNA.dot_attn_backward.__doc__


def test_driver_flags():
    from gnnadvisor_osdi21_amd import main as driver
    p = driver.build_parser()
    args = p.parse_args(["--model", "transformer", "--fused_attention", "True", "--attn_drop", "0.6", "--heads", "4", "--fanout", "5,5",
                         "--directed", "True"])
    assert (args.model, args.attn_drop, args.heads, args.fanout) == ("transformer", 0.6, 4, "5,5")
    assert "TransformerConv" in p.format_help()


@pytest.mark.parametrize("extra, message", [
    (["--model", "transformer", "--hip_graph", "True"],
     "--model transformer does not support --hip_graph True: run it with --hip_graph False"),
    (["--model", "transformer", "--dtype", "bfloat16"], "--dtype bfloat16: the attention layers .* are float32 only; run --model "
                                                        "transformer with --dtype float32"),
    (["--model", "transformer", "--dtype", "float16"], "run --model transformer with --dtype float32"),
    (["--model", "transformer", "--attn_drop", "1.0"], "--attn_drop must be in \\[0, 1\\)"),
    (["--model", "transformer", "--heads", "0"], "--heads must be >= 1"),
    (["--model", "transformer", "--fanout", "5,5"],
     "--model transformer --fanout runs on the fused attention kernels only .*add --fused_attention True"),
    (["--model", "transformer", "--fused_attention", "True", "--fanout", "5"], "--model transformer has 2 layers \\(got 1\\)"),
    (["--model", "transformer", "--fused_attention", "True", "--fanout", "5,5", "--batch_size", "0"], "--batch_size must be >= 1"),
    # the existing checks keep their text for the models they name today
    (["--model", "gat", "--hip_graph", "True"], "--model gat does not support --hip_graph True: run it with --hip_graph False"),
    (["--model", "gatv2", "--dtype", "bfloat16"], "run --model gatv2 with --dtype float32"),
    (["--model", "gatv2", "--fanout", "5,5"], "--model gatv2 --fanout runs on the fused attention kernels only"),
    (["--model", "gcn", "--fused_attention", "True"], "run it with --model gat \\(got --model gcn\\)"),
    (["--model", "gcn", "--attn_drop", "0.5"], "--attn_drop drops attention coefficients: run it with --model gat \\(got --model gcn\\)"),
    (["--model", "gcn", "--fanout", "5,5"], "--fanout trains GraphSAGE on sampled blocks: run it with --model sage, or with --model gat "
                                            "--fused_attention True \\(got --model gcn\\)"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    with pytest.raises(SystemExit, match=message):
        driver.main(["--synthetic", "no-such-config"] + extra)


def test_the_layer_and_its_argument_errors():
    import torch
    from gnnadvisor_osdi21_amd import ops
    sig = inspect.signature(ops.TransformerConv.__init__)
    assert list(sig.parameters) == ["self", "input_dim", "output_dim", "heads", "concat", "root_weight", "attn_drop", "fused"]
    assert [sig.parameters[n].default for n in ("heads", "concat", "root_weight", "attn_drop", "fused")] == [1, True, True, 0.0, True]
    assert inspect.signature(ops.TransformerConv.forward).parameters["rng_seed"].default is None
    conv = ops.TransformerConv(6, 5, heads=3, attn_drop=0.25)
    assert {n: tuple(q.shape) for n, q in conv.named_parameters()} == {"weights": (6, 45), "W_skip": (6, 15)}      # no biases
    assert conv.attn_drop == 0.25 and conv.last_rng_seed is None and conv.fused
    bound = 1 / 5 ** 0.5
    assert all(float(q.detach().abs().max()) <= bound for q in conv.parameters())
    mean = ops.TransformerConv(6, 5, heads=3, concat=False)
    assert tuple(mean.W_skip.shape) == (6, 5)
    bare = ops.TransformerConv(6, 5, heads=3, root_weight=False)
    assert [n for n, _ in bare.named_parameters()] == ["weights"] and bare.W_skip is None
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="attn_drop"):
            ops.TransformerConv(4, 4, attn_drop=bad)
    with pytest.raises(ValueError, match="heads"):
        ops.TransformerConv(4, 4, heads=0)
    # fp32 only, as GATv2Conv raises it; raised before the graph is looked at
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 only"):
            ops.TransformerConv(4, 4)(torch.zeros(3, 4, dtype=dtype), None)
    fwd = list(inspect.signature(ops.DotAttention.forward).parameters)
    assert fwd == ["ctx", "Q", "K", "V", "inputInfo", "heads", "scale", "attn_drop", "rng_seed"]
    defaults = inspect.signature(ops.DotAttention.forward).parameters
    assert defaults["scale"].default is None and defaults["attn_drop"].default == 0.0 and defaults["rng_seed"].default == 0
    H = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="attn_drop must be in \\[0, 1\\)"):
        ops.DotAttention.apply(H, H, H, None, 2, None, 1.0, 0)
    with pytest.raises(TypeError, match="float32 only"):
        ops.DotAttention.apply(H.double(), H.double(), H.double(), None, 2)
    with pytest.raises(ValueError, match="K and V \\[num_src, heads \\* F\\] with heads = 3 expected"):
        ops.DotAttention.apply(H, H, H, None, 3)
    with pytest.raises(ValueError, match="K and V \\[num_src, heads \\* F\\]"):
        ops.DotAttention.apply(H, H, torch.zeros(3, 4), None, 2)
    with pytest.raises(ValueError, match="scale must be finite"):
        ops.DotAttention.apply(H, H, H, None, 2, float("nan"))

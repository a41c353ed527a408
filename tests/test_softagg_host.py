"""Softmax neighbor aggregation and GENConv, the parts that need no GPU (the binding surface of include/gnna_softagg.h and
the build lists are pinned by test_binding_table_host.py): what the header leaves open, the refusals both entries make before any
device work, the wrappers, the modules' constructor errors and the driver's refusals."""
import ctypes
import inspect
import os

import pytest

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD, BWD = "gnna_agg_softmax_ld_f32", "gnna_agg_softmax_backward_ld_f32"


def test_the_header_says_what_it_does_not_pin():
    header = open(os.path.join(ROOT, "include", "gnna_softagg.h")).read()
    assert "not pinned" in header            # NaN / infinite features, a non-finite temperature


_B = [(ctypes.c_float * 64)() for _ in range(10)]
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = [ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p).value for _ in range(2)]


def _fwd(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(x=F[0], ld_in=8, n_in=2, temp=F[1], temp_len=1, rp=I[0], ci=I[1], out=F[2], ld_out=8, lse=F[3], ld_lse=8, sq=F[4],
             ld_sq=8, n_out=2, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_softmax_ld_f32(a["x"], a["ld_in"], a["n_in"], a["temp"], a["temp_len"], a["rp"], a["ci"], a["out"],
                                               a["ld_out"], a["lse"], a["ld_lse"], a["sq"], a["ld_sq"], a["n_out"], a["dim"],
                                               a["flags"], None)


def _bwd(**kw):
    a = dict(x=F[0], ld_in=8, n_in=2, temp=F[1], temp_len=1, lse=F[3], ld_lse=8, y=F[2], ld_y=8, dy=F[5], ld_dy=8, rp=I[0], ci=I[1],
             dx=F[6], ld_din=8, n_out=2, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_softmax_backward_ld_f32(a["x"], a["ld_in"], a["n_in"], a["temp"], a["temp_len"], a["lse"], a["ld_lse"],
                                                        a["y"], a["ld_y"], a["dy"], a["ld_dy"], a["rp"], a["ci"], a["dx"],
                                                        a["ld_din"], a["n_out"], a["dim"], a["flags"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


INVALID, UNSUPPORTED = -1, -3                                                # include/gnna.h


@pytest.mark.parametrize("call, name", [(_fwd, FWD), (_bwd, BWD)], ids=["forward", "backward"])
def test_refusals_both_entries_make_alike(call, name):
    for flags in (_lib.ACCUMULATE, _lib.EPILOGUE_RELU, 4):
        assert call(flags=flags) == INVALID
        assert _last() == f"{name} takes no flags (got 0x{flags:x}): GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning for a " \
                          "softmax aggregation"
    assert call(dim=0) == INVALID and _last() == f"{name}: dim must be >= 1 (got 0)"
    assert call(dim=-3) == INVALID and _last() == f"{name}: dim must be >= 1 (got -3)"
    assert call(n_out=-1) == INVALID and _last() == f"{name}: negative size (num_out_rows=-1 num_in_rows=2)"
    assert call(n_in=-2) == INVALID and _last() == f"{name}: negative size (num_out_rows=2 num_in_rows=-2)"
    for temp_len in (0, 2, 3, 5, -1):
        assert call(temp_len=temp_len) == INVALID and _last() == f"{name}: temp_len must be 1 or dim = 4 (got {temp_len})"
    assert call(temp_len=4, x=None) == INVALID and _last() == f"{name}: null feature pointer"     # (dim itself passes)
    for rows in ("n_out", "n_in"):
        assert call(**{rows: 1 << 29}) == UNSUPPORTED and _last() == f"{name}: 536870912 rows in one call (at most 536870911): shard the rows"
    assert call(x=F[7] + 2) == INVALID and "must be 4-byte aligned" in _last() and _last().startswith(name + ": ")
    assert call(temp=F[7] + 1) == INVALID and "must be 4-byte aligned" in _last()
    assert call(x=None) == INVALID and _last() == f"{name}: null feature pointer"
    assert call(temp=None) == INVALID and _last() == f"{name}: null temperature pointer"
    for idx in ("rp", "ci"):
        assert call(**{idx: None}) == INVALID and _last() == f"{name}: null index pointer", idx


def test_refusals_of_the_forward_entry():
    for ld in ("ld_in", "ld_out", "ld_lse", "ld_sq"):
        assert _fwd(**{ld: 3}) == INVALID and _last().startswith(FWD + ": row strides must be >= dim and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
        assert _fwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    # (a null sq's stride strides nothing: the call gets past the stride check to the next refusal)
    assert _fwd(sq=None, ld_sq=3, x=None) == INVALID and _last() == FWD + ": null feature pointer"
    for name in ("out", "lse", "sq"):
        assert _fwd(**{name: F[7] + 2}) == INVALID and _last() == FWD + ": feature, temperature and output pointers must be 4-byte aligned"
        assert _fwd(**{name: F[0]}) == INVALID and _last() == FWD + ": an output must not alias an input", name
        assert _fwd(**{name: F[1]}) == INVALID and _last() == FWD + ": an output must not alias an input", name
    assert _fwd(lse=F[2]) == INVALID and _last() == FWD + ": the outputs must not alias each other"
    assert _fwd(sq=F[2]) == INVALID and _last() == FWD + ": the outputs must not alias each other"
    assert _fwd(sq=F[3]) == INVALID and _last() == FWD + ": the outputs must not alias each other"
    for name in ("out", "lse"):
        assert _fwd(**{name: None}) == INVALID and _last() == FWD + ": null output pointer (out and lse are always written)"
    assert _fwd(n_out=0) == 0                                                 # no destination row: nothing to write


def test_refusals_of_the_backward_entry():
    for ld in ("ld_in", "ld_lse", "ld_y", "ld_dy", "ld_din"):
        assert _bwd(**{ld: 3}) == INVALID and _last().startswith(BWD + ": row strides must be >= dim and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
        assert _bwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    for name in ("lse", "y", "dy", "dx"):
        assert _bwd(**{name: F[7] + 2}) == INVALID and _last() == BWD + ": feature, temperature and gradient pointers must be 4-byte aligned"
    for inp in (0, 1, 2, 3, 5):                                              # input, temp, Y, lse, dY
        assert _bwd(dx=F[inp]) == INVALID and _last() == BWD + ": an output must not alias an input", inp
    assert _bwd(dx=None) == INVALID and _last() == BWD + ": null output pointer"
    for name in ("lse", "y", "dy"):
        assert _bwd(**{name: None}) == INVALID and _last() == BWD + ": null lse, Y or dY pointer", name
    assert _bwd(n_in=0) == 0                                                  # no source row: nothing to write


def test_deterministic_tuning_does_not_refuse_the_entries():
    try:
        _lib.set_tuning(deterministic=1)
        # (the next refusal is met instead of GNNA_ERR_UNSUPPORTED: no device is touched here)
        assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
        assert _bwd(x=None) == INVALID and _last() == BWD + ": null feature pointer"
    finally:
        _lib.reset_tuning()


def test_the_wrappers():
    sig = inspect.signature(_lib.agg_softmax).parameters
    assert list(sig)[:6] == ["X", "temp", "row_pointers", "column_index", "num_out_rows", "want_sq"] and sig["want_sq"].default is False
    sig = inspect.signature(_lib.agg_softmax_backward).parameters
    assert list(sig)[:7] == ["X", "temp", "lse", "Y", "dY", "t_row_pointers", "t_column_index"]
    assert "gnna_agg_softmax_ld_f32" in _lib.agg_softmax.__doc__ and "logsumexp" in _lib.agg_softmax.__doc__
    assert "gnna_agg_softmax_backward_ld_f32" in _lib.agg_softmax_backward.__doc__
    import torch
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.agg_softmax(torch.zeros(2, 4), torch.ones(1), torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 2)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.agg_softmax_backward(torch.zeros(2, 4), torch.ones(1), None, None, None, None, None)
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    assert "(out, lse, sq)" in GNNA.aggregate_softmax.__doc__ and "want_sq" in GNNA.aggregate_softmax.__doc__
    assert "transposed edges" in GNNA.aggregate_softmax_backward.__doc__


def test_the_modules_their_constructor_errors_and_the_dtypes_they_refuse():
    import types

    import torch
    from gnnadvisor_osdi21_amd import ops
    sig = inspect.signature(ops.SoftmaxAggregation.__init__).parameters
    assert list(sig) == ["self", "t", "learn", "channels", "fused"]
    assert (sig["t"].default, sig["learn"].default, sig["channels"].default, sig["fused"].default) == (1.0, False, 1, True)
    sig = inspect.signature(ops.GENConv.__init__).parameters
    assert list(sig) == ["self", "input_dim", "output_dim", "t", "learn_t", "channels", "eps", "bias", "fused"]
    assert (sig["t"].default, sig["learn_t"].default, sig["channels"].default, sig["eps"].default, sig["bias"].default,
            sig["fused"].default) == (1.0, False, 1, 1e-7, False, True)
    assert list(inspect.signature(ops.GENConv.forward).parameters) == ["self", "X", "inputInfo", "relu"]

    fixed = ops.SoftmaxAggregation(t=0.5)
    assert dict(fixed.named_parameters()) == {} and fixed.t.tolist() == [0.5] and "t" in dict(fixed.named_buffers())
    learnt = ops.SoftmaxAggregation(t=2.0, learn=True, channels=3)
    assert {n: tuple(q.shape) for n, q in learnt.named_parameters()} == {"t": (3,)} and learnt.t.tolist() == [2.0] * 3
    for kw, message in ((dict(channels=0), "channels must be a positive integer \\(got 0\\)"),
                        (dict(channels=-2), "channels must be a positive integer \\(got -2\\)"),
                        (dict(channels=1.5), "channels must be a positive integer \\(got 1.5\\)"),
                        (dict(t=float("inf")), "t must be finite \\(got inf\\)"), (dict(t=float("nan")), "t must be finite \\(got nan\\)")):
        with pytest.raises(ValueError, match=message):
            ops.SoftmaxAggregation(**kw)

    conv = ops.GENConv(6, 5, bias=True, learn_t=True, channels=5)
    assert {n: tuple(q.shape) for n, q in conv.named_parameters()} == {
        "weights_in": (6, 5), "aggr.t": (5,), "weights_mlp1": (5, 10), "weights_mlp2": (10, 5), "bias_mlp1": (10,), "bias_mlp2": (5,)}
    for name, q in conv.named_parameters():
        if name.startswith("weights"):
            assert float(q.detach().abs().max()) <= 1 / q.shape[1] ** 0.5 and float(q.detach().abs().max()) > 0
    square = ops.GENConv(5, 5)
    assert sorted(n for n, _ in square.named_parameters()) == ["weights_mlp1", "weights_mlp2"] and square.eps == 1e-7
    for kw, message in ((dict(channels=3), "channels must be 1 or output_dim = 5 \\(got 3\\)"),
                        (dict(channels=0), "channels must be 1 or output_dim = 5 \\(got 0\\)"),
                        (dict(eps=-1e-3), "eps must be >= 0 \\(got -0.001\\)"), (dict(t=float("inf")), "t must be finite \\(got inf\\)")):
        with pytest.raises(ValueError, match=message):
            ops.GENConv(6, 5, **kw)

    info = types.SimpleNamespace()
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="NeighborSoftmax computes in float32 only: 16-bit features and torch.autocast are not supported"):
            ops.NeighborSoftmax.apply(torch.zeros(3, 6, dtype=dtype), torch.ones(1), info)
        with pytest.raises(TypeError, match="GENConv computes in float32 only: 16-bit features and torch.autocast are not supported"):
            conv(torch.zeros(3, 6, dtype=dtype), info)
        with pytest.raises(TypeError, match="SoftmaxAggregation computes in float32 only"):
            ops.SoftmaxAggregation(fused=False)(torch.zeros(3, 6, dtype=dtype), info)
    with pytest.raises(ValueError, match="SoftmaxAggregation has 3 temperatures, the features 6 channels"):
        learnt(torch.zeros(3, 6), info)
    from gnnadvisor_osdi21_amd.sampling import SampledBlock
    block = SampledBlock(torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None, None, 32, 2, 3, None)
    with pytest.raises(TypeError, match="SoftmaxAggregation\\(fused=False\\) does not take a SampledBlock"):
        ops.SoftmaxAggregation(fused=False)(torch.zeros(3, 6), block)
    doc = " ".join(ops.GENConv.__doc__.split())
    assert "powermean" in doc and "edge attributes" in doc and "normalisation inside the MLP" in doc
    assert "never exp(-lse)" in " ".join(ops.NeighborSoftmax.__doc__.split())
    assert "timing baseline" in " ".join(ops.SoftmaxAggregation.__doc__.split())


@pytest.mark.parametrize("extra, message", [
    (["--dtype", "bfloat16"], "--dtype bfloat16: the GEN layers .* are float32 only; run --model gen with --dtype float32"),
    (["--dtype", "float16"], "run --model gen with --dtype float32"),
    (["--fanout", "5,5", "--hip_graph", "True"], "--fanout does not support --hip_graph True"),
    (["--fanout", "5"], "--fanout needs one entry per layer: --model gen has 2 layers \\(got 1\\)"),
    (["--fanout", "5,5", "--batch_size", "0"], "--batch_size must be >= 1"),
    (["--fused_attention", "True"], "run it with --model gat \\(got --model gen\\)"),
    (["--edge_dim", "4"], "run it with --model gat \\(got --model gen\\)"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    text = driver.build_parser().format_help()
    assert "gen" in text and "--learn_t" in text and "--softmax_t" in text
    with pytest.raises(SystemExit, match=message):
        driver.main(["--synthetic", "no-such-config", "--model", "gen"] + extra)
    with pytest.raises(SystemExit):
        driver.main(["--synthetic", "no-such-config", "--model", "gen", "--learn_t", "maybe"])

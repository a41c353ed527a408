"""Neighbor statistics from one gather and PNAConv, the parts that need no GPU (the binding surface of include/gnna_stats.h
and the build lists are pinned by test_binding_table_host.py): the refusals the entry makes before any device work, the wrappers,
the layer's constructor errors and the driver's refusals."""
import ctypes
import inspect

import pytest

from gnnadvisor_osdi21_amd import _lib


_B = [(ctypes.c_float * 64)() for _ in range(8)]
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p).value


def _call(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(x=F[0], ld_in=8, n_in=2, ci=I, pp=I, p2n=I, sum=F[1], ld_sum=8, sumsq=F[2], ld_sumsq=8, max=F[3], ld_max=8, argmax=F[4],
             ld_argmax=8, min=F[5], ld_min=8, argmin=F[6], ld_argmin=8, n_out=2, dim=4, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_stats_ld_f32(a["x"], a["ld_in"], a["n_in"], a["ci"], a["pp"], a["p2n"], a["sum"], a["ld_sum"], a["sumsq"],
                                             a["ld_sumsq"], a["max"], a["ld_max"], a["argmax"], a["ld_argmax"], a["min"], a["ld_min"],
                                             a["argmin"], a["ld_argmin"], a["n_out"], a["dim"], a["P"], a["ps"], a["flags"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


def test_refusals_made_before_any_device_work():
    INVALID, UNSUPPORTED = -1, -3                                            # include/gnna.h
    assert _call(sum=None, sumsq=None, max=None, argmax=None, min=None, argmin=None) == INVALID
    assert _last() == "no statistic asked for: sum, sumsq, max_out and min_out are all null"
    assert _call(max=None) == INVALID and _last() == "argmax without max_out: positions come with their values"
    assert _call(min=None) == INVALID and _last() == "argmin without min_out: positions come with their values"
    assert _call(dim=0) == INVALID and _last() == "dim must be >= 1 (got 0)"
    for flags in (_lib.ACCUMULATE, _lib.EPILOGUE_RELU, 4):
        assert _call(flags=flags) == INVALID
        assert _last() == f"gnna_agg_stats_ld_f32 takes no flags (got 0x{flags:x}): GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no " \
                          "meaning for several statistics"
    for ld in ("ld_in", "ld_sum", "ld_sumsq", "ld_max", "ld_argmax", "ld_min", "ld_argmin"):
        assert _call(**{ld: 3}) == INVALID and _last().startswith("row strides must be >= dim and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
    # (a null output's stride strides nothing: the call gets past the stride check to the next refusal)
    assert _call(sum=None, ld_sum=3, x=None) == INVALID and _last() == "null feature pointer"
    assert _call(ld_in=1 << 29) == INVALID
    assert _call(n_out=-1) == INVALID and _last().startswith("negative size (num_out_rows=-1 ")
    assert _call(ps=0) == INVALID and _last() == "partSize must be positive (got 0)"
    assert _call(n_out=1 << 29) == UNSUPPORTED and "shard the rows" in _last()
    for name in ("x", "sum", "sumsq", "max", "argmax", "min", "argmin"):
        assert _call(**{name: F[7] + 2}) == INVALID and _last() == "feature, statistic and arg pointers must be 4-byte aligned", name
    for name, shown in (("sum", "sum"), ("sumsq", "sumsq"), ("max", "max_out"), ("argmax", "argmax"), ("min", "min_out"), ("argmin", "argmin")):
        assert _call(**{name: F[0]}) == INVALID and _last() == f"{shown} must not alias input", name
    assert _call(sumsq=F[1]) == INVALID and _last() == "sumsq must not alias sum"
    assert _call(min=F[3]) == INVALID and _last() == "min_out must not alias max_out"
    assert _call(argmin=F[4]) == INVALID and _last() == "argmin must not alias argmax"
    assert _call(argmax=F[1]) == INVALID and _last() == "argmax must not alias sum"
    assert _call(x=None) == INVALID and _last() == "null feature pointer"
    for name in ("ci", "pp", "p2n"):
        assert _call(**{name: None}) == INVALID and _last() == "null index pointer", name
    assert _call(n_out=0) == 0                                                # no destination row: nothing to write


def test_deterministic_tuning_refuses_the_moments_only():
    try:
        _lib.set_tuning(deterministic=1)
        for kw in ({}, dict(sumsq=None, max=None, argmax=None, min=None, argmin=None), dict(sum=None)):
            assert _call(**kw) == -3, kw
            assert _last() == "gnna_agg_stats_ld_f32 with sum or sumsq has no deterministic schedule (gnna_tuning.deterministic = 1): " \
                              "its sums meet through float atomics"
        # extrema alone pass this check (the next refusal is met instead: no device is touched here)
        assert _call(sum=None, sumsq=None, x=None) == -1 and _last() == "null feature pointer"
    finally:
        _lib.reset_tuning()
    assert _call(sum=None, sumsq=None, x=None) == -1 and _last() == "null feature pointer"


def test_the_wrappers():
    sig = inspect.signature(_lib.agg_stats_ld).parameters
    assert list(sig)[:7] == ["X", "column_index", "part_pointers", "part2Node", "num_out_rows", "partSize", "want"]
    assert sig["want"].default == ("sum", "sumsq", "max", "min") and sig["partSize"].default == 32
    import torch
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.agg_stats_ld(torch.zeros(2, 4), None, None, None, 2)
    from gnnadvisor_osdi21_amd import load_extension
    assert "(sum, sumsq, max, argmax, min, argmin)" in load_extension().aggregate_stats.__doc__


def test_the_layer_its_constructor_errors_and_the_dtypes_it_refuses():
    import types

    import torch
    from gnnadvisor_osdi21_amd import ops
    sig = inspect.signature(ops.PNAConv.__init__).parameters
    assert list(sig) == ["self", "input_dim", "output_dim", "aggregators", "scalers", "delta", "bias", "eps"]
    assert sig["aggregators"].default == ("mean", "max", "min", "std")
    assert sig["scalers"].default == ("identity", "amplification", "attenuation")
    assert sig["delta"].default is None and sig["bias"].default is False and sig["eps"].default == 1e-5
    assert list(inspect.signature(ops.PNAConv.forward).parameters) == ["self", "X", "inputInfo", "relu"]
    conv = ops.PNAConv(6, 5, bias=True)
    assert {n: tuple(q.shape) for n, q in conv.named_parameters()} == {"weights_self": (6, 5), "bias": (5,), "weights_scaler.0": (24, 5),
                                                                      "weights_scaler.1": (24, 5), "weights_scaler.2": (24, 5)}
    assert all(float(q.detach().abs().max()) <= 1 / 5 ** 0.5 for q in conv.parameters())
    assert torch.isnan(conv.delta) and "delta" in dict(conv.named_buffers())
    small = ops.PNAConv(6, 5, aggregators=("std", "max"), scalers=("attenuation",), delta=2.5)
    assert tuple(small.weights_scaler[0].shape) == (12, 5) and len(small.weights_scaler) == 1 and float(small.delta) == 2.5
    for kw, message in ((dict(aggregators=("mean", "var")), "aggregators must be distinct names among"),
                        (dict(aggregators=()), "aggregators must be distinct names among"),
                        (dict(aggregators=("max", "max")), "aggregators must be distinct names among"),
                        (dict(scalers=("identity", "linear")), "scalers must be distinct names among"),
                        (dict(scalers=()), "scalers must be distinct names among"),
                        (dict(delta=0.0), "delta must be positive"), (dict(delta=-1.0), "delta must be positive")):
        with pytest.raises(ValueError, match=message):
            ops.PNAConv(6, 5, **kw)
    info = types.SimpleNamespace(inv_row_counts=lambda: torch.tensor([1.0, 0.5, 0.25]))
    assert ops.PNAConv.delta_of(info) == pytest.approx(float(torch.log(torch.tensor([2.0, 3.0, 5.0])).mean()))
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="PNAConv computes in float32 only: 16-bit features and torch.autocast are not supported"):
            small(torch.zeros(3, 6, dtype=dtype), info)
        with pytest.raises(TypeError, match="NeighborStats computes in float32 only"):
            ops.NeighborStats.apply(torch.zeros(3, 6, dtype=dtype), info)
    with pytest.raises(ValueError, match="want must name some of"):
        ops.NeighborStats.apply(torch.zeros(3, 6), info, 1e-5, ("mean", "median"))
    doc = " ".join(ops.PNAConv.__doc__.split())
    assert "without PyG's pre-MLP" in doc and "The messages are the source features themselves" in doc
    assert "unit scale" in ops.NeighborStats.__doc__


def test_expected_aggregations_of_the_driver_model():
    from gnnadvisor_osdi21_amd import decider
    assert decider.expected_aggregations("pna", 100, 16, 10, epochs=7) == [(100, 7), (16, 7), (32, 7)]


@pytest.mark.parametrize("extra, message", [
    (["--dtype", "bfloat16"], "--dtype bfloat16: the PNA layers .* are float32 only; run --model pna with --dtype float32"),
    (["--dtype", "float16"], "run --model pna with --dtype float32"),
    (["--fanout", "5,5", "--hip_graph", "True"], "--fanout does not support --hip_graph True"),
    (["--fanout", "5"], "--fanout needs one entry per layer: --model pna has 2 layers \\(got 1\\)"),
    (["--fanout", "5,5", "--batch_size", "0"], "--batch_size must be >= 1"),
    (["--fused_attention", "True"], "run it with --model gat \\(got --model pna\\)"),
    (["--edge_dim", "4"], "run it with --model gat \\(got --model pna\\)"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    assert "pna" in driver.build_parser().format_help()
    with pytest.raises(SystemExit, match=message):
        driver.main(["--synthetic", "no-such-config", "--model", "pna"] + extra)

"""The attention readout, the parts that need no GPU (the binding surface of include/gnna_attnpool.h and the build lists are pinned
by test_binding_table_host.py): the refusals both entries make before any device work, the wrappers, the ops' refusals and the
driver's new flag."""
import ctypes
import inspect

import pytest
import torch

from gnnadvisor_osdi21_amd import _lib

FWD, BWD = "gnna_segment_attn_pool_ld_f32", "gnna_segment_attn_pool_backward_ld_f32"


_B = [(ctypes.c_float * 64)() for _ in range(12)]
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = [ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p).value for _ in range(2)]


def _fwd(**kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(x=F[0], ld_in=8, n=6, gate=F[1], ld_gate=8, gate_dim=4, gp=I[0], g=2, out=F[2], ld_out=8, lse=F[3], ld_lse=8, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_attn_pool_ld_f32(a["x"], a["ld_in"], a["n"], a["gate"], a["ld_gate"], a["gate_dim"], a["gp"], a["g"],
                                                     a["out"], a["ld_out"], a["lse"], a["ld_lse"], a["dim"], a["flags"], None)


def _bwd(**kw):
    a = dict(x=F[0], ld_in=8, gate=F[1], ld_gate=8, gate_dim=4, lse=F[3], ld_lse=8, y=F[2], ld_y=8, dy=F[4], ld_dy=8, gp=I[0], g=2,
             dx=F[5], ld_din=8, dg=F[6], ld_dgate=8, n=6, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_segment_attn_pool_backward_ld_f32(a["x"], a["ld_in"], a["gate"], a["ld_gate"], a["gate_dim"], a["lse"],
                                                              a["ld_lse"], a["y"], a["ld_y"], a["dy"], a["ld_dy"], a["gp"], a["g"],
                                                              a["dx"], a["ld_din"], a["dg"], a["ld_dgate"], a["n"], a["dim"], a["flags"],
                                                              None)


def _last():
    return _lib.load().gnna_last_error().decode()


INVALID, UNSUPPORTED = -1, -3                                                # include/gnna.h


@pytest.mark.parametrize("call, name", [(_fwd, FWD), (_bwd, BWD)], ids=["forward", "backward"])
def test_refusals_both_entries_make_alike(call, name):
    for flags in (1, 2, 0x80000000):
        assert call(flags=flags) == INVALID and _last() == f"{name} takes no flags (got 0x{flags:x})"
    assert call(dim=0, gate_dim=1) == INVALID and _last() == f"{name}: dim must be >= 1 (got 0)"
    assert call(dim=-3) == INVALID and _last() == f"{name}: dim must be >= 1 (got -3)"
    assert call(gate_dim=2) == INVALID and _last() == f"{name}: gate_dim must be 1 or dim = 4 (got 2)"
    for gate_dim in (0, -1, 5):
        assert call(gate_dim=gate_dim) == INVALID and _last() == f"{name}: gate_dim must be 1 or dim = 4 (got {gate_dim})"
    assert call(n=-1) == INVALID and _last() == f"{name}: negative size (num_rows=-1 num_segments=2)"
    assert call(g=-2) == INVALID and _last() == f"{name}: negative size (num_rows=6 num_segments=-2)"
    assert call(g=1 << 29) == UNSUPPORTED and _last() == f"{name}: 536870912 segments in one call (at most 536870911): shard the batch"
    assert call(n=1 << 31) == UNSUPPORTED and _last() == f"{name}: 2147483648 rows in one call (at most 2147483647: graph_pointers is int32)"
    for ptr in ("x", "gate", "gp"):
        assert call(**{ptr: F[7] + 2}) == INVALID and "must be 4-byte aligned" in _last() and _last().startswith(name + ": "), ptr
    assert call(gp=None) == INVALID and _last() == f"{name}: null graph_pointers"
    # the gate's stride is checked against gate_dim: 1 is wide enough for a score per row, not for one per element
    assert call(ld_gate=3) == INVALID and "row strides must be >= the width they stride and < 2^29 elements" in _last() and "ld_gate=3" in _last()
    assert call(gate_dim=1, ld_gate=1, ld_lse=1, ld_dgate=1, gp=None) == INVALID and _last() == f"{name}: null graph_pointers"
    # input and gate may be one pointer
    assert call(gate=F[0], gp=None) == INVALID and _last() == f"{name}: null graph_pointers"


def test_refusals_of_the_forward_entry():
    for ld in ("ld_in", "ld_gate", "ld_out", "ld_lse"):
        assert _fwd(**{ld: 3}) == INVALID and _last().startswith(FWD + ": row strides must be >= the width they stride and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
        assert _fwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    # (a null lse's stride strides nothing: the call gets past the stride check to the next refusal)
    assert _fwd(lse=None, ld_lse=3, x=None) == INVALID and _last() == FWD + ": null feature pointer"
    for name in ("out", "lse"):
        assert _fwd(**{name: F[7] + 2}) == INVALID and _last() == FWD + ": feature, gate, pointer and output pointers must be 4-byte aligned"
        for inp in (F[0], F[1], I[0]):
            assert _fwd(**{name: inp}) == INVALID and _last() == FWD + ": an output must not alias an input", name
    assert _fwd(out=F[8], lse=F[8]) == INVALID and _last() == FWD + ": the outputs must not alias each other"
    assert _fwd(out=None) == INVALID and _last() == FWD + ": null output pointer (out is always written)"
    assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
    assert _fwd(gate=None) == INVALID and _last() == FWD + ": null gate pointer"
    assert _fwd(g=0) == 0                                                     # no graph: nothing to write
    assert _fwd(g=0, gp=None, x=None, gate=None, out=None, lse=None) == 0


def test_refusals_of_the_backward_entry():
    for ld in ("ld_in", "ld_gate", "ld_lse", "ld_y", "ld_dy", "ld_din", "ld_dgate"):
        assert _bwd(**{ld: 3}) == INVALID and _last().startswith(BWD + ": row strides must be >= the width they stride and < 2^29 elements (") \
            and f"{ld}=3" in _last(), ld
        assert _bwd(**{ld: 1 << 29}) == INVALID and f"{ld}=536870912" in _last(), ld
    assert _bwd(dx=None, ld_din=3, gp=None) == INVALID and _last() == BWD + ": null graph_pointers"
    assert _bwd(dg=None, ld_dgate=3, gp=None) == INVALID and _last() == BWD + ": null graph_pointers"
    for name in ("lse", "y", "dy", "dx", "dg"):
        assert _bwd(**{name: F[7] + 2}) == INVALID and _last() == BWD + ": feature, gate, lse, gradient and pointer pointers must be 4-byte aligned"
    for name in ("dx", "dg"):
        for inp in (F[0], F[1], F[2], F[3], F[4], I[0]):
            assert _bwd(**{name: inp}) == INVALID and _last() == BWD + ": an output must not alias an input", name
    assert _bwd(dx=F[8], dg=F[8]) == INVALID and _last() == BWD + ": the outputs must not alias each other"
    assert _bwd(dx=None, dg=None) == INVALID and _last() == BWD + ": null output pointers: d_input and d_gate are both null"
    assert _bwd(x=None) == INVALID and _last() == BWD + ": null feature or gate pointer"
    assert _bwd(gate=None) == INVALID and _last() == BWD + ": null feature or gate pointer"
    for name in ("lse", "y", "dy"):
        assert _bwd(**{name: None}) == INVALID and _last() == BWD + ": null lse, Y or dY pointer", name
    assert _bwd(n=0) == 0                                                     # no row: nothing to write
    assert _bwd(n=0, dx=None, dg=None, x=None, gate=None) == 0


def test_deterministic_tuning_does_not_refuse_the_entries():
    try:
        _lib.set_tuning(deterministic=1)
        # (the next refusal is met instead of GNNA_ERR_UNSUPPORTED: no device is touched here)
        assert _fwd(x=None) == INVALID and _last() == FWD + ": null feature pointer"
        assert _bwd(x=None) == INVALID and _last() == BWD + ": null feature or gate pointer"
    finally:
        _lib.reset_tuning()


def test_the_wrappers_and_the_ops():
    sig = inspect.signature(_lib.segment_attn_pool).parameters
    assert list(sig) == ["X", "gate", "graph_pointers", "out"] and sig["out"].default is None
    sig = inspect.signature(_lib.segment_attn_pool_backward).parameters
    assert list(sig) == ["X", "gate", "lse", "Y", "dY", "graph_pointers", "need_input", "need_gate", "out"]
    assert sig["need_input"].default is True and sig["need_gate"].default is True and sig["out"].default is None
    assert FWD in _lib.segment_attn_pool.__doc__ and BWD in _lib.segment_attn_pool_backward.__doc__
    gp = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.segment_attn_pool(torch.zeros(2, 4), torch.zeros(2), gp)
    with pytest.raises(_lib.GnnaError, match="needs device tensors"):
        _lib.segment_attn_pool_backward(torch.zeros(2, 4), torch.zeros(2), torch.zeros(2, 1), torch.zeros(2, 4), torch.zeros(2, 4), gp)
    with pytest.raises(ValueError, match="needs need_input or need_gate"):
        _lib.segment_attn_pool_backward(torch.zeros(2, 4), torch.zeros(2), torch.zeros(2, 1), torch.zeros(2, 4), torch.zeros(2, 4), gp,
                                        need_input=False, need_gate=False)
    from gnnadvisor_osdi21_amd import load_extension, ops
    GNNA = load_extension()
    assert "(out [num_graphs, dim], lse [num_graphs, gate_dim])" in GNNA.segment_attn_pool.__doc__
    assert "graph_pointers" in GNNA.segment_attn_pool.__doc__ and "row of no graph" in GNNA.segment_attn_pool_backward.__doc__
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="SegmentAttentionPool computes in float32 only: 16-bit features and torch.autocast are not supported"):
            ops.global_attention_pool(torch.zeros(3, 6, dtype=dtype), torch.zeros(3, dtype=dtype), gp)
        with pytest.raises(TypeError, match="SegmentAttentionPool computes in float32 only"):
            ops.SegmentAttentionPool.apply(torch.zeros(3, 6), torch.zeros(3, 6, dtype=dtype), gp)
        for fused in (True, False):
            with pytest.raises(TypeError, match="AttentionalReadout computes in float32 only"):
                ops.AttentionalReadout(torch.nn.Linear(6, 1).to(dtype), fused=fused)(torch.zeros(3, 6, dtype=dtype), gp)
    with pytest.raises(TypeError, match="an unsorted `batch` vector is not supported"):
        ops.global_attention_pool(torch.zeros(3, 6), torch.zeros(3), torch.zeros(3, dtype=torch.int64))
    for shape in ((3, 2), (4,), (3, 6, 1)):
        with pytest.raises(ValueError, match="gate must be \\[rows\\], \\[rows, 1\\] or \\[rows, F\\]"):
            ops.global_attention_pool(torch.zeros(3, 6), torch.zeros(shape), gp)
    readout = ops.AttentionalReadout(torch.nn.Linear(6, 1))
    assert readout.fused is True and readout.nn is None and len(list(readout.parameters())) == 2
    assert "no [N, F] temporary" in " ".join(ops.SegmentAttentionPool.__doc__.split())
    assert "timing baseline" in " ".join(ops.AttentionalReadout.__doc__.split())
    assert ops.POOL_MODES == ("sum", "mean", "max", "min") and _lib.POOL_STATS == ("sum", "max", "min")


@pytest.mark.parametrize("value", ["vector", "", "Scalar", "scalar,channel"])
def test_the_driver_refuses_an_unknown_attention_readout(value):
    from gnnadvisor_osdi21_amd import graph_main as driver
    text = driver.build_parser().format_help()
    assert "--attention_readout" in text and "none, scalar or channel" in text and "--readout" in text
    assert driver.build_parser().parse_args([]).attention_readout == "none"
    with pytest.raises(SystemExit) as refusal:
        driver.main(["--attention_readout", value])
    assert str(refusal.value) == "--attention_readout takes none, scalar or channel (got %r)" % value

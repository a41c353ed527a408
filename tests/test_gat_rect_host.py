"""The rectangular fused GAT attention as the host sees it (no GPU): the two symbols and their argument types, the header's
signatures, the version, the wrappers' refusals, the driver's flags."""
import ctypes
import os
import re

import pytest
import torch

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnna_gat_forward_rect_f32", "gnna_gat_backward_rect_f32")


def _squash(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    # the square argument lists with num_nodes replaced by (num_out_rows, num_in_rows)
    sq, rect = lib.gnna_gat_forward_f32.argtypes, lib.gnna_gat_forward_rect_f32.argtypes
    assert len(rect) == len(sq) + 1 and rect[:12] == sq[:12] and rect[12:14] == [i64, i64] and rect[14:] == sq[13:]
    sq, rect = lib.gnna_gat_backward_dir_f32.argtypes, lib.gnna_gat_backward_rect_f32.argtypes
    assert len(rect) == len(sq) + 1 and rect[:24] == sq[:24] and rect[24:26] == [i64, i64] and rect[26:] == sq[25:]
    assert rect[9:14] == rect[14:19] == [p, p, p, p, i64] and rect[26:29] == [i, i, i]
    assert lib.gnna_gat_forward_rect_f32.restype is i and lib.gnna_gat_backward_rect_f32.restype is i


def test_version_is_still_601():
    assert _lib.load().gnna_version() == 601
    assert "#define GNNA_VERSION 601" in open(os.path.join(ROOT, "include", "gnna.h")).read()


def test_header_declares_the_entries_with_the_contract_signatures():
    flat = _squash(open(os.path.join(ROOT, "include", "gnna.h")).read())
    assert ("GNNA_API int gnna_gat_forward_rect_f32(const float *H, int64_t ld_h, const float *el, const float *er, "
            "const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, "
            "float negative_slope, float *out, int64_t ld_out, float *lse, "
            "int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize, "
            "unsigned flags, void *stream);") in flat
    assert ("GNNA_API int gnna_gat_backward_rect_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse, "
            "const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy, "
            "const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, "
            "int64_t num_parts, "
            "const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node, "
            "int64_t t_num_parts, "
            "float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, "
            "int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags, void *stream);") in flat


def test_wrappers_refuse_cpu_tensors():
    H, er, el = torch.zeros(6, 8), torch.zeros(6, 2), torch.zeros(4, 2)
    Y = torch.zeros(4, 8)
    rp, i = torch.zeros(5, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError, match="device tensors"):
        _lib.gat_forward(H, el, er, rp, i, i, i)
    with pytest.raises(_lib.GnnaError, match="device tensors"):
        _lib.gat_backward(H, el, er, el, Y, Y, rp, i, i, i)
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        GNNA.gat_forward(H, el, er, rp, i, i, i, 32, 0.2)
    with pytest.raises(RuntimeError):
        GNNA.gat_backward(H, el, er, el, Y, Y, rp, i, i, i, 32, 0.2, None)


def test_size_rule_of_the_wrappers_raises_on_mismatched_shapes():
    """_lib._gat_sizes is what gat_forward / gat_backward read the two row counts with, before any device work (the tensors here
    are host tensors: only their shapes are looked at)."""
    H, er, el = torch.zeros(6, 8), torch.zeros(6, 2), torch.zeros(4, 2)
    rp = torch.zeros(5, dtype=torch.int32)
    assert _lib._gat_sizes(H, el, er, rp)[1:5] == (4, 6, 8, 2)            # num_out_rows, num_in_rows, width, heads
    with pytest.raises(AssertionError, match="row_pointers"):
        _lib._gat_sizes(H, el, er, torch.zeros(7, dtype=torch.int32))     # num_out_rows is el's and row_pointers'
    with pytest.raises(AssertionError):
        _lib._gat_sizes(H, el, torch.zeros(4, 2), rp)                     # er has H's rows
    with pytest.raises(AssertionError):
        _lib._gat_sizes(H, torch.zeros(4, 3), er, rp)                     # one head count
    with pytest.raises(AssertionError):
        _lib._gat_sizes(torch.zeros(6, 7), el, er, rp)                    # width = heads * dim


def test_driver_parses_gat_on_blocks():
    from gnnadvisor_osdi21_amd import main as driver
    args = driver.build_parser().parse_args(["--model", "gat", "--fused_attention", "True", "--fanout", "5,5"])
    assert (args.model, args.fused_attention, args.fanout) == ("gat", "True", "5,5")


@pytest.mark.parametrize("extra, message", [
    (["--model", "gat"], "fused_attention"),
    (["--model", "gat", "--fused_attention", "False"], "fused_attention"),
    (["--model", "gin"], "--model sage"),
    (["--model", "gat", "--fused_attention", "True", "--hip_graph", "True"], "hip_graph"),
    (["--model", "gat", "--fused_attention", "True", "--dtype", "float16"], "float32"),
    (["--model", "gat", "--fused_attention", "True", "--single_spmm", "True"], "--single_spmm"),
    (["--model", "gat", "--fused_attention", "True", "--verify_spmm", "True"], "--verify_spmm"),
    (["--model", "gat", "--fused_attention", "True", "--fanout", "5"], "one entry per layer"),
])
def test_driver_refusals_with_fanout(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    with pytest.raises(SystemExit, match=message):
        driver.main(["--fanout", "5,5", "--synthetic", "no-such-config"] + extra)

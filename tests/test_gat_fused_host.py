"""The fused GAT attention as the host sees it (no GPU): the two symbols, their Python wrappers, the header's signatures, the
build lists, the driver's flag and refusals, and the cached symmetry check in decider.py."""
import os
import re

import pytest
import torch

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _squash(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_library_exports_the_entries_and_lib_wraps_them():
    lib = _lib.load()
    for name in ("gnna_gat_forward_f32", "gnna_gat_backward_f32"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(_lib.gat_forward) and callable(_lib.gat_backward)
    assert lib.gnna_version() == 601


def test_header_declares_the_entries_with_the_contract_signatures():
    text = open(os.path.join(ROOT, "include", "gnna.h")).read()
    assert "#define GNNA_VERSION 601" in text
    flat = _squash(text)
    assert ("GNNA_API int gnna_gat_forward_f32(const float *H, int64_t ld_h, const float *el, const float *er, "
            "const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, "
            "float negative_slope, float *out, int64_t ld_out, float *lse, int64_t num_nodes, int heads, int dim, "
            "int64_t num_parts, int partSize, unsigned flags, void *stream);") in flat
    assert ("GNNA_API int gnna_gat_backward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse, "
            "const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy, "
            "const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, "
            "float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_nodes, int heads, int dim, "
            "int64_t num_parts, int partSize, unsigned flags, void *stream);") in flat


def test_build_lists_name_the_new_source():
    from gnnadvisor_osdi21_amd import build
    assert any(p.endswith("gnna_gat.hip") for p in build.LIB_SOURCES)
    assert any(p.endswith("gnna_gat.hip") for p in build.LIB_DEPS)          # so source_hash covers it
    assert "gnna_gat.hip" in open(os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc", "Makefile")).read()


def test_wrappers_refuse_cpu_tensors():
    H = torch.zeros(4, 8)
    e = torch.zeros(4, 2)
    i = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError):
        _lib.gat_forward(H, e, e, i, i, i, i)
    with pytest.raises(_lib.GnnaError):
        _lib.gat_backward(H, e, e, e, H, H, i, i, i, i)


def test_driver_parser_and_refusals():
    from gnnadvisor_osdi21_amd import main as driver
    assert driver.build_parser().parse_args([]).fused_attention == "False"
    args = driver.build_parser().parse_args(["--model", "gat", "--fused_attention", "True", "--heads", "2"])
    assert (args.model, args.fused_attention, args.heads) == ("gat", "True", 2)
    with pytest.raises(SystemExit):
        driver.build_parser().parse_args(["--model", "gat", "--fused_attention", "maybe"])
    with pytest.raises(SystemExit, match="fused_attention"):
        driver.main(["--synthetic", "cora-like", "--model", "gcn", "--fused_attention", "True"])
    with pytest.raises(SystemExit, match="hip_graph"):
        driver.main(["--synthetic", "cora-like", "--model", "gat", "--fused_attention", "True", "--hip_graph", "True"])
    with pytest.raises(SystemExit, match="dtype"):
        driver.main(["--synthetic", "cora-like", "--model", "gat", "--fused_attention", "True", "--dtype", "bfloat16"])


def test_gatconv_takes_the_fused_keyword_and_defaults_to_the_composed_path():
    import inspect
    from gnnadvisor_osdi21_amd import ops
    assert inspect.signature(ops.GATConv.__init__).parameters["fused"].default is False
    assert ops.GATConv(8, 4, heads=2).fused is False and ops.GATConv(8, 4, heads=2, fused=True).fused is True
    assert issubclass(ops.GATAttention, torch.autograd.Function)
    assert callable(ops.GNNA.gat_forward) and callable(ops.GNNA.gat_backward)


def test_require_symmetric_caches_the_answer_and_keeps_no_edge_array():
    from gnnadvisor_osdi21_amd.decider import inputProperty
    # symmetric: 0 - 1, 0 - 2, 2 - 2 (self loop), node 3 isolated
    rp = torch.tensor([0, 2, 3, 5, 5], dtype=torch.int32)
    ci = torch.tensor([1, 2, 0, 0, 2], dtype=torch.int32)
    info = inputProperty.__new__(inputProperty)
    info.row_pointers, info.column_index = rp, ci
    info.require_symmetric()
    cache = info._edge_arrays()
    assert cache.get("symmetric") is True and "rev" not in cache and "rows" not in cache
    info.require_symmetric()                                  # answered from the cache
    # directed: 0 <- 1 only
    bad = inputProperty.__new__(inputProperty)
    bad.row_pointers = torch.tensor([0, 1, 1], dtype=torch.int32)
    bad.column_index = torch.tensor([1], dtype=torch.int32)
    with pytest.raises(_lib.GnnaError):
        bad.require_symmetric()
    with pytest.raises(_lib.GnnaError):                       # a refusal is not cached as a pass
        bad.require_symmetric()

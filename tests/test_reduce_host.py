"""The max / min neighbor reduction as the host sees it (no GPU): the two symbols, their Python wrappers, the header's
constants and signatures, the build lists, the driver's flags and refusals, and the helpers in decider.py."""
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
    for name in ("gnna_agg_reduce_ld_f32", "gnna_scatter_arg_ld_f32"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(_lib.agg_reduce_ld) and callable(_lib.scatter_arg_ld)
    assert (_lib.REDUCE_MAX, _lib.REDUCE_MIN) == (0, 1)
    assert lib.gnna_version() == 601


def test_header_declares_the_entries_with_the_contract_signatures():
    text = open(os.path.join(ROOT, "include", "gnna.h")).read()
    assert re.search(r"#define GNNA_REDUCE_MAX 0\b", text) and re.search(r"#define GNNA_REDUCE_MIN 1\b", text)
    assert "#define GNNA_VERSION 601" in text
    flat = _squash(text)
    assert ("GNNA_API int gnna_agg_reduce_ld_f32(int op, const float *input, int64_t ld_in, int64_t num_in_rows, "
            "const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out, "
            "int32_t *arg , int64_t ld_arg, int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags, "
            "void *stream);") in flat
    assert ("GNNA_API int gnna_scatter_arg_ld_f32(const float *grad_out, int64_t ld_go, const int32_t *arg, int64_t ld_arg, "
            "const int32_t *column_index, int64_t num_out_rows, float *grad_in, int64_t ld_gi, int64_t num_in_rows, int dim, "
            "unsigned flags, void *stream);") in flat


def test_build_lists_name_the_new_source():
    from gnnadvisor_osdi21_amd import build
    assert any(p.endswith("gnna_reduce.hip") for p in build.LIB_SOURCES)
    assert "gnna_reduce.hip" in open(os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc", "Makefile")).read()


def test_wrappers_refuse_cpu_tensors():
    z = torch.zeros(4, 8)
    i = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError):
        _lib.agg_reduce_ld(_lib.REDUCE_MAX, z, i, i, i, 4)
    with pytest.raises(_lib.GnnaError):
        _lib.scatter_arg_ld(z, torch.zeros(4, 8, dtype=torch.int32), i, 4)


def test_driver_parser_and_refusal():
    from gnnadvisor_osdi21_amd import main as driver
    args = driver.build_parser().parse_args(["--model", "sage", "--aggregator", "max"])
    assert (args.model, args.aggregator) == ("sage", "max")
    assert driver.build_parser().parse_args([]).aggregator == "mean"
    assert driver.build_parser().parse_args(["--model", "sage"]).aggregator == "mean"
    with pytest.raises(SystemExit):
        driver.build_parser().parse_args(["--model", "sage", "--aggregator", "median"])
    with pytest.raises(SystemExit, match="dtype"):
        driver.main(["--synthetic", "cora-like", "--model", "sage", "--dtype", "bfloat16"])


def test_inv_row_counts_on_a_graph_with_an_isolated_node():
    from gnnadvisor_osdi21_amd.decider import inputProperty
    # rows: 0 -> {1, 2, 3}, 1 -> {0}, 2 -> {} (isolated), 3 -> {0, 1}
    rp = torch.tensor([0, 3, 4, 4, 6], dtype=torch.int32)
    ci = torch.tensor([1, 2, 3, 0, 0, 1], dtype=torch.int32)
    info = inputProperty.__new__(inputProperty)
    info.row_pointers, info.column_index = rp, ci
    inv = info.inv_row_counts()
    assert inv.dtype == torch.float32
    assert torch.equal(inv, torch.tensor([1 / 3, 1.0, 1.0, 0.5], dtype=torch.float32))
    assert info.inv_row_counts() is inv                       # cached per column_index
    info.column_index = ci.clone()                            # another CSR: rebuilt
    assert info.inv_row_counts() is not inv


def test_expected_aggregations_of_the_sage_models():
    from gnnadvisor_osdi21_amd.decider import expected_aggregations
    # Reddit shape, 10 steps.  mean: layer 1 narrows 602 -> 64 (10 sweeps against 1) and runs update-first: forward and backward
    # at 64; layer 2 (64 -> 41, one sweep either way) aggregates X at 64, forward and backward.
    assert expected_aggregations("sage", 602, 64, 41, 10, aggregator="mean") == [(64, 20), (64, 20)]
    assert expected_aggregations("sage", 602, 64, 41, 10) == [(64, 20), (64, 20)]
    # a widening first layer (16 -> 256): aggregate X at 16, forward only (the features need no gradient); layer 2 narrows
    # 256 -> 7: 2 * 1 < 2 * 4, update-first at 7
    assert expected_aggregations("sage", 16, 256, 7, 10, aggregator="mean") == [(16, 10), (7, 20)]
    # max / min: one gather per layer and step at the layer's input width (the backward is not a gather)
    assert expected_aggregations("sage", 602, 64, 41, 10, aggregator="max") == [(602, 10), (64, 10)]
    assert expected_aggregations("sage", 602, 64, 41, 10, aggregator="min") == [(602, 10), (64, 10)]
    # the existing models are untouched by the new argument
    assert expected_aggregations("gcn", 602, 64, 41, 10) == [(64, 20), (41, 20)]

"""The 16-bit aggregation entry as the host sees it (no GPU): the symbol, its Python wrapper, the header's constants and the
driver's refusals."""
import os
import re

import pytest

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_x16_entry_and_lib_wraps_it():
    lib = _lib.load()
    for name in ("gnna_agg_ld_x16", "gnna_prepare_x16"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(_lib.agg_ld_x16) and callable(_lib.prepare_x16)
    assert (_lib.F32, _lib.BF16, _lib.F16) == (0, 1, 2)


def test_header_declares_the_entry_and_the_type_codes():
    text = open(os.path.join(ROOT, "include", "gnna.h")).read()
    for name, value in (("GNNA_F32", 0), ("GNNA_BF16", 1), ("GNNA_F16", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), text)
    assert re.search(r"GNNA_API int gnna_agg_ld_x16\(int mode, int in_type, const void \*input, int64_t ld_in", text)
    assert "#define GNNA_VERSION 601" in text and _lib.load().gnna_version() == 601


def test_build_lists_name_the_new_source():
    from gnnadvisor_osdi21_amd import build
    assert any(p.endswith("gnna_x16.hip") for p in build.LIB_SOURCES)
    assert "gnna_x16.hip" in open(os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc", "Makefile")).read()


def test_wrapper_refuses_float32_and_cpu_tensors():
    import torch
    z = torch.zeros(4, 8)
    i = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError):
        _lib.agg_ld_x16(0, z.bfloat16(), i, i, i, 4)        # no CPU path


@pytest.mark.parametrize("extra", [["--model", "gat"], ["--hip_graph", "True"]])
def test_driver_refuses_what_the_16_bit_path_does_not_cover(extra):
    from gnnadvisor_osdi21_amd import main as driver
    with pytest.raises(SystemExit, match="dtype"):
        driver.main(["--synthetic", "cora-like", "--dtype", "bfloat16"] + extra)
    args = driver.build_parser().parse_args([])
    assert args.dtype == "float32"

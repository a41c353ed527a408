"""The relation-typed aggregation as the host sees it (no GPU): the three symbols, the header, the build lists, the argument
validation that returns before any device work, RGCNConv's constructor and the driver's refusals."""
import ctypes
import os
import re

import pytest
import torch

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnna_agg_typed_expand_ld_f32", "gnna_agg_typed_contract_ld_f32", "gnna_typed_coef_grad_ld_f32")
INVALID, UNSUPPORTED = -1, -3


def test_library_exports_the_three_entries_and_the_header_declares_them():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gnna.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
        assert re.search(r"GNNA_API\s+int\s+%s\s*\(" % name, header), name
    assert callable(_lib.agg_typed_expand) and callable(_lib.agg_typed_contract) and callable(_lib.typed_coef_grad)
    assert lib.gnna_version() == 601


def test_build_lists_name_the_new_source():
    from gnnadvisor_osdi21_amd import build
    assert any(p.endswith("gnna_typed.hip") for p in build.LIB_SOURCES)
    assert any(p.endswith("gnna_typed.hip") for p in build.LIB_DEPS)
    assert "gnna_typed.hip" in open(os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc", "Makefile")).read()


# Host buffers stand in for device memory: every call below must return before it touches the device or its arguments' contents.
_F = (ctypes.c_float * 64)()
_F2 = (ctypes.c_float * 64)()
_F3 = (ctypes.c_float * 64)()
_I = (ctypes.c_int32 * 64)()


def _p(buf):
    return ctypes.cast(buf, ctypes.c_void_p).value


def _expand(**kw):
    a = dict(X=_p(_F), ld_x=4, n_in=2, col=_p(_I), ety=_p(_I), enorm=None, coef=_p(_F2), R=3, B=2, pp=_p(_I), p2n=_p(_I),
             out=_p(_F3), ld_out=8, n_out=2, dim=4, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_typed_expand_ld_f32(a["X"], a["ld_x"], a["n_in"], a["col"], a["ety"], a["enorm"], a["coef"], a["R"],
                                                    a["B"], a["pp"], a["p2n"], a["out"], a["ld_out"], a["n_out"], a["dim"], a["P"],
                                                    a["ps"], a["flags"], None)


def _contract(**kw):
    a = dict(G=_p(_F), ld_g=8, n_in=2, col=_p(_I), ety=_p(_I), enorm=None, coef=_p(_F2), R=3, B=2, pp=_p(_I), p2n=_p(_I),
             out=_p(_F3), ld_out=4, n_out=2, dim=4, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_typed_contract_ld_f32(a["G"], a["ld_g"], a["n_in"], a["col"], a["ety"], a["enorm"], a["coef"], a["R"],
                                                      a["B"], a["pp"], a["p2n"], a["out"], a["ld_out"], a["n_out"], a["dim"], a["P"],
                                                      a["ps"], a["flags"], None)


def _coef_grad(**kw):
    a = dict(X=_p(_F), ld_x=4, n_in=2, G=_p(_F2), ld_g=8, n_out=2, col=_p(_I), ety=_p(_I), enorm=None, pp=_p(_I), p2n=_p(_I),
             dcoef=_p(_F3), R=3, B=2, dim=4, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_typed_coef_grad_ld_f32(a["X"], a["ld_x"], a["n_in"], a["G"], a["ld_g"], a["n_out"], a["col"], a["ety"],
                                                   a["enorm"], a["pp"], a["p2n"], a["dcoef"], a["R"], a["B"], a["dim"], a["P"],
                                                   a["ps"], a["flags"], None)


@pytest.mark.parametrize("call", [_expand, _contract, _coef_grad], ids=["expand", "contract", "coef_grad"])
def test_sizes_are_validated_before_any_device_work(call):
    err = lambda: _lib.load().gnna_last_error().decode()
    assert call(B=0) == INVALID and "num_bases" in err()
    assert call(B=17) == UNSUPPORTED and "bases" in err()
    assert call(R=0) == INVALID and "num_types" in err()
    assert call(dim=0) == INVALID
    assert call(ps=0) == INVALID and "partSize" in err()
    assert call(n_in=-1) == INVALID and call(n_out=-1) == INVALID and call(P=-1) == INVALID
    assert call(flags=2) == INVALID                                  # GNNA_EPILOGUE_RELU is not accepted
    assert call(col=None) == INVALID and call(ety=None) == INVALID and call(pp=None) == INVALID and call(p2n=None) == INVALID


def test_leading_dimensions_null_pointers_aliasing_and_flags():
    err = lambda: _lib.load().gnna_last_error().decode()
    # a leading dimension below the row width: dim for X / the contracted output, num_bases * dim for the wide side
    assert _expand(ld_x=3) == INVALID and "row strides" in err()
    assert _expand(ld_out=7) == INVALID
    assert _contract(ld_g=7) == INVALID and _contract(ld_out=3) == INVALID
    assert _coef_grad(ld_x=3) == INVALID and _coef_grad(ld_g=7) == INVALID
    # null pointers
    assert _expand(X=None) == INVALID and "null" in err()
    assert _expand(coef=None) == INVALID and _expand(out=None) == INVALID
    assert _contract(G=None) == INVALID and _contract(coef=None) == INVALID and _contract(out=None) == INVALID
    assert _coef_grad(X=None) == INVALID and _coef_grad(G=None) == INVALID and _coef_grad(dcoef=None) == INVALID
    # an output that is one of the inputs
    assert _expand(out=_p(_F)) == INVALID and "alias" in err()
    assert _expand(out=_p(_F2)) == INVALID
    assert _expand(out=_p(_F3), enorm=_p(_F3)) == INVALID
    assert _contract(out=_p(_F)) == INVALID and _contract(out=_p(_F2)) == INVALID
    assert _coef_grad(dcoef=_p(_F)) == INVALID and _coef_grad(dcoef=_p(_F2)) == INVALID
    # GNNA_ACCUMULATE: the coefficient gradient only
    assert _expand(flags=1) == UNSUPPORTED and "GNNA_ACCUMULATE" in err()
    assert _contract(flags=1) == UNSUPPORTED


def test_wrappers_refuse_cpu_tensors():
    X, C = torch.zeros(4, 8), torch.zeros(3, 2)
    i = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError):
        _lib.agg_typed_expand(X, C, i, i, None, i, i, 4)
    with pytest.raises(_lib.GnnaError):
        _lib.agg_typed_contract(X, C, i, i, None, i, i, 4)
    with pytest.raises(_lib.GnnaError):
        _lib.typed_coef_grad(X, X, i, i, None, i, i, 3)


def test_rgcnconv_constructor():
    from gnnadvisor_osdi21_amd import ops
    with pytest.raises(ValueError, match="num_bases"):
        ops.RGCNConv(8, 4, num_relations=17, num_bases=None)
    with pytest.raises(ValueError, match="num_bases"):
        ops.RGCNConv(8, 4, num_relations=3, num_bases=17)
    plain = ops.RGCNConv(8, 4, num_relations=16)
    assert not isinstance(plain.coef, torch.nn.Parameter) and torch.equal(plain.coef, torch.eye(16))
    assert tuple(plain.V.shape) == (16, 8, 4) and "coef" not in dict(plain.named_parameters())
    based = ops.RGCNConv(8, 4, num_relations=40, num_bases=3, bias=False, self_loop=False)
    assert isinstance(based.coef, torch.nn.Parameter) and tuple(based.coef.shape) == (40, 3)
    assert tuple(based.V.shape) == (3, 8, 4) and based.W_self is None and based.bias is None
    assert issubclass(ops.TypedAggregate, torch.autograd.Function)


def test_expected_aggregations_has_an_rgcn_entry():
    from gnnadvisor_osdi21_amd.decider import expected_aggregations
    got = expected_aggregations("rgcn", 96, 16, 10, epochs=5, num_relations=8, num_bases=4)
    assert {w for w, _ in got} == {96, 16, 4 * 16} and all(k > 0 for _, k in got)
    assert dict(expected_aggregations("rgcn", 96, 16, 10, epochs=5, num_relations=8))[8 * 16] == 5


def test_driver_parser_and_refusals():
    from gnnadvisor_osdi21_amd import main as driver
    args = driver.build_parser().parse_args(["--model", "rgcn", "--num_relations", "6", "--num_bases", "2"])
    assert (args.model, args.num_relations, args.num_bases) == ("rgcn", 6, 2)
    assert driver.build_parser().parse_args(["--model", "rgcn"]).num_bases == 0
    base = ["--synthetic", "cora-like", "--model", "rgcn"]
    with pytest.raises(SystemExit, match="--model rgcn does not support --hip_graph True"):
        driver.main(base + ["--hip_graph", "True"])
    with pytest.raises(SystemExit, match="--fanout.*--model rgcn"):
        driver.main(base + ["--fanout", "5,5"])
    with pytest.raises(SystemExit, match="--dtype bfloat16.*float32 only"):
        driver.main(base + ["--dtype", "bfloat16"])
    with pytest.raises(SystemExit, match="num_bases"):
        driver.main(base + ["--num_relations", "17"])

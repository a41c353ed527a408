"""The binding surface of ``_lib`` (no GPU), in one place: for every public header of ``include/``, the entries it declares, its
table in ``_lib.HEADERS`` and its record ``tests/abi/<header>.json`` name the same entries, and restype and argtypes of every entry
-- in the table and as ``load()`` leaves them on the loaded library -- are the recorded ones.  A wrong argtype does not fail loudly
-- a 64-bit count passed as c_int is truncated, a float passed as an integer is garbage -- so every table is pinned as a whole.  The
gnna.h record was taken from the hand-written assignments that ``load()`` held before the table replaced them; the others were
written from the declarations of their headers.  One letter per ctypes type (``CODE``; "d": a double by value); null: ``argtypes``
was never assigned; spaces in a record only group the letters.  Then the surface as a whole (the headers, disjoint names, the
version) and the build lists that must name every file.

Adding a header is four additions and no edit of this file or any other existing test: the header in ``include/``, its key at the
end of ``_lib.HEADERS``, its name at the end of ``build.PUBLIC_HEADERS`` and its record ``tests/abi/<header>.json``.  Every test
below then covers it; one of the four without the others fails ``test_every_header_has_a_table_and_every_table_a_header``."""
import ctypes
import json
import os
import re

import pytest

from gnnadvisor_osdi21_amd import _lib, build
from util import declared_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")
ABI = os.path.join(ROOT, "tests", "abi")

CODE = {None: "-", ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_float: "f", ctypes.c_uint: "u",
        ctypes.c_uint64: "Q", ctypes.c_char_p: "s", ctypes.POINTER(ctypes.c_double): "D", ctypes.POINTER(ctypes.c_int): "I",
        ctypes.POINTER(ctypes.c_int64): "L", ctypes.POINTER(_lib.Tuning): "T", ctypes.c_double: "d"}


def _record(file):
    """{name: (restype, argtypes)} of a file of tests/abi = {name: [restype letter, argtype letters or null]}."""
    with open(os.path.join(ABI, file)) as f:
        return {name: (restype, argtypes and argtypes.replace(" ", "")) for name, (restype, argtypes) in json.load(f).items()}


# header: {name: (restype, argtypes)}
RECORDED = {file[:-len(".json")]: _record(file) for file in sorted(os.listdir(ABI)) if file.endswith(".json")}
every_header = pytest.mark.parametrize("header", list(RECORDED))


def _codes(restype, argtypes):
    return CODE[restype], None if argtypes is None else "".join(CODE[t] for t in argtypes)


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


# ---- every header ----

@every_header
def test_header_table_and_record_name_the_same_entries(header):
    declared = declared_entries(_header(header))
    assert declared, "no GNNA_API declarations found"
    assert declared == set(_lib.HEADERS[header]) == set(RECORDED[header])


@every_header
def test_the_table_is_the_record(header):
    table = {name: _codes(restype, argtypes) for name, (restype, argtypes) in _lib.HEADERS[header].items()}
    assert table == RECORDED[header]


@every_header
def test_load_leaves_every_entry_with_the_recorded_signature(header):
    lib = _lib.load()
    got = {name: _codes(getattr(lib, name).restype, getattr(lib, name).argtypes) for name in _lib.HEADERS[header]}
    assert sorted(got) == sorted(RECORDED[header])
    wrong = {name: (got[name], want) for name, want in RECORDED[header].items() if got[name] != want}
    assert not wrong, wrong


# ---- the surface as a whole ----

def test_every_header_has_a_table_and_every_table_a_header():
    in_include = {f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")}
    assert set(_lib.HEADERS) == in_include == set(build.PUBLIC_HEADERS) == set(RECORDED)
    assert tuple(_lib.HEADERS) == build.PUBLIC_HEADERS and build.PUBLIC_HEADERS[0] == "gnna.h"          # in the order they were added


def test_the_entry_names_are_disjoint_and_as_many_as_recorded():
    assert [len(table) for table in _lib.HEADERS.values()][:13] == [63, 2, 2, 2, 3, 1, 2, 2, 2, 4, 3, 2, 2]     # 90 names in all
    recorded = sum(len(record) for record in RECORDED.values())
    names = [name for table in _lib.HEADERS.values() for name in table]
    assert len(names) == len(set(names)) == recorded
    declared = [name for header in _lib.HEADERS for name in sorted(declared_entries(_header(header)))]
    assert len(declared) == len(set(declared)) == recorded                # no header declares an entry of another


def test_load_refuses_an_entry_bound_under_two_headers(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.HEADERS, "gnna_twice.h", {"gnna_version": _lib.HEADERS["gnna.h"]["gnna_version"]})
    with pytest.raises(ImportError, match="gnna_version is bound under two headers of _lib.HEADERS: gnna.h and gnna_twice.h"):
        _lib.load()


def test_the_feature_headers_include_gnna_h_and_leave_the_version_alone():
    assert "#define GNNA_VERSION 601" in _header("gnna.h")
    for header in build.PUBLIC_HEADERS[1:]:
        text = _header(header)
        assert '#include "gnna.h"' in text and "#define GNNA_VERSION" not in text, header
    assert _lib.load().gnna_version() == 601


def test_exports_is_the_pinned_surface():
    assert isinstance(_lib.EXPORTS, tuple) and _lib.EXPORTS == tuple(_lib.HEADERS["gnna.h"]) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS) == 63


# ---- the build ----

def _makefile_list(name):
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^%s\s*=(.*)$" % name, makefile, re.M).group(1).split()


def test_every_source_is_built():
    in_csrc = {f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp"))}
    assert [os.path.basename(p) for p in build.EXT_SOURCES] == ["gnna_torch.cpp"]
    sources = [os.path.relpath(p, CSRC) for p in build.LIB_SOURCES]
    assert set(sources) == in_csrc - {"gnna_torch.cpp"} and len(set(sources)) == len(sources)
    assert set(_makefile_list("SOURCES")) == set(sources)


def test_every_header_is_a_dependency_and_hashed():
    internal = {f for f in os.listdir(CSRC) if f.endswith(".h")}
    assert set(build.INTERNAL_HEADERS) == internal
    public = [os.path.join(build.INCLUDE, f) for f in build.PUBLIC_HEADERS]
    assert set(build.LIB_DEPS) == set(build.LIB_SOURCES) | {os.path.join(CSRC, f) for f in internal} | set(public)    # so source_hash covers them
    assert set(build.EXT_DEPS) == set(build.EXT_SOURCES) | set(public)
    assert set(_makefile_list("HEADERS")) == internal | {"../../include/" + f for f in build.PUBLIC_HEADERS}


def test_the_library_was_built_from_these_sources():
    assert _lib.build_id() == "0.6.1+" + build.source_hash()

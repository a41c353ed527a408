"""The binding surface of ``_lib`` (no GPU), in one place: for every public header of ``include/``, the entries it declares, its
table in ``_lib.HEADERS`` and the record below name the same entries, and restype and argtypes of every entry -- in the table and as
``load()`` leaves them on the loaded library -- are the recorded ones.  A wrong argtype does not fail loudly -- a 64-bit count passed
as c_int is truncated, a float passed as an integer is garbage -- so every table is pinned as a whole.  The gnna.h record was taken
from the hand-written assignments that ``load()`` held before the table replaced them; the others were written from the
declarations of their headers.  One letter per ctypes type (``CODE``; "d": a double by value); None: ``argtypes`` was never
assigned.  Then the surface as a whole (the headers, disjoint names, the version) and the build lists that must name every file."""
import ctypes
import os
import re

import pytest

from gnnadvisor_osdi21_amd import _lib, build
from util import declared_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")

CODE = {None: "-", ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_float: "f", ctypes.c_uint: "u",
        ctypes.c_uint64: "Q", ctypes.c_char_p: "s", ctypes.POINTER(ctypes.c_double): "D", ctypes.POINTER(ctypes.c_int): "I",
        ctypes.POINTER(ctypes.c_int64): "L", ctypes.POINTER(_lib.Tuning): "T", ctypes.c_double: "d"}

# header: {name: (restype, argtypes)}
RECORDED = {}
RECORDED["gnna.h"] = {
    'gnna_agg_edge_ld_f32': ('i', 'pllppppplliliup'),
    'gnna_agg_gcn_f32': ('i', 'pppppppliliiip'),
    'gnna_agg_gin_f32': ('i', 'pppfpppliliiip'),
    'gnna_agg_ld_f32': ('i', 'ipllpppfppplliliup'),
    'gnna_agg_ld_x16': ('i', 'iipllpppfpppilliliup'),
    'gnna_agg_rect_f32': ('i', 'iplpppfpppliliip'),
    'gnna_agg_rect_windows_f32': ('i', 'iplpppfpppliliiiiip'),
    'gnna_agg_reduce_ld_f32': ('i', 'ipllpppplplliliup'),
    'gnna_agg_typed_contract_ld_f32': ('i', 'pllppppiippplliliup'),
    'gnna_agg_typed_expand_ld_f32': ('i', 'pllppppiippplliliup'),
    'gnna_build_id': ('s', None),
    'gnna_build_part_device_i32': ('i', 'iplpplp'),
    'gnna_build_part_i32': ('i', 'iplppl'),
    'gnna_count_parts': ('l', 'ipl'),
    'gnna_count_parts_device_i32': ('l', 'iplp'),
    'gnna_csr_from_edges_i32': ('l', 'ppllpp'),
    'gnna_csr_from_edges_range_i32': ('l', 'ppllllppl'),
    'gnna_debug_untrusted_copies': ('i', 'p'),
    'gnna_degrees_f32': ('i', 'plp'),
    'gnna_device_cus': ('i', None),
    'gnna_edge_softmax_backward_f32': ('i', 'pppllipp'),
    'gnna_edge_softmax_f32': ('i', 'ppllipp'),
    'gnna_edge_span': ('i', 'pplD'),
    'gnna_forget_graph': ('i', 'p'),
    'gnna_forget_plans': ('i', 'p'),
    'gnna_gat_backward_dir_f32': ('i', 'plpppplplpppplpppplfplppliiiup'),
    'gnna_gat_backward_f32': ('i', 'plpppplplppppfplppliiliup'),
    'gnna_gat_backward_rect_f32': ('i', 'plpppplplpppplpppplfplpplliiiup'),
    'gnna_gat_forward_f32': ('i', 'plppppppfplpliiliup'),
    'gnna_gat_forward_rect_f32': ('i', 'plppppppfplplliiliup'),
    'gnna_get_tuning': ('-', 'T'),
    'gnna_host_threads': ('i', None),
    'gnna_last_error': ('s', None),
    'gnna_last_num_launches': ('i', None),
    'gnna_last_num_phases': ('i', None),
    'gnna_preferred_ld': ('l', 'ill'),
    'gnna_prepare_graph': ('i', 'pppllliIiIp'),
    'gnna_prepare_x16': ('i', 'llpip'),
    'gnna_profile_begin': ('i', 'i'),
    'gnna_profile_end': ('i', 'DDI'),
    'gnna_relabel_csr_i32': ('i', 'pplppp'),
    'gnna_relabel_edges_i32': ('i', 'pplplD'),
    'gnna_release_graph': ('i', 'p'),
    'gnna_reorder_community_csr_i32': ('i', 'pplp'),
    'gnna_reorder_community_i32': ('i', 'ppllp'),
    'gnna_reorder_rcm_i32': ('i', 'ppllp'),
    'gnna_reverse_edges_i32': ('i', 'pplp'),
    'gnna_row_counts_i64': ('i', 'pllp'),
    'gnna_row_splits_i64': ('i', 'plipp'),
    'gnna_runtime_counters': ('-', 'L'),
    'gnna_runtime_counters_ex': ('i', 'Li'),
    'gnna_sag_f32': ('i', 'pppppppliliiip'),
    'gnna_sample_neighbors_i32': ('i', 'pplpliQippppppllLp'),
    'gnna_scatter_arg_ld_f32': ('i', 'plplplplliup'),
    'gnna_sddmm_f32': ('i', 'ppppppllilip'),
    'gnna_sddmm_ld_f32': ('i', 'plplppppllilip'),
    'gnna_set_graph_hints': ('i', 'pii'),
    'gnna_set_graph_phases': ('i', 'pii'),
    'gnna_set_tuning': ('i', 'T'),
    'gnna_transpose_csr_i32': ('i', 'ppllpppp'),
    'gnna_typed_coef_grad_ld_f32': ('i', 'pllpllppppppiiiliup'),
    'gnna_version': ('i', None),
    'gnna_xtg_f32': ('i', 'pppliip'),
}
# the rect entries' letters with "fQ" (attn_drop, rng_seed) after the slope's "f"
RECORDED["gnna_ext.h"] = {
    "gnna_gat_forward_drop_f32": ("i", "plppppppffQplplliiliup"),
    "gnna_gat_backward_drop_f32": ("i", "plpppplplpppplpppplffQplpplliiiup"),
}
RECORDED["gnna_gatv2.h"] = {
    "gnna_gatv2_forward_f32": ("i", "plplp" "pppp" "ffQ" "plp" "lliiliup"),
    "gnna_gatv2_backward_f32": ("i", "plplp" "p" "plpl" "ppppl" "ppppl" "ffQ" "plplp" "lliiiup"),
}
RECORDED["gnna_dotattn.h"] = {
    "gnna_dot_attn_forward_f32": ("i", "plplpl" "pppp" "ffQ" "plp" "lliiliup"),
    "gnna_dot_attn_backward_f32": ("i", "plplpl" "p" "plpl" "ppppl" "ppppl" "ffQ" "plplpl" "lliiiup"),
}
RECORDED["gnna_gat_edge.h"] = {
    "gnna_gat_edge_forward_f32": ("i", "plppp" "pppp" "ffQ" "plp" "llliiliup"),
    "gnna_gat_edge_backward_f32": ("i", "plppp" "p" "plpl" "ppppl" "ppppl" "p" "ffQ" "plppp" "llliiiup"),
    "gnna_gat_alpha_f32": ("i", "pppp" "pp" "f" "p" "llli" "p"),
}
RECORDED["gnna_stats.h"] = {
    "gnna_agg_stats_ld_f32": ("i", "pll" "ppp" "pl" "pl" "plpl" "plpl" "liliup"),
}
RECORDED["gnna_softagg.h"] = {
    "gnna_agg_softmax_ld_f32": ("i", "pll" "pi" "pp" "pl" "pl" "pl" "liup"),
    "gnna_agg_softmax_backward_ld_f32": ("i", "pll" "pi" "pl" "pl" "pl" "pp" "pl" "liup"),
}
RECORDED["gnna_pool.h"] = {
    "gnna_segment_pool_ld_f32": ("i", "pll" "pl" "pl" "plpl" "plpl" "iup"),
    "gnna_segment_pool_backward_ld_f32": ("i", "pl" "plpl" "plpl" "pl" "pl" "liup"),
}
RECORDED["gnna_attnpool.h"] = {
    "gnna_segment_attn_pool_ld_f32": ("i", "pll" "pli" "pl" "pl" "pl" "iup"),
    "gnna_segment_attn_pool_backward_ld_f32": ("i", "pl" "pli" "pl" "pl" "pl" "pl" "pl" "pl" "liup"),
}
RECORDED["gnna_topk.h"] = {
    "gnna_topk_keep_count": ("l", "ldl"),
    "gnna_segment_topk_i32": ("i", "plpl" "dl" "ppli" "ppp" "ppp" "pp" "lll" "Lp"),
    "gnna_gather_rows_scale_ld_f32": ("i", "pll" "pp" "pll" "ip"),
    "gnna_gather_rows_scale_backward_ld_f32": ("i", "pll" "p" "plp" "plp" "lip"),
}
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


def test_the_entry_names_are_disjoint_and_83():
    assert [len(table) for table in _lib.HEADERS.values()] == [63, 2, 2, 2, 3, 1, 2, 2, 2, 4]
    names = [name for table in _lib.HEADERS.values() for name in table]
    assert len(names) == len(set(names)) == 83
    declared = [name for header in _lib.HEADERS for name in sorted(declared_entries(_header(header)))]
    assert len(declared) == len(set(declared)) == 83                      # no header declares an entry of another


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

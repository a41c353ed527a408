"""The ctypes signature table of ``_lib`` (no GPU): restype and argtypes of every libgnna entry as ``load()`` leaves them, compared
entry for entry with a record taken from the hand-written assignments that ``load()`` held before the table replaced them.  A
wrong argtype does not fail loudly -- a 64-bit count passed as c_int is truncated, a float passed as an integer is garbage -- so
the table is pinned as a whole.  One letter per ctypes type (``CODE``); None: ``argtypes`` was never assigned."""
import ctypes
import os

from gnnadvisor_osdi21_amd import _lib
from util import declared_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = {None: "-", ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_float: "f", ctypes.c_uint: "u",
        ctypes.c_uint64: "Q", ctypes.c_char_p: "s", ctypes.POINTER(ctypes.c_double): "D", ctypes.POINTER(ctypes.c_int): "I",
        ctypes.POINTER(ctypes.c_int64): "L", ctypes.POINTER(_lib.Tuning): "T"}

# name: (restype, argtypes)
RECORDED = {
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


def _codes(restype, argtypes):
    return CODE[restype], None if argtypes is None else "".join(CODE[t] for t in argtypes)


def test_load_leaves_every_entry_with_the_recorded_signature():
    lib = _lib.load()
    got = {name: _codes(getattr(lib, name).restype, getattr(lib, name).argtypes) for name in _lib.EXPORTS}
    assert sorted(got) == sorted(RECORDED)
    wrong = {name: (got[name], RECORDED[name]) for name in RECORDED if got[name] != RECORDED[name]}
    assert not wrong, wrong


def test_the_table_is_what_load_applies():
    table = {name: _codes(restype, argtypes) for name, (restype, argtypes) in _lib.SIGNATURES.items()}
    assert table == RECORDED


def test_exports_table_and_header_name_the_same_entries():
    header = open(os.path.join(ROOT, "include", "gnna.h")).read()
    declared = declared_entries(header)
    assert declared, "no GNNA_API declarations found"
    assert isinstance(_lib.EXPORTS, tuple) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert set(_lib.EXPORTS) == set(_lib.SIGNATURES) == declared

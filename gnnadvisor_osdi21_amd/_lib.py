"""ctypes binding of the C ABI in ``include/gnna.h`` (``csrc/libgnna.so``).

PyTorch is used here only as the owner of device memory and streams: every call hands
raw ``data_ptr()`` addresses and the current HIP stream handle to the library.  There
is no CPU fallback -- if the shared library is missing the import of the product path
fails loudly.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GNNA_LIB") or os.path.join(_HERE, "csrc", "libgnna.so")  # GNNA_LIB: A/B builds

GNNA_OK = 0


class GnnaError(RuntimeError):
    pass


class Tuning(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int), ("groups_per_chunk", ctypes.c_int), ("loads_in_flight", ctypes.c_int),
                ("blocks_per_cu", ctypes.c_int), ("xcd_remap", ctypes.c_int),
                ("trust_canonical", ctypes.c_int), ("column_phases", ctypes.c_int),
                ("avg_degree", ctypes.c_int), ("nonlocal_ids", ctypes.c_int), ("gcn_prescale", ctypes.c_int),
                ("pad_rows", ctypes.c_int), ("zero_fill", ctypes.c_int),
                ("sweep", ctypes.c_int), ("sweep_slack", ctypes.c_int), ("deterministic", ctypes.c_int),
                ("pack_ids", ctypes.c_int), ("ids_check_every", ctypes.c_int), ("wide_blocks", ctypes.c_int)]


_lib = None

# ---- the C ABI as ctypes sees it, one table per public header of include/, in the order the headers were added:
# HEADERS[header] = {entry: (restype, argtypes; None: never assigned)}.  load() applies every table.  A new header is four additions
# and no edit of an existing test: the header in include/, its key at the end here, its name at the end of build.PUBLIC_HEADERS and
# its record tests/abi/<header>.json (read by tests/test_binding_table_host.py, which then checks it like every other) ----
p, i, i64, u, u64, f, s = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint, ctypes.c_uint64, ctypes.c_float, ctypes.c_char_p
pd, pi, pi64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
_REF_TAIL = [p, p, p, i64, i, i64, i, i, i, p]       # part_pointers, part2Node, out, num_nodes, dim, num_parts, partSize, dimWorker, warpPerBlock, stream
_RECT = [i, p, i64, p, p, p, f, p, p, p, i64, i, i64, i, i]    # gnna_agg_rect_f32 up to `accumulate`
_SIZES = [i64, i64, i, i64, i, u, p]                 # the tail of the *_ld entries: ld of the last output, num_out_rows, dim, num_parts, partSize, flags, stream
_GAT_FWD = [p, i64, p, p, p, p, p, p, f, p, i64, p]  # H, ld_h, el, er, the graph, slope, out, ld_out, lse
_GAT_BWD = [p, i64, p, p, p, p, i64, p, i64]         # H, ld_h, el, er, lse, Y, ld_y, dY, ld_dy
_GAT_BOTH = ([p] * 4 + [i64]) * 2 + [f, p, i64, p, p]   # the graph and its transpose with their num_parts, slope, dH, ld_dh, d_el, d_er
_TYPED = [p, i64, i64, p, p, p, p, i, i, p, p, p] + _SIZES
HEADERS = {}
HEADERS["gnna.h"] = {                # the pinned 601 surface
    "gnna_version": (i, None), "gnna_build_id": (s, None), "gnna_last_error": (s, None), "gnna_device_cus": (i, None),
    "gnna_host_threads": (i, None), "gnna_last_num_phases": (i, None), "gnna_last_num_launches": (i, None),
    "gnna_count_parts": (i64, [i, p, i64]),
    "gnna_build_part_i32": (i, [i, p, i64, p, p, i64]),
    "gnna_sag_f32": (i, [p, p, p, p] + _REF_TAIL),
    "gnna_agg_gcn_f32": (i, [p, p, p, p] + _REF_TAIL),
    "gnna_agg_gin_f32": (i, [p, p, p, f] + _REF_TAIL),
    "gnna_set_tuning": (i, [ctypes.POINTER(Tuning)]),
    "gnna_get_tuning": (None, [ctypes.POINTER(Tuning)]),
    "gnna_agg_rect_f32": (i, _RECT + [p]),
    "gnna_agg_rect_windows_f32": (i, _RECT + [i, i, i, p]),
    "gnna_agg_ld_f32": (i, [i, p, i64, i64, p, p, p, f, p, p, p] + _SIZES),
    "gnna_agg_ld_x16": (i, [i, i, p, i64, i64, p, p, p, f, p, p, p, i] + _SIZES),
    "gnna_prepare_x16": (i, [i64, i64, p, i, p]),
    "gnna_preferred_ld": (i64, [i, i64, i64]),
    "gnna_set_graph_hints": (i, [p, i, i]),
    "gnna_set_graph_phases": (i, [p, i, i]),
    "gnna_xtg_f32": (i, [p, p, p, i64, i, i, p]),
    "gnna_csr_from_edges_i32": (i64, [p, p, i64, i64, p, p]),
    "gnna_row_counts_i64": (i, [p, i64, i64, p]),
    "gnna_row_splits_i64": (i, [p, i64, i, p, p]),
    "gnna_csr_from_edges_range_i32": (i64, [p, p, i64, i64, i64, i64, p, p, i64]),
    "gnna_degrees_f32": (i, [p, i64, p]),
    "gnna_edge_span": (i, [p, p, i64, pd]),
    "gnna_reorder_rcm_i32": (i, [p, p, i64, i64, p]),
    "gnna_reorder_community_i32": (i, [p, p, i64, i64, p]),
    "gnna_reorder_community_csr_i32": (i, [p, p, i64, p]),
    "gnna_relabel_edges_i32": (i, [p, p, i64, p, i64, pd]),
    "gnna_relabel_csr_i32": (i, [p, p, i64, p, p, p]),
    "gnna_sddmm_ld_f32": (i, [p, i64, p, i64, p, p, p, p, i64, i64, i, i64, i, p]),
    "gnna_sddmm_f32": (i, [p, p, p, p, p, p, i64, i64, i, i64, i, p]),
    "gnna_prepare_graph": (i, [p, p, p, i64, i64, i64, i, pi, i, pi, p]),
    "gnna_release_graph": (i, [p]), "gnna_forget_graph": (i, [p]), "gnna_forget_plans": (i, [p]),
    "gnna_runtime_counters": (None, [pi64]),
    "gnna_runtime_counters_ex": (i, [pi64, i]),
    "gnna_debug_untrusted_copies": (i, [p]),
    "gnna_profile_begin": (i, [i]),
    "gnna_profile_end": (i, [pd, pd, pi]),
    "gnna_agg_edge_ld_f32": (i, [p, i64, i64, p, p, p, p, p] + _SIZES),
    "gnna_edge_softmax_f32": (i, [p, p, i64, i64, i, p, p]),
    "gnna_edge_softmax_backward_f32": (i, [p, p, p, i64, i64, i, p, p]),
    "gnna_reverse_edges_i32": (i, [p, p, i64, p]),
    "gnna_agg_reduce_ld_f32": (i, [i, p, i64, i64, p, p, p, p, i64, p] + _SIZES),
    "gnna_scatter_arg_ld_f32": (i, [p, i64, p, i64, p, i64, p, i64, i64, i, u, p]),
    "gnna_gat_forward_f32": (i, _GAT_FWD + [i64, i, i, i64, i, u, p]),
    "gnna_gat_forward_rect_f32": (i, _GAT_FWD + [i64, i64, i, i, i64, i, u, p]),       # (num_out_rows, num_in_rows) for num_nodes
    "gnna_gat_backward_f32": (i, _GAT_BWD + [p, p, p, p, f, p, i64, p, p, i64, i, i, i64, i, u, p]),
    "gnna_gat_backward_dir_f32": (i, _GAT_BWD + _GAT_BOTH + [i64, i, i, i, u, p]),
    "gnna_gat_backward_rect_f32": (i, _GAT_BWD + _GAT_BOTH + [i64, i64, i, i, i, u, p]),
    "gnna_transpose_csr_i32": (i, [p, p, i64, i64, p, p, p, p]),
    "gnna_count_parts_device_i32": (i64, [i, p, i64, p]),
    "gnna_build_part_device_i32": (i, [i, p, i64, p, p, i64, p]),
    "gnna_sample_neighbors_i32": (i, [p, p, i64, p, i64, i, u64, i, p, p, p, p, p, p, i64, i64, pi64, p]),
    "gnna_agg_typed_expand_ld_f32": (i, _TYPED),
    "gnna_agg_typed_contract_ld_f32": (i, _TYPED),
    "gnna_typed_coef_grad_ld_f32": (i, [p, i64, i64, p, i64, i64, p, p, p, p, p, p, i, i, i, i64, i, u, p]),
}
# entries added after the pinned 601 surface
HEADERS["gnna_ext.h"] = {
    "gnna_gat_forward_drop_f32": (i, _GAT_FWD[:9] + [f, u64] + _GAT_FWD[9:] + [i64, i64, i, i, i64, i, u, p]),     # attn_drop, rng_seed after the slope
    "gnna_gat_backward_drop_f32": (i, _GAT_BWD + _GAT_BOTH[:11] + [f, u64] + _GAT_BOTH[11:] + [i64, i64, i, i, i, u, p]),
}
# fused GATv2 attention
_GRAPH_T = ([p] * 4 + [i64]) * 2                         # the graph and its transpose, each with its num_parts
HEADERS["gnna_gatv2.h"] = {
    # Hs, ld_hs, Hd, ld_hd, att, the graph, slope, attn_drop, rng_seed, out, ld_out, lse, sizes
    "gnna_gatv2_forward_f32": (i, [p, i64, p, i64, p] + [p] * 4 + [f, f, u64, p, i64, p, i64, i64, i, i, i64, i, u, p]),
    # Hs, ld_hs, Hd, ld_hd, att, lse, Y, ld_y, dY, ld_dy, both structures, slope, attn_drop, rng_seed, dHs, ld_dhs, dHd, ld_dhd, d_att, sizes
    "gnna_gatv2_backward_f32": (i, [p, i64, p, i64, p, p, p, i64, p, i64] + _GRAPH_T + [f, f, u64, p, i64, p, i64, p,
                                                                                       i64, i64, i, i, i, u, p]),
}
# fused dot-product attention
HEADERS["gnna_dotattn.h"] = {
    # Q, ld_q, K, ld_k, V, ld_v, the graph, scale, attn_drop, rng_seed, out, ld_out, lse, sizes
    "gnna_dot_attn_forward_f32": (i, [p, i64] * 3 + [p] * 4 + [f, f, u64, p, i64, p, i64, i64, i, i, i64, i, u, p]),
    # Q, ld_q, K, ld_k, V, ld_v, lse, Y, ld_y, dY, ld_dy, both structures, scale, attn_drop, rng_seed, dQ, ld_dq, dK, ld_dk, dV, ld_dv, sizes
    "gnna_dot_attn_backward_f32": (i, [p, i64] * 3 + [p, p, i64, p, i64] + _GRAPH_T + [f, f, u64] + [p, i64] * 3 +
                                   [i64, i64, i, i, i, u, p]),
}
# fused GAT attention with a per-edge score term
HEADERS["gnna_gat_edge.h"] = {
    # gnna_gat_forward_drop_f32 with ee after er and num_edges after the row counts
    "gnna_gat_edge_forward_f32": (i, _GAT_FWD[:4] + [p] + _GAT_FWD[4:9] + [f, u64] + _GAT_FWD[9:] + [i64, i64, i64, i, i, i64, i, u, p]),
    # gnna_gat_backward_drop_f32 with ee after er, t_edge_pos after the transposed structure, d_ee after d_er, num_edges after the row counts
    "gnna_gat_edge_backward_f32": (i, _GAT_BWD[:4] + [p] + _GAT_BWD[4:] + _GAT_BOTH[:10] + [p, f, f, u64] + _GAT_BOTH[11:] +
                                   [p, i64, i64, i64, i, i, i, u, p]),
    # el, er, ee, lse, row_pointers, column_index, slope, alpha, num_out_rows, num_in_rows, num_edges, heads, stream
    "gnna_gat_alpha_f32": (i, [p] * 6 + [f, p, i64, i64, i64, i, p]),
}
# neighbor statistics from one gather
HEADERS["gnna_stats.h"] = {
    # input, ld_in, num_in_rows, the partition, (sum, ld) (sumsq, ld), (max, ld, argmax, ld) (min, ld, argmin, ld), num_out_rows, dim, num_parts, partSize, flags, stream
    "gnna_agg_stats_ld_f32": (i, [p, i64, i64, p, p, p] + [p, i64] * 6 + [i64, i, i64, i, u, p]),
}
# softmax neighbor aggregation
HEADERS["gnna_softagg.h"] = {
    # input, ld_in, num_in_rows, temp, temp_len, row_pointers, column_index, (out, ld) (lse, ld) (sq, ld), num_out_rows, dim, flags, stream
    "gnna_agg_softmax_ld_f32": (i, [p, i64, i64, p, i, p, p] + [p, i64] * 3 + [i64, i, u, p]),
    # input, ld_in, num_in_rows, temp, temp_len, (lse, ld) (Y, ld) (dY, ld), the transposed structure, d_input, ld_din, num_out_rows, dim, flags, stream
    "gnna_agg_softmax_backward_ld_f32": (i, [p, i64, i64, p, i] + [p, i64] * 3 + [p, p, p, i64, i64, i, u, p]),
}
# graph-level readout over the rows of every graph of a batch
HEADERS["gnna_pool.h"] = {
    # input, ld_in, num_rows, graph_pointers, num_segments, (sum, ld), (max, ld, argmax, ld) (min, ld, argmin, ld), dim, flags, stream
    "gnna_segment_pool_ld_f32": (i, [p, i64, i64, p, i64] + [p, i64] * 5 + [i, u, p]),
    # (d_sum, ld), (d_max, ld, argmax, ld) (d_min, ld, argmin, ld), graph_pointers, num_segments, d_input, ld_din, num_rows, dim, flags, stream
    "gnna_segment_pool_backward_ld_f32": (i, [p, i64] * 5 + [p, i64, p, i64, i64, i, u, p]),
}
# attention readout over the rows of every graph of a batch
HEADERS["gnna_attnpool.h"] = {
    # input, ld_in, num_rows, gate, ld_gate, gate_dim, graph_pointers, num_segments, (out, ld) (lse, ld), dim, flags, stream
    "gnna_segment_attn_pool_ld_f32": (i, [p, i64, i64, p, i64, i, p, i64] + [p, i64] * 2 + [i, u, p]),
    # input, ld_in, gate, ld_gate, gate_dim, (lse, ld) (Y, ld) (dY, ld), graph_pointers, num_segments, (d_input, ld) (d_gate, ld), num_rows, dim, flags, stream
    "gnna_segment_attn_pool_backward_ld_f32": (i, [p, i64, p, i64, i] + [p, i64] * 3 + [p, i64] + [p, i64] * 2 + [i64, i, u, p]),
}
# hierarchical pooling on graph batches
HEADERS["gnna_topk.h"] = {
    # n, ratio, k_fixed
    "gnna_topk_keep_count": (i64, [i64, ctypes.c_double, i64]),
    # score, num_rows, graph_pointers, num_segments, ratio, k_fixed, row_pointers, column_index, nnz, partSize, new_id, perm, new_graph_pointers,
    # new_row_pointers, new_column_index, edge_ids, partPtr, part2Node, row_capacity, edge_capacity, part_capacity, counts, stream
    "gnna_segment_topk_i32": (i, [p, i64, p, i64, ctypes.c_double, i64, p, p, i64, i] + [p] * 8 + [i64, i64, i64, pi64, p]),
    # input, ld_in, num_in_rows, perm, scale, out, ld_out, num_out_rows, dim, stream
    "gnna_gather_rows_scale_ld_f32": (i, [p, i64, i64, p, p, p, i64, i64, i, p]),
    # d_out, ld_dout, num_out_rows, new_id, input, ld_in, scale, d_input, ld_din, d_scale, num_in_rows, dim, stream
    "gnna_gather_rows_scale_backward_ld_f32": (i, [p, i64, i64, p, p, i64, p, p, i64, p, i64, i, p]),
}
# per-graph normalisation (GraphNorm) over the rows of every graph of a batch
HEADERS["gnna_segnorm.h"] = {
    # input, ld_in, num_rows, graph_pointers, num_segments, (mean, ld) (m2, ld), dim, flags, stream
    "gnna_segment_moments_ld_f32": (i, [p, i64, i64, p, i64] + [p, i64] * 2 + [i, u, p]),
    # input, ld_in, num_rows, graph_pointers, num_segments, weight, bias, alpha, eps, (out, ld) (mean, ld) (rstd, ld), dim, flags, stream
    "gnna_segment_norm_ld_f32": (i, [p, i64, i64, p, i64, p, p, p, f] + [p, i64] * 3 + [i, u, p]),
    # (d_out, ld) (input, ld) (mean, ld) (rstd, ld), weight, alpha, graph_pointers, num_segments, (d_input, ld) (seg_a, ld) (seg_b, ld), num_rows, dim, flags, stream
    "gnna_segment_norm_backward_ld_f32": (i, [p, i64] * 4 + [p, p, p, i64] + [p, i64] * 3 + [i64, i, u, p]),
}
# subgraph sampling: device random walks and the induced subgraph of a node list
HEADERS["gnna_walk.h"] = {
    # row_pointers, column_index, num_nodes, nnz, roots, num_roots, walk_length, rng_seed, walks, edge_ids, stream
    "gnna_random_walk_i32": (i, [p, p, i64, i64, p, i64, i, u64, p, p, p]),
    # row_pointers, column_index, num_nodes, nnz, nodes, num_ids, partSize, sub_nodes, new_id, sub_row_pointers, sub_column_index,
    # sub_edge_ids, partPtr, part2Node, node_capacity, edge_capacity, counts, stream
    "gnna_induced_subgraph_i32": (i, [p, p, i64, i64, p, i64, i] + [p] * 7 + [i64, i64, pi64, p]),
}
# message passing with a feature row per edge (GINE, SchNet's continuous-filter convolution)
HEADERS["gnna_edgefeat.h"] = {
    # input, ld_in, num_in_rows, edge_feat, ld_e, num_edges, row_pointers, column_index, out, ld_out, num_out_rows, dim, combine, act, flags, stream
    "gnna_agg_edge_feat_ld_f32": (i, [p, i64, i64, p, i64, i64, p, p, p, i64, i64, i, i, i, u, p]),
    # input, ld_in, num_in_rows, edge_feat, ld_e, num_edges, (dY, ld), the structure, the transposed structure, t_edge_pos, (d_input, ld)
    # (d_edge, ld), num_out_rows, dim, combine, act, flags, stream
    "gnna_agg_edge_feat_backward_ld_f32": (i, [p, i64, i64, p, i64, i64, p, i64] + [p] * 5 + [p, i64] * 2 + [i64, i, i, i, u, p]),
}
# graph construction from coordinates: the radius / k-nearest-neighbour graph of every point set of a batch
HEADERS["gnna_spatial.h"] = {
    # pos, ld_pos, num_rows, dim, graph_pointers, num_segments, radius, max_neighbors, loop, partSize, row_pointers, column_index,
    # dist2, partPtr, part2Node, edge_capacity, counts, stream
    "gnna_radius_graph_f32": (i, [p, i64, i64, i, p, i64, f, i, i, i] + [p] * 5 + [i64, pi64, p]),
}
del p, i, i64, u, u64, f, s, pd, pi, pi64
EXPORTS = tuple(HEADERS["gnna.h"])     # users: the build's check of the library, tests/test_host.py


def load() -> ctypes.CDLL:
    """dlopen libgnna.so (built by ``python -m gnnadvisor_osdi21_amd.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -m gnnadvisor_osdi21_amd.build`). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    bound = {}
    for header, table in HEADERS.items():
        for name, (restype, argtypes) in table.items():
            if bound.setdefault(name, header) != header:
                raise ImportError(f"{name} is bound under two headers of _lib.HEADERS: {bound[name]} and {header}")
            fn = getattr(L, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc != GNNA_OK:
        raise GnnaError(f"libgnna error {rc}: {load().gnna_last_error().decode()}")


def _check_counts(rc: int, counts) -> tuple:
    """The tail of the entries that report three int64 counts: the counts as a tuple, or the GnnaError of `rc` carrying them as
    ``.counts`` (what a capacity that was too small has to be)."""
    got = tuple(int(c) for c in counts)
    if rc != GNNA_OK:
        err = GnnaError(f"libgnna error {rc}: {load().gnna_last_error().decode()}")
        err.counts = got
        raise err
    return got


def _degree_sum(rp: torch.Tensor, ids: torch.Tensor) -> int:
    """The sum of the degrees of the rows `ids` of the row pointers `rp`, ids clamped to the graph (ids outside it are the
    library's to report) and a row whose pointers decrease counted as empty: the edges a list of rows can give at the most."""
    n = rp.numel() - 1
    if n <= 0 or ids.numel() == 0:
        return 0
    rows = ids.long().clamp(0, n - 1)
    return int((rp[rows + 1] - rp[rows]).clamp(min=0).sum())


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _call(device, fn_name: str, *args) -> None:
    """One call of a stream-taking entry: on `device`, with that device's current stream appended to `args`; raises GnnaError
    on an error code."""
    with torch.cuda.device(device):
        _check(getattr(load(), fn_name)(*args, _stream(device)))


def _need_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise GnnaError(f"{what} needs device tensors: there is no CPU path in libgnna")


def set_tuning(groups_per_chunk=-1, loads_in_flight=-1, blocks_per_cu=-1, xcd_remap=-1,
               trust_canonical=-1, column_phases=-1, avg_degree=-1, nonlocal_ids=-1, gcn_prescale=-1,
               pad_rows=-1, zero_fill=-1, sweep=-1, sweep_slack=-1, deterministic=-1, pack_ids=-1,
               wide_blocks=-1, ids_check_every=-1) -> None:
    """Fields < 0 (<= 0 where 0 has no meaning) keep the built-in choice; ids_check_every: 1 = a full hash of the ids
    behind a packed copy on every call, n = every n-th (built-in 64), >= 2**30 = never (include/gnna.h)."""
    t = Tuning(ctypes.sizeof(Tuning), groups_per_chunk, loads_in_flight, blocks_per_cu, xcd_remap, trust_canonical, column_phases,
               avg_degree, nonlocal_ids, gcn_prescale, pad_rows, zero_fill, sweep, sweep_slack, deterministic,
               pack_ids, ids_check_every, wide_blocks)
    _check(load().gnna_set_tuning(ctypes.byref(t)))


def reset_tuning() -> None:
    _check(load().gnna_set_tuning(None))


def device_cus() -> int:
    """Compute units of the current device (0: no device visible)."""
    return int(load().gnna_device_cus())


def host_threads() -> int:
    """Host threads the native builders and the renumbering use (affinity, cgroup quota, GNNA_HOST_THREADS)."""
    return int(load().gnna_host_threads())


def build_id() -> str:
    """"0.6.1+<source hash>" of the loaded libgnna.so (gnna_build_id)."""
    return load().gnna_build_id().decode()


_registered: dict = {}      # device address -> token of the storage that registered hints / schedules for it


def _forget_when_freed(column_index) -> None:
    """libgnna keys its per-graph tables by the device address of `column_index`; PyTorch's caching allocator
    hands that address to an unrelated tensor once this one is freed.  Drop the entries together with the
    memory.  The finalizer hangs on the tensor's STORAGE, not on the Python tensor object: hints registered
    through a temporary alias (a view, a slice, `.detach()`) must live as long as the graph does, not as long as
    the alias (unless a newer storage has registered the same address in the meantime)."""
    import weakref
    ptr = column_index.data_ptr()
    storage = column_index.untyped_storage()
    token = _registered.get(ptr)
    if token is not None and token[0]() is storage:
        return                                           # this storage already carries the finalizer for `ptr`
    token = (weakref.ref(storage),)
    _registered[ptr] = token

    def drop(ptr=ptr, token=token):
        if _registered.get(ptr) is token:
            del _registered[ptr]
            if _lib is not None:
                # (a finalizer runs whenever and wherever the garbage collector does: unlink only, free later --
                # gnna_release_graph would hipFree here, a device-wide synchronisation that breaks a capture in progress)
                _lib.gnna_forget_graph(ptr)
    weakref.finalize(storage, drop)


def set_graph_hints(column_index, avg_degree: float, nonlocal_ids: bool) -> None:
    """Per-graph hints (keyed by the device address of `column_index`): average edges per destination
    row and whether the source ids of a row are scattered over the whole id range.  avg_degree <= 0
    forgets the graph; column_index None forgets all.  The entry is dropped when the tensor is freed."""
    ptr = None if column_index is None else column_index.data_ptr()
    _check(load().gnna_set_graph_hints(ptr, int(avg_degree), 1 if nonlocal_ids else 0))
    if column_index is None:
        _registered.clear()
    elif avg_degree > 0:
        _forget_when_freed(column_index)


def get_tuning() -> dict:
    t = Tuning()
    load().gnna_get_tuning(ctypes.byref(t))
    return {name: getattr(t, name) for name, _ in Tuning._fields_ if name != "struct_size"}


def _host_i32(t) -> torch.Tensor:
    t = torch.as_tensor(t)
    return t.to(dtype=torch.int32, device="cpu").contiguous()


def csr_from_edges(src, dst, num_nodes: int):
    """Host CSR builder of the C ABI: (row_pointers int32 [N+1], column_index int32 [nnz])."""
    s, d = _host_i32(src), _host_i32(dst)
    assert s.numel() == d.numel()
    rp = torch.empty(int(num_nodes) + 1, dtype=torch.int32)
    ci = torch.empty(max(1, s.numel()), dtype=torch.int32)
    nnz = load().gnna_csr_from_edges_i32(s.data_ptr(), d.data_ptr(), s.numel(), int(num_nodes),
                                         rp.data_ptr(), ci.data_ptr())
    if nnz < 0:
        _check(int(nnz))
    return rp, ci[:nnz].clone()


def row_counts(rows, num_nodes: int, counts: torch.Tensor | None = None) -> torch.Tensor:
    """int64 [num_nodes]: list entries per row, accumulated into `counts` when given (feed a long list in pieces)."""
    r = _host_i32(rows)
    if counts is None:
        counts = torch.zeros(int(num_nodes), dtype=torch.int64)
    assert counts.dtype == torch.int64 and counts.numel() == int(num_nodes) and counts.is_contiguous()
    _check(load().gnna_row_counts_i64(r.data_ptr(), r.numel(), int(num_nodes), counts.data_ptr()))
    return counts


def row_splits(counts: torch.Tensor, world: int, want_row_pointers: bool = False):
    """-> (bounds: list of world + 1 row boundaries of nnz-balanced contiguous blocks[, global int64 row_pointers])."""
    assert counts.dtype == torch.int64 and counts.is_contiguous() and not counts.is_cuda
    n = counts.numel()
    bounds = torch.empty(int(world) + 1, dtype=torch.int64)
    rp = torch.empty(n + 1, dtype=torch.int64) if want_row_pointers else None
    _check(load().gnna_row_splits_i64(counts.data_ptr(), n, int(world), bounds.data_ptr(), _ptr(rp)))
    return (bounds.tolist(), rp) if want_row_pointers else bounds.tolist()


def csr_from_edges_range(src, dst, num_nodes: int, row_lo: int, row_hi: int, capacity: int | None = None):
    """The CSR rows [row_lo, row_hi) of an edge list: (local int32 row_pointers rebased to 0, GLOBAL int32 column ids)."""
    s, d = _host_i32(src), _host_i32(dst)
    assert s.numel() == d.numel()
    if capacity is None:
        capacity = int(((s >= row_lo) & (s < row_hi)).sum()) if s.numel() else 0
    rp = torch.empty(int(row_hi - row_lo) + 1, dtype=torch.int32)
    ci = torch.empty(max(1, int(capacity)), dtype=torch.int32)
    nnz = load().gnna_csr_from_edges_range_i32(s.data_ptr(), d.data_ptr(), s.numel(), int(num_nodes), int(row_lo),
                                               int(row_hi), rp.data_ptr(), ci.data_ptr(), int(capacity))
    if nnz < 0:
        _check(int(nnz))
    return rp, ci[:nnz].clone()


def degrees(row_pointers: torch.Tensor) -> torch.Tensor:
    rp = _host_i32(row_pointers)
    out = torch.empty(rp.numel() - 1, dtype=torch.float32)
    _check(load().gnna_degrees_f32(rp.data_ptr(), rp.numel() - 1, out.data_ptr()))
    return out


def edge_span(src, dst) -> float:
    s, d = _host_i32(src), _host_i32(dst)
    v = ctypes.c_double()
    _check(load().gnna_edge_span(s.data_ptr(), d.data_ptr(), s.numel(), ctypes.byref(v)))
    return v.value


def _reorder(entry: str, src, dst, num_nodes: int) -> torch.Tensor:
    s, d = _host_i32(src), _host_i32(dst)
    out = torch.empty(int(num_nodes), dtype=torch.int32)
    _check(getattr(load(), entry)(s.data_ptr(), d.data_ptr(), s.numel(), int(num_nodes), out.data_ptr()))
    return out


def reorder_rcm(src, dst, num_nodes: int) -> torch.Tensor:
    """new_id[old_id] from the native reverse Cuthill-McKee renumbering."""
    return _reorder("gnna_reorder_rcm_i32", src, dst, num_nodes)


def reorder_community(src, dst, num_nodes: int) -> torch.Tensor:
    """new_id[old_id] from the native community renumbering (label propagation + chain + barycentre sweeps)."""
    return _reorder("gnna_reorder_community_i32", src, dst, num_nodes)


def reorder_community_csr(row_pointers, column_index, num_nodes: int) -> torch.Tensor:
    """new_id[old_id] of the community renumbering from a host CSR with sorted, duplicate-free rows (the loader's): a symmetric
    CSR is the algorithm's adjacency as it stands (no second counting sort); same permutation as `reorder_community`."""
    rp, ci = _host_i32(row_pointers), _host_i32(column_index)
    assert rp.numel() == int(num_nodes) + 1
    out = torch.empty(int(num_nodes), dtype=torch.int32)
    _check(load().gnna_reorder_community_csr_i32(rp.data_ptr(), ci.data_ptr(), int(num_nodes), out.data_ptr()))
    return out


def relabel_edges_(src: torch.Tensor, dst: torch.Tensor, new_id: torch.Tensor, num_nodes: int) -> float:
    """src, dst (int32 host tensors, contiguous) <- new_id[...] IN PLACE; returns the new mean |src - dst|."""
    for t in (src, dst, new_id):
        assert t.dtype == torch.int32 and t.is_contiguous() and not t.is_cuda
    v = ctypes.c_double()
    _check(load().gnna_relabel_edges_i32(src.data_ptr(), dst.data_ptr(), src.numel(), new_id.data_ptr(), int(num_nodes), ctypes.byref(v)))
    return v.value


def relabel_csr(row_pointers, column_index, new_id, num_nodes: int):
    """The relabelled graph's CSR (rows sorted) from the old CSR and new_id[old] -- no global sort."""
    rp, ci, nid = _host_i32(row_pointers), _host_i32(column_index), _host_i32(new_id)
    out_rp = torch.empty(int(num_nodes) + 1, dtype=torch.int32)
    out_ci = torch.empty(max(1, ci.numel()), dtype=torch.int32)
    _check(load().gnna_relabel_csr_i32(rp.data_ptr(), ci.data_ptr(), int(num_nodes), nid.data_ptr(), out_rp.data_ptr(), out_ci.data_ptr()))
    return out_rp, out_ci[:ci.numel()]


def last_num_phases() -> int:
    return int(load().gnna_last_num_phases())


def last_num_launches() -> int:
    return int(load().gnna_last_num_launches())


def profile_begin(max_calls: int) -> None:
    _check(load().gnna_profile_begin(int(max_calls)))


def profile_end() -> dict:
    """-> {main_ms, prologue_ms, calls}: HIP-event averages of the two kernels per call."""
    a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _check(load().gnna_profile_end(ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
    return dict(main_ms=a.value, prologue_ms=b.value, calls=n.value)


def count_parts(partSize: int, indptr: torch.Tensor) -> int:
    assert indptr.dtype == torch.int32 and not indptr.is_cuda and indptr.is_contiguous()
    n = load().gnna_count_parts(int(partSize), indptr.data_ptr(), indptr.numel() - 1)
    if n < 0:
        _check(int(n))
    return int(n)


def build_part(partSize: int, indptr: torch.Tensor):
    """C-ABI partitioner -> (partPtr int32 [P+1], part2Node int32 [P]) on the CPU."""
    indptr = indptr.contiguous()
    P = count_parts(partSize, indptr)
    pp = torch.empty(P + 1, dtype=torch.int32)
    p2n = torch.empty(P, dtype=torch.int32)
    _check(load().gnna_build_part_i32(int(partSize), indptr.data_ptr(), indptr.numel() - 1,
                                      pp.data_ptr(), p2n.data_ptr(), P))
    return pp, p2n


def _fresh_output(shape, device, dtype=torch.float32) -> torch.Tensor:
    """A new output tensor: the library writes every element.  GNNA_DEBUG_POISON=1 (the test suite sets it) starts it
    as NaN (an int32 `arg` as INT_MIN), so that an element the library fails to write cannot hide behind whatever the
    allocator hands back or pass for one it wrote."""
    if os.environ.get("GNNA_DEBUG_POISON", "0") not in ("", "0"):
        return torch.full(tuple(shape), float("nan") if dtype.is_floating_point else -(2 ** 31), dtype=dtype, device=device)
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def _agg(fn_name, X, row_pointers, column_index, extra, part_pointers, part2Node, partSize, dimWorker,
         warpPerBlock, out):
    _need_device(X, "aggregation")
    assert X.dtype == torch.float32 and X.is_contiguous() and X.dim() == 2
    for t in (column_index, part_pointers, part2Node):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == X.device
    if out is None:
        out = _fresh_output(X.shape, X.device)
    _call(X.device, fn_name, X.data_ptr(), _ptr(row_pointers), column_index.data_ptr(), extra,
          part_pointers.data_ptr(), part2Node.data_ptr(), out.data_ptr(), X.shape[0], X.shape[1], part2Node.numel(),
          int(partSize), int(dimWorker), int(warpPerBlock))
    return out


def sag(X, row_pointers, column_index, degrees, part_pointers, part2Node, partSize=32, dimWorker=32,
        warpPerBlock=4, out=None):
    return _agg("gnna_sag_f32", X, row_pointers, column_index, _ptr(degrees), part_pointers,
                part2Node, partSize, dimWorker, warpPerBlock, out)


def agg_gcn(X, row_pointers, column_index, degrees, part_pointers, part2Node, partSize=32,
            dimWorker=32, warpPerBlock=4, out=None):
    assert degrees.dtype == torch.float32 and degrees.device == X.device
    return _agg("gnna_agg_gcn_f32", X, row_pointers, column_index, degrees.data_ptr(),
                part_pointers, part2Node, partSize, dimWorker, warpPerBlock, out)


def agg_gin(X, row_pointers, column_index, epsilon, part_pointers, part2Node, partSize=32,
            dimWorker=32, warpPerBlock=4, out=None):
    return _agg("gnna_agg_gin_f32", X, row_pointers, column_index, ctypes.c_float(epsilon),
                part_pointers, part2Node, partSize, dimWorker, warpPerBlock, out)


MODE_SAG, MODE_GCN, MODE_GIN = 0, 1, 2


def agg_rect(mode, X, column_index, part_pointers, part2Node, num_out_rows, partSize=32,
             degrees_out=None, degrees_in=None, epsilon=1.0, out=None, accumulate=False, windows=None):
    """Destination-shard aggregation: X is [num_in_rows, dim] (all sources), out is
    [num_out_rows, dim]; column_index indexes X.  ``windows=(K, begin, end)`` aggregates only the
    edges whose source lies in windows [begin, end) of K equal source windows
    (gnna_agg_rect_windows_f32: stateless; the column ids of every neighbor-group must be in increasing order -- the
    loader's CSR has them sorted -- else the call returns GNNA_ERR_UNSUPPORTED; the first call on a partition counts
    the ids per window and synchronises the stream once)."""
    _need_device(X, "aggregation")
    assert X.dtype == torch.float32 and X.is_contiguous() and X.dim() == 2
    if out is None:
        assert not accumulate, "accumulate needs an existing `out`"
        out = _fresh_output((num_out_rows, X.shape[1]), X.device)
    args = (int(mode), X.data_ptr(), X.shape[0], column_index.data_ptr(), _ptr(degrees_out), _ptr(degrees_in), float(epsilon),
            part_pointers.data_ptr(), part2Node.data_ptr(), out.data_ptr(), int(num_out_rows), X.shape[1], part2Node.numel(),
            int(partSize), 1 if accumulate else 0)
    if windows is not None:
        K, wb, we = (int(v) for v in windows)
        assert wb == 0 or out is not None
        _call(X.device, "gnna_agg_rect_windows_f32", *args, K, wb, we)
    else:
        _call(X.device, "gnna_agg_rect_f32", *args)
    return out


ACCUMULATE, EPILOGUE_RELU = 1, 2


def _flags(accumulate=False, relu=False) -> int:
    return (ACCUMULATE if accumulate else 0) | (EPILOGUE_RELU if relu else 0)


def _rows_view(t: torch.Tensor, what: str, dtype=torch.float32, unit="floats"):
    """(data pointer, rows, dim, leading dimension) of a 2-D device tensor whose rows are contiguous: float32, or of any
    element type with dtype=None (the leading dimension is counted in elements)."""
    assert (dtype is None or t.dtype == dtype) and t.dim() == 2, \
        f"{what} must be a 2-D {'' if dtype is None else str(dtype).replace('torch.', '') + ' '}tensor"
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise GnnaError(f"{what}: the {unit} of a row must be contiguous (stride(1) == 1)")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    if ld < t.shape[1]:
        raise GnnaError(f"{what}: rows overlap (stride(0) = {t.stride(0)} < {t.shape[1]})")
    return t.data_ptr(), t.shape[0], t.shape[1], ld


def _rows_view_any(t: torch.Tensor, what: str):
    return _rows_view(t, what, dtype=None, unit="elements")


def _out_rows(out, rows, width, device, accumulate=False):
    """(out, its data pointer, its leading dimension) of a float32 result [rows, width] on `device`: the caller's `out`, which
    may be a row-strided view, or a fresh tensor -- which there is nothing to accumulate into."""
    if out is None:
        assert not accumulate, "accumulate needs an existing `out`"
        out = _fresh_output((rows, width), device)
    ptr, n, w, ld = _rows_view(out, "out")
    assert n == int(rows) and w == width and out.device == device
    return out, ptr, ld


def agg_ld(mode, X, column_index, part_pointers, part2Node, num_out_rows, partSize=32, degrees_out=None,
           degrees_in=None, epsilon=1.0, out=None, accumulate=False, relu=False):
    """gnna_agg_ld_f32: the rectangular aggregation with leading dimensions and the ReLU epilogue.  `X` and `out` may be
    row-strided views (a column block ``M[:, a:b]``, a padded buffer ``P[:, :dim]``): stride(1) must be 1, stride(0) is
    handed over as the leading dimension.  relu: out = max(out, 0) after the aggregation."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    out, yp, ld_out = _out_rows(out, num_out_rows, dim, X.device, accumulate)
    _call(X.device, "gnna_agg_ld_f32", int(mode), xp, ld_in, n_in, column_index.data_ptr(), _ptr(degrees_out), _ptr(degrees_in),
          float(epsilon), part_pointers.data_ptr(), part2Node.data_ptr(), yp, ld_out, int(num_out_rows), dim, part2Node.numel(),
          int(partSize), _flags(accumulate, relu))
    return out


F32, BF16, F16 = 0, 1, 2        # GNNA_F32 / GNNA_BF16 / GNNA_F16
_X16_TYPES = {torch.bfloat16: BF16, torch.float16: F16}


def agg_ld_x16(mode, X, column_index, part_pointers, part2Node, num_out_rows, partSize=32, degrees_out=None,
               degrees_in=None, epsilon=1.0, out=None, out_dtype=None, accumulate=False, relu=False):
    """gnna_agg_ld_x16: agg_ld over bfloat16 / float16 `X`, accumulated in fp32.  The result is float32 or has X's dtype
    (`out_dtype`, default X's; or the dtype of a given `out`), rounded once.  Degrees stay float32.  accumulate needs a
    float32 `out`.  float16 results beyond +-65504 are +-inf (GCN coefficients get large: prefer bfloat16 / float32)."""
    _need_device(X, "aggregation")
    if X.dtype not in _X16_TYPES:
        raise GnnaError(f"agg_ld_x16 takes bfloat16 or float16 features (got {X.dtype}); float32 goes through agg_ld")
    xp, n_in, dim, ld_in = _rows_view_any(X, "X")
    if out is None:
        assert not accumulate, "accumulate needs an existing `out`"
        out = _fresh_output((int(num_out_rows), dim), X.device, X.dtype if out_dtype is None else out_dtype)
    elif out_dtype is not None and out.dtype != out_dtype:
        raise GnnaError(f"out is {out.dtype}, out_dtype says {out_dtype}")
    if out.dtype != torch.float32 and out.dtype != X.dtype:
        raise GnnaError(f"the output is float32 or has the input's dtype {X.dtype} (got {out.dtype})")
    out_type = F32 if out.dtype == torch.float32 else _X16_TYPES[out.dtype]
    yp, n_out, dim_o, ld_out = _rows_view_any(out, "out")
    assert n_out == int(num_out_rows) and dim_o == dim and out.device == X.device
    for t in (degrees_out, degrees_in):
        assert t is None or t.dtype == torch.float32, "degrees stay float32"
    _call(X.device, "gnna_agg_ld_x16", int(mode), _X16_TYPES[X.dtype], xp, ld_in, n_in, column_index.data_ptr(), _ptr(degrees_out),
          _ptr(degrees_in), float(epsilon), part_pointers.data_ptr(), part2Node.data_ptr(), yp, out_type, ld_out, int(num_out_rows),
          dim, part2Node.numel(), int(partSize), _flags(accumulate, relu))
    return out


def prepare_x16(num_in_rows: int, num_out_rows: int, dims, device=None) -> None:
    """gnna_prepare_x16: sizes the current stream's scratch of the 16-bit path for these widths, so that later eager
    agg_ld_x16 calls of those shapes on this stream neither allocate nor free."""
    dims = [int(d) for d in dims]
    arr = (ctypes.c_int * max(1, len(dims)))(*dims)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _call(device, "gnna_prepare_x16", int(num_in_rows), int(num_out_rows), arr, len(dims))


def preferred_ld(dim: int, num_in_rows: int, num_edges: int) -> int:
    """The leading dimension (floats) a producer should write `dim`-float source rows with so that the gather needs no
    staged copy (== dim: the contiguous layout is fine)."""
    return int(load().gnna_preferred_ld(int(dim), int(num_in_rows), int(num_edges)))


def empty_rows(num_rows: int, dim: int, ld: int, device) -> torch.Tensor:
    """A [num_rows, dim] float32 view with leading dimension `ld` of a fresh, (ld x 4)-byte aligned allocation."""
    if ld == dim:
        return torch.empty(num_rows, dim, dtype=torch.float32, device=device)
    buf = torch.empty(num_rows * ld + ld, dtype=torch.float32, device=device)
    off = (-buf.data_ptr() // 4) % ld
    return buf[off: off + num_rows * ld].view(num_rows, ld)[:, :dim]


def prepare_graph(column_index, part_pointers, part2Node, num_in_rows: int, num_out_rows: int, partSize: int,
                  dims=()) -> dict:
    """gnna_prepare_graph: counting pass, statistics, phase choice per width and scratch sizing up front (one stream
    synchronisation here, none in any later aggregation on this graph); the plan stays until the column_index storage
    is freed or `release_graph`.  CONTRACT: from here until the release, `column_index`, `part_pointers` and `part2Node`
    must not be rewritten in place -- the plan keeps a copy of the ids in the order the kernels read them (a sample
    checksum notices a rewritten buffer, not a few changed entries; `set_tuning(pack_ids=2)` turns the copy off).
    -> {dim: phases the library will use}."""
    dims = [int(d) for d in dims]
    arr = (ctypes.c_int * max(1, len(dims)))(*dims)
    out = (ctypes.c_int * max(1, len(dims)))()
    _call(column_index.device, "gnna_prepare_graph", column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(),
          part2Node.numel(), int(num_in_rows), int(num_out_rows), int(partSize), arr, len(dims), out)
    _forget_when_freed(column_index)
    return {d: int(out[i]) for i, d in enumerate(dims)}


def release_graph(column_index) -> None:
    """Drops the library's plans, hints and measured schedules for this graph (None: all graphs)."""
    ptr = None if column_index is None else column_index.data_ptr()
    _check(load().gnna_release_graph(ptr))
    if column_index is None:
        _registered.clear()
    else:
        _registered.pop(ptr, None)


def runtime_counters() -> dict:
    out = (ctypes.c_int64 * 16)()
    n = load().gnna_runtime_counters_ex(out, 16)
    names = ("plan_builds", "launch_syncs", "launch_frees", "launch_mallocs", "backoff_skips", "sweep_launches",
             "pack_builds", "packed_launches", "full_hashes", "capture_scratch", "dense_block_builds", "dense_block_launches")
    return {name: int(out[i]) for i, name in enumerate(names) if i < n}


def debug_untrusted_copies(column_index) -> int:
    """For tests: how many packed id copies of this graph a full hash has marked "never trust again" (synchronises)."""
    n = load().gnna_debug_untrusted_copies(column_index.data_ptr())
    _check(min(n, 0))
    return n


def set_graph_phases(column_index, dim: int, column_phases: int) -> None:
    """Measured schedule for `dim`-wide aggregations on this graph (0 removes it); see include/gnna.h."""
    _check(load().gnna_set_graph_phases(column_index.data_ptr(), int(dim), int(column_phases)))
    if column_phases > 0:
        _forget_when_freed(column_index)


def xtg(X, G, out=None):
    """dW[K, N] = X^T G for X [M, K], G [M, N] (fp32, MFMA): the weight gradient of the dense update."""
    _need_device(X, "xtg")
    assert X.dtype == torch.float32 and G.dtype == torch.float32 and X.dim() == 2 and G.dim() == 2
    assert X.shape[0] == G.shape[0]
    X, G = X.contiguous(), G.contiguous()
    if out is None:
        out = torch.empty(X.shape[1], G.shape[1], dtype=torch.float32, device=X.device)
    _call(X.device, "gnna_xtg_f32", X.data_ptr(), G.data_ptr(), out.data_ptr(), X.shape[0], X.shape[1], G.shape[1])
    return out


def sddmm(dst_feat, src_feat, column_index, part_pointers, part2Node, partSize=32, out=None):
    """edge_out[e] = <dst_feat[row(e)], src_feat[column_index[e]]> over the neighbor-group partition
    (build-defined extension, see include/gnna.h).  Both feature matrices may be row-strided views (stride(1) == 1):
    their stride(0) is handed over as the leading dimension (gnna_sddmm_ld_f32)."""
    _need_device(dst_feat, "sddmm")
    ap, n_out, dim, ld_dst = _rows_view(dst_feat, "dst_feat")
    bp, n_in, dim_b, ld_src = _rows_view(src_feat, "src_feat")
    assert dim == dim_b and dst_feat.device == src_feat.device
    if out is None:
        out = torch.zeros(column_index.numel(), dtype=torch.float32, device=dst_feat.device)
    tail = (column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(), out.data_ptr(), n_out, n_in, dim,
            part2Node.numel(), int(partSize))
    if ld_dst == dim and ld_src == dim:
        _call(dst_feat.device, "gnna_sddmm_f32", ap, bp, *tail)
    else:
        _call(dst_feat.device, "gnna_sddmm_ld_f32", ap, ld_dst, bp, ld_src, *tail)
    return out


def agg_edge(X, column_index, edge_weight, part_pointers, part2Node, num_out_rows, partSize=32, out=None,
             accumulate=False, relu=False):
    """gnna_agg_edge_ld_f32: out[i] (+)= sum_e w[e] * X[column_index[e]] with caller-supplied edge weights `edge_weight`
    ([nnz] float32, indexed like column_index).  Strided X / out as in agg_ld."""
    _need_device(X, "aggregation")
    assert edge_weight.dtype == torch.float32 and edge_weight.is_contiguous() and edge_weight.numel() == column_index.numel(), \
        "edge_weight must be a contiguous float32 tensor indexed like column_index"
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    out, yp, ld_out = _out_rows(out, num_out_rows, dim, X.device, accumulate)
    _call(X.device, "gnna_agg_edge_ld_f32", xp, ld_in, n_in, column_index.data_ptr(), edge_weight.data_ptr(), part_pointers.data_ptr(),
          part2Node.data_ptr(), yp, ld_out, int(num_out_rows), dim, part2Node.numel(), int(partSize), _flags(accumulate, relu))
    return out


def edge_softmax(scores, row_pointers, out=None):
    """gnna_edge_softmax_f32: softmax over every row's edges; scores [nnz] or head-major [heads, nnz] (contiguous)."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() in (1, 2)
    heads, nnz = (1, scores.numel()) if scores.dim() == 1 else scores.shape
    out = torch.empty_like(scores) if out is None else out
    _call(scores.device, "gnna_edge_softmax_f32", scores.data_ptr(), row_pointers.data_ptr(), row_pointers.numel() - 1, nnz, heads,
          out.data_ptr())
    return out


def edge_softmax_backward(probs, grad_probs, row_pointers, out=None):
    """gnna_edge_softmax_backward_f32: grad_scores = probs * (grad_probs - sum_row probs * grad_probs)."""
    assert probs.is_cuda and probs.dtype == torch.float32 and probs.is_contiguous() and probs.dim() in (1, 2)
    assert grad_probs.shape == probs.shape and grad_probs.dtype == torch.float32 and grad_probs.is_contiguous()
    heads, nnz = (1, probs.numel()) if probs.dim() == 1 else probs.shape
    out = torch.empty_like(probs) if out is None else out
    _call(probs.device, "gnna_edge_softmax_backward_f32", probs.data_ptr(), grad_probs.data_ptr(), row_pointers.data_ptr(),
          row_pointers.numel() - 1, nnz, heads, out.data_ptr())
    return out


def reverse_edges(row_pointers, column_index) -> torch.Tensor:
    """gnna_reverse_edges_i32 (host): rev[e] = position of the edge col(e) -> row(e) matching e, int32 [nnz] on the CPU.
    Raises GnnaError, naming the first unmatched edge, when the graph's structure is not symmetric."""
    rp, ci = _host_i32(row_pointers), _host_i32(column_index)
    rev = torch.empty(ci.numel(), dtype=torch.int32)
    _check(load().gnna_reverse_edges_i32(rp.data_ptr(), ci.data_ptr(), rp.numel() - 1, rev.data_ptr()))
    return rev


REDUCE_MAX, REDUCE_MIN = 0, 1   # GNNA_REDUCE_MAX / GNNA_REDUCE_MIN


def _arg_view(t: torch.Tensor, rows: int, dim: int, what: str):
    """(data pointer, leading dimension) of a 2-D int32 device tensor [rows, dim] whose rows are contiguous."""
    assert t.dtype == torch.int32 and t.dim() == 2 and tuple(t.shape) == (rows, dim), f"{what} must be int32 [{rows}, {dim}]"
    ptr, _, _, ld = _rows_view(t, what, dtype=torch.int32, unit="elements")
    return ptr, ld


def agg_reduce_ld(op, X, column_index, part_pointers, part2Node, partSize=32, *, num_out_rows=None, out=None, want_arg=True,
                  relu=False, arg=None):
    """gnna_agg_reduce_ld_f32: out[i, f] = max / min (op = REDUCE_MAX / REDUCE_MIN) over the edges e of row i of
    X[column_index[e], f] and arg[i, f] = the smallest such position e (int32; -1 and out = 0 for rows without edges).
    -> (out, arg); arg is None with want_arg=False.  `X`, `out` and a caller's `arg` may be row-strided views (stride(1) == 1):
    they are passed with their leading dimension, no copy.  relu: out = max(out, 0), arg unchanged."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    n_out = n_in if num_out_rows is None else int(num_out_rows)
    out, yp, ld_out = _out_rows(out, n_out, dim, X.device)
    ap, ld_arg = None, dim
    if arg is not None or want_arg:
        if arg is None:
            arg = _fresh_output((n_out, dim), X.device, torch.int32)
        assert arg.device == X.device
        ap, ld_arg = _arg_view(arg, n_out, dim, "arg")
    _call(X.device, "gnna_agg_reduce_ld_f32", int(op), xp, ld_in, n_in, column_index.data_ptr(), part_pointers.data_ptr(),
          part2Node.data_ptr(), yp, ld_out, ap, ld_arg, n_out, dim, part2Node.numel(), int(partSize), _flags(relu=relu))
    return out, arg


def scatter_arg_ld(grad_out, arg, column_index, num_in_rows, out=None, accumulate=False):
    """gnna_scatter_arg_ld_f32, the backward of agg_reduce_ld: out[column_index[arg[i, f]], f] += grad_out[i, f] for every
    arg[i, f] >= 0; `out` [num_in_rows, dim] is cleared first unless accumulate.  Strided views as in agg_reduce_ld."""
    _need_device(grad_out, "scatter_arg")
    gp, n_out, dim, ld_go = _rows_view(grad_out, "grad_out")
    ap, ld_arg = _arg_view(arg, n_out, dim, "arg")
    out, op_, ld_gi = _out_rows(out, int(num_in_rows), dim, grad_out.device, accumulate)
    assert arg.device == grad_out.device
    _call(grad_out.device, "gnna_scatter_arg_ld_f32", gp, ld_go, ap, ld_arg, column_index.data_ptr(), n_out, op_, ld_gi,
          int(num_in_rows), dim, _flags(accumulate))
    return out


STATS = ("sum", "sumsq", "max", "min")


def _stat_outputs(names, want, out, rows, dim, device):
    """(results, argument run) of the statistics `names` of agg_stats_ld / segment_pool: (value, ld) for each and (arg, ld_arg),
    the int32 positions, after "max" and "min".  One not in `want` is handed over as (None, dim).  A tensor of the dict `out` is
    used where it supplies one; the positions are not computed when `out` holds the value but not them."""
    out = dict(out or {})
    res, args = {}, []
    for name in names:
        vp, ld = None, dim
        if name in want:
            res[name], vp, ld = _out_rows(out.get(name), rows, dim, device)
        args += [vp, ld]
        if name in ("max", "min"):
            ap, ld_arg = None, dim
            if name in want and ("arg" + name in out or name not in out):
                arg = out.get("arg" + name)
                if arg is None:
                    arg = _fresh_output((rows, dim), device, torch.int32)
                assert arg.device == device
                ap, ld_arg = _arg_view(arg, rows, dim, "arg" + name)
                res["arg" + name] = arg
            args += [ap, ld_arg]
    return res, args


def agg_stats_ld(X, column_index, part_pointers, part2Node, num_out_rows=None, partSize=32, want=STATS, out=None):
    """gnna_agg_stats_ld_f32 (include/gnna_stats.h): the statistics named in `want` over the edges e of every row i of
    x = X[column_index[e], f], from one walk over the ids and one load of every source row -- "sum", "sumsq" (sum of x * x), "max"
    and "min", the last two with the smallest winning position e ("argmax" / "argmin", int32; -1 and 0 for rows without edges) and
    the bits agg_reduce_ld gives.  -> a dict with a tensor [num_out_rows, dim] for every name wanted, "argmax" / "argmin" next to
    "max" / "min".  `X` may be a row-strided view (stride(1) == 1), and so may the tensors of `out`, a dict that supplies some of
    the results (float32; int32 for the positions, which are not computed when `out` holds the value but not them)."""
    _need_device(X, "aggregation")
    want = tuple(want)
    unknown = [w for w in want if w not in STATS]
    if unknown or not want:
        raise ValueError(f"want must name some of {STATS} (got {want!r})")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    n_out = n_in if num_out_rows is None else int(num_out_rows)
    res, args = _stat_outputs(STATS, want, out, n_out, dim, X.device)
    _call(X.device, "gnna_agg_stats_ld_f32", xp, ld_in, n_in, column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(),
          *args, n_out, dim, part2Node.numel(), int(partSize), 0)
    return res


def _temp_arg(temp, dim, device):
    """(pointer, length) of a temperature: a float32 device tensor of 1 or `dim` elements, contiguous."""
    assert temp.dtype == torch.float32 and temp.device == device and temp.is_contiguous() and temp.numel() in (1, dim), \
        f"temp must be a contiguous float32 tensor of 1 or {dim} elements on {device}"
    return temp.data_ptr(), temp.numel()


def _ids_ptr(column_index, row_pointers):
    """column_index's address; a graph without edges has none, and row_pointers' stands for it (no id is ever read)."""
    return column_index.data_ptr() or row_pointers.data_ptr()


def agg_softmax(X, temp, row_pointers, column_index, num_out_rows=None, want_sq=False, out=None, lse=None, sq=None):
    """gnna_agg_softmax_ld_f32 (include/gnna_softagg.h): softmax aggregation with a temperature, per channel, in one gather.  Over the
    edges i <- j of row i of the CSR (row_pointers, column_index), with s = temp[f] * X[j, f]: lse[i, f] = logsumexp_j s,
    out[i, f] = sum_j exp(s - lse) X[j, f] and, with want_sq (or a given `sq`), sq[i, f] = sum_j exp(s - lse) X[j, f]^2; rows
    without edges get 0.  `temp`: a float32 device tensor of 1 or dim elements.  -> (out, lse, sq | None), each
    [num_out_rows, dim] (num_out_rows: row_pointers.numel() - 1 when not given).  `X` and a caller's `out` / `lse` / `sq` may be
    row-strided views (stride(1) == 1).  The same bits on every run; accepted under set_tuning(deterministic=1)."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    n_out = row_pointers.numel() - 1 if num_out_rows is None else int(num_out_rows)
    assert row_pointers.numel() == n_out + 1, f"row_pointers must be [num_out_rows + 1 = {n_out + 1}] (got {row_pointers.numel()} entries)"
    tp, tl = _temp_arg(temp, dim, X.device)
    out, op_, ld_out = _out_rows(out, n_out, dim, X.device)
    lse, lp, ld_lse = _out_rows(lse, n_out, dim, X.device)
    qp, ld_sq = None, dim
    if want_sq or sq is not None:
        sq, qp, ld_sq = _out_rows(sq, n_out, dim, X.device)
    _call(X.device, "gnna_agg_softmax_ld_f32", xp, ld_in, n_in, tp, tl, row_pointers.data_ptr(), _ids_ptr(column_index, row_pointers),
          op_, ld_out, lp, ld_lse, qp, ld_sq, n_out, dim, 0)
    return out, lse, sq


def agg_softmax_backward(X, temp, lse, Y, dY, t_row_pointers, t_column_index, out=None):
    """gnna_agg_softmax_backward_ld_f32: dX[j, f] = sum over the transposed edges j <- i of alpha * dY[i, f] *
    (1 + temp[f] * (X[j, f] - Y[i, f])) with alpha = exp(temp[f] * X[j, f] - lse[i, f]), from agg_softmax's `lse` and `out` (Y).
    (t_row_pointers, t_column_index): A^T as a CSR of X.shape[0] rows whose ids are destination rows.  -> dX like X; source rows
    without transposed edges get 0.  Strided views as in agg_softmax.  The gradient of `temp` needs no call:
    dt[f] = sum_i dY[i, f] * (sq[i, f] - Y[i, f]^2)."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    assert t_row_pointers.numel() == n_in + 1, f"t_row_pointers must be [num_in_rows + 1 = {n_in + 1}] (got {t_row_pointers.numel()} entries)"
    tp, tl = _temp_arg(temp, dim, X.device)
    lp, n_out, w, ld_lse = _rows_view(lse, "lse")
    yp, ny, wy, ld_y = _rows_view(Y, "Y")
    gp, ng, wg, ld_dy = _rows_view(dY, "dY")
    assert (ny, ng) == (n_out, n_out) and (w, wy, wg) == (dim, dim, dim), "lse, Y and dY must be [num_out_rows, dim]"
    out, op_, ld_din = _out_rows(out, n_in, dim, X.device)
    _call(X.device, "gnna_agg_softmax_backward_ld_f32", xp, ld_in, n_in, tp, tl, lp, ld_lse, yp, ld_y, gp, ld_dy,
          t_row_pointers.data_ptr(), _ids_ptr(t_column_index, t_row_pointers), op_, ld_din, n_out, dim, 0)
    return out


EDGE_ADD, EDGE_MUL = 0, 1               # GNNA_EDGE_ADD / GNNA_EDGE_MUL
EDGE_ACT_NONE, EDGE_ACT_RELU = 0, 1     # GNNA_EDGE_ACT_NONE / GNNA_EDGE_ACT_RELU


def _edge_rows(E, nnz, dim, device, what):
    """(pointer, leading dimension) of an edge-major float32 [nnz, dim] device tensor with contiguous rows."""
    assert E.dim() == 2 and tuple(E.shape) == (nnz, dim) and E.device == device, \
        f"{what} must be [nnz = {nnz}, dim = {dim}] on {device} (got {tuple(E.shape)})"
    if nnz == 0:                            # no row: nothing is strided, whatever strides an empty tensor carries
        assert E.dtype == torch.float32, f"{what} must be a float32 tensor"
        return None, dim
    ep, _, _, ld_e = _rows_view(E, what)
    return ep, ld_e


def agg_edge_feat(X, E, row_pointers, column_index, num_out_rows=None, combine=EDGE_ADD, act=EDGE_ACT_NONE, out=None):
    """gnna_agg_edge_feat_ld_f32 (include/gnna_edgefeat.h): out[i, f] = sum over the positions e of row i of the CSR (row_pointers,
    column_index) of act(X[column_index[e], f] (+ | *) E[e, f]) -- combine EDGE_ADD | EDGE_MUL, act EDGE_ACT_NONE | EDGE_ACT_RELU --
    in one gather that streams E once.  E: [nnz, dim], edge-major in the order of column_index.  -> out [num_out_rows, dim]
    (num_out_rows: row_pointers.numel() - 1 when not given); rows without edges get 0.  `X`, `E` and a caller's `out` may be
    row-strided views (stride(1) == 1).  The same bits on every run; accepted under set_tuning(deterministic=1)."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    n_out = row_pointers.numel() - 1 if num_out_rows is None else int(num_out_rows)
    assert row_pointers.numel() == n_out + 1, f"row_pointers must be [num_out_rows + 1 = {n_out + 1}] (got {row_pointers.numel()} entries)"
    nnz = column_index.numel()
    ep, ld_e = _edge_rows(E, nnz, dim, X.device, "E")
    out, op_, ld_out = _out_rows(out, n_out, dim, X.device)
    _call(X.device, "gnna_agg_edge_feat_ld_f32", xp, ld_in, n_in, ep, ld_e, nnz, row_pointers.data_ptr(), _ids_ptr(column_index, row_pointers),
          op_, ld_out, n_out, dim, int(combine), int(act), 0)
    return out


def agg_edge_feat_backward(X, E, dY, row_pointers, column_index, t_row_pointers=None, t_column_index=None, t_edge_pos=None,
                           combine=EDGE_ADD, act=EDGE_ACT_NONE, want_dx=True, want_de=True, dX=None, dE=None):
    """gnna_agg_edge_feat_backward_ld_f32: the gradients of agg_edge_feat from its inputs and dY [num_out_rows, dim] -> (dX | None,
    dE | None).  dE [nnz, dim] is made over the rows of the structure itself.  dX (like X) is made over A^T (t_row_pointers,
    t_column_index: X.shape[0] rows whose ids are destination rows) with t_edge_pos[p] = the position in column_index of the edge
    that transposed position p stands for (transpose_csr's perm, or reverse_edges of a symmetric structure); the three are needed
    only with want_dx.  The relu mask is recomputed from X and E: nothing was saved.  Strided views as in agg_edge_feat."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_in = _rows_view(X, "X")
    gp, n_out, wg, ld_dy = _rows_view(dY, "dY")
    assert wg == dim and row_pointers.numel() == n_out + 1, "dY must be [num_out_rows, dim] and row_pointers [num_out_rows + 1]"
    nnz = column_index.numel()
    ep, ld_e = _edge_rows(E, nnz, dim, X.device, "E")
    dxp, ld_din, dep, ld_de, t_args = None, dim, None, dim, (None, None, None)
    if want_dx:
        assert t_row_pointers is not None and t_column_index is not None and t_edge_pos is not None, \
            "want_dx needs the transposed structure and t_edge_pos"
        assert t_row_pointers.numel() == n_in + 1 and t_column_index.numel() == nnz and t_edge_pos.numel() == nnz and \
            t_edge_pos.dtype == torch.int32, "t_row_pointers must be [num_in_rows + 1], t_column_index and t_edge_pos int32 [nnz]"
        dX, dxp, ld_din = _out_rows(dX, n_in, dim, X.device)
        t_args = (t_row_pointers.data_ptr(), _ids_ptr(t_column_index, t_row_pointers), _ids_ptr(t_edge_pos, t_row_pointers))
    else:
        dX = None
    if want_de:
        dE, dep, ld_de = _out_rows(dE, nnz, dim, X.device)
    else:
        dE = None
    _call(X.device, "gnna_agg_edge_feat_backward_ld_f32", xp, ld_in, n_in, ep, ld_e, nnz, gp, ld_dy, row_pointers.data_ptr(),
          _ids_ptr(column_index, row_pointers), *t_args, dxp, ld_din, dep, ld_de, n_out, dim, int(combine), int(act), 0)
    return dX, dE


POOL_TILE_ROWS = 256            # GNNA_POOL_TILE_ROWS: the rows a wavefront walks; segments that cross a multiple of it are joined from pieces
POOL_LONG_STEPS = 16            # GNNA_POOL_LONG_STEPS: a segment of more than this many tiles per slot of a wavefront is joined by a workgroup
POOL_MEAN = 1                   # GNNA_POOL_MEAN
POOL_STATS = ("sum", "max", "min")


def _graph_pointers_arg(graph_pointers, device):
    assert graph_pointers.dtype == torch.int32 and graph_pointers.dim() == 1 and graph_pointers.numel() >= 1 and \
        graph_pointers.is_contiguous() and graph_pointers.device == device, \
        f"graph_pointers must be a contiguous int32 tensor [num_graphs + 1] on {device}"
    return graph_pointers.data_ptr(), graph_pointers.numel() - 1


def segment_pool(X, graph_pointers, want=("sum",), mean=False, out=None):
    """gnna_segment_pool_ld_f32 (include/gnna_pool.h): the statistics named in `want` -- "sum", "max", "min" -- over the rows
    [graph_pointers[g], graph_pointers[g + 1]) of X for every graph g of a batch, from one read of X.  "max" / "min" come with
    "argmax" / "argmin", the smallest winning row (int32; -1 and the value 0 for a graph without rows), in the order of
    agg_reduce_ld; mean=True divides the sum by the rows of the graph (0 for none).  -> a dict with a tensor [num_graphs, dim] for
    every name wanted.  `X` may be a row-strided view (stride(1) == 1), and so may the tensors of `out`, a dict that supplies some
    of the results (the rows are not computed when `out` holds the value but not them).  graph_pointers: int32 [num_graphs + 1] on
    X's device, not descending; rows outside [graph_pointers[0], graph_pointers[-1]) belong to no graph.  The same bits on every
    run; accepted under set_tuning(deterministic=1)."""
    want = tuple(want)
    if not want or [w for w in want if w not in POOL_STATS]:
        raise ValueError(f"want must name some of {POOL_STATS} (got {want!r})")
    _need_device(X, "segment_pool")
    xp, n, dim, ld_in = _rows_view(X, "X")
    gp, G = _graph_pointers_arg(graph_pointers, X.device)
    res, args = _stat_outputs(POOL_STATS, want, out, G, dim, X.device)
    if G > 0:           # (the outputs of a batch without graphs are empty and have no address)
        _call(X.device, "gnna_segment_pool_ld_f32", xp if n > 0 else None, ld_in, n, gp, G, *args, dim, POOL_MEAN if mean else 0)
    return res


def segment_pool_backward(graph_pointers, num_rows, d_sum=None, d_max=None, argmax=None, d_min=None, argmin=None, mean=False, out=None):
    """gnna_segment_pool_backward_ld_f32: dX[r, f] = s * d_sum[g, f] + (argmax[g, f] == r) * d_max[g, f] + (argmin[g, f] == r) *
    d_min[g, f] for the rows r of graph g, s = 1 or, with mean, 1 / the rows of the graph; a row of no graph gets 0.  One pass that
    writes every element of dX [num_rows, dim] once, nothing is cleared first.  Any of d_sum, (d_max, argmax), (d_min, argmin) may be
    None, not all.  Strided views as in segment_pool."""
    given = [t for t in (d_sum, d_max, d_min) if t is not None]
    if not given:
        raise ValueError("segment_pool_backward needs d_sum, d_max or d_min")
    if (d_max is None) != (argmax is None) or (d_min is None) != (argmin is None):
        raise ValueError("d_max comes with argmax, d_min with argmin")
    _need_device(given[0], "segment_pool_backward")
    device = given[0].device
    gp, G = _graph_pointers_arg(graph_pointers, device)
    dim = given[0].shape[1]
    args = []
    for grad, arg, name in ((d_sum, None, "d_sum"), (d_max, argmax, "d_max"), (d_min, argmin, "d_min")):
        if grad is None:
            args += [None, dim] * (1 if name == "d_sum" else 2)
            continue
        vp, rows, w, ld = _rows_view(grad, name)
        assert (rows, w) == (G, dim) and grad.device == device, f"{name} must be [num_graphs = {G}, dim = {dim}] on {device}"
        args += [vp, ld]
        if name != "d_sum":
            assert arg.device == device
            args += list(_arg_view(arg, G, dim, "arg" + name[2:]))
    out, op_, ld_din = _out_rows(out, int(num_rows), dim, device)
    if G == 0:          # (the gradients of a batch without graphs are empty and have no address: one row stands for them, unread)
        stand_in = torch.zeros(1, dim, dtype=torch.float32, device=device)
        args = [stand_in.data_ptr(), dim] + [None, dim] * 4
    _call(device, "gnna_segment_pool_backward_ld_f32", *args, gp, G, op_ if int(num_rows) > 0 else None, ld_din, int(num_rows), dim,
          POOL_MEAN if mean else 0)
    return out


def _param_arg(t, dim, device, what):
    """The address of a per-column parameter, a contiguous float32 tensor [dim] on `device`; None stands for the default."""
    if t is None:
        return None
    assert t.dtype == torch.float32 and t.device == device and t.is_contiguous() and tuple(t.shape) == (dim,), \
        f"{what} must be a contiguous float32 tensor [{dim}] on {device}"
    return t.data_ptr()


def segment_moments(X, graph_pointers, out=None):
    """gnna_segment_moments_ld_f32 (include/gnna_segnorm.h): mean[g, f] and m2[g, f] = sum (x - mean)^2 over the rows
    [graph_pointers[g], graph_pointers[g + 1]) of X for every graph g, from one read of X; both 0 for a graph without rows.  The
    moments are centred as they are gathered (pairwise merges of (count, mean, m2)), never made from sums of x and x^2.
    -> dict(mean=, m2=), each [num_graphs, dim].  `X` may be a row-strided view (stride(1) == 1), and so may the tensors of `out`,
    a dict that supplies some of the results.  graph_pointers as in segment_pool.  The same bits on every run; accepted under
    set_tuning(deterministic=1)."""
    _need_device(X, "segment_moments")
    xp, n, dim, ld_in = _rows_view(X, "X")
    gp, G = _graph_pointers_arg(graph_pointers, X.device)
    given = dict(out or {})
    mean, mp, ld_mean = _out_rows(given.get("mean"), G, dim, X.device)
    m2, qp, ld_m2 = _out_rows(given.get("m2"), G, dim, X.device)
    if G > 0:           # (the outputs of a batch without graphs are empty and have no address)
        _call(X.device, "gnna_segment_moments_ld_f32", xp if n > 0 else None, ld_in, n, gp, G, mp, ld_mean, qp, ld_m2, dim, 0)
    return {"mean": mean, "m2": m2}


def segment_norm(X, graph_pointers, weight=None, bias=None, alpha=None, eps=1e-5, out=None):
    """gnna_segment_norm_ld_f32: per-graph normalisation.  With mean and m2 as in segment_moments and n the rows of graph g:
    var = m2 / n + (1 - alpha)^2 mean^2, rstd = 1 / sqrt(var + eps), out[r, f] = weight * (x - alpha * mean) * rstd + bias for the
    rows r of graph g; a row of no graph gets 0, a graph without rows mean = rstd = 0.  weight / bias / alpha: float32 [dim] or
    None for 1 / 0 / 1.  -> dict(out= like X, mean=, rstd= [num_graphs, dim]): two reads of X, one write of `out`.  `X` and the
    tensors of `out`, a dict that supplies some of the results, may be row-strided views; "out" must not be X.  The same bits on
    every run; accepted under set_tuning(deterministic=1)."""
    _need_device(X, "segment_norm")
    xp, n, dim, ld_in = _rows_view(X, "X")
    gp, G = _graph_pointers_arg(graph_pointers, X.device)
    given = dict(out or {})
    y, yp, ld_out = _out_rows(given.get("out"), n, dim, X.device)
    mean, mp, ld_mean = _out_rows(given.get("mean"), G, dim, X.device)
    rstd, rp, ld_rstd = _out_rows(given.get("rstd"), G, dim, X.device)
    if n > 0 or G > 0:
        _call(X.device, "gnna_segment_norm_ld_f32", xp if n > 0 else None, ld_in, n, gp, G, _param_arg(weight, dim, X.device, "weight"),
              _param_arg(bias, dim, X.device, "bias"), _param_arg(alpha, dim, X.device, "alpha"), ctypes.c_float(eps),
              yp if n > 0 else None, ld_out, mp if G > 0 else None, ld_mean, rp if G > 0 else None, ld_rstd, dim, 0)
    return {"out": y, "mean": mean, "rstd": rstd}


def segment_norm_backward(dY, X, mean, rstd, graph_pointers, weight=None, alpha=None, need_input=True, out=None):
    """gnna_segment_norm_backward_ld_f32: from segment_norm's `mean` and `rstd` and the gradient dY of its `out`, with
    xhat = (x - alpha * mean) * rstd: seg_a[g, f] = sum dY and seg_b[g, f] = sum dY * xhat over the rows of graph g (one pass over dY
    and X), then d_input[r, f] = weight * rstd * (dY - xhat * B / n - alpha * (A / n - (1 - alpha) * mean * rstd * B / n)) in one
    pass that writes every element once; a row of no graph gets 0.  -> (d_input like X | None with need_input=False, seg_a, seg_b).
    The parameter gradients are [num_graphs, dim] arithmetic: d_bias = sum_g A, d_weight = sum_g B, d_alpha = -sum_g mean * weight *
    rstd * (A - (1 - alpha) * mean * rstd * B).  `out` may supply "d_input", "seg_a", "seg_b".  Strided views as in segment_norm."""
    _need_device(X, "segment_norm_backward")
    xp, n, dim, ld_in = _rows_view(X, "X")
    dp, nd, wd, ld_do = _rows_view(dY, "dY")
    gp, G = _graph_pointers_arg(graph_pointers, X.device)
    mp, gm, wm, ld_mean = _rows_view(mean, "mean")
    rp, gr, wr, ld_rstd = _rows_view(rstd, "rstd")
    assert (nd, wd) == (n, dim) and (gm, gr) == (G, G) and (wm, wr) == (dim, dim) and dY.device == mean.device == rstd.device == X.device, \
        f"dY must be [{n}, {dim}], mean and rstd [{G}, {dim}] on {X.device}"
    given = dict(out or {})
    d_input, dip, ld_din = None, None, dim
    if need_input:
        d_input, dip, ld_din = _out_rows(given.get("d_input"), n, dim, X.device)
    seg_a, ap, ld_a = _out_rows(given.get("seg_a"), G, dim, X.device)
    seg_b, bp, ld_b = _out_rows(given.get("seg_b"), G, dim, X.device)
    if G > 0 or (n > 0 and need_input):
        if G == 0:      # (the tensors of a batch without graphs are empty and have no address; none is read)
            mp = rp = ap = bp = None
        _call(X.device, "gnna_segment_norm_backward_ld_f32", dp if n > 0 else None, ld_do, xp if n > 0 else None, ld_in, mp, ld_mean,
              rp, ld_rstd, _param_arg(weight, dim, X.device, "weight"), _param_arg(alpha, dim, X.device, "alpha"), gp, G,
              dip if n > 0 else None, ld_din, ap, ld_a, bp, ld_b, n, dim, 0)
    return d_input, seg_a, seg_b


def _gate_view(gate, n, dim, device):
    """(pointer, gate_dim, leading dimension) of a gate [n], [n, 1] or [n, dim] on `device`: a score per row or per element."""
    g2 = gate.unsqueeze(1) if gate.dim() == 1 else gate
    gp_, rows, gate_dim, ld_gate = _rows_view(g2, "gate")
    assert rows == n and gate_dim in (1, dim) and gate.device == device, \
        f"gate must be [{n}], [{n}, 1] or [{n}, {dim}] on {device} (got {tuple(gate.shape)})"
    return gp_, gate_dim, ld_gate


def segment_attn_pool(X, gate, graph_pointers, out=None):
    """gnna_segment_attn_pool_ld_f32 (include/gnna_attnpool.h): attention pooling over the rows [graph_pointers[g],
    graph_pointers[g + 1]) of X for every graph g of a batch, from one read of X and of the gate.  `gate` is [N] or [N, 1] (a score
    per row) or [N, dim] (a score per element); with s = gate[r, c]: lse[g, c] = log sum_r exp(s) and out[g, f] =
    sum_r exp(s - lse[g, c]) * X[r, f]; a graph without rows gets 0 in both.  -> dict(out= [num_graphs, dim], lse= [num_graphs,
    gate_dim]).  `X`, `gate` (which may be `X` itself) and the tensors of `out`, a dict that supplies some of the results, may be
    row-strided views (stride(1) == 1); lse is not computed when `out` holds "out" but not "lse".  graph_pointers as in
    segment_pool.  Finite gates of any size neither overflow nor underflow to 0 / 0.  The same bits on every run; accepted under
    set_tuning(deterministic=1)."""
    _need_device(X, "segment_attn_pool")
    xp, n, dim, ld_in = _rows_view(X, "X")
    gtp, gate_dim, ld_gate = _gate_view(gate, n, dim, X.device)
    gp, G = _graph_pointers_arg(graph_pointers, X.device)
    given = dict(out or {})
    res = {}
    res["out"], op_, ld_out = _out_rows(given.get("out"), G, dim, X.device)
    lp, ld_lse = None, gate_dim
    if "lse" in given or "out" not in given:
        res["lse"], lp, ld_lse = _out_rows(given.get("lse"), G, gate_dim, X.device)
    if G > 0:           # (the outputs of a batch without graphs are empty and have no address)
        _call(X.device, "gnna_segment_attn_pool_ld_f32", xp if n > 0 else None, ld_in, n, gtp if n > 0 else None, ld_gate, gate_dim,
              gp, G, op_, ld_out, lp, ld_lse, dim, 0)
    return res


def segment_attn_pool_backward(X, gate, lse, Y, dY, graph_pointers, need_input=True, need_gate=True, out=None):
    """gnna_segment_attn_pool_backward_ld_f32: from segment_attn_pool's `lse` and `out` (Y) and the gradient dY of `out`, with
    alpha = exp(gate[r, c] - lse[g, c]) for the rows r of graph g: d_input[r, f] = alpha * dY[g, f] and d_gate[r, c] = alpha *
    dY[g, f] * (X[r, f] - Y[g, f]), summed over f for a gate per row; a row of no graph gets 0.  One pass that writes every element
    once, nothing is cleared first.  -> (d_input like X | None, d_gate [N, gate_dim] | None): need_input / need_gate (not both
    False) choose what is computed; `out` may supply "d_input" / "d_gate".  Strided views as in segment_attn_pool."""
    if not need_input and not need_gate:
        raise ValueError("segment_attn_pool_backward needs need_input or need_gate")
    _need_device(X, "segment_attn_pool_backward")
    xp, n, dim, ld_in = _rows_view(X, "X")
    gtp, gate_dim, ld_gate = _gate_view(gate, n, dim, X.device)
    gp, G = _graph_pointers_arg(graph_pointers, X.device)
    lp, gl, wl, ld_lse = _rows_view(lse, "lse")
    yp, gy, wy, ld_y = _rows_view(Y, "Y")
    dp, gd, wd, ld_dy = _rows_view(dY, "dY")
    assert (gl, gy, gd) == (G, G, G) and (wl, wy, wd) == (gate_dim, dim, dim) and lse.device == Y.device == dY.device == X.device, \
        f"lse must be [{G}, {gate_dim}], Y and dY [{G}, {dim}] on {X.device}"
    given = dict(out or {})
    d_input = d_gate = dip = dgp = None
    ld_din, ld_dgate = dim, gate_dim
    if need_input:
        d_input, dip, ld_din = _out_rows(given.get("d_input"), n, dim, X.device)
    if need_gate:
        d_gate, dgp, ld_dgate = _out_rows(given.get("d_gate"), n, gate_dim, X.device)
    if n > 0:
        if G == 0:      # (the tensors of a batch without graphs are empty and have no address; none is read)
            lp = yp = dp = None
        _call(X.device, "gnna_segment_attn_pool_backward_ld_f32", xp, ld_in, gtp, ld_gate, gate_dim, lp, ld_lse, yp, ld_y, dp, ld_dy,
              gp, G, dip, ld_din, dgp, ld_dgate, n, dim, 0)
    return d_input, d_gate


def _node_heads(t, n, what):
    """[n, heads] contiguous float32 device tensor -> heads."""
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == n and t.is_contiguous(), \
        f"{what} must be a contiguous float32 [{n}, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el " \
        f"have num_out_rows rows, er / d_er num_in_rows)"
    return t.shape[1]


def _gat_sizes(H, el, er, row_pointers):
    """(H's pointer, num_out_rows, num_in_rows, width, heads, ld_h) of a GAT attention call, taken from the tensors:
    num_in_rows = H.shape[0] = er.shape[0], num_out_rows = el.shape[0] = row_pointers.numel() - 1."""
    hp, n_in, width, ld_h = _rows_view(H, "H")
    assert el.dim() == 2 and row_pointers.dim() == 1, "el must be [num_out_rows, heads], row_pointers [num_out_rows + 1]"
    n_out = el.shape[0]
    assert row_pointers.numel() == n_out + 1, \
        f"row_pointers must be [num_out_rows + 1] with num_out_rows = el.shape[0] = {n_out} (got {row_pointers.numel()} entries)"
    heads = _node_heads(el, n_out, "el")
    assert _node_heads(er, n_in, "er") == heads and heads >= 1 and width % heads == 0, \
        "H must be [num_in_rows, heads * dim], er [num_in_rows, heads] and el [num_out_rows, heads]"
    return hp, n_out, n_in, width, heads, ld_h


def gat_forward(H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize=32, negative_slope=0.2, out=None,
                lse=None, relu=False):
    """gnna_gat_forward_f32: fused multi-head GAT attention.  H [N, heads * dim], el / er [N, heads] -> (out, lse) with
    out[i, h] = sum_e alpha(e, h) H[col(e), h], alpha = exp(leaky_relu(el[i, h] + er[j, h]) - lse[i, h]); no per-edge tensor.
    `H` and `out` may be row-strided views (stride(1) == 1): they are passed with their leading dimension.
    Rectangular structures (a sampled block): H [num_in_rows, heads * dim], er [num_in_rows, heads], el [num_out_rows, heads]
    with num_out_rows = row_pointers.numel() - 1 -> out [num_out_rows, heads * dim], lse [num_out_rows, heads]; when the two
    counts differ the call is gnna_gat_forward_rect_f32."""
    return _gat_forward(None, H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope, out, lse, relu)


def gat_forward_drop(H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope, attn_drop, rng_seed,
                     out=None, lse=None, relu=False):
    """gnna_gat_forward_drop_f32 (include/gnna_ext.h): gat_forward with attention dropout -- every alpha is scaled by
    k(rng_seed, i, j, h) = 0 or 1 / (1 - attn_drop), a function of the seed, the two row numbers and the head that every pass
    recomputes (no mask tensor).  lse is that of the undropped scores.  attn_drop in [0, 1), rng_seed in [0, 2^64).  -> (out, lse).
    Every structure goes through the one (rectangular) entry."""
    return _gat_forward((float(attn_drop), int(rng_seed)), H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize,
                        negative_slope, out, lse, relu)


def _gat_forward(drop, H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope, out, lse, relu):
    """What gat_forward and gat_forward_drop (drop = (attn_drop, rng_seed)) share."""
    _need_device(H, "GAT attention")
    hp, n_out, n_in, width, heads, ld_h = _gat_sizes(H, el, er, row_pointers)
    if out is None:
        out = _fresh_output((n_out, width), H.device)
    if lse is None:
        lse = _fresh_output((n_out, heads), H.device)
    op_, n_o, width_o, ld_out = _rows_view(out, "out")
    assert n_o == n_out and width_o == width and _node_heads(lse, n_out, "lse") == heads
    entry, sizes = ("gnna_gat_forward_f32", (n_out,)) if n_out == n_in else ("gnna_gat_forward_rect_f32", (n_out, n_in))
    if drop is not None:
        entry, sizes = "gnna_gat_forward_drop_f32", (n_out, n_in)
    _call(H.device, entry, hp, ld_h, el.data_ptr(), er.data_ptr(), row_pointers.data_ptr(), column_index.data_ptr(),
          part_pointers.data_ptr(), part2Node.data_ptr(), float(negative_slope), *(drop or ()), op_, ld_out, lse.data_ptr(), *sizes,
          heads, width // heads, part2Node.numel(), int(partSize), _flags(relu=relu))
    return out, lse


def gat_backward(H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize=32, negative_slope=0.2,
                 dH=None, transposed=None):
    """gnna_gat_backward_f32: (dH, d_el, d_er) of gat_forward for the gradient dY of its output Y, on a graph whose structure
    is symmetric (not checked here).  dH is the attention part only (sum alpha dY); strided H / Y / dY / dH as in gat_forward.
    transposed = (t_row_pointers, t_column_index, t_part_pointers, t_part2Node) of `transpose_csr` / `build_part_device` at the
    same partSize: gnna_gat_backward_dir_f32, exact on a directed graph.
    Rectangular structures (sizes as in gat_forward; Y, dY, lse have num_out_rows rows): gnna_gat_backward_rect_f32, which needs
    `transposed` (num_in_rows rows) -> dH [num_in_rows, heads * dim], d_el [num_out_rows, heads], d_er [num_in_rows, heads]."""
    return _gat_backward(None, H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope,
                         dH, transposed)


def gat_backward_drop(H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope,
                      attn_drop, rng_seed, dH=None, transposed=None):
    """gnna_gat_backward_drop_f32 (include/gnna_ext.h): (dH, d_el, d_er) of gat_forward_drop for the same attn_drop and rng_seed;
    Y is that call's output.  `transposed` as for gat_backward; without it (a square graph whose structure is symmetric, not
    checked here) the graph's own structure is passed as the transposed one."""
    return _gat_backward((float(attn_drop), int(rng_seed)), H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers,
                         part2Node, partSize, negative_slope, dH, transposed)


def _gat_backward(drop, H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope, dH,
                  transposed):
    """What gat_backward and gat_backward_drop (drop = (attn_drop, rng_seed)) share."""
    _need_device(H, "GAT attention")
    hp, n_out, n_in, width, heads, ld_h = _gat_sizes(H, el, er, row_pointers)
    yp, n_y, width_y, ld_y = _rows_view(Y, "Y")
    gp, n_g, width_g, ld_g = _rows_view(dY, "dY")
    assert _node_heads(lse, n_out, "lse") == heads
    assert (n_y, width_y) == (n_out, width) and (n_g, width_g) == (n_out, width), \
        "Y and dY must be [num_out_rows, heads * dim] (the shape of H on a square graph)"
    rect = n_out != n_in
    if rect and transposed is None:
        raise GnnaError(f"GAT attention backward on a rectangular structure ({n_out} destination rows, {n_in} source rows) needs "
                        "`transposed`: a rectangular structure is never its own transpose")
    if dH is None:
        dH = _fresh_output((n_in, width), H.device)
    dp, n_d, width_d, ld_d = _rows_view(dH, "dH")
    assert (n_d, width_d) == (n_in, width), "dH must have the shape of H"
    if transposed is not None:
        t_rp, t_ci, t_pp, t_p2n = transposed
        for t in (column_index, part_pointers, part2Node, t_rp, t_ci, t_pp, t_p2n):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == H.device, \
                "the graph and its transpose must be contiguous int32 tensors on H's device"
        assert t_rp.numel() == n_in + 1 and t_pp.numel() == t_p2n.numel() + 1, \
            "transposed: [num_in_rows + 1] row pointers, [P + 1] / [P] partition"
    d_el, d_er = _fresh_output((n_out, heads), H.device), _fresh_output((n_in, heads), H.device)
    head = (hp, ld_h, el.data_ptr(), er.data_ptr(), lse.data_ptr(), yp, ld_y, gp, ld_g, row_pointers.data_ptr(),
            column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr())
    outs = (float(negative_slope), *(drop or ()), dp, ld_d, d_el.data_ptr(), d_er.data_ptr())
    if drop is not None:
        if transposed is None:
            t_rp, t_ci, t_pp, t_p2n = row_pointers, column_index, part_pointers, part2Node
        _call(H.device, "gnna_gat_backward_drop_f32", *head, part2Node.numel(), t_rp.data_ptr(), t_ci.data_ptr(), t_pp.data_ptr(),
              t_p2n.data_ptr(), t_p2n.numel(), *outs, n_out, n_in, heads, width // heads, int(partSize), 0)
    elif transposed is not None:
        _call(H.device, "gnna_gat_backward_rect_f32" if rect else "gnna_gat_backward_dir_f32", *head, part2Node.numel(),
              t_rp.data_ptr(), t_ci.data_ptr(), t_pp.data_ptr(), t_p2n.data_ptr(), t_p2n.numel(), *outs,
              *((n_out, n_in) if rect else (n_out,)), heads, width // heads, int(partSize), 0)
    else:
        _call(H.device, "gnna_gat_backward_f32", *head, *outs, n_out, heads, width // heads, part2Node.numel(), int(partSize), 0)
    return dH, d_el, d_er


def _edge_heads(t, nnz, heads, what):
    assert t.dtype == torch.float32 and t.dim() == 2 and tuple(t.shape) == (nnz, heads) and t.is_contiguous(), \
        f"{what} must be a contiguous float32 [num_edges = {nnz}, heads = {heads}] tensor (edge-major, indexed like column_index)"


def gat_edge_forward(H, el, er, ee, row_pointers, column_index, part_pointers, part2Node, partSize=32, negative_slope=0.2,
                     attn_drop=0.0, rng_seed=0, out=None, lse=None, relu=False):
    """gnna_gat_edge_forward_f32 (include/gnna_gat_edge.h): gat_forward_drop with a per-edge score term, z = el[i, h] + er[j, h] +
    ee[e, h] for the edge at position e of column_index.  ee is [num_edges, heads] float32, contiguous.  -> (out, lse)."""
    _need_device(H, "GAT attention")
    hp, n_out, n_in, width, heads, ld_h = _gat_sizes(H, el, er, row_pointers)
    nnz = column_index.numel()
    _edge_heads(ee, nnz, heads, "ee")
    if out is None:
        out = _fresh_output((n_out, width), H.device)
    if lse is None:
        lse = _fresh_output((n_out, heads), H.device)
    op_, n_o, width_o, ld_out = _rows_view(out, "out")
    assert n_o == n_out and width_o == width and _node_heads(lse, n_out, "lse") == heads
    _call(H.device, "gnna_gat_edge_forward_f32", hp, ld_h, el.data_ptr(), er.data_ptr(), ee.data_ptr(), row_pointers.data_ptr(),
          column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(), float(negative_slope), float(attn_drop),
          int(rng_seed), op_, ld_out, lse.data_ptr(), n_out, n_in, nnz, heads, width // heads, part2Node.numel(), int(partSize),
          _flags(relu=relu))
    return out, lse


def gat_edge_backward(H, el, er, ee, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, t_edge_pos, partSize=32,
                      negative_slope=0.2, attn_drop=0.0, rng_seed=0, transposed=None, dH=None, d_ee=None, accumulate=False):
    """gnna_gat_edge_backward_f32: (dH, d_el, d_er, d_ee) of gat_edge_forward for the gradient dY of its output Y (same ee,
    attn_drop and rng_seed).  t_edge_pos int32 [num_edges]: the forward position of every position of the transposed structure --
    the `perm` of transpose_csr with `transposed` = (t_row_pointers, t_column_index, t_part_pointers, t_part2Node), or the
    reverse-edge map of a symmetric graph without `transposed` (its own structure is passed as the transposed one).  d_ee
    [num_edges, heads] has one writer per element: the same bits on every run."""
    _need_device(H, "GAT attention")
    hp, n_out, n_in, width, heads, ld_h = _gat_sizes(H, el, er, row_pointers)
    nnz = column_index.numel()
    _edge_heads(ee, nnz, heads, "ee")
    yp, n_y, width_y, ld_y = _rows_view(Y, "Y")
    gp, n_g, width_g, ld_g = _rows_view(dY, "dY")
    assert _node_heads(lse, n_out, "lse") == heads
    assert (n_y, width_y) == (n_out, width) and (n_g, width_g) == (n_out, width), "Y and dY must be [num_out_rows, heads * dim]"
    if n_out != n_in and transposed is None:
        raise GnnaError(f"GAT attention backward on a rectangular structure ({n_out} destination rows, {n_in} source rows) needs "
                        "`transposed`: a rectangular structure is never its own transpose")
    if transposed is None:
        transposed = (row_pointers, column_index, part_pointers, part2Node)
    t_rp, t_ci, t_pp, t_p2n = transposed
    for t in (column_index, part_pointers, part2Node, t_rp, t_ci, t_pp, t_p2n, t_edge_pos):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == H.device, \
            "the graph, its transpose and t_edge_pos must be contiguous int32 tensors on H's device"
    assert t_rp.numel() == n_in + 1 and t_pp.numel() == t_p2n.numel() + 1, \
        "transposed: [num_in_rows + 1] row pointers, [P + 1] / [P] partition"
    assert t_edge_pos.numel() == nnz and t_ci.numel() == nnz, "t_edge_pos and the transposed column_index must be [num_edges]"
    if dH is None:
        dH = _fresh_output((n_in, width), H.device)
    dp, n_d, width_d, ld_d = _rows_view(dH, "dH")
    assert (n_d, width_d) == (n_in, width), "dH must have the shape of H"
    if d_ee is None:
        d_ee = _fresh_output((nnz, heads), H.device)
    _edge_heads(d_ee, nnz, heads, "d_ee")
    d_el, d_er = _fresh_output((n_out, heads), H.device), _fresh_output((n_in, heads), H.device)
    _call(H.device, "gnna_gat_edge_backward_f32", hp, ld_h, el.data_ptr(), er.data_ptr(), ee.data_ptr(), lse.data_ptr(), yp, ld_y, gp,
          ld_g, row_pointers.data_ptr(), column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(), part2Node.numel(),
          t_rp.data_ptr(), t_ci.data_ptr(), t_pp.data_ptr(), t_p2n.data_ptr(), t_p2n.numel(), t_edge_pos.data_ptr(),
          float(negative_slope), float(attn_drop), int(rng_seed), dp, ld_d, d_el.data_ptr(), d_er.data_ptr(), d_ee.data_ptr(), n_out,
          n_in, nnz, heads, width // heads, int(partSize), _flags(accumulate))
    return dH, d_el, d_er, d_ee


def gat_alpha(el, er, ee, lse, row_pointers, column_index, negative_slope=0.2, alpha=None):
    """gnna_gat_alpha_f32: the attention coefficients edge for edge, alpha [num_edges, heads] = exp(leaky_relu(el[i, h] + er[j, h]
    + ee[e, h]) - lse[i, h]) (undropped; 0 for a skipped edge), from the lse of a forward call.  ee None: those of gat_forward."""
    _need_device(el, "GAT attention")
    n_out, n_in, nnz = el.shape[0], er.shape[0], column_index.numel()
    heads = _node_heads(el, n_out, "el")
    assert _node_heads(er, n_in, "er") == heads and _node_heads(lse, n_out, "lse") == heads and row_pointers.numel() == n_out + 1
    if ee is not None:
        _edge_heads(ee, nnz, heads, "ee")
    if alpha is None:
        alpha = _fresh_output((nnz, heads), el.device)
    _edge_heads(alpha, nnz, heads, "alpha")
    _call(el.device, "gnna_gat_alpha_f32", el.data_ptr(), er.data_ptr(), _ptr(ee), lse.data_ptr(), row_pointers.data_ptr(),
          column_index.data_ptr(), float(negative_slope), alpha.data_ptr(), n_out, n_in, nnz, heads)
    return alpha


def _gatv2_sizes(Hs, Hd, att, row_pointers):
    """(Hs's pointer, ld_hs, Hd's pointer, ld_hd, num_out_rows, num_in_rows, width, heads) of a GATv2 attention call, taken from
    the tensors: num_in_rows = Hs.shape[0], num_out_rows = Hd.shape[0] = row_pointers.numel() - 1, heads = att.shape[0]."""
    sp, n_in, width, ld_hs = _rows_view(Hs, "Hs")
    dp, n_out, width_d, ld_hd = _rows_view(Hd, "Hd")
    assert width_d == width and Hd.device == Hs.device, "Hs must be [num_in_rows, heads * dim] and Hd [num_out_rows, heads * dim]"
    assert row_pointers.dim() == 1 and row_pointers.numel() == n_out + 1, \
        f"row_pointers must be [num_out_rows + 1] with num_out_rows = Hd.shape[0] = {n_out} (got {row_pointers.numel()} entries)"
    assert att.dtype == torch.float32 and att.dim() == 2 and att.is_contiguous() and att.device == Hs.device \
        and att.shape[0] >= 1 and att.numel() == width, "att must be a contiguous float32 [heads, dim] tensor with heads * dim = Hs.shape[1]"
    return sp, ld_hs, dp, ld_hd, n_out, n_in, width, att.shape[0]


def gatv2_forward(Hs, Hd, att, row_pointers, column_index, part_pointers, part2Node, partSize=32, negative_slope=0.2, attn_drop=0.0,
                  rng_seed=0, out=None, lse=None, relu=False):
    """gnna_gatv2_forward_f32 (include/gnna_gatv2.h): fused multi-head GATv2 attention.  Hs [num_in_rows, heads * dim] (source
    side and message), Hd [num_out_rows, heads * dim] (destination side), att [heads, dim] -> (out, lse) with
    z = sum_d att[h, d] * leaky_relu(Hs[j, h, d] + Hd[i, h, d]), out[i, h] = sum_e exp(z - lse[i, h]) * k * Hs[col(e), h]; k is the
    dropout factor of gat_forward_drop (1 at attn_drop = 0).  No per-edge tensor.  `Hs`, `Hd` and `out` may be row-strided views
    (stride(1) == 1); Hs and Hd may be the same tensor."""
    _need_device(Hs, "GATv2 attention")
    sp, ld_hs, dp, ld_hd, n_out, n_in, width, heads = _gatv2_sizes(Hs, Hd, att, row_pointers)
    if out is None:
        out = _fresh_output((n_out, width), Hs.device)
    if lse is None:
        lse = _fresh_output((n_out, heads), Hs.device)
    op_, n_o, width_o, ld_out = _rows_view(out, "out")
    assert n_o == n_out and width_o == width and _node_heads(lse, n_out, "lse") == heads
    _call(Hs.device, "gnna_gatv2_forward_f32", sp, ld_hs, dp, ld_hd, att.data_ptr(), row_pointers.data_ptr(), column_index.data_ptr(),
          part_pointers.data_ptr(), part2Node.data_ptr(), float(negative_slope), float(attn_drop), int(rng_seed), op_, ld_out,
          lse.data_ptr(), n_out, n_in, heads, width // heads, part2Node.numel(), int(partSize), _flags(relu=relu))
    return out, lse


def gatv2_backward(Hs, Hd, att, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize=32, negative_slope=0.2,
                   attn_drop=0.0, rng_seed=0, transposed=None, dHs=None, dHd=None, d_att=None):
    """gnna_gatv2_backward_f32: (dHs, dHd, d_att) of gatv2_forward for the gradient dY of its output Y (same attn_drop and
    rng_seed).  transposed = (t_row_pointers, t_column_index, t_part_pointers, t_part2Node) at the same partSize; without it (a
    square graph whose structure is symmetric, not checked here) the graph's own structure is passed as the transposed one."""
    _need_device(Hs, "GATv2 attention")
    sp, ld_hs, dp, ld_hd, n_out, n_in, width, heads = _gatv2_sizes(Hs, Hd, att, row_pointers)
    yp, n_y, width_y, ld_y = _rows_view(Y, "Y")
    gp, n_g, width_g, ld_g = _rows_view(dY, "dY")
    assert _node_heads(lse, n_out, "lse") == heads
    assert (n_y, width_y) == (n_out, width) and (n_g, width_g) == (n_out, width), "Y and dY must be [num_out_rows, heads * dim]"
    if n_out != n_in and transposed is None:
        raise GnnaError(f"GATv2 attention backward on a rectangular structure ({n_out} destination rows, {n_in} source rows) needs "
                        "`transposed`: a rectangular structure is never its own transpose")
    if transposed is None:
        transposed = (row_pointers, column_index, part_pointers, part2Node)
    t_rp, t_ci, t_pp, t_p2n = transposed
    for t in (column_index, part_pointers, part2Node, t_rp, t_ci, t_pp, t_p2n):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == Hs.device, \
            "the graph and its transpose must be contiguous int32 tensors on Hs's device"
    assert t_rp.numel() == n_in + 1 and t_pp.numel() == t_p2n.numel() + 1, \
        "transposed: [num_in_rows + 1] row pointers, [P + 1] / [P] partition"
    if dHs is None:
        dHs = _fresh_output((n_in, width), Hs.device)
    if dHd is None:
        dHd = _fresh_output((n_out, width), Hs.device)
    if d_att is None:
        d_att = _fresh_output(tuple(att.shape), Hs.device)
    sgp, n_s, width_s, ld_dhs = _rows_view(dHs, "dHs")
    dgp, n_d, width_dd, ld_dhd = _rows_view(dHd, "dHd")
    assert (n_s, width_s) == (n_in, width) and (n_d, width_dd) == (n_out, width), "dHs / dHd must have the shapes of Hs / Hd"
    assert d_att.dtype == torch.float32 and d_att.is_contiguous() and d_att.numel() == width and d_att.device == Hs.device
    _call(Hs.device, "gnna_gatv2_backward_f32", sp, ld_hs, dp, ld_hd, att.data_ptr(), lse.data_ptr(), yp, ld_y, gp, ld_g,
          row_pointers.data_ptr(), column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(), part2Node.numel(),
          t_rp.data_ptr(), t_ci.data_ptr(), t_pp.data_ptr(), t_p2n.data_ptr(), t_p2n.numel(), float(negative_slope),
          float(attn_drop), int(rng_seed), sgp, ld_dhs, dgp, ld_dhd, d_att.data_ptr(), n_out, n_in, heads, width // heads,
          int(partSize), 0)
    return dHs, dHd, d_att


def _dot_attn_sizes(Q, K, V, heads, row_pointers):
    """(Q's pointer, ld_q, K's pointer, ld_k, V's pointer, ld_v, num_out_rows, num_in_rows, width) of a dot-product attention call,
    taken from the tensors: num_out_rows = Q.shape[0] = row_pointers.numel() - 1, num_in_rows = K.shape[0] = V.shape[0]."""
    qp, n_out, width, ld_q = _rows_view(Q, "Q")
    kp, n_in, width_k, ld_k = _rows_view(K, "K")
    vp, n_v, width_v, ld_v = _rows_view(V, "V")
    assert width_k == width and width_v == width and n_v == n_in and K.device == Q.device and V.device == Q.device, \
        "Q must be [num_out_rows, heads * dim], K and V [num_in_rows, heads * dim]"
    assert int(heads) >= 1 and width % int(heads) == 0, f"heads = {heads} must divide the row width {width}"
    assert row_pointers.dim() == 1 and row_pointers.numel() == n_out + 1, \
        f"row_pointers must be [num_out_rows + 1] with num_out_rows = Q.shape[0] = {n_out} (got {row_pointers.numel()} entries)"
    return qp, ld_q, kp, ld_k, vp, ld_v, n_out, n_in, width


def dot_attn_forward(Q, K, V, heads, row_pointers, column_index, part_pointers, part2Node, partSize=32, scale=None, attn_drop=0.0,
                     rng_seed=0, out=None, lse=None, relu=False):
    """gnna_dot_attn_forward_f32 (include/gnna_dotattn.h): fused multi-head scaled dot-product graph attention.  Q [num_out_rows,
    heads * dim], K and V [num_in_rows, heads * dim] -> (out, lse) with z = scale * <Q[i, h], K[j, h]>,
    out[i, h] = sum_e exp(z - lse[i, h]) * k * V[col(e), h]; k is the dropout factor of gat_forward_drop (1 at attn_drop = 0);
    scale defaults to 1 / sqrt(dim).  No per-edge tensor.  `Q`, `K`, `V` and `out` may be row-strided views (stride(1) == 1), for
    instance column slices of one projection matrix."""
    _need_device(Q, "dot-product attention")
    qp, ld_q, kp, ld_k, vp, ld_v, n_out, n_in, width = _dot_attn_sizes(Q, K, V, heads, row_pointers)
    heads = int(heads)
    if scale is None:
        scale = 1.0 / math.sqrt(width // heads)
    if out is None:
        out = _fresh_output((n_out, width), Q.device)
    if lse is None:
        lse = _fresh_output((n_out, heads), Q.device)
    op_, n_o, width_o, ld_out = _rows_view(out, "out")
    assert n_o == n_out and width_o == width and _node_heads(lse, n_out, "lse") == heads
    _call(Q.device, "gnna_dot_attn_forward_f32", qp, ld_q, kp, ld_k, vp, ld_v, row_pointers.data_ptr(), column_index.data_ptr(),
          part_pointers.data_ptr(), part2Node.data_ptr(), float(scale), float(attn_drop), int(rng_seed), op_, ld_out,
          lse.data_ptr(), n_out, n_in, heads, width // heads, part2Node.numel(), int(partSize), _flags(relu=relu))
    return out, lse


def dot_attn_backward(Q, K, V, heads, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize=32, scale=None,
                      attn_drop=0.0, rng_seed=0, transposed=None, dQ=None, dK=None, dV=None):
    """gnna_dot_attn_backward_f32: (dQ, dK, dV) of dot_attn_forward for the gradient dY of its output Y (same scale, attn_drop and
    rng_seed).  transposed = (t_row_pointers, t_column_index, t_part_pointers, t_part2Node) at the same partSize; without it (a
    square graph whose structure is symmetric, not checked here) the graph's own structure is passed as the transposed one."""
    _need_device(Q, "dot-product attention")
    qp, ld_q, kp, ld_k, vp, ld_v, n_out, n_in, width = _dot_attn_sizes(Q, K, V, heads, row_pointers)
    heads = int(heads)
    if scale is None:
        scale = 1.0 / math.sqrt(width // heads)
    yp, n_y, width_y, ld_y = _rows_view(Y, "Y")
    gp, n_g, width_g, ld_g = _rows_view(dY, "dY")
    assert _node_heads(lse, n_out, "lse") == heads
    assert (n_y, width_y) == (n_out, width) and (n_g, width_g) == (n_out, width), "Y and dY must be [num_out_rows, heads * dim]"
    if n_out != n_in and transposed is None:
        raise GnnaError(f"dot-product attention backward on a rectangular structure ({n_out} destination rows, {n_in} source rows) "
                        "needs `transposed`: a rectangular structure is never its own transpose")
    if transposed is None:
        transposed = (row_pointers, column_index, part_pointers, part2Node)
    t_rp, t_ci, t_pp, t_p2n = transposed
    for t in (column_index, part_pointers, part2Node, t_rp, t_ci, t_pp, t_p2n):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == Q.device, \
            "the graph and its transpose must be contiguous int32 tensors on Q's device"
    assert t_rp.numel() == n_in + 1 and t_pp.numel() == t_p2n.numel() + 1, \
        "transposed: [num_in_rows + 1] row pointers, [P + 1] / [P] partition"
    if dQ is None:
        dQ = _fresh_output((n_out, width), Q.device)
    if dK is None:
        dK = _fresh_output((n_in, width), Q.device)
    if dV is None:
        dV = _fresh_output((n_in, width), Q.device)
    dqp, n_q, width_q, ld_dq = _rows_view(dQ, "dQ")
    dkp, n_k, width_k, ld_dk = _rows_view(dK, "dK")
    dvp, n_v, width_v, ld_dv = _rows_view(dV, "dV")
    assert (n_q, width_q) == (n_out, width) and (n_k, width_k) == (n_in, width) and (n_v, width_v) == (n_in, width), \
        "dQ / dK / dV must have the shapes of Q / K / V"
    _call(Q.device, "gnna_dot_attn_backward_f32", qp, ld_q, kp, ld_k, vp, ld_v, lse.data_ptr(), yp, ld_y, gp, ld_g,
          row_pointers.data_ptr(), column_index.data_ptr(), part_pointers.data_ptr(), part2Node.data_ptr(), part2Node.numel(),
          t_rp.data_ptr(), t_ci.data_ptr(), t_pp.data_ptr(), t_p2n.data_ptr(), t_p2n.numel(), float(scale),
          float(attn_drop), int(rng_seed), dqp, ld_dq, dkp, ld_dk, dvp, ld_dv, n_out, n_in, heads, width // heads,
          int(partSize), 0)
    return dQ, dK, dV


def _device_i32(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise GnnaError(f"{what} must be a device tensor: the builder runs on the GPU (the host builders take host tensors)")
    assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous(), f"{what} must be a contiguous 1-D int32 tensor"
    return t


def transpose_csr(row_pointers, column_index, num_in_rows=None, want_perm=True):
    """gnna_transpose_csr_i32 (device): the CSR of A^T for device row_pointers [num_out_rows + 1] / column_index [nnz] ->
    (t_row_pointers [num_in_rows + 1], t_column_index [nnz], t_perm [nnz] or None).  Row j lists the rows i of the edges i <- j in
    increasing position e, t_perm[p] = e (= numpy.argsort(column_index, kind="stable")); ids outside [0, num_in_rows) are dropped:
    t_row_pointers[-1] edges are kept and both arrays are -1 behind them.  num_in_rows defaults to num_out_rows.  Synchronises
    the current stream; refuses to run inside a stream capture."""
    rp, ci = _device_i32(row_pointers, "row_pointers"), _device_i32(column_index, "column_index")
    assert rp.numel() >= 1 and ci.device == rp.device, "row_pointers must be [num_out_rows + 1], on column_index's device"
    n_out = rp.numel() - 1
    n_in = n_out if num_in_rows is None else int(num_in_rows)
    assert n_in >= 0, "num_in_rows must not be negative"
    nnz = ci.numel()
    t_rp = torch.empty(n_in + 1, dtype=torch.int32, device=rp.device)
    t_ci = torch.empty(nnz, dtype=torch.int32, device=rp.device)
    t_perm = torch.empty(nnz, dtype=torch.int32, device=rp.device) if want_perm else None
    with torch.cuda.device(rp.device):
        # (the library trusts row_pointers[num_out_rows] for the edge count: it must not exceed what column_index holds)
        if n_out > 0 and int(rp[-1]) != nnz:
            raise GnnaError(f"row_pointers[-1] = {int(rp[-1])} but column_index holds {nnz} ids")
        _call(rp.device, "gnna_transpose_csr_i32", rp.data_ptr(), _ptr(ci), n_out, n_in, t_rp.data_ptr(), _ptr(t_ci), _ptr(t_perm))
    return t_rp, t_ci, t_perm


def count_parts_device(partSize: int, indptr) -> int:
    """gnna_count_parts_device_i32: count_parts for device row pointers (reads the count back: synchronises)."""
    ip = _device_i32(indptr, "indptr")
    assert ip.numel() >= 1
    with torch.cuda.device(ip.device):
        n = load().gnna_count_parts_device_i32(int(partSize), ip.data_ptr(), ip.numel() - 1, _stream(ip.device))
    if n < 0:
        _check(int(n))
    return int(n)


def build_part_device(partSize: int, indptr):
    """gnna_build_part_device_i32: build_part for device row pointers -> (partPtr int32 [P + 1], part2Node int32 [P]) on the
    same device, element for element what build_part gives for the same row pointers."""
    ip = _device_i32(indptr, "indptr")
    P = count_parts_device(partSize, ip)
    pp = torch.empty(P + 1, dtype=torch.int32, device=ip.device)
    p2n = torch.empty(P, dtype=torch.int32, device=ip.device)
    _call(ip.device, "gnna_build_part_device_i32", int(partSize), ip.data_ptr(), ip.numel() - 1, pp.data_ptr(), _ptr(p2n), P)
    return pp, p2n


def sample_neighbors(row_pointers, column_index, seeds, fanout, rng_seed, partSize=None, want_edge_ids=True, *,
                     edge_capacity=None, src_capacity=None):
    """gnna_sample_neighbors_i32 (device): one mini-batch block for the destination rows `seeds` (distinct int32 ids) of the
    device CSR row_pointers [N + 1] / column_index [nnz].  Every row keeps all its edges when fanout <= 0 or it has at most
    `fanout`, else the `fanout` positions with the smallest splitmix64(rng_seed, position) key, in increasing position (the
    rule is spelled out in include/gnna.h).  -> dict: row_pointers [S + 1], column_index [nnz_b] (LOCAL source ids: 0 .. S-1
    are the seeds in the order given, the other sources follow in increasing global id), edge_ids [nnz_b] (positions in
    column_index; None with want_edge_ids=False), src_nodes [num_src] (global ids), partPtr [P + 1] / part2Node [P] (what
    build_part gives for the block's row pointers; None without partSize), num_dst, num_src.  The arrays are trimmed views of
    buffers sized here (S * fanout edges, or the sum of the seeds' degrees).  One stream synchronisation; refuses to run inside
    a stream capture.  O(N) device work per call.  edge_capacity / src_capacity override the sizes chosen here; a GnnaError
    raised for a capacity that is too small carries the needed (nnz, num_src, num_parts) as ``.counts``."""
    rp, ci = _device_i32(row_pointers, "row_pointers"), _device_i32(column_index, "column_index")
    sd = _device_i32(seeds, "seeds")
    assert rp.numel() >= 1 and ci.device == rp.device and sd.device == rp.device, \
        "row_pointers must be [num_nodes + 1]; column_index and seeds live on its device"
    n, S, fanout = rp.numel() - 1, sd.numel(), int(fanout)
    rng_seed = int(rng_seed) & 0xFFFFFFFFFFFFFFFF
    want_part = partSize is not None
    if want_part and int(partSize) <= 0:
        raise GnnaError(f"partSize must be positive (got {partSize})")
    dev = rp.device
    with torch.cuda.device(dev):
        edge_cap = min(S * fanout if fanout >= 1 else _degree_sum(rp, sd), ci.numel())      # fanout <= 0: every neighbour
        src_cap = min(S + edge_cap, max(n, S))
        if edge_capacity is not None:
            edge_cap = int(edge_capacity)
        if src_capacity is not None:
            src_cap = int(src_capacity)
        if edge_cap < 0 or src_cap < 0:
            raise GnnaError("capacities must not be negative")
        blk_rp = torch.empty(S + 1, dtype=torch.int32, device=dev)
        blk_ci = torch.empty(edge_cap, dtype=torch.int32, device=dev)
        eid = torch.empty(edge_cap, dtype=torch.int32, device=dev) if want_edge_ids else None
        src = torch.empty(src_cap, dtype=torch.int32, device=dev)
        pp = torch.empty(edge_cap + 1, dtype=torch.int32, device=dev) if want_part else None
        p2n = torch.empty(edge_cap, dtype=torch.int32, device=dev) if want_part else None
        counts = (ctypes.c_int64 * 3)()
        rc = load().gnna_sample_neighbors_i32(rp.data_ptr(), _ptr(ci), n, _ptr(sd), S, fanout, rng_seed,
                                              int(partSize) if want_part else 0, blk_rp.data_ptr(), _ptr(blk_ci), _ptr(eid),
                                              _ptr(src), _ptr(pp), _ptr(p2n), edge_cap, src_cap, counts, _stream(dev))
    nnz, num_src, P = _check_counts(rc, counts)
    return {"row_pointers": blk_rp, "column_index": blk_ci[:nnz], "edge_ids": eid[:nnz] if want_edge_ids else None,
            "src_nodes": src[:num_src], "partPtr": pp[:P + 1] if want_part else None,
            "part2Node": p2n[:P] if want_part else None, "num_dst": S, "num_src": num_src}


# ---- subgraph sampling (gnna_walk.hip) -------------------------------------------------------------------------------------
def _graph_ids(row_pointers, column_index, ids, what):
    rp, ci = _device_i32(row_pointers, "row_pointers"), _device_i32(column_index, "column_index")
    t = _device_i32(ids, what)
    assert rp.numel() >= 1 and ci.device == rp.device and t.device == rp.device, \
        f"row_pointers must be [num_nodes + 1]; column_index and {what} live on its device"
    return rp, ci, t


def random_walk(row_pointers, column_index, roots, walk_length, rng_seed, want_edge_ids=False):
    """gnna_random_walk_i32 (device): one uniform first-order walk of `walk_length` steps from every entry of `roots` (int32
    [R]) on the device CSR row_pointers [N + 1] / column_index [nnz] -> (walks int32 [R, walk_length + 1], edge_ids int32
    [R, walk_length] or None).  Step t of walk w takes position lo + floor(key * d / 2^64) of its row, key = the splitmix64 key of
    u = w * walk_length + t under rng_seed; a row without positions and an edge to an id outside the graph make the walk stay
    (edge id -1); a root outside the graph gives a row of -1 (the rule is spelled out in include/gnna_walk.h).  A function of
    (rng_seed, w, t) and the graph only.  No synchronisation, no read-back: capturable, accepted under
    set_tuning(deterministic=1)."""
    rp, ci, rt = _graph_ids(row_pointers, column_index, roots, "roots")
    n, R, L = rp.numel() - 1, rt.numel(), int(walk_length)
    if L < 0:
        raise GnnaError(f"walk_length must not be negative (got {walk_length})")
    rng_seed = int(rng_seed) & 0xFFFFFFFFFFFFFFFF
    dev = rp.device
    with torch.cuda.device(dev):
        walks = torch.empty((R, L + 1), dtype=torch.int32, device=dev)
        eid = torch.empty((R, L), dtype=torch.int32, device=dev) if want_edge_ids else None
    _call(dev, "gnna_random_walk_i32", rp.data_ptr(), _ptr(ci) if ci.numel() else None, n, ci.numel(), _ptr(rt) if R else None, R, L,
          rng_seed, _ptr(walks) if R else None, _ptr(eid) if want_edge_ids and R * L else None)
    return walks, eid


def induced_subgraph(row_pointers, column_index, nodes, partSize=None, want_edge_ids=True, want_new_id=False, *,
                     node_capacity=None, edge_capacity=None):
    """gnna_induced_subgraph_i32 (device): the subgraph that the node list `nodes` (int32 [num_ids]: duplicates welcome, -1
    skipped, any other id outside the graph an error) induces in the device CSR row_pointers [N + 1] / column_index [nnz].  The
    kept set S is the distinct ids in increasing global id; row a holds the positions of row S[a] whose column is in S, in
    increasing position (the rule is spelled out in include/gnna_walk.h).  -> dict: row_pointers [n + 1], column_index [nnz']
    (ranks in S), edge_ids [nnz'] (positions in column_index; None with want_edge_ids=False), nodes [n] (= S, global ids),
    new_id [N] (the rank of a kept node, -1 otherwise; None unless want_new_id), partPtr [P + 1] / part2Node [P] (what build_part
    gives for the new row pointers; None without partSize), num_nodes (= n).  The arrays are trimmed views of buffers sized here:
    min(num_ids, N) nodes and min(nnz, the degree sum over `nodes`) edges.  One stream synchronisation; refuses to run inside a
    stream capture; the same bits on every run.  node_capacity / edge_capacity override the sizes chosen here; a GnnaError raised
    for a capacity that is too small carries the needed (nodes, edges, parts) as ``.counts``."""
    rp, ci, nd = _graph_ids(row_pointers, column_index, nodes, "nodes")
    n, K, nnz = rp.numel() - 1, nd.numel(), ci.numel()
    want_part = partSize is not None
    if want_part and int(partSize) <= 0:
        raise GnnaError(f"partSize must be positive (got {partSize})")
    dev = rp.device
    with torch.cuda.device(dev):
        node_cap = min(K, n) if node_capacity is None else int(node_capacity)
        edge_cap = min(nnz, _degree_sum(rp, nd)) if edge_capacity is None else int(edge_capacity)
        if node_cap < 0 or edge_cap < 0:
            raise GnnaError("capacities must not be negative")
        i32 = dict(dtype=torch.int32, device=dev)
        sub_nodes, sub_rp = torch.empty(node_cap, **i32), torch.empty(node_cap + 1, **i32)
        sub_ci = torch.empty(edge_cap, **i32)
        eid = torch.empty(edge_cap, **i32) if want_edge_ids else None
        new_id = torch.empty(n, **i32) if want_new_id else None
        pp = torch.empty(edge_cap + 1, **i32) if want_part else None
        p2n = torch.empty(edge_cap, **i32) if want_part else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None                 # noqa: E731
        counts = (ctypes.c_int64 * 3)()
        rc = load().gnna_induced_subgraph_i32(rp.data_ptr(), ptr(ci), n, nnz, ptr(nd), K, int(partSize) if want_part else 0,
                                              ptr(sub_nodes), ptr(new_id), sub_rp.data_ptr(), ptr(sub_ci), ptr(eid), _ptr(pp),
                                              ptr(p2n), node_cap, edge_cap, counts, _stream(dev))
    m, e, P = _check_counts(rc, counts)
    return {"row_pointers": sub_rp[:m + 1], "column_index": sub_ci[:e], "edge_ids": eid[:e] if want_edge_ids else None,
            "nodes": sub_nodes[:m], "new_id": new_id, "partPtr": pp[:P + 1] if want_part else None,
            "part2Node": p2n[:P] if want_part else None, "num_nodes": m}


# ---- graph construction from coordinates (gnna_spatial.hip) ------------------------------------------------------------------
SPATIAL_LONG_ROWS = 256         # GNNA_SPATIAL_LONG_ROWS: a segment of more rows is taken by the tile kernel (a row per lane, LDS tiles)
SPATIAL_SOURCE_TILE = 8192      # GNNA_SPATIAL_SOURCE_TILE: floats of a staged source tile (SPATIAL_SOURCE_TILE // dim rows, 256 at most)
SPATIAL_REGISTER_DIM = 4        # GNNA_SPATIAL_REGISTER_DIM: the tile kernel keeps a destination row of up to this many columns in registers
SPATIAL_MAX_DIM = 64            # GNNA_SPATIAL_MAX_DIM
SPATIAL_MAX_NEIGHBORS = 64      # GNNA_SPATIAL_MAX_NEIGHBORS
SPATIAL_DEFAULT_EDGES = 1 << 22  # edges the default capacity of radius_graph holds at least (or 64 per row), before the one retry


def radius_graph(pos, graph_pointers, radius, max_neighbors=None, loop=False, partSize=None, want_dist2=True, *, edge_capacity=None):
    """gnna_radius_graph_f32 (device): for every point set g of a batch -- the rows [graph_pointers[g], graph_pointers[g + 1]) of
    `pos` (float32 [N, dim], 1 <= dim <= 64; a column slice is fine) -- the graph that joins row i to the rows j of its set with
    d2(i, j) = sum_c (pos[j, c] - pos[i, c])^2 <= radius * radius, every operation rounded to fp32, columns in order; j == i only
    with loop=True.  max_neighbors (1 .. 64) keeps the that many candidates with the smallest (d2, j) per row; radius = inf with a
    cap is the k-nearest-neighbour graph (the rule is spelled out in include/gnna_spatial.h).  -> dict: row_pointers [N + 1],
    column_index [nnz'] (global row ids, increasing within a row), dist2 [nnz'] (None with want_dist2=False), partPtr [P + 1] /
    part2Node [P] (what build_part gives for the row pointers; None without partSize), num_edges.  The arrays are trimmed views of
    buffers sized here: min(U, max(2^22, 64 N)) edges, U = sum_g n_g * min(n_g - 1 + loop, max_neighbors or n_g) from a host copy of
    graph_pointers; when that is too small the call is repeated once at the size it reported.  One stream synchronisation per
    call; refuses to run inside a stream capture; the same bits on every run; accepted under set_tuning(deterministic=1).
    edge_capacity overrides the size chosen here (no retry then); a GnnaError raised for a capacity that is too small carries the
    needed (rows, edges, parts) as ``.counts``."""
    radius = float(radius)
    if not radius >= 0.0:
        raise GnnaError(f"radius must be >= 0 or inf (got {radius})")
    cap = 0 if max_neighbors is None else int(max_neighbors)
    if max_neighbors is not None and not 1 <= cap <= SPATIAL_MAX_NEIGHBORS:
        raise GnnaError(f"max_neighbors must be in [1, {SPATIAL_MAX_NEIGHBORS}] or None (got {max_neighbors})")
    want_part = partSize is not None
    if want_part and int(partSize) <= 0:
        raise GnnaError(f"partSize must be positive (got {partSize})")
    if edge_capacity is not None and int(edge_capacity) < 0:
        raise GnnaError("capacities must not be negative")
    if not (isinstance(pos, torch.Tensor) and pos.dim() == 2 and pos.dtype == torch.float32):
        raise GnnaError("pos must be a float32 tensor [N, dim]")
    if not 1 <= pos.shape[1] <= SPATIAL_MAX_DIM:
        raise GnnaError(f"pos must have 1 .. {SPATIAL_MAX_DIM} columns (got {pos.shape[1]})")
    _need_device(pos, "radius_graph")
    # (a tensor without rows has no strides worth checking)
    xp, n, dim, ld = _rows_view(pos, "pos") if pos.shape[0] > 0 else (None, 0, pos.shape[1], pos.shape[1])
    dev = pos.device
    gp, G = _graph_pointers_arg(graph_pointers, dev)
    loop = bool(loop)
    if edge_capacity is None:
        sizes = graph_pointers.cpu().long().clamp(0, n).diff().clamp(min=0)
        per_row = (sizes - 1 + int(loop)).clamp(min=0)
        upper = int((sizes * (per_row.clamp(max=cap) if cap else per_row)).sum())
        edge_cap = min(upper, max(SPATIAL_DEFAULT_EDGES, 64 * n))
    else:
        edge_cap = int(edge_capacity)

    def call(edge_cap):
        with torch.cuda.device(dev):
            i32 = dict(dtype=torch.int32, device=dev)
            rp, ci = torch.empty(n + 1, **i32), torch.empty(edge_cap, **i32)
            d2 = torch.empty(edge_cap, dtype=torch.float32, device=dev) if want_dist2 else None
            pp = torch.empty(edge_cap + 1, **i32) if want_part else None
            p2n = torch.empty(edge_cap, **i32) if want_part else None
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None                 # noqa: E731
            counts = (ctypes.c_int64 * 3)()
            rc = load().gnna_radius_graph_f32(xp if n > 0 else None, ld, n, dim, gp, G, radius, cap, int(loop),
                                              int(partSize) if want_part else 0, rp.data_ptr(), ptr(ci), ptr(d2), _ptr(pp), ptr(p2n),
                                              edge_cap, counts, _stream(dev))
        _, e, P = _check_counts(rc, counts)
        return {"row_pointers": rp, "column_index": ci[:e], "dist2": d2[:e] if want_dist2 else None,
                "partPtr": pp[:P + 1] if want_part else None, "part2Node": p2n[:P] if want_part else None, "num_edges": e}

    try:
        return call(edge_cap)
    except GnnaError as err:
        needed = getattr(err, "counts", (0, 0, 0))[1]
        if edge_capacity is not None or not edge_cap < needed < 2 ** 31:
            raise
    return call(needed)                                    # once, from what it reported


# ---- hierarchical pooling on graph batches (gnna_topk.hip) -------------------------------------------------------------------
TOPK_WAVE_ROWS = 256           # GNNA_TOPK_WAVE_ROWS: a segment of up to this many rows is selected by one wavefront


def topk_keep_count(n: int, ratio=None, k=None) -> int:
    """gnna_topk_keep_count: the rows a segment of `n` rows keeps under `ratio` (min(n, ceil(ratio * n)) in double) or under a
    fixed `k` (min(n, k)); -1 for arguments segment_topk refuses."""
    return int(load().gnna_topk_keep_count(int(n), 0.0 if ratio is None else float(ratio), 0 if k is None else int(k)))


def segment_topk(score, graph_pointers, ratio=None, k=None, row_pointers=None, column_index=None, partSize=None, want_edge_ids=False, *,
                 row_capacity=None, edge_capacity=None, part_capacity=None):
    """gnna_segment_topk_i32 (device): for every graph g of a batch -- the rows [graph_pointers[g], graph_pointers[g + 1]) -- the
    min(n, ceil(ratio * n)) (or min(n, k)) rows with the largest `score` (float32 [N]) in the library's total order, ties to the
    smaller row, kept in increasing row order; with row_pointers / column_index the induced CSR, with partSize its neighbor-group
    partition (the rule is spelled out in include/gnna_topk.h).  Exactly one of `ratio` (in (0, 1]) and `k` (>= 1) is given.
    -> dict: new_id [N] (the new row of a kept row, -1 otherwise), perm [N'] (the old row of every new row), graph_pointers
    [G + 1], num_rows; row_pointers [N' + 1], column_index [nnz'] (relabelled) and edge_ids [nnz'] (positions in the old
    column_index; None without want_edge_ids) or None without a CSR; partPtr [P + 1] / part2Node [P] or None without partSize.
    The arrays are trimmed views of buffers sized here (N rows, nnz edges).  One stream synchronisation; refuses to run inside a
    stream capture; the same bits on every run.  row_capacity / edge_capacity / part_capacity override the sizes chosen here; a
    GnnaError raised for a capacity that is too small carries the needed (rows, edges, parts) as ``.counts``."""
    if not (isinstance(score, torch.Tensor) and score.is_cuda):
        raise GnnaError("segment_topk needs device tensors: there is no CPU path in libgnna")
    assert score.dtype == torch.float32 and score.dim() == 1 and score.is_contiguous(), "score must be a contiguous float32 tensor [N]"
    dev = score.device
    gp, G = _graph_pointers_arg(graph_pointers, dev)
    if (row_pointers is None) != (column_index is None):
        raise ValueError("row_pointers and column_index come together")
    csr = row_pointers is not None
    want_part = partSize is not None
    if want_part and not csr:
        raise ValueError("a partition needs row_pointers and column_index")
    if want_part and int(partSize) <= 0:
        raise GnnaError(f"partSize must be positive (got {partSize})")
    n = score.numel()
    nnz = 0
    if csr:
        rp, ci = _device_i32(row_pointers, "row_pointers"), _device_i32(column_index, "column_index")
        assert rp.numel() == n + 1 and rp.device == dev and ci.device == dev, "row_pointers must be [N + 1]; it and column_index live on score's device"
        nnz = ci.numel()
    row_cap = n if row_capacity is None else int(row_capacity)
    edge_cap = nnz if edge_capacity is None else int(edge_capacity)
    part_cap = (edge_cap if part_capacity is None else int(part_capacity)) if want_part else 0
    if row_cap < 0 or edge_cap < 0 or part_cap < 0:
        raise GnnaError("capacities must not be negative")
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        new_id, perm, new_gp = torch.empty(n, **i32), torch.empty(row_cap, **i32), torch.empty(G + 1, **i32)
        new_rp = torch.empty(row_cap + 1, **i32) if csr else None
        new_ci = torch.empty(edge_cap, **i32) if csr else None
        eid = torch.empty(edge_cap, **i32) if csr and want_edge_ids else None
        pp = torch.empty(part_cap + 1, **i32) if want_part else None
        p2n = torch.empty(part_cap, **i32) if want_part else None
        counts = (ctypes.c_int64 * 3)()
        rc = load().gnna_segment_topk_i32(_ptr(score) if n > 0 else None, n, gp, G, 0.0 if ratio is None else float(ratio),
                                          0 if k is None else int(k), _ptr(rp) if csr else None,
                                          (_ptr(ci) if nnz > 0 else None) if csr else None, nnz, int(partSize) if want_part else 0,
                                          _ptr(new_id) if n > 0 else None, _ptr(perm) if row_cap > 0 else None, new_gp.data_ptr(),
                                          _ptr(new_rp), _ptr(new_ci) if csr and edge_cap > 0 else None,
                                          _ptr(eid) if eid is not None and edge_cap > 0 else None, _ptr(pp),
                                          _ptr(p2n) if want_part and part_cap > 0 else None, row_cap, edge_cap, part_cap, counts,
                                          _stream(dev))
    rows, edges, P = _check_counts(rc, counts)
    return {"new_id": new_id, "perm": perm[:rows], "graph_pointers": new_gp, "num_rows": rows,
            "row_pointers": new_rp[:rows + 1] if csr else None, "column_index": new_ci[:edges] if csr else None,
            "edge_ids": eid[:edges] if eid is not None else None, "partPtr": pp[:P + 1] if want_part else None,
            "part2Node": p2n[:P] if want_part else None}


def _row_ids_arg(t, n, device, what):
    assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.numel() == n and t.device == device, \
        f"{what} must be a contiguous int32 tensor [{n}] on {device}"
    return t.data_ptr() if n > 0 else None


def _scale_arg(scale, n, device):
    if scale is None:
        return None
    assert scale.dtype == torch.float32 and scale.dim() == 1 and scale.is_contiguous() and scale.numel() == n and scale.device == device, \
        f"scale must be a contiguous float32 tensor [{n}] on {device}"
    return scale.data_ptr() if n > 0 else None


def gather_rows_scale(X, perm, scale=None, out=None):
    """gnna_gather_rows_scale_ld_f32 (include/gnna_topk.h): out[i, :] = scale[perm[i]] * X[perm[i], :], one fp32 multiplication
    per element; scale=None is a plain gather; a perm[i] outside [0, rows of X) gives a row of zeros.  perm: int32 [M] on X's
    device, scale: float32 [N].  -> out [M, dim].  `X` and `out` may be row-strided views (stride(1) == 1).  Capturable; the same
    bits on every run; accepted under set_tuning(deterministic=1)."""
    _need_device(X, "gather_rows_scale")
    xp, n, dim, ld_in = _rows_view(X, "X")
    m = perm.numel()
    pp = _row_ids_arg(perm, m, X.device, "perm")
    sp = _scale_arg(scale, n, X.device)
    out, op_, ld_out = _out_rows(out, m, dim, X.device)
    if m > 0:
        _call(X.device, "gnna_gather_rows_scale_ld_f32", xp if n > 0 else None, ld_in, n, pp, sp, op_, ld_out, m, dim)
    return out


def gather_rows_scale_backward(dY, new_id, X=None, scale=None, need_input=True, need_scale=True, out=None):
    """gnna_gather_rows_scale_backward_ld_f32: with j = new_id[r] (kept: 0 <= j < rows of dY), d_input[r, :] = scale[r] * dY[j, :]
    and d_scale[r] = <dY[j, :], X[r, :]> for a kept row, 0 for every other.  One pass that writes every element once, nothing is
    cleared first.  -> (d_input [N, dim] | None, d_scale [N] | None): need_input / need_scale (not both False) choose what is
    computed; need_scale needs X; `out` may supply "d_input" / "d_scale".  With scale=None and need_scale=False this is the
    unpooling of a Graph U-Net: the rows of dY placed back at their old rows, zeros elsewhere.  Strided views as in
    gather_rows_scale."""
    if not need_input and not need_scale:
        raise ValueError("gather_rows_scale_backward needs need_input or need_scale")
    if need_scale and X is None:
        raise ValueError("gather_rows_scale_backward: need_scale needs X")
    _need_device(dY, "gather_rows_scale_backward")
    dp, m, dim, ld_dout = _rows_view(dY, "dY")
    n = new_id.numel()
    ip = _row_ids_arg(new_id, n, dY.device, "new_id")
    xp, ld_in = None, dim
    if need_scale:
        xp, xn, xw, ld_in = _rows_view(X, "X")
        assert (xn, xw) == (n, dim) and X.device == dY.device, f"X must be [{n}, {dim}] on {dY.device}"
    sp = _scale_arg(scale, n, dY.device)
    given = dict(out or {})
    d_input = d_scale = dip = dsp = None
    ld_din = dim
    if need_input:
        d_input, dip, ld_din = _out_rows(given.get("d_input"), n, dim, dY.device)
    if need_scale:
        d_scale = given.get("d_scale")
        if d_scale is None:
            d_scale = _fresh_output((n,), dY.device)
        assert d_scale.dtype == torch.float32 and d_scale.dim() == 1 and d_scale.is_contiguous() and d_scale.numel() == n and \
            d_scale.device == dY.device, f"d_scale must be a contiguous float32 tensor [{n}] on {dY.device}"
        dsp = d_scale.data_ptr() if n > 0 else None
    if n > 0:
        _call(dY.device, "gnna_gather_rows_scale_backward_ld_f32", dp if m > 0 else None, ld_dout, m, ip, xp, ld_in, sp, dip, ld_din,
              dsp, n, dim)
    return d_input, d_scale


# ---- relation-typed aggregation (gnna_typed.hip) ---------------------------------------------------------------------------
TYPED_LDS_CELLS = 4096      # kTypedLdsCells: the coefficient table (rows padded to the kernel's stride) lives in LDS up to here
TYPED_MAX_BASES = 16


def _typed_edges(column_index, edge_type, edge_norm, device):
    assert edge_type.dtype == torch.int32 and edge_type.is_contiguous() and edge_type.numel() == column_index.numel() \
        and edge_type.device == device, "edge_type must be a contiguous int32 tensor indexed like column_index"
    assert edge_norm is None or (edge_norm.dtype == torch.float32 and edge_norm.is_contiguous()
                                 and edge_norm.numel() == column_index.numel() and edge_norm.device == device), \
        "edge_norm must be a contiguous float32 tensor indexed like column_index"


def _coef_table(coef, device):
    assert coef.dtype == torch.float32 and coef.dim() == 2 and coef.is_contiguous() and coef.device == device, \
        "coef must be a contiguous float32 [num_types, num_bases] tensor on the features' device"
    return coef.shape[0], coef.shape[1]


def agg_typed_expand(X, coef, column_index, edge_type, edge_norm, part_pointers, part2Node, num_out_rows, partSize=32, out=None):
    """gnna_agg_typed_expand_ld_f32: out[i, b * dim + f] = sum_e n[e] * coef[t[e], b] * X[column_index[e], f] -> [num_out_rows,
    num_bases * dim].  edge_type int32 / edge_norm float32 (or None: 1) are indexed like column_index.  Strided X / out as in
    agg_ld."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_x = _rows_view(X, "X")
    R, B = _coef_table(coef, X.device)
    _typed_edges(column_index, edge_type, edge_norm, X.device)
    out, yp, ld_out = _out_rows(out, num_out_rows, B * dim, X.device)
    _call(X.device, "gnna_agg_typed_expand_ld_f32", xp, ld_x, n_in, column_index.data_ptr(), edge_type.data_ptr(), _ptr(edge_norm),
          coef.data_ptr(), R, B, part_pointers.data_ptr(), part2Node.data_ptr(), yp, ld_out, int(num_out_rows), dim,
          part2Node.numel(), int(partSize), 0)
    return out


def agg_typed_contract(G, coef, column_index, edge_type, edge_norm, part_pointers, part2Node, num_out_rows, partSize=32, out=None):
    """gnna_agg_typed_contract_ld_f32: out[i, f] = sum_e n[e] * sum_b coef[t[e], b] * G[column_index[e], b * dim + f] for G
    [num_in_rows, num_bases * dim] -> [num_out_rows, dim], over the structure given (the backward of agg_typed_expand: the
    transposed structure, with edge_type / edge_norm permuted by its perm)."""
    _need_device(G, "aggregation")
    gp, n_in, width, ld_g = _rows_view(G, "G")
    R, B = _coef_table(coef, G.device)
    assert width % B == 0, "G must be [num_in_rows, num_bases * dim]"
    dim = width // B
    _typed_edges(column_index, edge_type, edge_norm, G.device)
    out, yp, ld_out = _out_rows(out, num_out_rows, dim, G.device)
    _call(G.device, "gnna_agg_typed_contract_ld_f32", gp, ld_g, n_in, column_index.data_ptr(), edge_type.data_ptr(), _ptr(edge_norm),
          coef.data_ptr(), R, B, part_pointers.data_ptr(), part2Node.data_ptr(), yp, ld_out, int(num_out_rows), dim,
          part2Node.numel(), int(partSize), 0)
    return out


def typed_coef_grad(X, G, column_index, edge_type, edge_norm, part_pointers, part2Node, num_types, partSize=32, out=None,
                    accumulate=False):
    """gnna_typed_coef_grad_ld_f32: out[r, b] (+)= sum_{e: t[e] = r} n[e] * <X[column_index[e]], G[row(e), b * dim : (b + 1) * dim]>
    for X [num_in_rows, dim] and G [num_out_rows, num_bases * dim] over the forward structure -> [num_types, num_bases]."""
    _need_device(X, "aggregation")
    xp, n_in, dim, ld_x = _rows_view(X, "X")
    gp, n_out, width, ld_g = _rows_view(G, "G")
    assert width % dim == 0 and G.device == X.device, "G must be [num_out_rows, num_bases * dim] on X's device"
    B = width // dim
    _typed_edges(column_index, edge_type, edge_norm, X.device)
    if out is None:
        assert not accumulate, "accumulate needs an existing `out`"
        out = _fresh_output((int(num_types), B), X.device)
    assert tuple(out.shape) == (int(num_types), B)
    _coef_table(out, X.device)
    _call(X.device, "gnna_typed_coef_grad_ld_f32", xp, ld_x, n_in, gp, ld_g, n_out, column_index.data_ptr(), edge_type.data_ptr(),
          _ptr(edge_norm), part_pointers.data_ptr(), part2Node.data_ptr(), out.data_ptr(), int(num_types), B, dim,
          part2Node.numel(), int(partSize), _flags(accumulate))
    return out

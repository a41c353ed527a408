"""Every refusal of the two binding layers that is reachable without a device, pinned (no GPU): exception type and the whole
message, for the ctypes wrappers of ``_lib``, their private checkers and the extension functions of the ``GNNAdvisor`` module.
The pairs were recorded from the wrappers as they stood when every operator carried its own copy of these checks; the text is
what a caller sees (and greps for), so it is compared as a whole.  ``CASES`` maps a name to a call; ``EXPECTED`` holds what the
call did: (exception type, message), or ("returned", value) where the record shows that a rule does not apply."""
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, load_extension

GNNA = load_extension()

# a 6-row graph on the CPU: nothing below gets as far as reading it
RP = torch.tensor([0, 5, 6, 7, 8, 9, 9], dtype=torch.int32)
CI = torch.tensor([0, 1, 2, 3, 4, 0, 0, 0, 0], dtype=torch.int32)
PP, P2N = _lib.build_part(2, RP)
X = torch.ones(6, 3)
DEG = torch.ones(6)
W = torch.ones(9)
ARG = torch.zeros(6, 3, dtype=torch.int32)
H, EL, ER = torch.ones(6, 4), torch.ones(6, 2), torch.ones(6, 2)
COEF = torch.ones(2, 2)
ETYPE = torch.zeros(9, dtype=torch.int32)
SCORES = torch.ones(9)
WEIGHT = torch.ones(3, 2)
CPU = torch.device("cpu")


def _strip(value):
    """A returned row view without its data pointer (which differs from run to run)."""
    return tuple(value[1:]) if isinstance(value, tuple) else value


def outcome(call):
    try:
        value = call()
    except Exception as exc:                                     # noqa: BLE001 -- the type is part of what is compared
        return type(exc).__name__, str(exc)
    return "returned", _strip(value)


CASES = {
    # ---- the ctypes wrappers with CPU tensors ----
    "lib.sag": lambda: _lib.sag(X, RP, CI, DEG, PP, P2N),
    "lib.agg_gcn": lambda: _lib.agg_gcn(X, RP, CI, DEG, PP, P2N),
    "lib.agg_gin": lambda: _lib.agg_gin(X, RP, CI, 0.5, PP, P2N),
    "lib.agg_rect": lambda: _lib.agg_rect(0, X, CI, PP, P2N, 6),
    "lib.agg_ld": lambda: _lib.agg_ld(0, X, CI, PP, P2N, 6),
    "lib.agg_ld_x16": lambda: _lib.agg_ld_x16(0, X.bfloat16(), CI, PP, P2N, 6),
    "lib.xtg": lambda: _lib.xtg(X, X),
    "lib.sddmm": lambda: _lib.sddmm(X, X, CI, PP, P2N),
    "lib.agg_edge": lambda: _lib.agg_edge(X, CI, W, PP, P2N, 6),
    "lib.agg_reduce_ld": lambda: _lib.agg_reduce_ld(0, X, CI, PP, P2N),
    "lib.scatter_arg_ld": lambda: _lib.scatter_arg_ld(X, ARG, CI, 6),
    "lib.gat_forward": lambda: _lib.gat_forward(H, EL, ER, RP, CI, PP, P2N),
    "lib.gat_backward": lambda: _lib.gat_backward(H, EL, ER, EL, H, H, RP, CI, PP, P2N),
    "lib.agg_typed_expand": lambda: _lib.agg_typed_expand(X, COEF, CI, ETYPE, None, PP, P2N, 6),
    "lib.agg_typed_contract": lambda: _lib.agg_typed_contract(H, COEF, CI, ETYPE, None, PP, P2N, 6),
    "lib.typed_coef_grad": lambda: _lib.typed_coef_grad(X, torch.ones(6, 6), CI, ETYPE, None, PP, P2N, 2),
    "lib.edge_softmax": lambda: _lib.edge_softmax(SCORES, RP),
    "lib.edge_softmax_backward": lambda: _lib.edge_softmax_backward(SCORES, SCORES, RP),
    "lib.transpose_csr": lambda: _lib.transpose_csr(RP, CI),
    "lib.count_parts_device": lambda: _lib.count_parts_device(2, RP),
    "lib.build_part_device": lambda: _lib.build_part_device(2, RP),
    "lib.sample_neighbors": lambda: _lib.sample_neighbors(RP, CI, torch.tensor([0], dtype=torch.int32), 2, 1),
    # ---- the row views: float32, any element type, the int32 `arg` ----
    "rows.f32.plain": lambda: _lib._rows_view(torch.ones(6, 5)[:, 1:4], "X"),
    "rows.f32.transposed": lambda: _lib._rows_view(torch.ones(3, 6).t(), "X"),
    "rows.f32.overlapping": lambda: _lib._rows_view(torch.ones(20).as_strided((6, 3), (2, 1)), "X"),
    "rows.f32.dtype": lambda: _lib._rows_view(torch.ones(6, 3, dtype=torch.float64), "X"),
    "rows.f32.1d": lambda: _lib._rows_view(torch.ones(6), "X"),
    "rows.f32.one_row": lambda: _lib._rows_view(torch.ones(20).as_strided((1, 3), (2, 1)), "X"),
    "rows.any.plain": lambda: _lib._rows_view_any(torch.ones(6, 5, dtype=torch.bfloat16)[:, 1:4], "out"),
    "rows.any.transposed": lambda: _lib._rows_view_any(torch.ones(3, 6, dtype=torch.bfloat16).t(), "out"),
    "rows.any.overlapping": lambda: _lib._rows_view_any(torch.ones(20, dtype=torch.float16).as_strided((6, 3), (2, 1)), "out"),
    "rows.any.dtype": lambda: _lib._rows_view_any(torch.ones(6, 3, dtype=torch.int64), "out"),
    "rows.any.1d": lambda: _lib._rows_view_any(torch.ones(6, dtype=torch.bfloat16), "out"),
    "rows.arg.plain": lambda: _lib._arg_view(torch.zeros(6, 5, dtype=torch.int32)[:, 1:4], 6, 3, "arg"),
    "rows.arg.transposed": lambda: _lib._arg_view(torch.zeros(3, 6, dtype=torch.int32).t(), 6, 3, "arg"),
    "rows.arg.overlapping": lambda: _lib._arg_view(torch.zeros(20, dtype=torch.int32).as_strided((6, 3), (2, 1)), 6, 3, "arg"),
    "rows.arg.dtype": lambda: _lib._arg_view(torch.zeros(6, 3, dtype=torch.int64), 6, 3, "arg"),
    "rows.arg.1d": lambda: _lib._arg_view(torch.zeros(6, dtype=torch.int32), 6, 3, "arg"),
    "rows.arg.shape": lambda: _lib._arg_view(torch.zeros(5, 3, dtype=torch.int32), 6, 3, "arg"),
    # ---- the private checkers, one rule broken each ----
    "gat_sizes.ok": lambda: _lib._gat_sizes(H, EL, ER, RP),
    "gat_sizes.H_dtype": lambda: _lib._gat_sizes(H.double(), EL, ER, RP),
    "gat_sizes.el_1d": lambda: _lib._gat_sizes(H, EL[:, 0], ER, RP),
    "gat_sizes.row_pointers_2d": lambda: _lib._gat_sizes(H, EL, ER, RP[None]),
    "gat_sizes.row_pointers_length": lambda: _lib._gat_sizes(H, EL, ER, RP[:-1]),
    "gat_sizes.el_dtype": lambda: _lib._gat_sizes(H, EL.double(), ER, RP),
    "gat_sizes.er_rows": lambda: _lib._gat_sizes(H, EL, ER[:5], RP),
    "gat_sizes.er_heads": lambda: _lib._gat_sizes(H, EL, torch.ones(6, 4), RP),
    "gat_sizes.width": lambda: _lib._gat_sizes(torch.ones(6, 5), EL, ER, RP),
    "node_heads.ok": lambda: _lib._node_heads(EL, 6, "el"),
    "node_heads.dtype": lambda: _lib._node_heads(EL.double(), 6, "lse"),
    "node_heads.1d": lambda: _lib._node_heads(EL[:, 0], 6, "lse"),
    "node_heads.rows": lambda: _lib._node_heads(EL, 5, "lse"),
    "node_heads.strided": lambda: _lib._node_heads(torch.ones(6, 4)[:, :2], 6, "lse"),
    "typed_edges.ok": lambda: _lib._typed_edges(CI, ETYPE, W, CPU),
    "typed_edges.type_dtype": lambda: _lib._typed_edges(CI, ETYPE.long(), None, CPU),
    "typed_edges.type_length": lambda: _lib._typed_edges(CI, ETYPE[:8], None, CPU),
    "typed_edges.type_strided": lambda: _lib._typed_edges(CI, torch.zeros(18, dtype=torch.int32)[::2], None, CPU),
    "typed_edges.type_device": lambda: _lib._typed_edges(CI, ETYPE, None, torch.device("meta")),
    "typed_edges.norm_dtype": lambda: _lib._typed_edges(CI, ETYPE, W.double(), CPU),
    "typed_edges.norm_length": lambda: _lib._typed_edges(CI, ETYPE, W[:8], CPU),
    "coef_table.ok": lambda: _lib._coef_table(COEF, CPU),
    "coef_table.dtype": lambda: _lib._coef_table(COEF.double(), CPU),
    "coef_table.1d": lambda: _lib._coef_table(COEF[0], CPU),
    "coef_table.strided": lambda: _lib._coef_table(torch.ones(2, 4)[:, :2], CPU),
    "coef_table.device": lambda: _lib._coef_table(COEF, torch.device("meta")),
    "device_i32.list": lambda: _lib._device_i32([0, 1], "seeds"),
    "device_i32.cpu": lambda: _lib._device_i32(RP, "indptr"),
    # ---- the extension functions with CPU tensors: each names the argument it looks at first ----
    "ext.SAG": lambda: GNNA.SAG(X, RP, CI, DEG, PP, P2N, 2, 32, 4),
    "ext.forward": lambda: GNNA.forward(X, WEIGHT, RP, CI, DEG, PP, P2N, 2, 32, 4),
    "ext.backward": lambda: GNNA.backward(X, X, WEIGHT, RP, CI, DEG, PP, P2N, 2, 32, 4),
    "ext.backward_weight": lambda: GNNA.backward_weight(X, X, RP, CI, DEG, PP, P2N, 2, 32, 4),
    "ext.forward_gin": lambda: GNNA.forward_gin(X, WEIGHT, RP, CI, 0.5, PP, P2N, 2, 32, 4),
    "ext.backward_gin": lambda: GNNA.backward_gin(X, X, WEIGHT, RP, CI, 0.5, PP, P2N, 2, 32, 4),
    "ext.aggregate_gin": lambda: GNNA.aggregate_gin(X, RP, CI, 0.5, PP, P2N, 2, 32, 4),
    "ext.xtg": lambda: GNNA.xtg(X, X),
    "ext.aggregate_ld": lambda: GNNA.aggregate_ld(0, X, CI, None, 1.0, PP, P2N, 2),
    "ext.aggregate_edge": lambda: GNNA.aggregate_edge(X, CI, W, PP, P2N, 2),
    "ext.aggregate_reduce": lambda: GNNA.aggregate_reduce(0, X, CI, PP, P2N, 2),
    "ext.scatter_arg": lambda: GNNA.scatter_arg(X, ARG, CI, 6),
    "ext.edge_softmax": lambda: GNNA.edge_softmax(SCORES, RP),
    "ext.edge_softmax_backward": lambda: GNNA.edge_softmax_backward(SCORES, SCORES, RP),
    "ext.gat_forward": lambda: GNNA.gat_forward(H, EL, ER, RP, CI, PP, P2N, 2),
    "ext.gat_backward": lambda: GNNA.gat_backward(H, EL, ER, EL, H, H, RP, CI, PP, P2N, 2),
    "ext.gat_backward.rect": lambda: GNNA.gat_backward(H, EL[:3], ER, EL[:3], H[:3], H[:3], RP[:4], CI, PP, P2N, 2),
    "ext.sddmm": lambda: GNNA.sddmm(X, X, CI, PP, P2N, 2),
    "ext.transpose_csr": lambda: GNNA.transpose_csr(RP, CI),
    "ext.build_part_device": lambda: GNNA.build_part_device(2, RP),
    "ext.forget_graph": lambda: GNNA.forget_graph(CI),
    "ext.build_part.dtype": lambda: GNNA.build_part(2, RP.long()),
    "ext.build_part.2d": lambda: GNNA.build_part(2, RP[None]),
}

EXPECTED = {
    'lib.sag': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_gcn': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_gin': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_rect': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_ld': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_ld_x16': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.xtg': ('GnnaError', 'xtg needs device tensors: there is no CPU path in libgnna'),
    'lib.sddmm': ('GnnaError', 'sddmm needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_edge': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_reduce_ld': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.scatter_arg_ld': ('GnnaError', 'scatter_arg needs device tensors: there is no CPU path in libgnna'),
    'lib.gat_forward': ('GnnaError', 'GAT attention needs device tensors: there is no CPU path in libgnna'),
    'lib.gat_backward': ('GnnaError', 'GAT attention needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_typed_expand': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.agg_typed_contract': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.typed_coef_grad': ('GnnaError', 'aggregation needs device tensors: there is no CPU path in libgnna'),
    'lib.edge_softmax': ('AssertionError', ''),
    'lib.edge_softmax_backward': ('AssertionError', ''),
    'lib.transpose_csr': ('GnnaError', 'row_pointers must be a device tensor: the builder runs on the GPU (the host builders take host tensors)'),
    'lib.count_parts_device': ('GnnaError', 'indptr must be a device tensor: the builder runs on the GPU (the host builders take host tensors)'),
    'lib.build_part_device': ('GnnaError', 'indptr must be a device tensor: the builder runs on the GPU (the host builders take host tensors)'),
    'lib.sample_neighbors': ('GnnaError', 'row_pointers must be a device tensor: the builder runs on the GPU (the host builders take host tensors)'),
    'rows.f32.plain': ('returned', (6, 3, 5)),
    'rows.f32.transposed': ('GnnaError', 'X: the floats of a row must be contiguous (stride(1) == 1)'),
    'rows.f32.overlapping': ('GnnaError', 'X: rows overlap (stride(0) = 2 < 3)'),
    'rows.f32.dtype': ('AssertionError', 'X must be a 2-D float32 tensor'),
    'rows.f32.1d': ('AssertionError', 'X must be a 2-D float32 tensor'),
    'rows.f32.one_row': ('returned', (1, 3, 3)),
    'rows.any.plain': ('returned', (6, 3, 5)),
    'rows.any.transposed': ('GnnaError', 'out: the elements of a row must be contiguous (stride(1) == 1)'),
    'rows.any.overlapping': ('GnnaError', 'out: rows overlap (stride(0) = 2 < 3)'),
    'rows.any.dtype': ('returned', (6, 3, 3)),
    'rows.any.1d': ('AssertionError', 'out must be a 2-D tensor'),
    'rows.arg.plain': ('returned', (5,)),
    'rows.arg.transposed': ('GnnaError', 'arg: the elements of a row must be contiguous (stride(1) == 1)'),
    'rows.arg.overlapping': ('GnnaError', 'arg: rows overlap (stride(0) = 2 < 3)'),
    'rows.arg.dtype': ('AssertionError', 'arg must be int32 [6, 3]'),
    'rows.arg.1d': ('AssertionError', 'arg must be int32 [6, 3]'),
    'rows.arg.shape': ('AssertionError', 'arg must be int32 [6, 3]'),
    'gat_sizes.ok': ('returned', (6, 6, 4, 2, 4)),
    'gat_sizes.H_dtype': ('AssertionError', 'H must be a 2-D float32 tensor'),
    'gat_sizes.el_1d': ('AssertionError', 'el must be [num_out_rows, heads], row_pointers [num_out_rows + 1]'),
    'gat_sizes.row_pointers_2d': ('AssertionError', 'el must be [num_out_rows, heads], row_pointers [num_out_rows + 1]'),
    'gat_sizes.row_pointers_length': ('AssertionError', 'row_pointers must be [num_out_rows + 1] with num_out_rows = el.shape[0] = 6 (got 6 entries)'),
    'gat_sizes.el_dtype': ('AssertionError',
                           'el must be a contiguous float32 [6, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el have '
                           'num_out_rows rows, er / d_er num_in_rows)'),
    'gat_sizes.er_rows': ('AssertionError',
                          'er must be a contiguous float32 [6, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el have '
                          'num_out_rows rows, er / d_er num_in_rows)'),
    'gat_sizes.er_heads': ('AssertionError', 'H must be [num_in_rows, heads * dim], er [num_in_rows, heads] and el [num_out_rows, heads]'),
    'gat_sizes.width': ('AssertionError', 'H must be [num_in_rows, heads * dim], er [num_in_rows, heads] and el [num_out_rows, heads]'),
    'node_heads.ok': ('returned', 2),
    'node_heads.dtype': ('AssertionError',
                         'lse must be a contiguous float32 [6, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el have '
                         'num_out_rows rows, er / d_er num_in_rows)'),
    'node_heads.1d': ('AssertionError',
                      'lse must be a contiguous float32 [6, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el have num_out_rows '
                      'rows, er / d_er num_in_rows)'),
    'node_heads.rows': ('AssertionError',
                        'lse must be a contiguous float32 [5, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el have '
                        'num_out_rows rows, er / d_er num_in_rows)'),
    'node_heads.strided': ('AssertionError',
                           'lse must be a contiguous float32 [6, heads] tensor (num_nodes rows; on a rectangular structure el / lse / d_el have '
                           'num_out_rows rows, er / d_er num_in_rows)'),
    'typed_edges.ok': ('returned', None),
    'typed_edges.type_dtype': ('AssertionError', 'edge_type must be a contiguous int32 tensor indexed like column_index'),
    'typed_edges.type_length': ('AssertionError', 'edge_type must be a contiguous int32 tensor indexed like column_index'),
    'typed_edges.type_strided': ('AssertionError', 'edge_type must be a contiguous int32 tensor indexed like column_index'),
    'typed_edges.type_device': ('AssertionError', 'edge_type must be a contiguous int32 tensor indexed like column_index'),
    'typed_edges.norm_dtype': ('AssertionError', 'edge_norm must be a contiguous float32 tensor indexed like column_index'),
    'typed_edges.norm_length': ('AssertionError', 'edge_norm must be a contiguous float32 tensor indexed like column_index'),
    'coef_table.ok': ('returned', (2,)),
    'coef_table.dtype': ('AssertionError', "coef must be a contiguous float32 [num_types, num_bases] tensor on the features' device"),
    'coef_table.1d': ('AssertionError', "coef must be a contiguous float32 [num_types, num_bases] tensor on the features' device"),
    'coef_table.strided': ('AssertionError', "coef must be a contiguous float32 [num_types, num_bases] tensor on the features' device"),
    'coef_table.device': ('AssertionError', "coef must be a contiguous float32 [num_types, num_bases] tensor on the features' device"),
    'device_i32.list': ('GnnaError', 'seeds must be a device tensor: the builder runs on the GPU (the host builders take host tensors)'),
    'device_i32.cpu': ('GnnaError', 'indptr must be a device tensor: the builder runs on the GPU (the host builders take host tensors)'),
    'ext.SAG': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.forward': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.backward': ('RuntimeError', 'd_output must be a CUDA tensor'),
    'ext.backward_weight': ('RuntimeError', 'd_output must be a CUDA tensor'),
    'ext.forward_gin': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.backward_gin': ('RuntimeError', 'd_output must be a CUDA tensor'),
    'ext.aggregate_gin': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.xtg': ('RuntimeError', 'X must be a CUDA tensor'),
    'ext.aggregate_ld': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.aggregate_edge': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.aggregate_reduce': ('RuntimeError', 'input must be a CUDA tensor'),
    'ext.scatter_arg': ('RuntimeError', 'grad_out must be a CUDA tensor'),
    'ext.edge_softmax': ('RuntimeError', 'scores must be a CUDA tensor'),
    'ext.edge_softmax_backward': ('RuntimeError', 'probs must be a CUDA tensor'),
    'ext.gat_forward': ('RuntimeError', 'el must be a CUDA tensor'),
    'ext.gat_backward': ('RuntimeError', 'el must be a CUDA tensor'),
    'ext.gat_backward.rect': ('RuntimeError', 'el must be a CUDA tensor'),
    'ext.sddmm': ('RuntimeError', 'A must be a CUDA tensor'),
    'ext.transpose_csr': ('RuntimeError', 'row_pointers must be a CUDA tensor (the builder runs on the device)'),
    'ext.build_part_device': ('RuntimeError', 'indptr must be a CUDA tensor (the builder runs on the device)'),
    'ext.forget_graph': ('RuntimeError', 'column_index must be a CUDA tensor'),
    'ext.build_part.dtype': ('RuntimeError', 'indptr must be int32 (got Long)'),
    'ext.build_part.2d': ('RuntimeError', 'indptr must be 1-D with num_nodes + 1 entries'),
}


def test_every_case_has_a_record():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal_is_the_recorded_one(name):
    assert outcome(CASES[name]) == EXPECTED[name]

"""Edge-feature message passing (include/gnna_edgefeat.h), the part that needs no GPU: the header's contract sentences and constants
(its entries, table and signatures are checked with every other header's in test_binding_table_host.py); every refusal of both
entries with its return code and whole message, on host buffers; the fp64 restatement (edgefeat_ref.py) equals fp64 torch autograd
of the composed formula; constructor and dtype errors of the op and the layers; ``GraphDataset.batch`` and ``carry_edge_attr``
carry edge_attr rows to the right edges; the driver's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import edgefeat_ref as ref
from gnnadvisor_osdi21_amd import _lib
from gnnadvisor_osdi21_amd import graph_main
from gnnadvisor_osdi21_amd.batching import GraphBatch, GraphDataset, TopKSelection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")
HEADER = "gnna_edgefeat.h"
FWD, BWD = "gnna_agg_edge_feat_ld_f32", "gnna_agg_edge_feat_backward_ld_f32"


# ---- the header ----

def test_the_header_states_the_contract_and_the_constants_and_the_module_includes_it():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert 'extern "C"' in text and '#include "gnna_edgefeat.h"' in open(os.path.join(CSRC, "gnna_torch.cpp")).read()
    flat = " ".join(text.replace("\n *", " ").split())
    for sentence in ("that behaviour is not pinned", "the mask is recomputed from x and E in every pass",
                     "a position >= num_edges is skipped", "a t_edge_pos outside [0, num_edges) is skipped",
                     "columns from `dim` to the leading dimension are never touched",
                     "accepted under gnna_tuning.deterministic = 1", "num_edges = 0 gives zero outputs"):
        assert sentence in flat, sentence
    for name, value in (("GNNA_EDGE_ADD", _lib.EDGE_ADD), ("GNNA_EDGE_MUL", _lib.EDGE_MUL), ("GNNA_EDGE_ACT_NONE", _lib.EDGE_ACT_NONE),
                        ("GNNA_EDGE_ACT_RELU", _lib.EDGE_ACT_RELU)):
        assert re.search(r"#define %s %d\b" % (name, value), text)


# ---- the argument checks: every call returns before it touches the device ----

_F = (ctypes.c_float * 256)()
_BASE = ctypes.cast(_F, ctypes.c_void_p).value
A, B, C, D, E_ = (_BASE + 64 * k for k in range(5))            # five distinct 4-byte aligned host addresses
_I = (ctypes.c_int32 * 64)()
I = ctypes.cast(_I, ctypes.c_void_p).value
INVALID, UNSUPPORTED = -1, -3


def _fwd(**kw):
    a = dict(x=A, ld_in=4, n_in=3, e=B, ld_e=4, nnz=5, rp=I, ci=I, out=C, ld_out=4, n_out=2, dim=4, combine=0, act=0, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_edge_feat_ld_f32(a["x"], a["ld_in"], a["n_in"], a["e"], a["ld_e"], a["nnz"], a["rp"], a["ci"], a["out"],
                                                 a["ld_out"], a["n_out"], a["dim"], a["combine"], a["act"], a["flags"], None)


def _bwd(**kw):
    a = dict(x=A, ld_in=4, n_in=3, e=B, ld_e=4, nnz=5, dy=C, ld_dy=4, rp=I, ci=I, trp=I, tci=I, tpos=I, dx=D, ld_din=4, de=E_, ld_de=4,
             n_out=2, dim=4, combine=0, act=1, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_edge_feat_backward_ld_f32(a["x"], a["ld_in"], a["n_in"], a["e"], a["ld_e"], a["nnz"], a["dy"], a["ld_dy"],
                                                          a["rp"], a["ci"], a["trp"], a["tci"], a["tpos"], a["dx"], a["ld_din"], a["de"],
                                                          a["ld_de"], a["n_out"], a["dim"], a["combine"], a["act"], a["flags"], None)


_NO_FLAGS = ("%s takes no flags (got 0x1): GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning for an edge-feature aggregation, "
             "whose activation is `act`")
_BOTH = [
    (dict(flags=1), INVALID, _NO_FLAGS),
    (dict(dim=0), INVALID, "%s: dim must be >= 1 (got 0)"),
    (dict(n_out=-1), INVALID, "%s: negative size (num_out_rows=-1 num_in_rows=3 num_edges=5)"),
    (dict(n_in=-2), INVALID, "%s: negative size (num_out_rows=2 num_in_rows=-2 num_edges=5)"),
    (dict(nnz=-3), INVALID, "%s: negative size (num_out_rows=2 num_in_rows=3 num_edges=-3)"),
    (dict(combine=2), INVALID, "%s: combine must be GNNA_EDGE_ADD (0) or GNNA_EDGE_MUL (1) (got 2)"),
    (dict(combine=-1), INVALID, "%s: combine must be GNNA_EDGE_ADD (0) or GNNA_EDGE_MUL (1) (got -1)"),
    (dict(act=2), INVALID, "%s: act must be GNNA_EDGE_ACT_NONE (0) or GNNA_EDGE_ACT_RELU (1) (got 2)"),
    (dict(n_out=1 << 29), UNSUPPORTED, "%s: 536870912 rows in one call (at most 536870911): shard the rows"),
    (dict(n_in=1 << 29), UNSUPPORTED, "%s: 536870912 rows in one call (at most 536870911): shard the rows"),
    (dict(nnz=1 << 31), UNSUPPORTED, "%s: 2147483648 edges in one call (at most 2147483647): shard the rows"),
    (dict(x=A + 2), INVALID, None),
    (dict(e=B + 1), INVALID, None),
    (dict(x=None), INVALID, "%s: null feature pointer"),
    (dict(e=None), INVALID, "%s: null edge-feature pointer"),
]
_ALIGN = {FWD: "%s: feature, edge-feature and output pointers must be 4-byte aligned",
          BWD: "%s: feature, edge-feature and gradient pointers must be 4-byte aligned"}
_FWD_ONLY = [
    (dict(ld_in=3), INVALID, "%s: row strides must be >= dim and < 2^29 elements (ld_in=3 ld_e=4 ld_out=4 dim=4)"),
    (dict(ld_e=1 << 29), INVALID, "%s: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_e=536870912 ld_out=4 dim=4)"),
    (dict(ld_out=0), INVALID, "%s: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_e=4 ld_out=0 dim=4)"),
    (dict(out=C + 3), INVALID, _ALIGN[FWD]),
    (dict(out=A), INVALID, "%s: an output must not alias an input"),
    (dict(out=B), INVALID, "%s: an output must not alias an input"),
    (dict(out=None), INVALID, "%s: null output pointer"),
    (dict(rp=None), INVALID, "%s: null index pointer"),
    (dict(ci=None), INVALID, "%s: null index pointer"),
]
_BWD_ONLY = [
    (dict(ld_dy=3), INVALID, "%s: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_e=4 ld_dy=3 ld_din=4 ld_de=4 dim=4)"),
    (dict(ld_din=2), INVALID, "%s: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_e=4 ld_dy=4 ld_din=2 ld_de=4 dim=4)"),
    (dict(ld_de=1 << 29), INVALID, "%s: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_e=4 ld_dy=4 ld_din=4 ld_de=536870912 dim=4)"),
    (dict(dx=None, ld_din=1 << 29), INVALID,
     "%s: row strides must be >= dim and < 2^29 elements (ld_in=4 ld_e=4 ld_dy=4 ld_din=536870912 ld_de=4 dim=4)"),
    (dict(de=E_ + 2), INVALID, _ALIGN[BWD]),
    (dict(dy=C + 1), INVALID, _ALIGN[BWD]),
    (dict(dx=A), INVALID, "%s: an output must not alias an input"),
    (dict(de=C), INVALID, "%s: an output must not alias an input"),
    (dict(de=D), INVALID, "%s: the outputs must not alias each other"),
    (dict(dy=None), INVALID, "%s: null dY pointer"),
    (dict(rp=None), INVALID, "%s: null index pointer"),
    (dict(ci=None), INVALID, "%s: null index pointer"),
    (dict(trp=None), INVALID, "%s: null transposed index pointer (t_row_pointers, t_column_index and t_edge_pos are needed for d_input)"),
    (dict(tci=None), INVALID, "%s: null transposed index pointer (t_row_pointers, t_column_index and t_edge_pos are needed for d_input)"),
    (dict(tpos=None), INVALID, "%s: null transposed index pointer (t_row_pointers, t_column_index and t_edge_pos are needed for d_input)"),
]
_CASES = [(_fwd, FWD, *c) for c in _BOTH + _FWD_ONLY] + [(_bwd, BWD, *c) for c in _BOTH + _BWD_ONLY]


def _case_id(v):
    """str(v)[:40], with a host address of _F written as its name and offset (A+2): an id must not change from run to run."""
    if isinstance(v, dict):
        v = {k: "ABCDE"[(x - _BASE) // 64] + ("+%d" % ((x - _BASE) % 64) if (x - _BASE) % 64 else "")
             if isinstance(x, int) and _BASE <= x < _BASE + 320 else x for k, x in v.items()}
    return None if callable(v) else str(v)[:40]


@pytest.mark.parametrize("call, name, change, code, message", _CASES, ids=_case_id)
def test_every_refusal_returns_before_any_device_work(call, name, change, code, message):
    assert call(**change) == code
    got = _lib.load().gnna_last_error().decode()
    assert got == (message or _ALIGN[name]) % name


def test_calls_that_have_nothing_to_do_return_ok_without_a_device():
    assert _fwd(n_out=0, out=None, rp=None, ci=None) == 0
    assert _bwd(dx=None, de=None, trp=None, tci=None, tpos=None, rp=None, ci=None, dy=None) == 0
    assert _bwd(n_in=0, nnz=0, x=None, e=None) == 0                 # no row of d_input and no row of d_edge
    # a pass that is not wanted needs none of its arrays: the checks reach the launch only with both outputs NULL, so the null
    # transposed arrays are refused only when d_input is wanted
    assert _bwd(trp=None) == INVALID and "needed for d_input" in _lib.load().gnna_last_error().decode()


# ---- the restatement against fp64 autograd of the composed formula ----

@pytest.mark.parametrize("combine, act", ref.MODES)
def test_the_restatement_equals_fp64_autograd_of_the_composed_formula(combine, act):
    rp, ci = ref.small_rows_graph(40, 25, seed=5, lo=0, hi=6)
    x, e, dy = ref.operands(25, 40, len(ci), 7, seed=6)
    X = torch.from_numpy(x).double().requires_grad_()
    E = torch.from_numpy(e).double().requires_grad_()
    Y = ref.composed_torch(X, E, torch.from_numpy(rp), torch.from_numpy(ci), combine, act)
    Y.backward(torch.from_numpy(dy).double())
    out, scale = ref.forward(rp, ci, x, e, combine, act)
    d_in, s_in, d_e, s_e = ref.backward(rp, ci, x, e, dy, combine, act)
    assert (np.diff(rp) == 0).any()
    np.testing.assert_allclose(out, Y.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(d_in, X.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(d_e, E.grad.numpy(), rtol=0, atol=1e-12)
    assert (scale >= np.abs(out) - 1e-12).all() and (s_in >= np.abs(d_in) - 1e-12).all() and (s_e == np.abs(d_e)).all()


def test_the_restatement_skips_bad_ids_and_positions_and_zeroes_at_pre_zero():
    rp, ci = np.array([0, 2, 4], dtype=np.int32), np.array([0, 7, -1, 1], dtype=np.int32)
    x = np.array([[1.0], [-2.0]], dtype=np.float32)
    e = np.array([[-1.0], [5.0], [5.0], [3.0]], dtype=np.float32)
    dy = np.array([[2.0], [3.0]], dtype=np.float32)
    out, _ = ref.forward(rp, ci, x, e, "add", "relu")
    assert out.tolist() == [[0.0], [1.0]]                           # pre == 0 gives 0; ids 7 and -1 are skipped
    d_in, _, d_e, _ = ref.backward(rp, ci, x, e, dy, "add", "relu")
    assert d_in.tolist() == [[0.0], [3.0]] and d_e.tolist() == [[0.0], [0.0], [0.0], [3.0]]
    out, _ = ref.forward(rp, ci, x, e, "add", "none", num_edges=3)  # position 3 is beyond num_edges
    assert out.tolist() == [[0.0], [0.0]]


# ---- the op and the layers: errors raised before any device work ----

def _tiny_info():
    from gnnadvisor_osdi21_amd.decider import inputProperty  # noqa: F401  (the bundle type the op documents)
    rp, ci = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    return GraphBatch(rp, ci, torch.tensor([0, 2], dtype=torch.int32))


def test_op_and_layer_errors():
    from gnnadvisor_osdi21_amd.edgeconv import CFConv, EdgeFeatureSum, GINEConv
    info = _tiny_info()
    X, E = torch.zeros(2, 3), torch.zeros(2, 3)
    with pytest.raises(TypeError, match=r"EdgeFeatureSum: float32 only \(got X torch.float64 and E torch.float32\)"):
        EdgeFeatureSum.apply(X.double(), E, info)
    with pytest.raises(TypeError, match=r"EdgeFeatureSum: float32 only \(got X torch.float32 and E torch.bfloat16\)"):
        EdgeFeatureSum.apply(X, E.bfloat16(), info)
    with pytest.raises(ValueError, match=r"E must be \[nnz = 2, F = 3\]"):
        EdgeFeatureSum.apply(X, torch.zeros(3, 3), info)
    with pytest.raises(ValueError, match="combine must be 'add' or 'mul'"):
        EdgeFeatureSum.apply(X, E, info, "sub")
    with pytest.raises(ValueError, match="act must be 'none' or 'relu'"):
        EdgeFeatureSum.apply(X, E, info, "add", "gelu")
    with pytest.raises(TypeError, match="nn must be a torch.nn.Module"):
        GINEConv(lambda x: x)
    with pytest.raises(ValueError, match="edge_dim must be a positive integer"):
        GINEConv(torch.nn.Linear(3, 3), edge_dim=0)
    with pytest.raises(ValueError, match="nn has no Linear to read it from"):
        GINEConv(torch.nn.ReLU(), edge_dim=2)
    layer = GINEConv(torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU()), edge_dim=2, train_eps=True)
    assert layer.lin_edge.in_features == 2 and layer.lin_edge.out_features == 3 and isinstance(layer.eps, torch.nn.Parameter)
    with pytest.raises(ValueError, match="edge_attr is required"):
        layer(X, info, None)
    with pytest.raises(ValueError, match="num_filters must be a positive integer"):
        CFConv(3, 3, 0, torch.nn.Linear(2, 3))
    with pytest.raises(TypeError, match="filter_nn must be a torch.nn.Module"):
        CFConv(3, 3, 4, None)


def test_composed_layers_run_on_the_cpu_and_match_the_restatement():
    from gnnadvisor_osdi21_amd.edgeconv import composed_edge_feature_sum
    rp, ci = ref.small_rows_graph(12, 12, seed=2)
    x, e, _ = ref.operands(12, 12, len(ci), 5, seed=3)
    info = GraphBatch(torch.from_numpy(rp), torch.from_numpy(ci), torch.tensor([0, 12], dtype=torch.int32))
    for combine, act in ref.MODES:
        got = composed_edge_feature_sum(torch.from_numpy(x), torch.from_numpy(e), info, combine, act)
        want, scale = ref.forward(rp, ci, x, e, combine, act)
        assert (np.abs(got.numpy() - want) <= 1e-5 * np.maximum(1, scale)).all()


# ---- edge attributes on batches ----

def _three_graphs():
    graphs = [(torch.tensor([0, 2, 3, 4]), torch.tensor([1, 2, 0, 0])), (torch.tensor([0]), torch.tensor([], dtype=torch.int64)),
              (torch.tensor([0, 1, 2]), torch.tensor([1, 0]))]
    edge_attr = torch.arange(6, dtype=torch.float32).reshape(6, 1) * torch.ones(1, 2)          # row e holds (e, e)
    return graphs, edge_attr


def test_dataset_batches_carry_the_edge_rows_of_their_edges():
    graphs, edge_attr = _three_graphs()
    ds = GraphDataset.from_graphs(graphs, edge_attr=edge_attr)
    assert ds.edge_attr is edge_attr or torch.equal(ds.edge_attr, edge_attr)
    b = ds.batch([2, 1, 0, 2])
    assert b.edge_attr[:, 0].tolist() == [4, 5, 0, 1, 2, 3, 4, 5] and b.column_index.tolist() == [1, 0, 3, 4, 2, 2, 6, 5]
    assert ds.batch([1]).edge_attr.shape == (0, 2)
    assert GraphDataset.from_graphs(graphs).batch([0]).edge_attr is None            # nothing changes for a caller that passes none
    whole = GraphBatch.from_graphs(graphs, edge_attr=edge_attr)
    assert torch.equal(whole.edge_attr, edge_attr) and torch.equal(whole.to("cpu").edge_attr, edge_attr)
    with pytest.raises(ValueError, match=r"edge_attr must be \[nnz = 6, K\]"):
        GraphBatch.from_graphs(graphs, edge_attr=edge_attr[:5])
    with pytest.raises(ValueError, match=r"edge_attr must be \[nnz = 6, K\]"):
        GraphDataset(whole.row_pointers, whole.column_index, whole.graph_pointers, edge_attr=edge_attr[:5])


def test_carry_edge_attr_follows_the_edge_ids_of_a_coarsening():
    from gnnadvisor_osdi21_amd.ops import _composed_coarsen
    graphs, edge_attr = _three_graphs()
    b = GraphBatch.from_graphs(graphs, edge_attr=edge_attr)
    score = torch.tensor([3.0, 1.0, 2.0, 1.0, 2.0])                  # graph 0 keeps rows 0 and 2, graph 2 keeps row 4
    small, sel = _composed_coarsen(b, score, ratio=0.5)
    assert sel.perm.tolist() == [0, 2, 4] and sel.edge_ids.tolist() == [1, 3]
    assert b.carry_edge_attr(small, sel) is small and small.edge_attr[:, 0].tolist() == [1, 3]
    plain = GraphBatch.from_graphs(graphs)
    assert plain.carry_edge_attr(small, TopKSelection(sel.perm, sel.new_id, None, 5)).edge_attr is None


# ---- the driver ----

@pytest.mark.parametrize("extra, message", [
    (["--model", "gat"], r"--model gat: graph_main trains gcn or gin \(the other layers take a GraphBatch too: build the model with "
                         r"ops\), or gine with --edge_dim K"),
    (["--model", "gine"], r"--model gine needs --edge_dim K with K >= 1: the features per edge \(got 0\)"),
    (["--model", "gine", "--edge_dim", "-2"], r"--model gine needs --edge_dim K with K >= 1"),
    (["--model", "gin", "--edge_dim", "4"], r"--edge_dim 4: only --model gine takes edge features \(got --model gin\)"),
])
def test_driver_refusals(extra, message):
    with pytest.raises(SystemExit, match=message):
        graph_main.main(extra)


def test_driver_flags_parse():
    args = graph_main.build_parser().parse_args(["--model", "gine", "--edge_dim", "4", "--fused_edge", "False"])
    assert (args.model, args.edge_dim, args.fused_edge) == ("gine", 4, False)
    assert graph_main.build_parser().parse_args([]).edge_dim == 0 and graph_main.build_parser().parse_args([]).fused_edge is True

"""structure.py, the parts that need no GPU: the rule of ``backward_structure`` on graphs that are not ``directed`` (what it returns,
what it checks, which cache entries exist afterwards) and the class relations the bundles rely on."""
import types

import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, decider, sampling, structure
from gnnadvisor_osdi21_amd.batching import GraphBatch
from gnnadvisor_osdi21_amd.decider import inputProperty
from gnnadvisor_osdi21_amd.structure import GraphStructure, backward_structure

# symmetric: 0 - 1, 0 - 2, 2 - 2 (self loop), node 3 isolated
SYM_RP, SYM_CI = [0, 2, 3, 5, 5], [1, 2, 0, 0, 2]
# directed: 0 <- 1 only
DIR_RP, DIR_CI = [0, 1, 1], [1]


def _bundle(kind, rp, ci):
    """The CSR as a profile made without its constructor, or as a bare object with the two arrays and nothing else."""
    info = inputProperty.__new__(inputProperty) if kind == "profile" else types.SimpleNamespace()
    info.row_pointers, info.column_index = torch.tensor(rp, dtype=torch.int32), torch.tensor(ci, dtype=torch.int32)
    return info


@pytest.mark.parametrize("kind", ["profile", "bare"])
def test_the_rule_on_a_symmetric_graph(kind):
    info = _bundle(kind, SYM_RP, SYM_CI)
    assert backward_structure(info) is info                           # nothing checked, nothing built
    assert set(GraphStructure._edge_arrays(info)) == {"column_index"}
    assert backward_structure(info, require_symmetric=True) is info
    cache = GraphStructure._edge_arrays(info)
    assert cache.get("symmetric") is True and "rev" not in cache and set(cache) == {"column_index", "symmetric"}
    same, pos = backward_structure(info, edge_pos=True)
    assert same is info and pos.dtype == torch.int32
    assert torch.equal(pos, _lib.reverse_edges(info.row_pointers, info.column_index))
    assert pos is GraphStructure._edge_arrays(info)["rev"]


@pytest.mark.parametrize("kind", ["profile", "bare"])
def test_the_map_alone_makes_no_symmetric_entry_and_both_flags_keep_the_operators_order(kind):
    info = _bundle(kind, SYM_RP, SYM_CI)
    backward_structure(info, edge_pos=True)
    assert set(GraphStructure._edge_arrays(info)) == {"column_index", "rev"}      # a graph that has the map is known symmetric
    backward_structure(info, require_symmetric=True)
    assert "symmetric" not in GraphStructure._edge_arrays(info)
    fresh = _bundle(kind, SYM_RP, SYM_CI)
    same, pos = backward_structure(fresh, require_symmetric=True, edge_pos=True)   # the edge-term operators: check, then map
    assert same is fresh and set(GraphStructure._edge_arrays(fresh)) == {"column_index", "symmetric", "rev"}
    assert torch.equal(pos, _lib.reverse_edges(fresh.row_pointers, fresh.column_index))


@pytest.mark.parametrize("kind", ["profile", "bare"])
@pytest.mark.parametrize("flags", [{"require_symmetric": True}, {"edge_pos": True}, {"require_symmetric": True, "edge_pos": True}])
def test_a_structure_that_is_not_symmetric_is_refused_every_time(kind, flags):
    bad = _bundle(kind, DIR_RP, DIR_CI)
    with pytest.raises(_lib.GnnaError):
        backward_structure(bad, **flags)
    with pytest.raises(_lib.GnnaError):                               # a refusal is not cached as a pass
        backward_structure(bad, **flags)
    assert set(GraphStructure._edge_arrays(bad)) == {"column_index"}
    assert backward_structure(bad) is bad                             # unasked, nothing is checked: the reference's assumption


def test_the_unbound_calls_work_on_a_bare_bundle():
    info = _bundle("bare", SYM_RP, SYM_CI)
    inputProperty.require_symmetric(info)
    assert torch.equal(inputProperty.reverse_edges(info), _lib.reverse_edges(info.row_pointers, info.column_index))
    assert inputProperty.edge_rows(info).tolist() == [0, 0, 1, 2, 2]
    assert set(inputProperty._edge_arrays(info)) == {"column_index", "symmetric", "rev", "rows"}


def test_the_bundles_derive_from_one_base():
    assert issubclass(inputProperty, GraphStructure) and issubclass(GraphBatch, GraphStructure)
    assert issubclass(sampling.Subgraph, GraphStructure)
    for name in ("_edge_arrays", "reverse_edges", "require_symmetric", "transposed", "backward_graph", "edge_rows", "inv_row_counts"):
        assert name in vars(GraphStructure)
        assert name not in vars(inputProperty) and name not in vars(GraphBatch), f"{name} is defined twice"
    borrowed = [n for n, v in vars(GraphBatch).items() if isinstance(v, types.FunctionType) and "inputProperty." in v.__qualname__]
    assert borrowed == []


def test_one_class_owns_the_lazy_perm():
    assert decider.TransposedGraph is structure.TransposedGraph
    owners = [{c for c in cls.__mro__ if "perm" in vars(c)} for cls in (decider.TransposedGraph, sampling._BlockTranspose)]
    assert owners[0] == owners[1] == {structure.Transpose}
    assert isinstance(structure.Transpose.perm, property)
    assert "degrees" in vars(decider.TransposedGraph) and not hasattr(sampling._BlockTranspose, "degrees")


def test_structure_imports_neither_decider_nor_sampling():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(structure))
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) for a in n.names}
    names |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) if n.module}
    assert not names & {"decider", "sampling"}

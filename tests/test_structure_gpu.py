"""structure.backward_structure on ``directed`` bundles: a profile, a batch of two graphs, an induced subgraph and a sampled block
of one small directed graph.  The structure it returns is the bundle's own transposed one, the position map is that one's
``perm`` and agrees with a transpose made on the host, and nothing is built that was not asked for."""
import types

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd.batching import GraphBatch
from gnnadvisor_osdi21_amd.decider import inputProperty
from gnnadvisor_osdi21_amd.sampling import SampledBlock, Subgraph, induced_subgraph
from gnnadvisor_osdi21_amd.structure import GraphStructure, backward_structure

pytestmark = pytest.mark.gpu

# 6 nodes, 9 directed edges: row 2 has no edges, id 4 is in no row, row 3 has a self loop
RP = [0, 2, 3, 3, 6, 8, 9]
CI = [1, 2, 2, 0, 1, 3, 0, 5, 1]


def _profile():
    ds = types.SimpleNamespace(num_nodes=6, avg_degree=1.5, avg_edgeSpan=1.0, num_features=4)
    rp, ci = torch.tensor(RP, dtype=torch.int32).cuda(), torch.tensor(CI, dtype=torch.int32).cuda()
    ip = inputProperty(rp, ci, torch.ones(6, device="cuda"), 32, 32, 4, hiddenDim=4, dataset_obj=ds)
    ip.directed = True
    return ip


def _bundle(kind):
    if kind == "profile":
        return _profile()
    if kind == "batch":
        pair = (torch.tensor(RP), torch.tensor(CI))
        return GraphBatch.from_graphs([pair, pair], directed=True).to("cuda")
    if kind == "subgraph":
        sub = induced_subgraph(_profile(), [0, 1, 3, 4, 5])
        assert isinstance(sub, Subgraph) and sub.directed and sub.column_index.numel() > 0
        return sub
    ip = _profile()
    seeds = torch.tensor([3, 0, 4], dtype=torch.int32).cuda()
    return SampledBlock.sample(ip.row_pointers, ip.column_index, seeds, 2, rng_seed=7)


def _nothing_else_was_built(x):
    cache = getattr(x, "_edge_cache", {})             # (a block keeps no such cache at all)
    return not {"rev", "rows", "symmetric"} & set(cache)


@pytest.mark.parametrize("kind", ["profile", "batch", "subgraph", "block"])
def test_a_directed_bundle_walks_its_own_transpose(kind):
    x = _bundle(kind)
    t = backward_structure(x)
    assert t is x.transposed() and t is backward_structure(x, require_symmetric=True)      # (no symmetry question is asked)
    assert t._perm is None and _nothing_else_was_built(x)
    if isinstance(x, GraphStructure):
        assert t is x.backward_graph() and t.degrees is x.degrees
    for name in ("row_pointers", "column_index", "partPtr", "part2Node", "partSize"):
        assert getattr(t, name) is not None
    same, pos = backward_structure(x, edge_pos=True)
    assert same is t and pos is t.perm and t._perm is not None and pos.dtype == torch.int32
    assert backward_structure(x, require_symmetric=True, edge_pos=True)[1] is pos
    assert _nothing_else_was_built(x)

    # against a transpose made on the host: transposed row j holds, at position p, the edge perm[p] = (i <- j) and names i
    rp, ci = x.row_pointers.cpu().numpy().astype(np.int64), x.column_index.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    num_in = int(x.num_src) if kind == "block" else rp.size - 1
    t_rp, t_ci, perm = (a.cpu().numpy().astype(np.int64) for a in (t.row_pointers, t.column_index, pos))
    assert t_rp.size - 1 == num_in and np.array_equal(np.diff(t_rp), np.bincount(ci, minlength=num_in))
    assert np.array_equal(np.sort(perm), np.arange(ci.size))           # every forward edge exactly once
    t_rows = np.repeat(np.arange(num_in), np.diff(t_rp))
    assert np.array_equal(ci[perm], t_rows) and np.array_equal(rows[perm], t_ci)

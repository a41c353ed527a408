"""Four device builders, one partition: gnna_build_part_device_i32, gnna_sample_neighbors_i32, gnna_segment_topk_i32 and
gnna_induced_subgraph_i32 write their neighbor-group partition by the one rule of csrc/gnna_parts.h.  Asked for the whole of one
graph -- every row a seed with every edge, one segment kept whole, every node listed -- each gives the graph's own row pointers
back, and then partPtr / part2Node element for element what the host's gnna_build_part_i32 gives for them."""
import functools

import numpy as np
import pytest
import torch

import sampling_ref
import topk_ref
import walk_ref
from gnnadvisor_osdi21_amd import _lib

pytestmark = pytest.mark.gpu

PART_SIZES = [1, 3, 32, 4096]
GRAPHS = ["mixed", "no_rows", "no_edges"]
BUILDERS = ["build_part_device", "sample_neighbors", "segment_topk", "induced_subgraph"]


def _mixed_degrees():
    """About 300 rows: an empty first and last row, a run of five empty rows, rows of exactly 32, 33 and 1 edges and one hub of
    2,100 edges (beyond the 2,048 positions at which sampling and the subgraph cut give a row a whole block)."""
    rng = np.random.default_rng(20261020)
    deg = rng.integers(0, 13, size=300)
    deg[0] = deg[-1] = 0
    deg[100:105] = 0
    deg[99], deg[105] = 4, 7
    deg[10], deg[11], deg[12], deg[50] = 32, 33, 1, 2100
    return rng, deg


@functools.lru_cache(maxsize=None)
def graph(name):
    """(row_pointers, column_index) int32 numpy; every column id is valid.  The three host restatements are checked here to give
    the row pointers back for the arguments the tests use: the tests rely on it."""
    if name == "mixed":
        rng, deg = _mixed_degrees()
    else:
        rng, deg = np.random.default_rng(7), np.zeros(0 if name == "no_rows" else 7, dtype=np.int64)
    n = len(deg)
    rp = np.concatenate(([0], np.cumsum(deg))).astype(np.int32)
    ci = rng.integers(0, max(n, 1), size=int(rp[-1])).astype(np.int32)
    every = np.arange(n, dtype=np.int32)
    assert (sampling_ref.sample_block(rp, ci, every, 0, 1)["row_pointers"] == rp).all()
    assert (topk_ref.segment_topk(scores(n), [0, n], ratio=1.0, row_pointers=rp, column_index=ci)["row_pointers"] == rp).all()
    assert (walk_ref.induced_subgraph(rp, ci, every)["row_pointers"] == rp).all()
    return rp, ci


def scores(n):
    return np.random.default_rng(11).standard_normal(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_partition(name, partSize):
    pp, p2n = _lib.build_part(partSize, torch.from_numpy(graph(name)[0]))
    return pp.numpy().copy(), p2n.numpy().copy()


def device_partition(builder, name, partSize):
    """-> (row pointers the builder gave back or None, partPtr, part2Node) as numpy"""
    rp, ci = (torch.from_numpy(a).cuda() for a in graph(name))
    n = rp.numel() - 1
    every = torch.arange(n, dtype=torch.int32, device="cuda")
    if builder == "build_part_device":
        pp, p2n = _lib.build_part_device(partSize, rp)
        return None, pp.cpu().numpy(), p2n.cpu().numpy()
    if builder == "sample_neighbors":
        got = _lib.sample_neighbors(rp, ci, every, 0, 1, partSize=partSize)
    elif builder == "segment_topk":
        gp = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        got = _lib.segment_topk(torch.from_numpy(scores(n)).cuda(), gp, ratio=1.0, row_pointers=rp, column_index=ci, partSize=partSize)
    else:
        got = _lib.induced_subgraph(rp, ci, every, partSize=partSize)
    return got["row_pointers"].cpu().numpy(), got["partPtr"].cpu().numpy(), got["part2Node"].cpu().numpy()


@pytest.mark.parametrize("partSize", PART_SIZES)
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_every_builder_writes_the_hosts_partition(builder, name, partSize):
    want_pp, want_p2n = host_partition(name, partSize)
    got_rp, pp, p2n = device_partition(builder, name, partSize)
    if got_rp is not None:
        assert np.array_equal(got_rp, graph(name)[0])
    assert pp.dtype == np.int32 and p2n.dtype == np.int32
    assert np.array_equal(pp, want_pp)
    assert np.array_equal(p2n, want_p2n)


def test_the_graph_has_the_rows_the_partition_can_get_wrong():
    rp, _ = graph("mixed")
    deg = np.diff(rp)
    assert deg[0] == 0 and deg[-1] == 0 and (deg[100:105] == 0).all() and deg[99] > 0 and deg[105] > 0
    assert {1, 32, 33, 2100} <= set(deg.tolist()) and deg.max() == 2100 > 2048

"""Neighbor sampling for mini-batch GraphSAGE: ``NeighborSampler`` draws, on the device, the blocks of a batch of seed
nodes (libgnna ``gnna_sample_neighbors_i32``: one launch sequence and one read-back per block) and ``SampledBlock`` is what a
layer gets in place of a ``decider.inputProperty``.

A block is a rectangular graph: ``num_dst`` destination rows (the seeds, local ids ``0 .. num_dst-1``) gather from ``num_src``
source rows (the seeds first, then every other sampled node in increasing global id).  The destination features of a block
are therefore the first ``num_dst`` rows of its source features, and the blocks of consecutive layers chain without any
indexing: ``blocks[l-1].num_dst == blocks[l].num_src``.

libgnna keys its per-graph tables (slice plans, hints) by the device address of ``column_index``, and PyTorch's caching
allocator hands the address of a dropped block to the next one: a block drops the library's entries together with its
storage (``_lib._forget_when_freed``) and never calls ``prepare_graph``.

Subgraph sampling is the other family: ``RandomWalkSampler`` walks on the device (libgnna ``gnna_random_walk_i32``),
``induced_subgraph`` cuts the subgraph of an arbitrary node list out on the device (``gnna_induced_subgraph_i32``: one launch
sequence and one read-back) and ``SaintRWSampler`` puts the two together as GraphSAINT's random-walk sampler.  A ``Subgraph`` is a
``batching.GraphBatch`` of one graph -- an ordinary square CSR bundle -- so every layer that takes a graph batch runs on it
unchanged, at full-graph depth, where a ``SampledBlock`` needs one block per layer.
"""
from __future__ import annotations

import torch

from . import _lib
from .batching import GraphBatch
from .structure import Transpose


class _BlockTranspose(Transpose):
    """A^T of a block with its partition: [num_src] rows gathering from [num_dst] rows (what the backward of a sum runs on).
    ``perm`` is the base's: built at its first use, which only the operators with a per-edge operand make."""

    def __init__(self, block):
        source = (block.row_pointers, block.column_index)
        t_rp, t_ci, _ = _lib.transpose_csr(*source, num_in_rows=block.num_src, want_perm=False)
        super().__init__(t_rp, t_ci, block.partSize, source)
        if self.column_index.numel() > 0:
            _lib._forget_when_freed(self.column_index)


class SampledBlock(object):
    """One sampled block.  It has the attributes a layer reads from a graph bundle -- ``row_pointers column_index partPtr
    part2Node partSize`` -- over LOCAL source ids, plus ``num_dst``, ``num_src``, ``src_nodes`` (int32 [num_src]: the global id
    of every local source; ``src_nodes[:num_dst]`` are the seeds in the order given) and ``edge_ids`` (int32 [nnz]: the
    position of every block edge in the full graph's column_index).  ``directed`` is true by nature: a block is never
    symmetric, so the backward of a neighbor sum runs on ``transposed()``."""

    directed = True

    def __init__(self, row_pointers, column_index, partPtr, part2Node, partSize, num_dst, num_src, src_nodes, edge_ids=None):
        self.row_pointers, self.column_index = row_pointers, column_index
        self.partPtr, self.part2Node, self.partSize = partPtr, part2Node, int(partSize)
        self.num_dst, self.num_src = int(num_dst), int(num_src)
        self.src_nodes, self.edge_ids = src_nodes, edge_ids
        self._inv_counts = self._transposed = None
        if column_index.numel() > 0:
            _lib._forget_when_freed(column_index)

    @classmethod
    def sample(cls, row_pointers, column_index, seeds, fanout, rng_seed, partSize=32, want_edge_ids=True):
        """The block of the destination rows `seeds` (distinct int32 ids on the graph's device) of a device CSR."""
        r = _lib.sample_neighbors(row_pointers, column_index, seeds, fanout, rng_seed, partSize=partSize,
                                  want_edge_ids=want_edge_ids)
        return cls(r["row_pointers"], r["column_index"], r["partPtr"], r["part2Node"], partSize, r["num_dst"], r["num_src"],
                   r["src_nodes"], r["edge_ids"])

    def inv_row_counts(self):
        """float32 [num_dst]: 1 / max(sampled edges of the row, 1) -- the block's OWN counts, the row factor of a neighbor mean."""
        if self._inv_counts is None:
            rp = self.row_pointers.long()
            self._inv_counts = 1.0 / (rp[1:] - rp[:-1]).clamp(min=1).float()
        return self._inv_counts

    def transposed(self):
        """The transposed block (built on the device at its first use and kept): gnna_transpose_csr_i32 with
        num_in_rows = num_src, and the partition of the result at the same partSize.  Synchronises."""
        if self._transposed is None:
            self._transposed = _BlockTranspose(self)
        return self._transposed


class NeighborSampler(object):
    """``NeighborSampler(inputInfo, fanouts)``: `inputInfo` holds the full graph's device ``row_pointers`` / ``column_index``
    (a ``decider.inputProperty``, or any bundle with them); ``fanouts[l]`` is the number of neighbours layer `l` samples per
    destination (<= 0: all of them).  partSize defaults to the bundle's.  want_edge_ids: the blocks keep ``edge_ids`` (what
    per-edge data of the full graph -- relation types -- is read through)."""

    def __init__(self, inputInfo, fanouts, partSize=None, want_edge_ids=False):
        self.fanouts = [int(f) for f in fanouts]
        if not self.fanouts:
            raise ValueError("fanouts must name at least one layer")
        ci = inputInfo.column_index
        if not getattr(ci, "is_cuda", False):
            raise ValueError("the sampler runs on the device: move row_pointers and column_index to the GPU first")
        self.column_index = ci
        self.row_pointers = inputInfo.row_pointers.to(ci.device)
        self.partSize = int(partSize if partSize is not None else (getattr(inputInfo, "partSize", None) or 32))
        self.want_edge_ids = bool(want_edge_ids)

    def sample(self, seeds, rng_seed):
        """-> (blocks, input_nodes).  Sampled from the batch outwards: the last layer's block has `seeds` as destinations, the
        block of layer l-1 takes ALL of block l's src_nodes as its seeds, in that order; hop l uses rng_seed + l.
        input_nodes = blocks[0].src_nodes: the rows of the feature matrix the first layer reads."""
        dst = torch.as_tensor(seeds).to(device=self.column_index.device, dtype=torch.int32).contiguous()
        blocks = []
        for layer in reversed(range(len(self.fanouts))):
            blk = SampledBlock.sample(self.row_pointers, self.column_index, dst, self.fanouts[layer], int(rng_seed) + layer,
                                      self.partSize, want_edge_ids=self.want_edge_ids)
            blocks.append(blk)
            dst = blk.src_nodes
        blocks.reverse()
        return blocks, blocks[0].src_nodes


# ---- subgraph sampling: walks, induced subgraphs, GraphSAINT-RW ----------------------------------------------------------------

def _device_graph(inputInfo, who):
    ci = inputInfo.column_index
    if not getattr(ci, "is_cuda", False):
        raise ValueError(f"{who} runs on the device: move row_pointers and column_index to the GPU first")
    return inputInfo.row_pointers.to(ci.device), ci


class Subgraph(GraphBatch):
    """The subgraph a node set induces in a parent graph, as a ``GraphBatch`` of ONE graph (``graph_pointers = [0, n]``): every
    layer that takes a graph batch takes it.  Beyond the batch it carries ``nodes`` (int32 [n]: the global id of every row,
    increasing), ``edge_ids`` (int32 [nnz']: the position of every edge in the parent's column_index, or None) and
    ``parent_num_nodes``.  ``directed``, ``partSize`` and the launch knobs are the parent bundle's; the degrees come from the new
    row pointers.  ``node_weight`` (float32 [n]) and ``edge_weight`` (float32 [nnz']) are GraphSAINT's normalisation
    coefficients read through ``nodes`` / ``edge_ids``; None unless the sampler that made the subgraph has estimated them."""

    def __init__(self, result, parent, norms=None):
        n = int(result["num_nodes"])
        dev = result["row_pointers"].device
        super().__init__(result["row_pointers"], result["column_index"], torch.tensor([0, n], dtype=torch.int32, device=dev),
                         partSize=int(getattr(parent, "partSize", None) or 32), dimWorker=getattr(parent, "dimWorker", None),
                         warpPerBlock=getattr(parent, "warpPerBlock", None), directed=bool(getattr(parent, "directed", False)),
                         partPtr=result["partPtr"], part2Node=result["part2Node"])
        self.nodes, self.edge_ids = result["nodes"], result["edge_ids"]
        self.parent_num_nodes = int(parent.row_pointers.numel()) - 1
        self._norms = norms
        if self.column_index.numel() > 0:
            _lib._forget_when_freed(self.column_index)

    @property
    def node_weight(self):
        return None if self._norms is None else self._norms[0].index_select(0, self.nodes.long())

    @property
    def edge_weight(self):
        if self._norms is None:
            return None
        if self.edge_ids is None:
            raise ValueError("edge_weight is read through edge_ids: cut the subgraph with want_edge_ids=True")
        return self._norms[1].index_select(0, self.edge_ids.long())


def induced_subgraph(inputInfo, nodes, want_edge_ids=True, *, edge_capacity=None, _norms=None):
    """The ``Subgraph`` that `nodes` (ids on the graph's device, or anything ``torch.as_tensor`` takes; duplicates welcome, -1
    skipped) induces in the graph bundle `inputInfo`: its kept nodes are the distinct ids in increasing global id, every row keeps
    its edges to kept nodes in their order.  One libgnna call and one read-back; the partition comes with it."""
    rp, ci = _device_graph(inputInfo, "induced_subgraph")
    ids = torch.as_tensor(nodes).to(device=ci.device, dtype=torch.int32).reshape(-1).contiguous()
    partSize = int(getattr(inputInfo, "partSize", None) or 32)
    r = _lib.induced_subgraph(rp, ci, ids, partSize=partSize, want_edge_ids=want_edge_ids, edge_capacity=edge_capacity)
    return Subgraph(r, inputInfo, _norms)


class RandomWalkSampler(object):
    """``RandomWalkSampler(inputInfo, walk_length).walk(roots, rng_seed)`` -> (walks int32 [R, walk_length + 1], edge_ids int32
    [R, walk_length] or None): uniform first-order walks on the device, a function of (rng_seed, walk, step) and the graph only
    (DeepWalk / node2vec corpora with p = q = 1, PinSAGE visit counts, the GraphSAINT-RW sampler).  No read-back: capturable."""

    def __init__(self, inputInfo, walk_length):
        self.row_pointers, self.column_index = _device_graph(inputInfo, "the walk sampler")
        self.walk_length = int(walk_length)
        if self.walk_length < 0:
            raise ValueError("walk_length must not be negative")

    def walk(self, roots, rng_seed, want_edge_ids=False):
        roots = torch.as_tensor(roots).to(device=self.column_index.device, dtype=torch.int32).reshape(-1).contiguous()
        return _lib.random_walk(self.row_pointers, self.column_index, roots, self.walk_length, rng_seed, want_edge_ids=want_edge_ids)


class SaintRWSampler(object):
    """GraphSAINT's random-walk sampler: ``sample(step)`` draws `num_roots` roots from a device generator seeded with
    (seed, step), walks `walk_length` steps from each (one call) and returns the ``Subgraph`` that the visited nodes induce (one
    call on ``walks.reshape(-1)``).  The same (seed, step) gives the same subgraph.  The edge buffer of the next call is sized at
    1.25x the largest subgraph seen so far; a call it was too small for is repeated once with the size the library reported.

    ``estimate_norms(T)`` is GraphSAINT's pre-sampling: over the subgraphs of the steps -1 .. -T, C_v counts those holding node
    v and C_e those holding edge position e (``node_count`` / ``edge_count``, int64; integer ``index_add_`` is order-independent);
    a zero count then counts 0.1.  ``node_weight[v] = T / (N C_v)`` weighs the loss of node v, ``edge_weight[e] =
    clamp(C_row(e) / C_e, 0, 1e4)`` the aggregation over edge e (``ops.EdgeWeightedAggregate``); every later ``Subgraph`` reads
    them through its ``nodes`` / ``edge_ids``."""

    def __init__(self, inputInfo, num_roots, walk_length, seed=0):
        self.inputInfo = inputInfo
        self.walker = RandomWalkSampler(inputInfo, walk_length)
        self.num_roots, self.walk_length, self.seed = int(num_roots), int(walk_length), int(seed)
        if self.num_roots < 1:
            raise ValueError("num_roots must be >= 1")
        self.num_nodes = int(self.walker.row_pointers.numel()) - 1
        self.max_edges = 0                    # the largest nnz' seen
        self.node_count = self.edge_count = self.node_weight = self.edge_weight = None

    def _step_seed(self, step):
        return (self.seed * 0x9E3779B97F4A7C15 + int(step)) & 0x7FFFFFFFFFFFFFFF

    def roots(self, step):
        dev = self.walker.column_index.device
        gen = torch.Generator(device=dev).manual_seed(self._step_seed(step))
        return torch.randint(0, max(self.num_nodes, 1), (self.num_roots,), generator=gen, device=dev, dtype=torch.int32)

    def sample(self, step):
        walks, _ = self.walker.walk(self.roots(step), self._step_seed(step))
        ids = walks.reshape(-1)
        norms = None if self.node_weight is None else (self.node_weight, self.edge_weight)
        capacity = min(int(self.max_edges * 1.25) + 1, int(self.walker.column_index.numel())) if self.max_edges > 0 else None
        try:
            sub = induced_subgraph(self.inputInfo, ids, edge_capacity=capacity, _norms=norms)
        except _lib.GnnaError as err:
            counts = getattr(err, "counts", None)
            if capacity is None or counts is None or "capacity too small" not in str(err):
                raise
            sub = induced_subgraph(self.inputInfo, ids, edge_capacity=counts[1], _norms=norms)      # once, from what it reported
        self.max_edges = max(self.max_edges, int(sub.column_index.numel()))
        return sub

    def estimate_norms(self, num_subgraphs):
        T = int(num_subgraphs)
        if T < 1:
            raise ValueError("num_subgraphs must be >= 1")
        rp, ci = self.walker.row_pointers, self.walker.column_index
        dev = ci.device
        self.node_weight = self.edge_weight = None                      # (the pre-sampled subgraphs carry no weights)
        node_count = torch.zeros(self.num_nodes, dtype=torch.int64, device=dev)
        edge_count = torch.zeros(ci.numel(), dtype=torch.int64, device=dev)
        for i in range(T):
            sub = self.sample(-(i + 1))
            node_count.index_add_(0, sub.nodes.long(), torch.ones(sub.nodes.numel(), dtype=torch.int64, device=dev))
            edge_count.index_add_(0, sub.edge_ids.long(), torch.ones(sub.edge_ids.numel(), dtype=torch.int64, device=dev))
        self.node_count, self.edge_count = node_count, edge_count
        c_v = node_count.double().masked_fill(node_count == 0, 0.1)
        c_e = edge_count.double().masked_fill(edge_count == 0, 0.1)
        rows = torch.repeat_interleave(torch.arange(self.num_nodes, device=dev), (rp[1:] - rp[:-1]).long().clamp(min=0),
                                       output_size=ci.numel())
        self.node_weight = (T / (self.num_nodes * c_v)).float()
        self.edge_weight = (c_v[rows] / c_e).clamp(0, 1e4).float()
        return self.node_weight, self.edge_weight

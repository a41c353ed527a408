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
"""
from __future__ import annotations

import torch

from . import _lib


class _BlockTranspose(object):
    """A^T of a block with its partition: [num_src] rows gathering from [num_dst] rows (what the backward of a sum runs on).
    ``perm`` (int32 [nnz]: position in the block's column_index of every transposed edge) is built at its first use, which only
    the attention with an edge term makes."""

    def __init__(self, block):
        self._source, self._num_src, self._perm = (block.row_pointers, block.column_index), block.num_src, None
        self.row_pointers, self.column_index, _ = _lib.transpose_csr(block.row_pointers, block.column_index,
                                                                     num_in_rows=block.num_src, want_perm=False)
        self.partSize = block.partSize
        self.partPtr, self.part2Node = _lib.build_part_device(self.partSize, self.row_pointers)
        if self.column_index.numel() > 0:
            _lib._forget_when_freed(self.column_index)

    @property
    def perm(self):
        if self._perm is None:
            # (the builder gives the same bits on every run; an edge dropped for an id outside the block sits behind every row)
            self._perm = _lib.transpose_csr(*self._source, num_in_rows=self._num_src)[2].clamp_(min=0)
        return self._perm


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

"""Graphs whose edges carry a relation type: ``RelationalGraph`` is what ``ops.TypedAggregate`` / ``ops.RGCNConv`` take next to
the features.  It wraps a graph bundle -- a ``decider.inputProperty`` (after ``decider()``, CSR and partition on the device) or
a ``sampling.SampledBlock`` -- and adds, per edge position of ``column_index``, the type and the factor the relation-typed
kernels of libgnna read (``gnna_agg_typed_expand_ld_f32`` and its two backward passes, include/gnna.h).

Both per-edge arrays are made once, at construction: that is prepare time, like the partition.  A training step makes no
tensor of the size of the edge list.
"""
from __future__ import annotations

import torch

from . import _lib


def synthetic_edge_types(row_pointers, column_index, num_relations: int, seed: int = 0) -> torch.Tensor:
    """int32 [nnz] on column_index's device: t[e] = hash(seed, row(e), col(e)) mod num_relations.  A function of the edge's end
    points in the CSR it is given, so it is made after any renumbering, from the final CSR."""
    ci = column_index
    rp = row_pointers.to(ci.device).long()
    n = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=ci.device), rp[1:] - rp[:-1])
    mask = 0x7FFFFFFF
    h = (rows * 0x9E3779B1 + ci.long() * 0x85EBCA77 + (int(seed) & mask)) & mask
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & mask
    h = ((h ^ (h >> 12)) * 0x297A2D39) & mask
    h = h ^ (h >> 15)
    return (h % int(num_relations)).to(torch.int32)


class _TypedTranspose(object):
    """A^T of the wrapped structure with the forward edge arrays read through its permutation."""

    def __init__(self, graph, perm, edge_type, edge_norm):
        self.graph = graph
        idx = perm.long()
        self.edge_type = edge_type.index_select(0, idx).contiguous()
        self.edge_norm = None if edge_norm is None else edge_norm.index_select(0, idx).contiguous()


class RelationalGraph(object):
    """``RelationalGraph(info, edge_type, num_relations, norm="relation" | None)``.

    ``edge_type``: one integer in [0, num_relations) per position of ``info.column_index`` (kept as device int32; an edge whose
    type is outside the range counts for nothing).  ``norm="relation"`` gives every edge R-GCN's factor 1 / |N_r(i)|: one over
    the number of edges of its destination row that have its type; ``None`` gives none.

    The transposed structure, with the two edge arrays permuted to its order, is what the gradient of the features runs on.  It
    is built at the first backward pass that needs that gradient and kept; it is always built, whatever ``info.directed`` says: a
    symmetric structure does not make the types symmetric."""

    def __init__(self, info, edge_type, num_relations, norm="relation"):
        if norm not in ("relation", None):
            raise ValueError(f"norm must be 'relation' or None (got {norm!r})")
        ci = info.column_index
        if not getattr(ci, "is_cuda", False):
            raise ValueError("RelationalGraph lives on the device: move the graph's row_pointers, column_index and partition "
                             "to the GPU first")
        if getattr(info, "partPtr", None) is None or getattr(info, "part2Node", None) is None:
            raise ValueError("RelationalGraph needs the neighbor-group partition (partPtr, part2Node) of the graph")
        self.info = info
        self.num_relations = int(num_relations)
        if self.num_relations < 1:
            raise ValueError("num_relations must be >= 1")
        edge_type = torch.as_tensor(edge_type)
        if edge_type.dim() != 1 or edge_type.numel() != ci.numel():
            raise ValueError(f"edge_type must have one entry per edge ({ci.numel()}; got {tuple(edge_type.shape)})")
        self.edge_type = edge_type.to(device=ci.device, dtype=torch.int32).contiguous()
        self.is_block = hasattr(info, "num_src") and hasattr(info, "num_dst")
        self.num_dst = int(info.num_dst) if self.is_block else int(info.row_pointers.numel()) - 1
        self.num_src = int(info.num_src) if self.is_block else self.num_dst
        self.norm = norm
        self.edge_norm = self._relation_norm() if norm == "relation" else None
        self._transposed = None

    @classmethod
    def for_block(cls, block, edge_type_full, num_relations, norm="relation"):
        """The relational view of a sampled block: its edges take their types from the full graph's, through ``edge_ids``."""
        if getattr(block, "edge_ids", None) is None:
            raise ValueError("the block has no edge_ids: sample it with want_edge_ids=True")
        full = torch.as_tensor(edge_type_full).to(block.edge_ids.device)
        return cls(block, full.index_select(0, block.edge_ids.long()), num_relations, norm)

    def _rows(self):
        rp = self.info.row_pointers.to(self.edge_type.device).long()
        return torch.repeat_interleave(torch.arange(rp.numel() - 1, dtype=torch.int64, device=rp.device), rp[1:] - rp[:-1])

    def _relation_norm(self):
        if self.edge_type.numel() == 0:
            return torch.empty(0, dtype=torch.float32, device=self.edge_type.device)
        # an edge whose type is outside [0, num_relations) is skipped by the kernels: it is in nobody's count (one bucket of its
        # own behind all rows; its own factor is never read)
        t = self.edge_type.long()
        valid = (t >= 0) & (t < self.num_relations)
        key = torch.where(valid, self._rows() * self.num_relations + t, torch.full_like(t, self.num_dst * self.num_relations))
        _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        return (1.0 / counts.float()).index_select(0, inverse).contiguous()

    @property
    def partSize(self):
        return int(self.info.partSize)

    def transposed(self):
        """The transposed structure with its permuted edge arrays (built once; synchronises; not inside a stream capture)."""
        if self._transposed is None:
            t = self.info.transposed()
            self._transposed = _TypedTranspose(t, t.perm, self.edge_type, self.edge_norm)
        return self._transposed

    # ---- the three passes ---------------------------------------------------------------------------------------------------
    def expand(self, X, coef):
        g = self.info
        return _lib.agg_typed_expand(X, coef, g.column_index, self.edge_type, self.edge_norm, g.partPtr, g.part2Node,
                                     self.num_dst, g.partSize)

    def contract(self, G, coef):
        t = self.transposed()
        g = t.graph
        return _lib.agg_typed_contract(G, coef, g.column_index, t.edge_type, t.edge_norm, g.partPtr, g.part2Node,
                                       self.num_src, g.partSize)

    def coef_grad(self, X, G):
        g = self.info
        return _lib.typed_coef_grad(X, G, g.column_index, self.edge_type, self.edge_norm, g.partPtr, g.part2Node,
                                    self.num_relations, g.partSize)

"""Batches of graphs for graph-level tasks: many small graphs as ONE block-diagonal CSR, which every kernel of the library takes
as it stands, plus ``graph_pointers`` (int32 [G + 1]: the rows of graph g are [graph_pointers[g], graph_pointers[g + 1])), which
the readout (ops.Readout, ops.global_*_pool; libgnna gnna_segment_pool_ld_f32) reduces over.

* ``GraphBatch`` -- one batch.  It carries the attributes a layer reads from a graph bundle (``row_pointers column_index degrees
  partPtr part2Node partSize dimWorker warpPerBlock directed``, ``set_input() / set_hidden()``) and is a
  ``structure.GraphStructure``, so every layer takes it where it takes a ``decider.inputProperty``.
* ``GraphBatch.from_graphs`` collates a list of ``graph.CSRGraph`` on the host.
* ``GraphDataset`` keeps many graphs as one concatenated CSR on the device; ``GraphDataset.batch(ids)`` cuts the batch of the chosen
  graphs out of it with torch arithmetic on the device (one read-back: the batch's sizes).

A batch is never renumbered: a renumbering would scatter the rows of a graph, and the readout needs them contiguous.
"""
from __future__ import annotations

import torch

from . import _lib
from .decider import WAVES_PER_BLOCK, lanes_per_row
from .graph import degrees_from_rowptr
from .structure import GraphStructure


class TopKSelection(object):
    """What ``GraphBatch.coarsen`` kept: ``perm`` int32 [N'] (the old row of every new row, increasing), ``new_id`` int32 [N] (the
    new row of a kept row, -1 otherwise), ``edge_ids`` int32 [nnz'] or None (the old position of every surviving edge) and
    ``num_nodes`` (the old N)."""

    def __init__(self, perm, new_id, edge_ids, num_nodes):
        self.perm, self.new_id, self.edge_ids, self.num_nodes = perm, new_id, edge_ids, int(num_nodes)


class GraphBatch(GraphStructure):
    """A block-diagonal CSR of ``num_graphs`` graphs and ``graph_pointers``.  ``batch`` (int64 [N]: the graph of every row) and
    ``inv_counts`` (float32 [G]: 1 / max(rows of the graph, 1)) are built at their first use; the fused readout needs neither."""

    def __init__(self, row_pointers, column_index, graph_pointers, degrees=None, partSize=32, dimWorker=None, warpPerBlock=None,
                 hiddenDim=64, directed=False, x=None, y=None, edge_attr=None, partPtr=None, part2Node=None):
        for name, t in (("row_pointers", row_pointers), ("column_index", column_index), ("graph_pointers", graph_pointers)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
                raise TypeError(f"{name} must be a 1-D int32 tensor")
        if graph_pointers.numel() < 1:
            raise ValueError("graph_pointers must be [num_graphs + 1]")
        self.row_pointers, self.column_index = row_pointers.contiguous(), column_index.contiguous()
        self.graph_pointers = graph_pointers.contiguous()
        self.num_graphs = int(graph_pointers.numel()) - 1
        self.num_nodes = int(row_pointers.numel()) - 1
        self.degrees = degrees_from_rowptr(self.row_pointers) if degrees is None else degrees
        self.partSize = int(partSize)
        self.dimWorker = int(dimWorker) if dimWorker is not None else lanes_per_row(int(hiddenDim))
        self.warpPerBlock = int(warpPerBlock) if warpPerBlock is not None else WAVES_PER_BLOCK
        self.directed = bool(directed)
        self.x, self.y = x, y
        if edge_attr is not None and (edge_attr.dim() != 2 or edge_attr.shape[0] != column_index.numel()):
            raise ValueError(f"edge_attr must be [nnz = {column_index.numel()}, K] in the order of column_index "
                             f"(got {tuple(edge_attr.shape)})")
        self.edge_attr = edge_attr                                 # [nnz, K] or None: one row per position of column_index
        if (partPtr is None) != (part2Node is None):
            raise ValueError("partPtr and part2Node come together")
        if partPtr is not None:                                    # the partition of these row pointers at partSize, already built
            self.partPtr, self.part2Node = partPtr, part2Node
        elif self.row_pointers.is_cuda:
            self.partPtr, self.part2Node = _lib.build_part_device(self.partSize, self.row_pointers)
        else:
            self.partPtr, self.part2Node = _lib.build_part(self.partSize, self.row_pointers)
        self._batch = self._inv_counts = None

    # ---- what a layer reads from a graph bundle beyond the arrays -------------------------------------------------------------
    def set_input(self):
        """The layers of a batch share one set of launch knobs (the library's kernels derive their lane layout from the width)."""
        return self

    def set_hidden(self):
        return self

    # ---- the batch ------------------------------------------------------------------------------------------------------------
    @property
    def batch(self):
        """int64 [N]: the graph of every row -- what the torch composition of a readout indexes by."""
        if self._batch is None:
            gp = self.graph_pointers.long()
            ids = torch.arange(self.num_graphs, device=gp.device)
            self._batch = torch.repeat_interleave(ids, gp[1:] - gp[:-1])
        return self._batch

    @property
    def inv_counts(self):
        """float32 [G]: 1 / max(rows of the graph, 1)."""
        if self._inv_counts is None:
            gp = self.graph_pointers.long()
            self._inv_counts = 1.0 / (gp[1:] - gp[:-1]).clamp(min=1).float()
        return self._inv_counts

    def coarsen(self, score, ratio=None, k=None, want_edge_ids=False):
        """``(GraphBatch, selection)``: every graph keeps its min(n, ceil(ratio * n)) -- or min(n, k) -- rows with the largest
        `score` (float32 [N] on the batch's device; its values decide, no gradient flows through the choice), and the induced
        sub-batch is cut out on the device in ONE call (libgnna gnna_segment_topk_i32: rows, graph_pointers, CSR and partition; one
        read-back).  The kept rows stay in row order, so the rows of a graph stay contiguous.  The new batch carries `directed`,
        `partSize` and the launch knobs of this one, its degrees come from the new row pointers, and `x` / `y` are not moved: gather
        the rows with ops.SelectRows.  `selection` is a TopKSelection: perm [N'] (the old row of every new row), new_id [N] (-1 for
        a dropped row), edge_ids [nnz'] (the old position of every edge; None unless asked for) and num_nodes (the old N)."""
        if not self.row_pointers.is_cuda:
            raise _lib.GnnaError("GraphBatch.coarsen needs a batch on the device: there is no CPU path in libgnna")
        if (ratio is None) == (k is None):
            raise ValueError("coarsen takes exactly one of ratio and k")
        score = score.detach().reshape(-1)
        if score.dtype != torch.float32 or score.numel() != self.num_nodes or score.device != self.row_pointers.device:
            raise TypeError(f"score must be float32 [{self.num_nodes}] on {self.row_pointers.device}")
        r = _lib.segment_topk(score.contiguous(), self.graph_pointers, ratio=ratio, k=k, row_pointers=self.row_pointers,
                              column_index=self.column_index, partSize=self.partSize, want_edge_ids=want_edge_ids)
        small = GraphBatch(r["row_pointers"], r["column_index"], r["graph_pointers"], partSize=self.partSize, dimWorker=self.dimWorker,
                           warpPerBlock=self.warpPerBlock, directed=self.directed, partPtr=r["partPtr"], part2Node=r["part2Node"])
        return small, TopKSelection(r["perm"], r["new_id"], r["edge_ids"], self.num_nodes)

    def carry_edge_attr(self, small, selection):
        """Gives the coarsened batch `small` the edge_attr rows of its surviving edges (``coarsen(..., want_edge_ids=True)``);
        nothing when this batch has none.  -> small."""
        small.edge_attr = None if self.edge_attr is None else self.edge_attr[selection.edge_ids.long()]
        return small

    def to(self, device):
        move = lambda t: None if t is None else t.to(device)                                       # noqa: E731
        return GraphBatch(self.row_pointers.to(device), self.column_index.to(device), self.graph_pointers.to(device),
                          self.degrees.to(device), self.partSize, self.dimWorker, self.warpPerBlock, directed=self.directed,
                          x=move(self.x), y=move(self.y), edge_attr=move(self.edge_attr))

    @staticmethod
    def from_graphs(graphs, partSize=32, x=None, y=None, edge_attr=None, **kw):
        """Collates a list of ``graph.CSRGraph`` (or of (row_pointers, column_index) pairs) on the host: the rows and the column
        ids of graph g are shifted by the rows before it.  A graph without nodes is an empty segment.  Refuses row pointers that
        do not ascend.  `edge_attr` [nnz, K]: the edge rows of the graphs one after the other, which is the batch's edge order."""
        rps, cis, sizes = [], [], []
        for k, g in enumerate(graphs):
            rp, ci = (g.row_pointers, g.column_index) if hasattr(g, "row_pointers") else g
            rp, ci = torch.as_tensor(rp).cpu().long().reshape(-1), torch.as_tensor(ci).cpu().long().reshape(-1)
            if rp.numel() < 1 or int(rp[0]) != 0 or bool((rp[1:] < rp[:-1]).any()) or int(rp[-1]) != ci.numel():
                raise ValueError(f"graph {k}: row_pointers must start at 0, ascend and end at the number of edges "
                                 f"({ci.numel()})")
            n = rp.numel() - 1
            if ci.numel() and (int(ci.min()) < 0 or int(ci.max()) >= n):
                raise ValueError(f"graph {k}: a column id lies outside its {n} nodes")
            rps.append(rp)
            cis.append(ci)
            sizes.append(n)
        gp = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        if sizes:
            gp[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
        row_pointers, column_index, edges = [torch.zeros(1, dtype=torch.int64)], [], 0
        for k, (rp, ci) in enumerate(zip(rps, cis)):
            row_pointers.append(rp[1:] + edges)
            column_index.append(ci + gp[k])
            edges += ci.numel()
        if int(gp[-1]) >= 2 ** 31 or edges >= 2 ** 31:
            raise ValueError("a batch holds fewer than 2^31 nodes and edges (int32 CSR)")
        column_index = torch.cat(column_index) if column_index else torch.zeros(0, dtype=torch.int64)
        return GraphBatch(torch.cat(row_pointers).to(torch.int32), column_index.to(torch.int32), gp.to(torch.int32),
                          partSize=partSize, x=x, y=y, edge_attr=edge_attr, **kw)


class GraphDataset(object):
    """Many graphs as one concatenated CSR on a device: ``row_pointers`` [N + 1] and ``column_index`` with ids LOCAL to their
    graph, ``graph_pointers`` [G + 1], node features ``x`` [N, F], one label ``y`` per graph and, optionally, edge features
    ``edge_attr`` [nnz, K] in the order of ``column_index``."""

    def __init__(self, row_pointers, column_index, graph_pointers, x=None, y=None, edge_attr=None):
        self.row_pointers, self.column_index, self.graph_pointers = row_pointers, column_index, graph_pointers
        self.x, self.y = x, y
        if edge_attr is not None and (edge_attr.dim() != 2 or edge_attr.shape[0] != column_index.numel()):
            raise ValueError(f"edge_attr must be [nnz = {column_index.numel()}, K] in the order of column_index "
                             f"(got {tuple(edge_attr.shape)})")
        self.edge_attr = edge_attr
        self.num_graphs = int(graph_pointers.numel()) - 1
        self.num_nodes = int(row_pointers.numel()) - 1

    @staticmethod
    def from_graphs(graphs, x=None, y=None, device="cpu", edge_attr=None):
        """From a list of ``graph.CSRGraph``: the arrays of ``GraphBatch.from_graphs`` with the column ids left local."""
        b = GraphBatch.from_graphs(graphs)
        local = b.column_index.long() - b.graph_pointers.long()[:-1][b.batch[b.edge_rows().long()]] if b.column_index.numel() \
            else b.column_index.long()
        move = lambda t: None if t is None else t.to(device)                                       # noqa: E731
        return GraphDataset(b.row_pointers.to(device), local.to(torch.int32).to(device), b.graph_pointers.to(device), move(x), move(y),
                            move(edge_attr))

    def __len__(self):
        return self.num_graphs

    def batch(self, graph_ids, partSize=32, **kw):
        """The ``GraphBatch`` of the graphs `graph_ids` (in that order; an id may repeat), cut out on the dataset's device: torch
        arithmetic for the row and edge ranges and the id offsets, libgnna for the partition.  One read-back: the batch's number
        of rows and edges."""
        dev = self.row_pointers.device
        ids = torch.as_tensor(graph_ids, dtype=torch.int64, device=dev).reshape(-1)
        gp, rp = self.graph_pointers.long(), self.row_pointers.long()
        first, sizes = gp[ids], gp[ids + 1] - gp[ids]
        new_gp = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=dev)
        new_gp[1:] = torch.cumsum(sizes, 0)
        e_first, e_sizes = rp[first], rp[first + sizes] - rp[first]
        new_ep = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=dev)
        new_ep[1:] = torch.cumsum(e_sizes, 0)
        n, e = (int(v) for v in torch.stack([new_gp[-1], new_ep[-1]]).tolist())          # the one read-back
        which = torch.repeat_interleave(torch.arange(ids.numel(), device=dev), sizes, output_size=n)
        rows = torch.arange(n, device=dev) - new_gp[which] + first[which]               # the dataset's row of every batch row
        new_rp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        new_rp[1:] = rp[rows + 1] - e_first[which] + new_ep[which]
        which_e = torch.repeat_interleave(torch.arange(ids.numel(), device=dev), e_sizes, output_size=e)
        edges = torch.arange(e, device=dev) - new_ep[which_e] + e_first[which_e]
        ci = self.column_index.long()[edges] + new_gp[which_e]
        x = None if self.x is None else self.x[rows]
        y = None if self.y is None else self.y[ids]
        b = GraphBatch(new_rp.to(torch.int32), ci.to(torch.int32), new_gp.to(torch.int32), partSize=partSize, x=x, y=y, **kw)
        b._batch = which
        if self.edge_attr is not None:
            b.edge_attr = self.edge_attr[edges]
        return b

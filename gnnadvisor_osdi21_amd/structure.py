"""What every graph bundle knows about its own structure, and the one rule by which a backward pass picks the structure it walks.

* ``GraphStructure`` -- the base of ``decider.inputProperty`` and ``batching.GraphBatch`` (so of ``sampling.Subgraph``): the
  per-``column_index`` cache and what is built into it (the reverse-edge map, the symmetry answer, the transposed structure, the
  destination row of every edge, the row factors of a mean).  Its functions also serve as unbound calls on any object that has
  ``row_pointers`` and ``column_index`` (``GraphStructure.require_symmetric(bundle)``).
* ``Transpose`` -- A^T of a CSR with its neighbor-group partition and the lazy ``perm``; ``TransposedGraph`` (a graph's) and
  ``sampling._BlockTranspose`` (a sampled block's) derive from it.
* ``backward_structure`` -- the rule.  Every autograd Function of ``ops`` and ``edgeconv`` asks it, and so does the driver's
  warm-up before the first epoch.

This module imports neither ``decider`` nor ``sampling``: they import it.
"""
from __future__ import annotations


class Transpose(object):
    """A^T of a CSR, built on the device, with its neighbor-group partition at ``partSize``.  It has the attributes a kernel reads
    from a graph bundle: ``row_pointers column_index partPtr part2Node partSize``.  ``perm`` (int32 [nnz]: position in the forward
    column_index of every transposed edge) costs another nnz x 4 bytes and is built at its first use, which only the operators
    with per-edge operands make.  `source`: the forward (row_pointers, column_index), what perm is built from."""

    def __init__(self, row_pointers, column_index, partSize, source, perm=None):
        from . import _lib
        self._source = source
        self.row_pointers, self.column_index = row_pointers, column_index
        self.partSize = int(partSize)
        self.partPtr, self.part2Node = _lib.build_part_device(self.partSize, row_pointers)
        self._perm = perm

    @property
    def perm(self):
        if self._perm is None:
            from . import _lib
            # (the builder gives the same bits on every run: this second pass orders the edges exactly as the first did)
            perm = _lib.transpose_csr(*self._source, num_in_rows=self.row_pointers.numel() - 1)[2]
            # edges dropped for an id outside the graph sit behind every row and are read by nobody; as an index they must
            # still be one
            self._perm = perm.clamp_(min=0)
        return self._perm


class TransposedGraph(Transpose):
    """The structure a backward pass on a directed graph runs on (``GraphStructure.transposed()``): the ``Transpose`` of the graph
    at the same ``partSize`` plus the forward graph's ``degrees`` (the same vector: D A^T D scales rows and columns alike), so every
    kernel runs the backward pass on it unchanged."""

    def __init__(self, row_pointers, column_index, owner, partSize, source, perm=None):
        super().__init__(row_pointers, column_index, partSize, source, perm)
        self._owner = owner                           # the forward profile: `degrees` is its vector, whatever it is set to

    @property
    def degrees(self):
        return self._owner.degrees


class GraphStructure(object):
    """The structure methods of a graph bundle with ``row_pointers`` and ``column_index`` (``transposed()`` also reads
    ``partSize``, ``backward_graph()`` ``directed``)."""

    # ------------------------------------------------------------------ per-edge arrays (edge-valued aggregation, GAT)
    def _edge_arrays(self):
        """The cache of reverse_edges / edge_rows, emptied when `column_index` is another object than the one it was built
        from (a renumbered CSR)."""
        cache = getattr(self, "_edge_cache", None)
        if cache is None or cache["column_index"] is not self.column_index:
            cache = self._edge_cache = {"column_index": self.column_index}
        return cache

    def reverse_edges(self):
        """int32 [nnz] on the graph's device: rev[e] = position of the edge col(e) -> row(e) matching e (libgnna,
        gnna_reverse_edges_i32; built once per column_index).  Raises when the graph's structure is not symmetric."""
        cache = GraphStructure._edge_arrays(self)
        if "rev" not in cache:
            from . import _lib
            cache["rev"] = _lib.reverse_edges(self.row_pointers, self.column_index).to(self.column_index.device)
        return cache["rev"]

    def require_symmetric(self):
        """Raises unless the graph's structure is symmetric (every edge i <- j has its j <- i); the answer is kept per
        column_index.  Checked on the host by gnna_reverse_edges_i32 (a copy of the CSR to the host and one pass over it: about
        a second at 1e8 edges); the map it builds there is dropped -- nothing of the size of the edge list stays on the device
        (reverse_edges() keeps such a map, and a graph that has one is known to be symmetric).  Works on any graph bundle with
        row_pointers and column_index (``GraphStructure.require_symmetric(bundle)``)."""
        cache = GraphStructure._edge_arrays(self)
        if "rev" not in cache and "symmetric" not in cache:
            from . import _lib
            _lib.reverse_edges(self.row_pointers, self.column_index)
            cache["symmetric"] = True

    def transposed(self):
        """The ``TransposedGraph`` of this graph -- what the backward passes use when ``directed`` is true.  Built on the device
        (libgnna gnna_transpose_csr_i32 + gnna_build_part_device_i32: nothing is copied to the host), once per column_index and
        ``partSize``; the graph hints of ``apply_tuning`` are registered for the transposed ids too.  The builders synchronise
        and cannot run inside a stream capture: call this once before capturing a training step."""
        cache = GraphStructure._edge_arrays(self)
        t = cache.get("transposed")
        if t is None or t.partSize != int(self.partSize):
            from . import _lib
            ci = self.column_index
            if not getattr(ci, "is_cuda", False):
                raise ValueError("transposed() is built on the device: move row_pointers and column_index to the GPU first")
            rp = self.row_pointers.to(ci.device)
            if t is None:
                t_rp, t_ci, _ = _lib.transpose_csr(rp, ci, want_perm=False)
                t = TransposedGraph(t_rp, t_ci, self, self.partSize, (rp, ci))
                hints = getattr(self, "_graph_hints", None)           # what apply_tuning registered for the forward ids
                if hints is not None:
                    _lib.set_graph_hints(t_ci, *hints)
            else:                                                      # another partSize: only the partition changes
                t = TransposedGraph(t.row_pointers, t.column_index, self, self.partSize, (rp, ci), perm=t._perm)
            cache["transposed"] = t
        return t

    def backward_graph(self):
        """The graph bundle a backward pass runs on: ``transposed()`` when ``directed``, else this graph itself."""
        return backward_structure(self)

    def edge_rows(self):
        """int32 [nnz] on the graph's device: the destination row of every edge (built once per column_index)."""
        cache = GraphStructure._edge_arrays(self)
        if "rows" not in cache:
            import torch
            rp = self.row_pointers.to(self.column_index.device).long()
            n = rp.numel() - 1
            cache["rows"] = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=rp.device), rp[1:] - rp[:-1])
        return cache["rows"]

    def inv_row_counts(self):
        """float32 [num_nodes] on the graph's device: 1 / max(edges of the row, 1), from row_pointers (`degrees` holds square
        roots).  The row factor of a neighbor mean; a row without edges keeps the factor 1.  Built once per column_index."""
        cache = GraphStructure._edge_arrays(self)
        if "inv_counts" not in cache:
            rp = self.row_pointers.to(self.column_index.device).long()
            cache["inv_counts"] = 1.0 / (rp[1:] - rp[:-1]).clamp(min=1).float()
        return cache["inv_counts"]


def backward_structure(info, *, require_symmetric=False, edge_pos=False):
    """The structure the backward pass of an operator over the graph bundle `info` walks -- a bundle with ``row_pointers
    column_index partPtr part2Node partSize`` (and ``degrees`` where `info` has them) -- or, with ``edge_pos=True``, the pair
    (bundle, int32 [nnz] map from every edge position of the bundle to the position of the same edge in ``info.column_index``:
    where the backward finds a per-edge operand of the forward).

    A sum over the edges i <- j sends row i's gradient to row j, i.e. it aggregates over A^T:

    * ``info.directed`` true (a ``sampling.SampledBlock`` is, by class): ``info.transposed()``, built on the device at its first
      use and kept; the map is its ``perm``, built only when asked for.  Nothing is assumed, nothing is checked.
    * otherwise `info` itself: the structure is taken to be symmetric (the reference's assumption).  ``require_symmetric=True``
      establishes it first (``GraphStructure.require_symmetric``: once per column_index, raises on a structure that is not) --
      for the operators whose backward would be silently wrong, not merely transposed, on another structure.  The map is the
      reverse-edge map, which raises likewise.

    Nothing is built by a call that does not need it, so an operator calls this inside its backward, behind its own
    ``needs_input_grad`` test."""
    if getattr(info, "directed", False):
        t = info.transposed()
        return (t, t.perm) if edge_pos else t
    if require_symmetric:
        GraphStructure.require_symmetric(info)
    return (info, GraphStructure.reverse_edges(info)) if edge_pos else info

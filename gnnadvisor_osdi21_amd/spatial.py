"""Graphs from coordinates: the radius graph and the k-nearest-neighbour graph of every point set of a batch, built on the device
(libgnna ``gnna_radius_graph_f32``; the rule is spelled out in ``include/gnna_spatial.h``), and the SchNet pieces that read them.

* ``radius_graph(pos, r, graph_pointers, ...)`` / ``knn_graph(pos, k, graph_pointers, ...)`` -> ``batching.GraphBatch`` with
  ``edge_dist2`` (float32 [nnz]: the squared length of every edge, in the order of ``column_index``).  Without a cap the structure is
  symmetric (``directed=False``); with one it is in general not, and the batch says ``directed=True`` so that every backward pass
  walks the transposed structure.  ``fused=False`` composes the same rule from torch ops on a padded ``[G, n_max, n_max]`` distance
  tensor -- the timing baseline and a second opinion, bit for bit the same edges.
* ``GaussianSmearing``, ``CosineCutoff``: plain torch modules on the edge lengths ``sqrt(edge_dist2)``.
* ``SchNetInteraction``: the filter network ``Linear -> shifted softplus -> Linear`` over the Gaussian expansion, times the cosine
  cutoff, then ``edgeconv.CFConv`` and the output MLP with the residual.

No gradient flows into ``pos``: a user who needs forces differentiates ``pos[column_index] - pos[row]`` in torch.
"""
from __future__ import annotations

import math

import torch
from torch.nn import Linear, Module

from . import _lib
from .batching import GraphBatch
from .edgeconv import CFConv


def composed_radius_graph(pos, graph_pointers, radius, max_neighbors=None, loop=False):
    """The rule of include/gnna_spatial.h from torch ops, on any device: the squares are accumulated column by column with an
    explicit ``+`` (one rounding per operation, as the kernel's), the cap takes the smallest 64-bit keys (d2 bits, row id).
    -> (row_pointers int32 [N + 1], column_index int32 [nnz], dist2 float32 [nnz]).  Memory is G * n_max^2 elements."""
    pos = pos.detach()
    n, dim = pos.shape
    dev = pos.device
    gp = graph_pointers.to(dev).long().clamp(0, n)
    sizes = gp[1:] - gp[:-1]
    if bool((sizes < 0).any()):
        raise ValueError(f"graph_pointers decreases at segment {int(torch.nonzero(sizes < 0)[0])}")
    G = sizes.numel()
    n_max = int(sizes.max()) if G else 0
    if n == 0 or n_max == 0:
        return (torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev))
    local = torch.arange(n_max, device=dev)
    rows = gp[:-1, None] + local[None, :]                               # [G, n_max]: the global row of every padded slot
    valid = local[None, :] < sizes[:, None]
    P = pos[rows.clamp(max=n - 1)]                                      # [G, n_max, dim] (slots beyond a set hold some row: masked)
    d2 = None
    for c in range(dim):
        diff = P[:, None, :, c] - P[:, :, None, c]                      # [g, i, j] = pos[j, c] - pos[i, c]
        sq = diff * diff
        d2 = sq if d2 is None else d2 + sq
    r = torch.tensor(float(radius), dtype=torch.float32, device=dev)
    keep = (d2 <= r * r) & valid[:, :, None] & valid[:, None, :]
    if not loop:
        keep &= ~torch.eye(n_max, dtype=torch.bool, device=dev)[None]
    if max_neighbors is not None and n_max > int(max_neighbors):
        key = (d2.contiguous().view(torch.int32).long() << 32) | rows[:, None, :]
        key = torch.where(keep, key, torch.full_like(key, torch.iinfo(torch.int64).max))
        best = torch.topk(key, int(max_neighbors), dim=-1, largest=False).indices
        chosen = torch.zeros_like(keep).scatter_(-1, best, True)
        keep &= chosen
    g, i, j = torch.nonzero(keep, as_tuple=True)                        # lexicographic: rows in order, j increasing
    counts = torch.bincount(rows[g, i], minlength=n)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rp[1:] = torch.cumsum(counts, 0)
    return rp.to(torch.int32), rows[g, j].to(torch.int32), d2[g, i, j]


def radius_graph(pos, r, graph_pointers, loop=False, max_num_neighbors=None, partSize=32, fused=True, **kw) -> GraphBatch:
    """The ``GraphBatch`` that joins every row of `pos` (float32 [N, dim]) to the rows of its own point set -- the rows
    [graph_pointers[g], graph_pointers[g + 1]) -- within distance `r` (a point exactly at the cutoff is a neighbour; itself only
    with ``loop=True``), `max_num_neighbors` (1 .. 64) keeping the nearest, ties to the smaller row.  It carries ``edge_dist2``.
    ``directed`` is False without a cap and True with one.  fused=True builds it with one library call on the device, fused=False
    composes it from torch ops (any device).  **kw goes to GraphBatch (x, y, hiddenDim, ...)."""
    if max_num_neighbors is not None and not 1 <= int(max_num_neighbors) <= _lib.SPATIAL_MAX_NEIGHBORS:
        raise _lib.GnnaError(f"max_neighbors must be in [1, {_lib.SPATIAL_MAX_NEIGHBORS}] or None (got {max_num_neighbors})")
    if not float(r) >= 0.0:
        raise _lib.GnnaError(f"radius must be >= 0 or inf (got {r})")
    directed = max_num_neighbors is not None
    if fused:
        res = _lib.radius_graph(pos.detach(), graph_pointers, r, max_num_neighbors, loop, partSize=partSize)
        batch = GraphBatch(res["row_pointers"], res["column_index"], graph_pointers, partSize=partSize, directed=directed,
                           partPtr=res["partPtr"], part2Node=res["part2Node"], **kw)
        batch.edge_dist2 = res["dist2"]
        return batch
    rp, ci, d2 = composed_radius_graph(pos, graph_pointers, r, max_num_neighbors, loop)
    batch = GraphBatch(rp, ci, graph_pointers.to(rp.device), partSize=partSize, directed=directed, **kw)
    batch.edge_dist2 = d2
    return batch


def knn_graph(pos, k, graph_pointers, loop=False, partSize=32, fused=True, **kw) -> GraphBatch:
    """``radius_graph`` with r = inf and a cap of `k`: every row's k nearest rows of its own set (all of them in a smaller set)."""
    return radius_graph(pos, math.inf, graph_pointers, loop=loop, max_num_neighbors=int(k), partSize=partSize, fused=fused, **kw)


class GaussianSmearing(Module):
    """``GaussianSmearing(start, stop, num_gaussians)(d)``: d [E] -> exp(-0.5 / delta^2 * (d - mu_k)^2) [E, num_gaussians] with
    `num_gaussians` centres mu_k evenly from `start` to `stop` and delta their spacing (SchNet's distance expansion)."""

    def __init__(self, start=0.0, stop=5.0, num_gaussians=32):
        super().__init__()
        if not isinstance(num_gaussians, int) or num_gaussians < 2:
            raise ValueError(f"GaussianSmearing: num_gaussians must be an integer >= 2 (got {num_gaussians!r})")
        offset = torch.linspace(float(start), float(stop), num_gaussians)
        self.coeff = -0.5 / float(offset[1] - offset[0]) ** 2
        self.register_buffer("offset", offset)

    def forward(self, d):
        diff = d.reshape(-1, 1) - self.offset.to(d.dtype).reshape(1, -1)
        return torch.exp(self.coeff * diff * diff)


class CosineCutoff(Module):
    """``CosineCutoff(r)(d)``: 0.5 * (cos(pi * d / r) + 1) for d < r, else 0."""

    def __init__(self, cutoff):
        super().__init__()
        self.cutoff = float(cutoff)

    def forward(self, d):
        return 0.5 * (torch.cos(d * (math.pi / self.cutoff)) + 1.0) * (d < self.cutoff).to(d.dtype)


class ShiftedSoftplus(Module):
    """softplus(x) - log 2."""

    def forward(self, x):
        return torch.nn.functional.softplus(x) - math.log(2.0)


class _SchNetFilter(Module):
    """d [E] -> (Linear -> shifted softplus -> Linear)(GaussianSmearing(d)) * CosineCutoff(d)[:, None]: what CFConv multiplies
    the source rows by."""

    def __init__(self, num_gaussians, num_filters, cutoff):
        super().__init__()
        self.smearing = GaussianSmearing(0.0, cutoff, num_gaussians)
        self.cutoff = CosineCutoff(cutoff)
        self.lin1, self.act, self.lin2 = Linear(num_gaussians, num_filters), ShiftedSoftplus(), Linear(num_filters, num_filters)

    def forward(self, d):
        return self.lin2(self.act(self.lin1(self.smearing(d)))) * self.cutoff(d).reshape(-1, 1)


class SchNetInteraction(Module):
    """``SchNetInteraction(hidden, num_filters, num_gaussians, cutoff, fused=True)(x, batch)``:

        x + lin(ssp(CFConv(x, batch, W)))        W_e = (Linear -> ssp -> Linear)(gauss(d_e)) * cos_cutoff(d_e),  d_e = sqrt(edge_dist2_e)

    `batch`: a GraphBatch of ``radius_graph`` / ``knn_graph`` (it carries ``edge_dist2``; or give ``edge_dist2=``).  The sum over
    the edges runs on edgeconv.CFConv (fused=True: libgnna's edge-feature gather, no [nnz, F] message tensor)."""

    def __init__(self, hidden, num_filters, num_gaussians, cutoff, fused=True):
        super().__init__()
        self.conv = CFConv(hidden, hidden, num_filters, _SchNetFilter(num_gaussians, num_filters, cutoff), fused=fused)
        self.act, self.lin = ShiftedSoftplus(), Linear(hidden, hidden)

    def forward(self, x, batch, edge_dist2=None):
        d2 = getattr(batch, "edge_dist2", None) if edge_dist2 is None else edge_dist2
        if d2 is None:
            raise ValueError("SchNetInteraction: the batch carries no edge_dist2 (build it with spatial.radius_graph) and none was given")
        return x + self.lin(self.act(self.conv(x, batch, torch.sqrt(d2))))

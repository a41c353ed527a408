"""Message passing with a feature vector per edge: the autograd op over libgnna's fused gather (include/gnna_edgefeat.h) and the two
layers everybody runs on molecular and material graphs.

* ``EdgeFeatureSum`` -- ``Y[i] = sum over the edges e = (i <- j) of act(X[j] (+ | *) E[e])`` with E [nnz, F], one row per position of
  ``column_index``.  One gather forward; backward one pass on the destination side (dE) and one on the source side over A^T (dX).
* ``GINEConv`` -- GIN with edge features (Hu et al., "Strategies for Pre-training Graph Neural Networks"; PyG's GINEConv):
  ``nn((1 + eps) x_i + sum_j relu(x_j + e_ij))``.
* ``CFConv`` -- SchNet's continuous-filter convolution (Schuett et al.; PyG's schnet.CFConv without its cutoff envelope, which is
  a per-edge scalar the caller folds into the filter): ``lin2(sum_j lin1(x)_j * filter_nn(edge_attr)_e)``.

``fused=False`` composes the same functions from torch indexing and ``index_add_``, which makes several [nnz, F] tensors in each
direction: it is the yardstick for tests and timing.  No counterpart in the reference (its layers take no edge data).
"""
import torch
from torch.autograd import Function
from torch.nn import Linear, Module, Parameter

from . import _lib
from .ops import GNNA, _block_features, _is_block, _laid_out
from .structure import backward_structure

_COMBINE = {"add": _lib.EDGE_ADD, "mul": _lib.EDGE_MUL}
_ACT = {"none": _lib.EDGE_ACT_NONE, "relu": _lib.EDGE_ACT_RELU}


def _codes(combine, act, who):
    if combine not in _COMBINE:
        raise ValueError(f"{who}: combine must be 'add' or 'mul' (got {combine!r})")
    if act not in _ACT:
        raise ValueError(f"{who}: act must be 'none' or 'relu' (got {act!r})")
    return _COMBINE[combine], _ACT[act]


def _check_operands(X, E, info, who):
    if X.dtype != torch.float32 or E.dtype != torch.float32:
        raise TypeError(f"{who}: float32 only (got X {X.dtype} and E {E.dtype})")
    nnz = info.column_index.numel()
    if X.dim() != 2 or E.dim() != 2 or tuple(E.shape) != (nnz, X.shape[1]):
        raise ValueError(f"{who}: E must be [nnz = {nnz}, F = {X.shape[-1]}] in the order of column_index, X [rows, F] "
                         f"(got X {tuple(X.shape)} and E {tuple(E.shape)})")


class EdgeFeatureSum(Function):
    """``EdgeFeatureSum.apply(X, E, inputInfo, combine="add", act="none") -> Y`` (libgnna gnna_agg_edge_feat_ld_f32 /
    gnna_agg_edge_feat_backward_ld_f32):

        Y[i, f] = sum over the positions e of row i of act(X[column_index[e], f] (+ | *) E[e, f])

    E is [nnz, F] float32, edge-major in the order of ``inputInfo.column_index``; combine "add" | "mul", act "none" | "relu" (the
    mask is pre > 0, gradient 0 at 0).  A row without edges gives 0.  `inputInfo`: a decider.inputProperty, a batching.GraphBatch or
    a sampling.Subgraph, or a sampling.SampledBlock (X [num_src, F] -> Y [num_dst, F]; E rows are those of the block's own edges).

    Saved: X and E only -- the relu mask is recomputed in each backward pass, and nothing else of edge-list size is made but dE
    itself.  The source-side pass finds an edge's E row through a position map of nnz x 4 bytes, picked as ops.GATEdgeAttention
    picks it: the ``perm`` of ``inputInfo.transposed()`` on a ``directed`` graph or a block, ``reverse_edges()`` after
    ``require_symmetric`` otherwise.  Only the gradients that ``needs_input_grad`` names are computed, and no transposed structure
    is built when X needs none.  Strided X, E and dY are taken as they are where their rows are contiguous.  The same bits on
    every run.  float32 only."""

    @staticmethod
    def forward(ctx, X, E, inputInfo, combine="add", act="none"):
        info = inputInfo
        ctx.combine, ctx.act = _codes(combine, act, "EdgeFeatureSum")
        _check_operands(X, E, info, "EdgeFeatureSum")
        if _is_block(info):
            X = _block_features(X, info, "EdgeFeatureSum")
        else:
            X = _laid_out(X)
        E = _laid_out(E)
        ctx.info = info
        ctx.save_for_backward(X, E)
        return GNNA.aggregate_edge_feat(X, E, info.row_pointers, info.column_index, ctx.combine, ctx.act)

    @staticmethod
    def backward(ctx, dY):
        X, E = ctx.saved_tensors
        info = ctx.info
        want_dx, want_de = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_dx or want_de):
            return None, None, None, None, None
        transposed = (None, None, None)
        if want_dx:
            t, edge_pos = backward_structure(info, require_symmetric=True, edge_pos=True)
            transposed = (t.row_pointers, t.column_index, edge_pos)
        dX, dE = GNNA.aggregate_edge_feat_backward(X, E, _laid_out(dY), info.row_pointers, info.column_index, *transposed,
                                                   ctx.combine, ctx.act, bool(want_dx), bool(want_de))
        return dX, dE, None, None, None


def composed_edge_feature_sum(X, E, info, combine="add", act="none"):
    """EdgeFeatureSum from torch ops, with [nnz, F] temporaries (X[column_index], the message, its mask) and an index_add_: the
    timing baseline and a second opinion.  Takes what EdgeFeatureSum takes."""
    _codes(combine, act, "composed_edge_feature_sum")
    rp, ci = info.row_pointers.long(), info.column_index.long()
    n = rp.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n, device=X.device), rp[1:] - rp[:-1], output_size=ci.numel())
    xj = X.index_select(0, ci)
    msg = xj + E if combine == "add" else xj * E
    if act == "relu":
        msg = torch.relu(msg)
    return torch.zeros((n, X.shape[1]), dtype=X.dtype, device=X.device).index_add_(0, dst, msg)


def _edge_sum(X, E, info, combine, act, fused):
    if fused:
        return EdgeFeatureSum.apply(X, E, info, combine, act)
    return composed_edge_feature_sum(X, E, info, combine, act)


def _dst_rows(x, info):
    """The rows of `x` that are destinations: all of them, or the first num_dst of a block's sources."""
    return x[:info.num_dst] if _is_block(info) else x


class GINEConv(Module):
    """``GINEConv(nn, eps=0.0, train_eps=False, edge_dim=None, fused=True)(x, info, edge_attr)``:

        nn((1 + eps) * x_i + sum over the edges i <- j of relu(x_j + e_ij))

    `nn`: any module [rows, F] -> [rows, F'].  `edge_attr` is [nnz, F] in the order of ``info.column_index``; with `edge_dim` it is
    [nnz, edge_dim] and a ``Linear(edge_dim, in_channels)`` maps it first, as PyG does -- `in_channels` is then read from the first
    Linear inside `nn` (or give ``in_channels=``).  eps is a Parameter when `train_eps`.  fused=True runs the sum on EdgeFeatureSum,
    fused=False composes it from torch ops."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None, fused=True, in_channels=None):
        super().__init__()
        if not isinstance(nn, Module):
            raise TypeError(f"GINEConv: nn must be a torch.nn.Module (got {type(nn).__name__})")
        self.nn, self.fused = nn, bool(fused)
        if train_eps:
            self.eps = Parameter(torch.tensor(float(eps)))
        else:
            self.register_buffer("eps", torch.tensor(float(eps)))
        self.lin_edge = None
        if edge_dim is not None:
            if not isinstance(edge_dim, int) or edge_dim < 1:
                raise ValueError(f"GINEConv: edge_dim must be a positive integer (got {edge_dim!r})")
            if in_channels is None:
                first = next((m for m in nn.modules() if isinstance(m, Linear)), None)
                if first is None:
                    raise ValueError("GINEConv: edge_dim needs the input width: nn has no Linear to read it from, give in_channels=")
                in_channels = first.in_features
            self.lin_edge = Linear(edge_dim, int(in_channels))

    def forward(self, x, info, edge_attr):
        if edge_attr is None:
            raise ValueError("GINEConv: edge_attr is required ([nnz, F], or [nnz, edge_dim] with edge_dim)")
        e = self.lin_edge(edge_attr) if self.lin_edge is not None else edge_attr
        agg = _edge_sum(x, e, info, "add", "relu", self.fused)
        return self.nn((1.0 + self.eps) * _dst_rows(x, info) + agg)


class CFConv(Module):
    """``CFConv(in_channels, out_channels, num_filters, filter_nn, fused=True)(x, info, edge_attr)``:

        lin2(sum over the edges i <- j of lin1(x)_j * filter_nn(edge_attr)_e)

    lin1: Linear(in_channels, num_filters, bias=False); lin2: Linear(num_filters, out_channels); `filter_nn`: any module
    [nnz, K] -> [nnz, num_filters] (SchNet: a two-layer MLP over the distance expansion).  fused as in GINEConv."""

    def __init__(self, in_channels, out_channels, num_filters, filter_nn, fused=True):
        super().__init__()
        for name, v in (("in_channels", in_channels), ("out_channels", out_channels), ("num_filters", num_filters)):
            if not isinstance(v, int) or v < 1:
                raise ValueError(f"CFConv: {name} must be a positive integer (got {v!r})")
        if not isinstance(filter_nn, Module):
            raise TypeError(f"CFConv: filter_nn must be a torch.nn.Module (got {type(filter_nn).__name__})")
        self.lin1 = Linear(in_channels, num_filters, bias=False)
        self.lin2 = Linear(num_filters, out_channels)
        self.filter_nn, self.fused = filter_nn, bool(fused)

    def forward(self, x, info, edge_attr):
        w = self.filter_nn(edge_attr)
        return self.lin2(_edge_sum(self.lin1(x), w, info, "mul", "none", self.fused))

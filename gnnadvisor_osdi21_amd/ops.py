"""Operator layer over the ``GNNAdvisor`` extension: autograd functions and the GCN / GIN
convolution modules.

API counterpart of the reference's GNNAdvisor/gnn_conv.py -- the names and call
signatures its driver uses are kept (``ScatterAndGather`` :7-27, ``GNNAFunction`` :30-78,
``GCNConv`` :80-98, ``GNNAFunction_GIN`` :101-126, ``GINConv`` :128-147; weights drawn from
U(-1/sqrt(out), 1/sqrt(out)) :86-88; GIN epsilon fixed at 0.5 and spelled ``eplison``
:132) -- but the implementation is this package's own: every op unpacks the graph
bundle once through ``_graph_args`` and calls the HIP extension.  No fallback exists.
"""
import math

import torch
from torch.autograd import Function
from torch.nn import Module, Parameter

from . import _lib, load_extension
from .sampling import SampledBlock
from .structure import backward_structure

GNNA = load_extension()


def _graph_args(info):
    """(row_pointers, column_index, degrees, partPtr, part2Node) of a decider.inputProperty."""
    return (info.row_pointers, info.column_index, info.degrees, info.partPtr, info.part2Node)


def _knobs(info):
    return (info.partSize, info.dimWorker, info.warpPerBlock)


# ---- layouts: every float [n, W] operand and every incoming gradient passes one of these two before it reaches a binding ------
# autograd hands a backward whatever layout the graph downstream produced (the gradient of a sum() is an expanded scalar, that
# of a sum readout has stride(0) == 0, that of a column slice a leading dimension, a product keeps a column-major operand's
# layout), and forward operands vary the same way (``emb.expand(n, F)``, a column block, ``lin.weight.t()``).

def _laid_out(t):
    """`t` for a binding that takes a leading dimension: itself when its rows are contiguous and do not overlap (stride(1) == 1,
    stride(0) >= width: nothing is copied), a contiguous copy otherwise; None stays None."""
    if t is None or ((t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])):
        return t
    return t.contiguous()


def _packed(t):
    """`t` for a binding that takes contiguous tensors only (the reference-shaped entries: SAG, forward / backward and their GIN
    forms): itself when contiguous, a contiguous copy otherwise; None stays None."""
    return t if t is None else t.contiguous()


# ---- sampled blocks (sampling.SampledBlock): rectangular, [num_src, F] -> [num_dst, F] ------------------------------------
# The GraphSAGE operators take a block where they take an inputProperty.  Forward and backward go through the rectangular
# entries of libgnna (gnna_agg_ld_f32, gnna_agg_reduce_ld_f32, gnna_scatter_arg_ld_f32); the backward of a sum aggregates dY over
# the transposed block, which is only built when the layer's input needs a gradient (the first layer's does not).
# The fused attention (GATAttention, GATConv(fused=True)) takes a block too, through gnna_gat_forward_rect_f32 /
# gnna_gat_backward_rect_f32; its backward always runs on the transposed block (the gradient of the layer's own weight needs dH).
# Which structure a backward walks is structure.backward_structure's decision for every operator here, blocks included.

def _is_block(info):
    return isinstance(info, SampledBlock)


def _refuse_block(info, layer):
    if _is_block(info):
        raise TypeError(f"{layer} does not take a SampledBlock: blocks are supported by the GraphSAGE operators "
                        "(ScatterAndGather, NeighborMean, NeighborMax, NeighborMin, SAGEConv) and by the fused attention "
                        "(GATAttention, GATConv(fused=True))")


def _block_features(X, block, what):
    if X.dtype != torch.float32:
        raise TypeError(f"{what} on a SampledBlock: float32 features only (got {X.dtype})")
    if X.dim() != 2 or X.shape[0] != block.num_src:
        raise ValueError(f"{what} on a SampledBlock: X must be [num_src = {block.num_src}, F] (got {tuple(X.shape)})")
    return _laid_out(X)


def _block_sum(X, graph, num_out_rows):
    """Neighbor sum over a block or its transpose: X [rows gathered from, F] -> [num_out_rows, F]."""
    return _lib.agg_ld(_lib.MODE_SAG, X, graph.column_index, graph.partPtr, graph.part2Node, num_out_rows, graph.partSize)


def _sum_backward(ctx, dY):
    """A^T dY of a float32 neighbor sum over ``backward_structure(ctx.info)``; a block's through the rectangular entry, and not
    at all when its input needs no gradient (the first layer's: no transposed block is built for it)."""
    if ctx.block is None:
        return GNNA.SAG(_packed(dY), *_graph_args(backward_structure(ctx.info)), *ctx.knobs)
    if not ctx.needs_input_grad[0]:
        return None
    return _block_sum(_laid_out(dY), backward_structure(ctx.info), ctx.block.num_src)


# ---- features stored in bfloat16 / float16 (libgnna gnna_agg_ld_x16: fp32 accumulation, one rounding of the result) ------
_X16 = (torch.bfloat16, torch.float16)


def _x16_dtype(X):
    """The 16-bit dtype a layer computes in: X's own when the model was cast, the autocast dtype inside
    torch.autocast("cuda", dtype=bfloat16 / float16), else None (the fp32 path, unchanged)."""
    if X.dtype in _X16:
        return X.dtype
    if X.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in _X16:
        return torch.get_autocast_dtype("cuda")
    return None


def _aggregate_x16(mode, X, graph, partSize, epsilon=1.0, relu=False):
    """mode 0 sag / 1 gcn / 2 gin over 16-bit X -> the same dtype; the degrees stay fp32."""
    _rp, ci, deg, pp, p2n = graph
    return GNNA.aggregate_ld(mode, _laid_out(X), ci, deg if mode == 1 else None, float(epsilon), pp, p2n, partSize, None, False, bool(relu))


class GNNAFunction_X16(Function):
    """A GCN (mode 1) or GIN (mode 2) layer on 16-bit features, update-first -- Y = agg(X W), the GCN order -- or
    aggregate-first -- Y = agg(X) W.  Both aggregations (forward, and backward on the 16-bit gradient, over the transposed
    structure when the graph is ``directed``) run on gnna_agg_ld_x16 and return the compute dtype; the dense products
    (X W, G W^T, X^T G) are torch.mm on 16-bit operands.  X and the weights may be fp32 (torch.autocast) or 16-bit (a cast
    model): their gradients come back in their own dtype."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, X, weight, inputInfo, mode, epsilon, update_first, relu, dtype):
        ctx.info, ctx.partSize = inputInfo, inputInfo.partSize
        graph = _graph_args(inputInfo)
        ctx.mode, ctx.eps, ctx.update_first, ctx.relu, ctx.dtype = int(mode), float(epsilon), bool(update_first), bool(relu), dtype
        ctx.in_dtypes = (X.dtype, weight.dtype)
        Xh, Wh = X.to(dtype), weight.to(dtype)
        if ctx.update_first:
            Y = _aggregate_x16(ctx.mode, torch.mm(Xh, Wh), graph, ctx.partSize, ctx.eps, ctx.relu)
            ctx.save_for_backward(Xh, Wh, *((Y,) if ctx.relu else ()))
        else:
            T = _aggregate_x16(ctx.mode, Xh, graph, ctx.partSize, ctx.eps)
            Y = torch.mm(T, Wh)
            if ctx.relu:
                Y = torch.relu(Y)
            ctx.save_for_backward(T, Wh, *((Y,) if ctx.relu else ()))
        return Y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_output):
        saved, Wh = ctx.saved_tensors[0], ctx.saved_tensors[1]
        dY = d_output.to(ctx.dtype)
        if ctx.relu:
            dY = dY * (ctx.saved_tensors[2] > 0)
        d_input = None
        bgraph = _graph_args(backward_structure(ctx.info))
        if ctx.update_first:
            G = _aggregate_x16(ctx.mode, dY, bgraph, ctx.partSize, ctx.eps)
            d_weight = torch.mm(saved.t(), G)
            if ctx.needs_input_grad[0]:
                d_input = torch.mm(G, Wh.t())
        else:
            d_weight = torch.mm(saved.t(), dY)
            if ctx.needs_input_grad[0]:
                d_input = _aggregate_x16(ctx.mode, torch.mm(dY, Wh.t()), bgraph, ctx.partSize, ctx.eps)
        if d_input is not None:
            d_input = d_input.to(ctx.in_dtypes[0])
        return d_input, d_weight.to(ctx.in_dtypes[1]), None, None, None, None, None, None


class ScatterAndGather(Function):
    """Y = A X (unweighted neighbor sum).  Backward is A^T dY: the same op on the same graph when the structure is symmetric,
    on the transposed structure when ``inputInfo.directed``."""

    @staticmethod
    def forward(ctx, X, inputInfo):
        ctx.info, ctx.block = inputInfo, inputInfo if _is_block(inputInfo) else None
        if ctx.block is not None:
            return _block_sum(_block_features(X, inputInfo, "ScatterAndGather"), inputInfo, inputInfo.num_dst)
        ctx.knobs = _knobs(inputInfo)
        if X.dtype in _X16:
            return _aggregate_x16(0, X, _graph_args(inputInfo), ctx.knobs[0])
        return GNNA.SAG(_packed(X), *_graph_args(inputInfo), *ctx.knobs)

    @staticmethod
    def backward(ctx, d_output):
        if ctx.block is None and d_output.dtype in _X16:
            return _aggregate_x16(0, d_output, _graph_args(backward_structure(ctx.info)), ctx.knobs[0]), None
        return _sum_backward(ctx, d_output), None


class GNNAFunction(Function):
    """GCN layer: dense update X W, then degree-weighted aggregation (update -> aggregate)."""

    @staticmethod
    def forward(ctx, X, weight, inputInfo):
        X, weight = _packed(X), _packed(weight)
        ctx.save_for_backward(X, weight)
        ctx.info, ctx.knobs = inputInfo, _knobs(inputInfo)
        return GNNA.forward(X, weight, *_graph_args(inputInfo), *ctx.knobs)[0]

    @staticmethod
    def backward(ctx, d_output):
        X, weight = ctx.saved_tensors
        return _gcn_backward(ctx, d_output, X, weight)


def _gcn_backward(ctx, d_output, X, weight):
    """(d_input, d_weight, None) of a GCN layer from the gradient of its (pre-activation) output: D A^T D dY, then the two
    dense products.  Whatever layout the three arrive in (d_output may be a product that kept a column-major operand's)."""
    bgraph = _graph_args(backward_structure(ctx.info))
    d_output, X, weight = _packed(d_output), _packed(X), _packed(weight)
    if not ctx.needs_input_grad[0]:
        # first layer: the features need no gradient (the reference computes and drops d_input)
        return None, GNNA.backward_weight(d_output, X, *bgraph, *ctx.knobs)[0], None
    d_input, d_weight = GNNA.backward(d_output, X, weight, *bgraph, *ctx.knobs)
    return d_input, d_weight, None


class GNNAFunction_ReLU(Function):
    """relu(GCN layer) in one pass: the aggregation's epilogue clamps every row where it is written (libgnna
    GNNA_EPILOGUE_RELU; reference call site F.relu(conv1(...)), GNNA_main.py:151) -- one elementwise pass over [N, hidden]
    less per layer.  Backward masks dY with (Y > 0), which the saved output itself provides."""

    @staticmethod
    def forward(ctx, X, weight, inputInfo):
        rp, ci, deg, pp, p2n = _graph_args(inputInfo)
        ctx.info, ctx.knobs = inputInfo, _knobs(inputInfo)
        Y = GNNA.aggregate_ld(1, torch.mm(X, weight), ci, deg, 1.0, pp, p2n, inputInfo.partSize, None, False, True)
        ctx.save_for_backward(X, weight, Y)
        return Y

    @staticmethod
    def backward(ctx, d_output):
        X, weight, Y = ctx.saved_tensors
        return _gcn_backward(ctx, d_output * (Y > 0), X, weight)


class GNNAFunction_GIN(Function):
    """GIN layer: epsilon-scaled aggregation T = eps A X, then update T W (aggregate -> update).
    T is what backward needs, so it is saved instead of X (reference gnn_conv.py:109,119)."""

    @staticmethod
    def forward(ctx, X, weight, inputInfo, eplison):
        rp, ci, _deg, pp, p2n = _graph_args(inputInfo)
        ctx.info, ctx.knobs, ctx.eplison = inputInfo, _knobs(inputInfo), eplison
        weight = _packed(weight)
        X_prime, X_agg = GNNA.forward_gin(_packed(X), weight, rp, ci, eplison, pp, p2n, *ctx.knobs)
        ctx.save_for_backward(X_agg, weight)
        return X_prime

    @staticmethod
    def backward(ctx, d_output):
        X_agg, weight = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            # first layer: d_weight = T^T dY needs no aggregation at all; the reference aggregates
            # dY W^T at the input width (F = 602 on Reddit) and drops the result
            return None, GNNA.xtg(X_agg, _packed(d_output)), None, None
        rp, ci, _deg, pp, p2n = _graph_args(backward_structure(ctx.info))
        d_input, d_weight = GNNA.backward_gin(_packed(d_output), X_agg, weight, rp, ci,
                                              ctx.eplison, pp, p2n, *ctx.knobs)
        return d_input, d_weight, None, None


def _mm_for_gather(X, weight, column_index):
    """X W written in the layout the following (unweighted) aggregation gathers best: rows with the leading dimension
    `gnna_preferred_ld` names (e.g. 128 floats for 64-float rows that are gathered hundreds of times -- every row on its own
    512-byte boundary), so that the library needs no staged copy of them.  rocBLAS writes a leading dimension for free."""
    from . import _lib
    n, dim = X.shape[0], weight.shape[1]
    ld = _lib.preferred_ld(dim, n, column_index.numel())
    if ld == dim:
        return torch.mm(X, weight)
    out = _lib.empty_rows(n, dim, ld, X.device)
    torch.mm(X, weight, out=out)
    return out


def _row_units(width: int) -> int:
    """Cost of aggregating one neighbor row of `width` floats, in 64-float wavefront sweeps."""
    return (int(width) + 63) // 64


class GNNAFunction_GIN_UpdateFirst(Function):
    """The same GIN layer, Y = (eps A X) W, evaluated as eps A (X W): identical function (the
    layer's "MLP" is one linear map, so it commutes with the neighbor sum; only the fp32
    association differs), but both aggregations -- forward on X W, backward on dY -- run at the
    output width.  Chosen by GINConv when the layer narrows (Reddit layer 1: 602 -> 64)."""

    @staticmethod
    def forward(ctx, X, weight, inputInfo, eplison, relu=False):
        rp, ci, _deg, pp, p2n = _graph_args(inputInfo)
        ctx.info, ctx.knobs, ctx.eplison = inputInfo, _knobs(inputInfo), eplison
        ctx.relu = bool(relu)
        with torch.no_grad():
            XW = _mm_for_gather(X, weight, ci)
        Y = GNNA.aggregate_ld(2, XW, ci, None, eplison, pp, p2n, inputInfo.partSize, None, False, bool(relu))
        if relu:      # (the aggregation is the layer's last step here, so its epilogue can clamp)
            ctx.save_for_backward(X, weight, Y)
        else:
            ctx.save_for_backward(X, weight)
        return Y

    @staticmethod
    def backward(ctx, d_output):
        X, weight = ctx.saved_tensors[:2]
        rp, ci, _deg, pp, p2n = _graph_args(backward_structure(ctx.info))
        if ctx.relu:
            d_output = d_output * (ctx.saved_tensors[2] > 0)
        G = GNNA.aggregate_gin(_packed(d_output), rp, ci, ctx.eplison, pp, p2n, *ctx.knobs)   # eps A^T dY
        d_input = torch.mm(G, weight.t()) if ctx.needs_input_grad[0] else None
        return d_input, GNNA.xtg(X, G), None, None, None


class _NeighborConv(Module):
    """Shared parameter handling of the two convolution modules."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.weights = Parameter(torch.empty(input_dim, output_dim))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.weights.size(1))
        with torch.no_grad():
            self.weights.uniform_(-bound, bound)


class GCNConv(_NeighborConv):
    def forward(self, X, inputInfo, relu=False):
        """X: [num_nodes, input_dim]; inputInfo: decider.inputProperty holding the CSR, the
        sqrt-degree vector and the neighbor-group partition on X's device.  relu=True returns relu(layer) with the
        clamp fused into the aggregation (same values as F.relu(conv(X, inputInfo)))."""
        _refuse_block(inputInfo, "GCNConv")
        dt = _x16_dtype(X)
        if dt is not None:      # bfloat16 / float16 features (a cast model, or torch.autocast): fp32 accumulation, 16-bit result
            return GNNAFunction_X16.apply(X, self.weights, inputInfo, 1, 1.0, True, relu, dt)
        return (GNNAFunction_ReLU if relu else GNNAFunction).apply(X, self.weights, inputInfo)


class GINConv(_NeighborConv):
    def __init__(self, input_dim, output_dim, update_first="auto"):
        """update_first: False = the reference's order (aggregate at the input width, then X W);
        True = update first; "auto" = whichever aggregates fewer 64-float sweeps per neighbor."""
        self.eplison = 0.5
        self.update_first = update_first
        super().__init__(input_dim, output_dim)

    def _use_update_first(self, X) -> bool:
        if self.update_first != "auto":
            return bool(self.update_first)
        fin, fout = _row_units(self.weights.size(0)), _row_units(self.weights.size(1))
        # aggregate-first: forward at Fin, plus backward at Fin when the input needs a gradient;
        # update-first: forward and backward at Fout
        needs_dx = X.requires_grad and torch.is_grad_enabled()
        return 2 * fout < (2 * fin if needs_dx else fin)

    def forward(self, X, inputInfo, relu=False):
        """relu=True returns relu(layer): fused into the aggregation when the layer runs update-first (the aggregation is
        its last step), an ordinary F.relu behind the dense update otherwise."""
        _refuse_block(inputInfo, "GINConv")
        dt = _x16_dtype(X)
        if dt is not None:
            return GNNAFunction_X16.apply(X, self.weights, inputInfo, 2, self.eplison, self._use_update_first(X), relu, dt)
        if self._use_update_first(X):
            return GNNAFunction_GIN_UpdateFirst.apply(X, self.weights, inputInfo, self.eplison, relu)
        Y = GNNAFunction_GIN.apply(X, self.weights, inputInfo, self.eplison)
        return torch.relu(Y) if relu else Y


# ---- max / min / mean over the neighbours, GraphSAGE ------------------------------------------------------------------

def _extreme_forward(op, ctx, X, inputInfo):
    ctx.block = inputInfo if _is_block(inputInfo) else None
    if ctx.block is not None:
        X = _block_features(X, inputInfo, "neighbor max / min")
        ci = inputInfo.column_index
        ctx.num_in_rows = X.shape[0]
        Y, arg = _lib.agg_reduce_ld(op, X, ci, inputInfo.partPtr, inputInfo.part2Node, inputInfo.partSize,
                                    num_out_rows=inputInfo.num_dst)
        ctx.save_for_backward(arg, ci)
        return Y
    if X.dtype != torch.float32:
        raise TypeError(f"neighbor max / min: float32 features only (got {X.dtype})")
    ci = inputInfo.column_index
    ctx.num_in_rows = X.shape[0]
    Y, arg = GNNA.aggregate_reduce(op, _laid_out(X), ci, inputInfo.partPtr, inputInfo.part2Node, inputInfo.partSize)
    ctx.save_for_backward(arg, ci)
    return Y


def _extreme_backward(ctx, dY):
    arg, ci = ctx.saved_tensors
    if ctx.block is not None:
        if not ctx.needs_input_grad[0]:
            return None, None
        return _lib.scatter_arg_ld(_laid_out(dY), arg, ci, ctx.num_in_rows), None
    return GNNA.scatter_arg(_laid_out(dY), arg, ci, ctx.num_in_rows), None


class NeighborMax(Function):
    """Y[i, f] = max over the neighbours j of i of X[j, f] (libgnna gnna_agg_reduce_ld_f32; a row without edges gives 0).
    The forward records which edge supplied every element -- among equal values the one earliest in column_index -- and the
    backward sends that element's gradient to that one source row (gnna_scatter_arg_ld_f32).  This backward needs neither a symmetric
    structure nor the transposed one: it is exact on any graph, whatever ``directed`` says."""

    @staticmethod
    def forward(ctx, X, inputInfo):
        return _extreme_forward(0, ctx, X, inputInfo)

    backward = staticmethod(_extreme_backward)


class NeighborMin(Function):
    """NeighborMax with the element-wise minimum; the same tie rule and the same backward (no symmetry assumed)."""

    @staticmethod
    def forward(ctx, X, inputInfo):
        return _extreme_forward(1, ctx, X, inputInfo)

    backward = staticmethod(_extreme_backward)


class NeighborMean(Function):
    """Y = diag(1 / max(count, 1)) A X: the mean over every row's neighbours (0 for a row without edges), composed from the
    neighbor sum GNNA.SAG and a row scaling.  Backward is A^T (dY / count) -- count is the forward graph's; A^T is A itself
    unless the graph is ``directed``."""

    @staticmethod
    def forward(ctx, X, inputInfo):
        ctx.info, ctx.block = inputInfo, inputInfo if _is_block(inputInfo) else None
        if ctx.block is not None:
            inv = inputInfo.inv_row_counts()
            ctx.save_for_backward(inv)
            return _block_sum(_block_features(X, inputInfo, "NeighborMean"), inputInfo, inputInfo.num_dst).mul_(inv.unsqueeze(1))
        if X.dtype != torch.float32:
            raise TypeError(f"NeighborMean: float32 features only (got {X.dtype})")
        ctx.knobs = _knobs(inputInfo)
        inv = inputInfo.inv_row_counts()
        ctx.save_for_backward(inv)
        return GNNA.SAG(_packed(X), *_graph_args(inputInfo), *ctx.knobs).mul_(inv.unsqueeze(1))

    @staticmethod
    def backward(ctx, dY):
        inv, = ctx.saved_tensors
        return _sum_backward(ctx, dY * inv.unsqueeze(1)), None


class SAGEConv(Module):
    """GraphSAGE layer: Y = X W_self + agg(X) W_neigh (+ b), agg the mean, the element-wise max or the element-wise min over
    every node's neighbours.  Both weights are drawn like the other layers' (U(-1/sqrt(out), 1/sqrt(out))).
    mean: when the layer narrows, X W_neigh is aggregated instead of X (the linear map commutes with the mean; the rule is
    GINConv's).  max / min: the order is fixed -- aggregate, then multiply.  float32 only.
    `inputInfo` may be a sampling.SampledBlock: X is then [num_src, F], the result [num_dst, F], and the self term reads the
    block's destination rows X[:num_dst]."""

    _AGG = {"mean": NeighborMean, "max": NeighborMax, "min": NeighborMin}

    def __init__(self, input_dim, output_dim, aggregator="mean", bias=False):
        super().__init__()
        if aggregator not in self._AGG:
            raise ValueError(f"aggregator must be one of {sorted(self._AGG)} (got {aggregator!r})")
        self.aggregator = aggregator
        self.weights_self = Parameter(torch.empty(input_dim, output_dim))
        self.weights_neigh = Parameter(torch.empty(input_dim, output_dim))
        self.bias = Parameter(torch.empty(output_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.weights_self.size(1))
        with torch.no_grad():
            self.weights_self.uniform_(-bound, bound)
            self.weights_neigh.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def _update_first(self, X) -> bool:
        if self.aggregator != "mean":
            return False
        fin, fout = _row_units(self.weights_neigh.size(0)), _row_units(self.weights_neigh.size(1))
        needs_dx = X.requires_grad and torch.is_grad_enabled()
        return 2 * fout < (2 * fin if needs_dx else fin)

    def forward(self, X, inputInfo, relu=False):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("SAGEConv computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        agg = self._AGG[self.aggregator]
        if self._update_first(X):
            N = agg.apply(torch.mm(X, self.weights_neigh), inputInfo)
        else:
            N = torch.mm(agg.apply(X, inputInfo), self.weights_neigh)
        Y = torch.addmm(N, X[:inputInfo.num_dst] if _is_block(inputInfo) else X, self.weights_self)
        if self.bias is not None:
            Y = Y + self.bias
        return torch.relu(Y) if relu else Y


# ---- several statistics of the neighbours from one gather, PNA --------------------------------------------------------

_STAT_NEEDS = {"mean": ("sum",), "std": ("sum", "sumsq"), "max": ("max",), "min": ("min",)}


class NeighborStats(Function):
    """``NeighborStats.apply(X, inputInfo, eps=1e-5) -> (mean, std, max, min)`` of every node's neighbours, from ONE gather
    (libgnna gnna_agg_stats_ld_f32: sum, sum of squares, max and min while a source row is in registers).  With c = max(count, 1):
    mean = sum / c, var = relu(sumsq / c - mean^2), std = sqrt(var + eps) (PyG's StdAggregation); max / min are NeighborMax's /
    NeighborMin's bits, a row without edges gives 0 (std: sqrt(eps)).  A fourth argument names the results wanted
    (``want=("mean", "std")``): the others come back as None and only the statistics they need are computed.

    Backward: dX[j] = (A^T a)[j] + X[j] * (A^T b)[j] + the gradients of max and min routed to their winning sources, with
    a = (g_mean - g_std * mean / std) / c and b = g_std / (c * std); A^T a and A^T b are ONE neighbor sum of [a | b] at width 2F
    over the backward graph (the graph itself, ``transposed()`` when ``directed``, the transposed block).  The derivative of the
    relu on var is left out on purpose: where var is that close to 0 its sign is rounding noise, and a gate would switch a whole
    row's gradient on or off by it.  Outputs that receive no gradient cost nothing; an X that needs none, nothing at all.

    The variance is the uncentred form in fp32: keep the features at unit scale.  With a large common offset (10 * randn + 3)
    rows whose std sits at the sqrt(eps) floor (degree 1, duplicate edges) amplify the rounding of sumsq / c - mean^2 in dX.
    float32 only.  `inputInfo`: a decider.inputProperty (symmetric or ``directed``) or a sampling.SampledBlock (X [num_src, F]
    -> results [num_dst, F])."""

    @staticmethod
    def forward(ctx, X, inputInfo, eps=1e-5, want=("mean", "std", "max", "min")):
        unknown = [w for w in want if w not in _STAT_NEEDS]
        if unknown or not want:
            raise ValueError(f"want must name some of {sorted(_STAT_NEEDS)} (got {tuple(want)!r})")
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("NeighborStats computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        ctx.set_materialize_grads(False)
        ctx.info, ctx.block = inputInfo, inputInfo if _is_block(inputInfo) else None
        if ctx.block is not None:
            X = _block_features(X, inputInfo, "NeighborStats")
            n_out = inputInfo.num_dst
        else:
            ctx.knobs = _knobs(inputInfo)
            X = _laid_out(X)
            n_out = X.shape[0]
        need = {k for w in want for k in _STAT_NEEDS[w]}
        ci = inputInfo.column_index
        s, q, mx, amx, mn, amn = GNNA.aggregate_stats(X, ci, inputInfo.partPtr, inputInfo.part2Node, inputInfo.partSize, n_out,
                                                      "sum" in need, "sumsq" in need, "max" in need, "min" in need)
        inv = inputInfo.inv_row_counts().unsqueeze(1)
        mean = std = None
        if s is not None:
            mean = s.mul_(inv)
        if q is not None:
            std = torch.relu_(q.mul_(inv).addcmul_(mean, mean, value=-1.0)).add_(eps).sqrt_()
        ctx.save_for_backward(X, inv, mean, std, amx, amn, ci)
        out = {"mean": mean, "std": std, "max": mx, "min": mn}
        return tuple(out[k] if k in want else None for k in ("mean", "std", "max", "min"))

    @staticmethod
    def backward(ctx, g_mean, g_std, g_max, g_min):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        X, inv, mean, std, amx, amn, ci = ctx.saved_tensors
        F = X.shape[1]
        dX = None
        if g_mean is not None or g_std is not None:
            # one neighbor sum over the backward graph: of [a | b] when the std has a gradient, of a alone otherwise
            if g_std is None:
                ab = g_mean * inv
            else:
                ab = torch.empty(mean.shape[0], 2 * F, device=X.device, dtype=X.dtype)
                b = torch.div(g_std * inv, std, out=ab[:, F:])
                torch.mul(b, mean, out=ab[:, :F]).neg_()
                if g_mean is not None:
                    ab[:, :F].addcmul_(g_mean, inv)
            T = _sum_backward(ctx, ab)
            dX = T if g_std is None else torch.addcmul(T[:, :F], X, T[:, F:])
        for g, arg in ((g_max, amx), (g_min, amn)):
            if g is not None:
                dX = _lib.scatter_arg_ld(_laid_out(g), arg, ci, X.shape[0], out=dX, accumulate=dX is not None)
        return dX, None, None, None


class PNAConv(Module):
    """Principal Neighbourhood Aggregation layer (Corso et al., 2020) on the one-gather statistics of NeighborStats:

        Y = X[:num_dst] W_self + sum over the scalers s of  s(d) * ([a_1(X) | ... | a_k(X)] W_s)  (+ b)

    with the aggregators a_i among mean, max, min and std of a node's neighbours, d = max(count, 1), and the scalers
    identity (1), amplification (log(d + 1) / delta) and attenuation (delta / log(d + 1)).  The messages are the source
    features themselves: this is the form without PyG's pre-MLP on (x_i, x_j), towers and edge features, which would need
    [nnz, F] tensors.  Whatever subset of aggregators is asked for, only the statistics it needs are computed.

    delta: the value given, else the mean of log(d + 1) over the rows of the graph of the first forward, kept in the buffer
    ``delta``; ``PNAConv.delta_of(inputInfo)`` computes it, so that mini-batch training can pass the full graph's value.
    The weights are drawn like the other layers' (U(-1/sqrt(out), 1/sqrt(out))).  float32 only.  `inputInfo` may be a
    sampling.SampledBlock: X is then [num_src, F], the result [num_dst, F]."""

    AGGREGATORS = ("mean", "max", "min", "std")
    SCALERS = ("identity", "amplification", "attenuation")

    def __init__(self, input_dim, output_dim, aggregators=AGGREGATORS, scalers=SCALERS, delta=None, bias=False, eps=1e-5):
        super().__init__()
        aggregators, scalers = tuple(aggregators), tuple(scalers)
        for what, got, known in (("aggregator", aggregators, self.AGGREGATORS), ("scaler", scalers, self.SCALERS)):
            unknown = [a for a in got if a not in known]
            if unknown or not got or len(set(got)) != len(got):
                raise ValueError(f"{what}s must be distinct names among {known} (got {got!r})")
        if delta is not None and not float(delta) > 0.0:
            raise ValueError(f"delta must be positive (got {delta!r})")
        self.aggregators, self.scalers, self.eps = aggregators, scalers, float(eps)
        self.weights_self = Parameter(torch.empty(input_dim, output_dim))
        self.weights_scaler = torch.nn.ParameterList(Parameter(torch.empty(len(aggregators) * input_dim, output_dim)) for _ in scalers)
        self.bias = Parameter(torch.empty(output_dim)) if bias else None
        self.register_buffer("delta", torch.tensor(float("nan") if delta is None else float(delta)))
        self._delta_checked = delta is not None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.weights_self.size(1))
        with torch.no_grad():
            for w in (self.weights_self, *self.weights_scaler):
                w.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    @staticmethod
    def delta_of(inputInfo):
        """mean over the rows of log(max(count, 1) + 1): the delta of the graph (or block) `inputInfo`."""
        return float(torch.log(1.0 / inputInfo.inv_row_counts() + 1.0).mean())

    def forward(self, X, inputInfo, relu=False):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("PNAConv computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        if not self._delta_checked:           # (a loaded state may have brought a value: NaN means "not set yet")
            if bool(torch.isnan(self.delta)):
                self.delta.fill_(self.delta_of(inputInfo))
            self._delta_checked = True
        stats = dict(zip(("mean", "std", "max", "min"), NeighborStats.apply(X, inputInfo, self.eps, self.aggregators)))
        A = torch.cat([stats[a] for a in self.aggregators], dim=1)
        Y = torch.mm(X[:inputInfo.num_dst] if _is_block(inputInfo) else X, self.weights_self)
        logd = torch.log(1.0 / inputInfo.inv_row_counts() + 1.0).unsqueeze(1)
        for name, W in zip(self.scalers, self.weights_scaler):
            M = torch.mm(A, W)
            if name == "identity":
                Y = Y + M
            elif name == "amplification":
                Y = Y + M * (logd / self.delta)
            else:
                Y = Y + M * (self.delta / logd)
        if self.bias is not None:
            Y = Y + self.bias
        return torch.relu(Y) if relu else Y


# ---- softmax aggregation with a temperature (the learnable aggregator), GENConv -------------------------------------------

def _temp_vector(temp, F, device, what):
    """`temp` as the contiguous float32 vector of 1 or F elements the library takes."""
    if not isinstance(temp, torch.Tensor) or temp.dtype != torch.float32 or temp.numel() not in (1, F):
        raise ValueError(f"{what}: temp must be a float32 tensor of 1 or F = {F} elements "
                         f"(got {tuple(temp.shape) if isinstance(temp, torch.Tensor) else temp!r})")
    return temp.detach().reshape(-1).to(device).contiguous()


class NeighborSoftmax(Function):
    """``NeighborSoftmax.apply(X, temp, inputInfo) -> Y``: softmax aggregation with a temperature, per channel (PyG's
    aggr.SoftmaxAggregation, the aggregator of DeeperGCN's GENConv), from ONE gather (libgnna gnna_agg_softmax_ld_f32):

        Y[i, f] = sum over the edges i <- j of alpha * X[j, f],   alpha = softmax_j(temp[f] * X[j, f])

    `temp`: a float32 tensor of 1 or F elements; 0 gives the mean, a large value approaches the max, a negative one is a soft min.
    A row without edges gives 0.  Nothing of edge-list size is made: the op saves X, temp, Y and lse [rows, F], and
    sq = sum_j alpha X[j]^2 only when `temp` needs a gradient.

    Backward: dX from one gather over the backward graph (the graph itself, ``transposed()`` when ``directed``, the transposed
    block; libgnna gnna_agg_softmax_backward_ld_f32, alpha = exp(temp * x - lse) per edge, never exp(-lse)), and
    dtemp[f] = sum_i dY[i, f] * (sq[i, f] - Y[i, f]^2) in node-sized torch arithmetic.  What needs no gradient is not computed.
    The same bits on every run.  float32 only.  `inputInfo`: a decider.inputProperty (symmetric or ``directed``) or a
    sampling.SampledBlock (X [num_src, F] -> Y [num_dst, F])."""

    @staticmethod
    def forward(ctx, X, temp, inputInfo):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("NeighborSoftmax computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        ctx.set_materialize_grads(False)
        ctx.info = inputInfo
        X = _block_features(X, inputInfo, "NeighborSoftmax") if _is_block(inputInfo) else _laid_out(X)
        t = _temp_vector(temp, X.shape[1], X.device, "NeighborSoftmax")
        ctx.temp_shape = temp.shape
        Y, lse, sq = GNNA.aggregate_softmax(X, t, inputInfo.row_pointers, inputInfo.column_index, bool(ctx.needs_input_grad[1]))
        ctx.save_for_backward(X, t, Y, lse, sq)
        return Y

    @staticmethod
    def backward(ctx, dY):
        if dY is None:
            return None, None, None
        X, t, Y, lse, sq = ctx.saved_tensors
        dX = dt = None
        if ctx.needs_input_grad[0]:
            dY = _laid_out(dY)
            bgraph = backward_structure(ctx.info)
            dX = GNNA.aggregate_softmax_backward(X, t, lse, Y, dY, bgraph.row_pointers, bgraph.column_index)
        if ctx.needs_input_grad[1]:
            per_channel = torch.addcmul(sq, Y, Y, value=-1.0).mul_(dY).sum(0)
            dt = (per_channel if t.numel() > 1 else per_channel.sum()).reshape(ctx.temp_shape)
        return dX, dt, None


def _composed_softmax_aggregation(X, temp, info):
    """The same function from torch ops, with [nnz, F] tensors: the timing baseline and a second opinion."""
    rp, ci = info.row_pointers.long(), info.column_index.long()
    n = rp.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n, device=X.device), rp[1:] - rp[:-1])
    xj = X.index_select(0, ci)
    s = xj * temp.reshape(1, -1)
    idx = dst.unsqueeze(1).expand_as(s)
    m = torch.full((n, X.shape[1]), float("-inf"), device=X.device, dtype=X.dtype).scatter_reduce(0, idx, s.detach(), "amax")
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m.index_select(0, dst))
    l = torch.zeros_like(m).index_add_(0, dst, e)
    a = torch.zeros_like(m).index_add_(0, dst, e * xj)
    return torch.where(l > 0, a / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(a))


class SoftmaxAggregation(Module):
    """``SoftmaxAggregation(t=1.0, learn=False, channels=1, fused=True)(X, inputInfo) -> [rows, F]``: NeighborSoftmax with its
    temperature kept in the module -- `channels` values (1, or the feature width F for one temperature per channel) that start at
    `t`; a Parameter ``t`` when `learn`, a buffer otherwise.  fused=False is the composition from torch ops (index_select,
    scatter_reduce("amax"), index_add_), which makes several [nnz, F] tensors: it exists as the timing baseline and as a second
    opinion, and does not take a SampledBlock."""

    def __init__(self, t=1.0, learn=False, channels=1, fused=True):
        super().__init__()
        if not isinstance(channels, int) or channels < 1:
            raise ValueError(f"channels must be a positive integer (got {channels!r})")
        if not math.isfinite(float(t)):
            raise ValueError(f"t must be finite (got {t!r})")
        self.learn, self.fused = bool(learn), bool(fused)
        init = torch.full((channels,), float(t))
        if self.learn:
            self.t = Parameter(init)
        else:
            self.register_buffer("t", init)

    def forward(self, X, inputInfo):
        if self.t.numel() not in (1, X.shape[1]):
            raise ValueError(f"SoftmaxAggregation has {self.t.numel()} temperatures, the features {X.shape[1]} channels")
        if self.fused:
            return NeighborSoftmax.apply(X, self.t, inputInfo)
        _refuse_block(inputInfo, "SoftmaxAggregation(fused=False)")
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("SoftmaxAggregation computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        return _composed_softmax_aggregation(X, self.t, inputInfo)


class GENConv(Module):
    """GENeralized graph convolution (DeeperGCN; Li et al., 2020) on the one-gather softmax aggregation:

        h = X W_in  (X itself when input_dim == output_dim),   m = relu(h) + eps,   a = SoftmaxAggregation(m)
        Y = MLP(h[:num_dst] + a),   MLP = Linear(out, 2 * out) -> ReLU -> Linear(2 * out, out)

    The messages are node-sized: this is the form without edge features.  Left out against PyG's GENConv: the normalisation
    inside the MLP, the ``powermean`` aggregator and edge attributes (which would need an [nnz, F] input).  `t`, `learn_t` and
    `channels` are SoftmaxAggregation's (channels: 1 or output_dim).  The weights are drawn like the other layers'
    (U(-1/sqrt(columns), 1/sqrt(columns))); `bias` adds one to each Linear of the MLP.  float32 only.  `inputInfo` may be a
    sampling.SampledBlock (fused=True): X is then [num_src, F], the result [num_dst, F]."""

    def __init__(self, input_dim, output_dim, t=1.0, learn_t=False, channels=1, eps=1e-7, bias=False, fused=True):
        super().__init__()
        if channels not in (1, output_dim):
            raise ValueError(f"channels must be 1 or output_dim = {output_dim} (got {channels!r})")
        if not float(eps) >= 0.0:
            raise ValueError(f"eps must be >= 0 (got {eps!r})")
        self.eps = float(eps)
        self.weights_in = Parameter(torch.empty(input_dim, output_dim)) if input_dim != output_dim else None
        self.aggr = SoftmaxAggregation(t, learn_t, channels, fused)
        self.weights_mlp1 = Parameter(torch.empty(output_dim, 2 * output_dim))
        self.weights_mlp2 = Parameter(torch.empty(2 * output_dim, output_dim))
        self.bias_mlp1 = Parameter(torch.empty(2 * output_dim)) if bias else None
        self.bias_mlp2 = Parameter(torch.empty(output_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for w in (self.weights_in, self.weights_mlp1, self.weights_mlp2):
                if w is not None:
                    bound = 1.0 / math.sqrt(w.size(1))
                    w.uniform_(-bound, bound)
            for b in (self.bias_mlp1, self.bias_mlp2):
                if b is not None:
                    b.zero_()

    def forward(self, X, inputInfo, relu=False):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("GENConv computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        h = X if self.weights_in is None else torch.mm(X, self.weights_in)
        a = self.aggr(torch.relu(h) + self.eps, inputInfo)
        z = (h[:inputInfo.num_dst] if _is_block(inputInfo) else h) + a
        z = torch.mm(z, self.weights_mlp1)
        if self.bias_mlp1 is not None:
            z = z + self.bias_mlp1
        Y = torch.mm(torch.relu(z), self.weights_mlp2)
        if self.bias_mlp2 is not None:
            Y = Y + self.bias_mlp2
        return torch.relu(Y) if relu else Y


# ---- relation-typed aggregation, R-GCN -------------------------------------------------------------------------------

def _typed_features(X, rel, what):
    from .relational import RelationalGraph
    if not isinstance(rel, RelationalGraph):
        raise TypeError(f"{what} takes a relational.RelationalGraph (got {type(rel).__name__})")
    if X.dtype != torch.float32 or _x16_dtype(X) is not None:
        raise TypeError(f"{what} computes in float32 only: 16-bit features and torch.autocast are not supported "
                        f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
    if X.dim() != 2 or X.shape[0] != rel.num_src:
        raise ValueError(f"{what}: X must be [{rel.num_src}, F] (got {tuple(X.shape)})")
    return _laid_out(X)


class TypedAggregate(Function):
    """``TypedAggregate.apply(X, coef, rel) -> T`` with T[i, b F + f] = sum_e n[e] coef[t[e], b] X[col(e), f] over the edges of
    row i (libgnna gnna_agg_typed_expand_ld_f32): X [num_src, F], coef [num_relations, B], T [num_dst, B F]; t and n are
    ``rel``'s edge types and factors.  One pass over the ids gathers every source row once for all B bases; no per-edge tensor is
    made in forward or backward.  dX runs over ``rel.transposed()`` (gnna_agg_typed_contract_ld_f32), built at the first backward
    that needs it and skipped when X needs no gradient; dcoef (gnna_typed_coef_grad_ld_f32) is skipped when coef needs none."""

    @staticmethod
    def forward(ctx, X, coef, rel):
        X = _typed_features(X, rel, "TypedAggregate")
        coef = _packed(coef.detach().float())
        ctx.rel = rel
        ctx.save_for_backward(X, coef)
        return rel.expand(X, coef)

    @staticmethod
    def backward(ctx, dT):
        X, coef = ctx.saved_tensors
        dT = _laid_out(dT)
        dX = ctx.rel.contract(dT, coef) if ctx.needs_input_grad[0] else None
        dcoef = ctx.rel.coef_grad(X, dT) if ctx.needs_input_grad[1] else None
        return dX, dcoef, None


class RGCNConv(Module):
    """Relational GCN layer in basis form: W_r = sum_b coef[r, b] V_b and
        Y[i] = sum_r sum_{j in N_r(i)} n W_r^T X[j] + W_self^T X[i] + bias,
    evaluated aggregate-first as ONE typed aggregation into a B-times wider matrix and ONE product:
        T = TypedAggregate(X, coef, rel)  [num_dst, B in_dim],   Y = T V.view(B in_dim, out_dim) + X_dst W_self + bias.
    num_bases=None is R-GCN without decomposition: B = num_relations (<= 16) and coef is the fixed identity.  ``rel`` is a
    relational.RelationalGraph; over a SampledBlock the self term reads the block's destination rows X[:num_dst].  float32 only.
    (The update-first order -- X V_b first, then a contraction -- is not implemented.)"""

    def __init__(self, in_dim, out_dim, num_relations, num_bases=None, bias=True, self_loop=True):
        super().__init__()
        R = int(num_relations)
        if R < 1:
            raise ValueError("num_relations must be >= 1")
        if num_bases is None:
            if R > _lib.TYPED_MAX_BASES:
                raise ValueError(f"RGCNConv without bases keeps one weight per relation and supports at most "
                                 f"{_lib.TYPED_MAX_BASES} of them (got num_relations = {R}): pass num_bases")
            B = R
            self.register_buffer("coef", torch.eye(R))
        else:
            B = int(num_bases)
            if not 1 <= B <= _lib.TYPED_MAX_BASES:
                raise ValueError(f"num_bases must be in 1 .. {_lib.TYPED_MAX_BASES} (got {num_bases})")
            self.coef = Parameter(torch.empty(R, B))
        self.in_dim, self.out_dim, self.num_relations, self.num_bases = int(in_dim), int(out_dim), R, B
        self.V = Parameter(torch.empty(B, self.in_dim, self.out_dim))
        self.W_self = Parameter(torch.empty(self.in_dim, self.out_dim)) if self_loop else None
        self.bias = Parameter(torch.empty(self.out_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.out_dim)
        with torch.no_grad():
            self.V.uniform_(-bound, bound)
            if isinstance(self.coef, Parameter):
                self.coef.uniform_(-1.0 / math.sqrt(self.num_bases), 1.0 / math.sqrt(self.num_bases))
            if self.W_self is not None:
                self.W_self.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, X, rel, relu=False):
        X = _typed_features(X, rel, "RGCNConv")
        if rel.num_relations != self.num_relations:
            raise ValueError(f"the graph has {rel.num_relations} relations, the layer {self.num_relations}")
        T = TypedAggregate.apply(X, self.coef, rel)
        Y = torch.mm(T, self.V.view(self.num_bases * self.in_dim, self.out_dim))
        if self.W_self is not None:
            Y = torch.addmm(Y, X[:rel.num_dst] if rel.is_block else X, self.W_self)
        if self.bias is not None:
            Y = Y + self.bias
        return torch.relu(Y) if relu else Y


# ---- edge-valued aggregation, edge softmax, GAT ----------------------------------------------------------------------

def _heads_of(w):
    """[heads, nnz] view of per-edge values given as [nnz] or [heads, nnz]."""
    return w.view(1, -1) if w.dim() == 1 else w


def _sddmm_at_least_4(A, B, ci, pp, p2n, partSize):
    """<A[row(e)], B[col(e)]> for every edge; the kernel takes rows of >= 4 floats, narrower ones are zero-padded."""
    if A.shape[1] < 4:
        A = torch.nn.functional.pad(A, (0, 4 - A.shape[1]))
        B = torch.nn.functional.pad(B, (0, 4 - B.shape[1]))
    return GNNA.sddmm(A, B, ci, pp, p2n, partSize)


class EdgeWeightedAggregate(Function):
    """Y = A_w X with caller-supplied edge values: Y[i] = sum_e w[e] X[column_index[e]] (libgnna gnna_agg_edge_ld_f32).
    Multi-head: X is [N, heads * F] and w is [heads, nnz]; head h aggregates the column block X[:, h F : (h + 1) F] with w[h]
    into the same block of Y (the strided forms: no copies).  Backward on a graph whose structure is symmetric:
    dX = A_{w[rev]} dY (the same partition, weights read through the reverse-edge map) and dw = sddmm(dY, X).  On a ``directed``
    graph dX is the aggregation of dY over the transposed structure with the weights w[:, perm] (perm: the forward position of
    every transposed edge); dw is the same."""

    @staticmethod
    def forward(ctx, X, w, inputInfo):
        wh = _heads_of(w)
        heads = wh.shape[0]
        assert X.dim() == 2 and X.shape[1] % heads == 0, "X must be [num_nodes, heads * F]"
        assert wh.shape[1] == inputInfo.column_index.numel(), "w must be indexed like column_index"
        ctx.info, ctx.w_shape = inputInfo, w.shape
        X, wh = _laid_out(X), _packed(wh)
        ctx.save_for_backward(X, wh)
        return _edge_aggregate(X, wh, inputInfo)

    @staticmethod
    def backward(ctx, dY):
        X, wh = ctx.saved_tensors
        info = ctx.info
        dY = _laid_out(dY)
        heads, F = wh.shape[0], X.shape[1] // wh.shape[0]
        dX = dw = None
        if ctx.needs_input_grad[0]:
            bgraph, edge_pos = backward_structure(info, edge_pos=True)
            dX = _edge_aggregate(dY, wh.index_select(1, edge_pos).contiguous(), bgraph)
        if ctx.needs_input_grad[1]:
            dw = torch.stack([_sddmm_at_least_4(dY[:, h * F:(h + 1) * F], X[:, h * F:(h + 1) * F], info.column_index,
                                                info.partPtr, info.part2Node, info.partSize) for h in range(heads)])
            dw = dw.view(ctx.w_shape)
        return dX, dw, None


def _edge_aggregate(X, wh, info):
    heads = wh.shape[0]
    F = X.shape[1] // heads
    if heads == 1:
        return GNNA.aggregate_edge(X, info.column_index, wh[0], info.partPtr, info.part2Node, info.partSize)
    Y = torch.empty(X.shape[0], X.shape[1], dtype=X.dtype, device=X.device)
    for h in range(heads):
        GNNA.aggregate_edge(X[:, h * F:(h + 1) * F], info.column_index, wh[h], info.partPtr, info.part2Node, info.partSize,
                            out=Y[:, h * F:(h + 1) * F])
    return Y


class EdgeSoftmax(Function):
    """Softmax of per-edge scores ([nnz] or head-major [heads, nnz]) over the edges of every destination row."""

    @staticmethod
    def forward(ctx, scores, row_pointers):
        p = GNNA.edge_softmax(_packed(scores), row_pointers)
        ctx.save_for_backward(p, row_pointers)
        return p

    @staticmethod
    def backward(ctx, dp):
        p, rp = ctx.saved_tensors
        return GNNA.edge_softmax_backward(p, _packed(dp), rp), None


# ---- the frame the fused attention Functions share ------------------------------------------------------------------------

def _drop_args(who, attn_drop, rng_seed):
    """(attn_drop as a float in [0, 1), rng_seed mod 2^64 -- the key arithmetic is mod 2^64) of the Function `who`."""
    attn_drop, rng_seed = float(attn_drop), int(rng_seed) & (2 ** 64 - 1)
    if not 0.0 <= attn_drop < 1.0:
        raise ValueError(f"{who}: attn_drop must be in [0, 1) (got {attn_drop})")
    return attn_drop, rng_seed


def _grads(ctx, grads=()):
    """What a backward returns: `grads` for the forward's leading tensor arguments, each kept only where ``needs_input_grad``
    asks for it, then None for every other argument (inputInfo, negative_slope, ... whichever the call gave)."""
    need = ctx.needs_input_grad
    return tuple(g if n else None for g, n in zip(grads, need)) + (None,) * (len(need) - len(grads))


def _transposed_args(info, t):
    """The `transposed` argument of an attention backward entry: None when the backward walks the forward structure itself (a
    symmetric graph: the binding then passes its structure as the transposed one)."""
    return None if t is info else [t.row_pointers, t.column_index, t.partPtr, t.part2Node]


def _step_seed(module, rng_seed):
    """The seed of this forward of a layer with attention dropout: the caller's, else 63 bits from torch's CPU default generator
    (a CPU tensor: no device synchronisation); kept as ``module.last_rng_seed``."""
    if rng_seed is None:
        rng_seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
    module.last_rng_seed = int(rng_seed)
    return module.last_rng_seed


class GATAttention(Function):
    """The attention of a GAT layer in one fused call per direction (libgnna gnna_gat_forward_f32 / gnna_gat_backward_f32):
    ``GATAttention.apply(H, el, er, inputInfo, negative_slope) -> Y`` with H [N, heads * F], el / er [N, heads] and
    Y[i, h] = sum_e alpha(e, h) H[col(e), h], alpha = softmax over row i of leaky_relu(el[i, h] + er[col(e), h]).  alpha is
    computed from el, er and the saved log-sum-exp of every row wherever a kernel gathers a row: no [nnz] tensor is made, saved
    or cached (saved: H, el, er, lse, Y -- all node-sized), and all heads run in one call.  The gradient of H returned here is the
    attention part (sum alpha dY); the paths through el and er are autograd's.

    On a ``directed`` graph the backward's source-side pass walks the transposed structure (decider.inputProperty.transposed:
    nnz x 4 bytes of ids and a partition stay on the device) and nothing is assumed.  Otherwise the backward reads row j's edges
    as the edges j -> i, so before its first backward on a graph it establishes that the structure is symmetric and raises otherwise (``decider.inputProperty.require_symmetric``): once per column_index, on the host -- a
    copy of the CSR to the host and a pass of gnna_reverse_edges_i32 over it, about a second at 1e8 edges; only the answer is
    kept, nothing of the size of the edge list stays on the device.

    `inputInfo` may be a sampling.SampledBlock (gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32): H is
    [num_src, heads * F], er [num_src, heads], el [num_dst, heads] and Y [num_dst, heads * F].  The backward runs on
    ``block.transposed()``, built at the first backward in which H, el or er needs a gradient (the forward alone builds
    nothing); no symmetry check is made for a block.

    Attention dropout: ``GATAttention.apply(H, el, er, inputInfo, negative_slope, attn_drop, rng_seed)`` scales every alpha by
    k = 0 (with probability attn_drop) or 1 / (1 - attn_drop) after the softmax (libgnna gnna_gat_forward_drop_f32 /
    gnna_gat_backward_drop_f32, include/gnna_ext.h).  Whether an edge i <- j of head h is kept is a function of (rng_seed, i, j, h)
    that the forward and both backward passes recompute: there is no mask tensor, the saved tensors stay node-sized and the seed
    is a Python int on ctx.  Duplicate edges (i, j) are kept or dropped together.  attn_drop = 0 (or the five-argument call) runs
    the plain entries."""

    @staticmethod
    def forward(ctx, H, el, er, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0):
        info = inputInfo
        attn_drop, rng_seed = _drop_args("GATAttention", attn_drop, rng_seed)
        if _is_block(info):
            H = _block_features(H, info, "GATAttention")
            if er.dim() != 2 or er.shape[0] != info.num_src or el.dim() != 2 or el.shape[0] != info.num_dst or \
                    el.shape[1] != er.shape[1]:
                raise ValueError(f"GATAttention on a SampledBlock: el must be [num_dst = {info.num_dst}, heads] and er "
                                 f"[num_src = {info.num_src}, heads] (got {tuple(el.shape)} and {tuple(er.shape)})")
            if el.dtype != torch.float32 or er.dtype != torch.float32:
                raise TypeError(f"GATAttention on a SampledBlock: float32 scores only (got {el.dtype}, {er.dtype})")
        el, er = _packed(el), _packed(er)
        graph = (info.row_pointers, info.column_index, info.partPtr, info.part2Node, info.partSize, float(negative_slope))
        if attn_drop > 0.0:
            Y, lse = GNNA.gat_forward_drop(H, el, er, *graph, attn_drop, rng_seed)
        else:
            Y, lse = GNNA.gat_forward(H, el, er, *graph)
        ctx.info, ctx.negative_slope, ctx.attn_drop, ctx.rng_seed = info, float(negative_slope), attn_drop, rng_seed
        ctx.save_for_backward(H, el, er, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        H, el, er, lse, Y = ctx.saved_tensors
        info = ctx.info
        if not any(ctx.needs_input_grad[:3]):
            return _grads(ctx)
        transposed = _transposed_args(info, backward_structure(info, require_symmetric=True))
        graph = (info.row_pointers, info.column_index, info.partPtr, info.part2Node, info.partSize, ctx.negative_slope)
        if ctx.attn_drop > 0.0:
            return _grads(ctx, GNNA.gat_backward_drop(H, el, er, lse, Y, dY, *graph, ctx.attn_drop, ctx.rng_seed, transposed))
        return _grads(ctx, GNNA.gat_backward(H, el, er, lse, Y, dY, *graph, transposed))


class GATEdgeAttention(Function):
    """GATAttention with a per-edge score term (libgnna gnna_gat_edge_forward_f32 / gnna_gat_edge_backward_f32,
    include/gnna_gat_edge.h): ``GATEdgeAttention.apply(H, el, er, ee, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0) -> Y``
    with ee [nnz, heads] float32, edge-major in the order of ``inputInfo.column_index``, and
    alpha = softmax over row i of leaky_relu(el[i, h] + er[col(e), h] + ee[e, h]).  ee is one scalar per (edge, head) -- what
    PyG's GATConv(edge_dim=...) adds to the score -- and a gradient-carrying input: the backward returns d_ee [nnz, heads] beside
    the gradients of H, el and er.  Saved: the node-sized tensors of GATAttention and ee; alpha is still made inside the gathers.

    The source-side pass of the backward finds an edge's ee through a position map of nnz x 4 bytes: ``info.reverse_edges()`` on
    a graph whose structure is symmetric (``require_symmetric`` first, as GATAttention), the ``perm`` of ``info.transposed()`` on
    a ``directed`` graph or a sampling.SampledBlock (whose ee rows are those of the block's own edges)."""

    @staticmethod
    def forward(ctx, H, el, er, ee, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0):
        info = inputInfo
        attn_drop, rng_seed = _drop_args("GATEdgeAttention", attn_drop, rng_seed)
        if _is_block(info):
            H = _block_features(H, info, "GATEdgeAttention")
            if er.dim() != 2 or er.shape[0] != info.num_src or el.dim() != 2 or el.shape[0] != info.num_dst or \
                    el.shape[1] != er.shape[1]:
                raise ValueError(f"GATEdgeAttention on a SampledBlock: el must be [num_dst = {info.num_dst}, heads] and er "
                                 f"[num_src = {info.num_src}, heads] (got {tuple(el.shape)} and {tuple(er.shape)})")
        nnz = info.column_index.numel()
        if ee.dim() != 2 or el.dim() != 2 or tuple(ee.shape) != (nnz, el.shape[1]):
            raise ValueError(f"GATEdgeAttention: ee must be [nnz = {nnz}, heads = {el.shape[-1]}] in the order of column_index "
                             f"(got {tuple(ee.shape)})")
        if any(t.dtype != torch.float32 for t in (H, el, er, ee)):
            raise TypeError(f"GATEdgeAttention: float32 only (got {H.dtype}, {el.dtype}, {er.dtype}, {ee.dtype})")
        el, er, ee = _packed(el), _packed(er), _packed(ee)
        graph = (info.row_pointers, info.column_index, info.partPtr, info.part2Node, info.partSize, float(negative_slope))
        Y, lse = GNNA.gat_edge_forward(H, el, er, ee, *graph, attn_drop, rng_seed)
        ctx.info, ctx.negative_slope, ctx.attn_drop, ctx.rng_seed = info, float(negative_slope), attn_drop, rng_seed
        ctx.save_for_backward(H, el, er, ee, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        H, el, er, ee, lse, Y = ctx.saved_tensors
        info = ctx.info
        if not any(ctx.needs_input_grad[:4]):
            return _grads(ctx)
        t, t_edge_pos = backward_structure(info, require_symmetric=True, edge_pos=True)
        return _grads(ctx, GNNA.gat_edge_backward(H, el, er, ee, lse, Y, dY, info.row_pointers, info.column_index, info.partPtr,
                                                  info.part2Node, t_edge_pos, info.partSize, ctx.negative_slope, ctx.attn_drop,
                                                  ctx.rng_seed, _transposed_args(info, t)))


class GATConv(Module):
    """Additive graph attention (GAT): H = X W; per head h, s[e] = leaky_relu(<H_h[row(e)], a_l[h]> + <H_h[col(e)], a_r[h]>),
    alpha = edge softmax of s over every row, Y_h = A_alpha H_h.  Heads are concatenated (concat=True, [N, heads * out]) or
    averaged ([N, out]).  The scores are nnz-sized elementwise torch work; softmax and aggregation are libgnna kernels.
    Needs the graph's structure to be symmetric (the backward gathers through the reverse-edge map) unless the graph is
    ``directed`` (then it gathers over the transposed structure).
    fused=True: the attention runs on GATAttention instead -- the same function, with alpha made from node-sized values inside
    the gathers: no per-edge tensor, one call for all heads.
    With fused=True `inputInfo` may be a sampling.SampledBlock: X is [num_src, in], H = X W covers all num_src rows, er comes
    from all of H and el from H[:num_dst] (a block's destination rows are its first source rows); the result is
    [num_dst, heads * out] ([num_dst, out] with concat=False).  float32 only.  fused=False refuses a block: the composed path
    would build per-edge tensors for every batch.
    attn_drop: dropout on the attention coefficients after the softmax (the `attn_drop` of DGL's GATConv, the `dropout` of PyG's),
    active only in training mode; ``model.eval()`` or attn_drop = 0 takes exactly the path without it.  fused=True: the mask is a
    function of (seed, destination row, source row, head) made inside the kernels (GATAttention); one 63-bit seed per forward,
    drawn on the host from torch's CPU default generator (no device synchronisation; ``torch.manual_seed`` reproduces a run)
    unless ``forward(..., rng_seed=...)`` gives it, and kept as ``self.last_rng_seed``.  fused=False:
    ``torch.nn.functional.dropout`` on alpha -- the same distribution from another generator (torch's device generator, one draw
    per edge position), so the two paths drop different edges for the same seed, and only the fused one drops duplicate edges
    together.
    edge_dim: edge features in the score, as PyG's GATConv(edge_dim=...): ``forward(..., edge_attr=...)`` takes edge_attr
    [nnz, edge_dim] float32 in the order of ``inputInfo.column_index`` (for a block: the rows of the block's own edges, which the
    caller selects with ``block.edge_ids``), and every edge adds ee[e, h] = <(edge_attr[e] weights_edge)_h, att_e[h]> to the
    score before the leaky ReLU.  The layer forms M[d, h] = sum_c weights_edge[d, h out + c] att_e[h, c] and ee = edge_attr @ M
    -- the same function without the [nnz, heads * out] intermediate; autograd carries d_ee to weights_edge, att_e and
    edge_attr.  fused=True runs GATEdgeAttention (ee and d_ee, [nnz, heads], are the only per-edge tensors); fused=False adds ee
    to the composed score.
    ``forward(..., return_attention_weights=True)`` returns (Y, alpha) with alpha [nnz, heads], the undropped coefficients
    edge for edge, detached (fused: libgnna gnna_gat_alpha_f32 after a second forward pass for the log-sum-exp; composed: its softmax)."""

    def __init__(self, input_dim, output_dim, heads=1, concat=True, negative_slope=0.2, fused=False, attn_drop=0.0, edge_dim=None):
        super().__init__()
        self.attn_drop = float(attn_drop)
        if not 0.0 <= self.attn_drop < 1.0:
            raise ValueError(f"GATConv: attn_drop must be in [0, 1) (got {attn_drop})")
        self.last_rng_seed = None
        self.heads, self.out_dim, self.concat, self.negative_slope = int(heads), int(output_dim), bool(concat), float(negative_slope)
        self.fused = bool(fused)
        self.weights = Parameter(torch.empty(input_dim, self.heads * self.out_dim))
        self.att_l = Parameter(torch.empty(self.heads, self.out_dim))
        self.att_r = Parameter(torch.empty(self.heads, self.out_dim))
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        if self.edge_dim is not None:
            if self.edge_dim < 1:
                raise ValueError(f"GATConv: edge_dim must be positive (got {edge_dim})")
            self.weights_edge = Parameter(torch.empty(self.edge_dim, self.heads * self.out_dim))
            self.att_e = Parameter(torch.empty(self.heads, self.out_dim))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.out_dim)
        with torch.no_grad():
            self.weights.uniform_(-bound, bound)
            self.att_l.uniform_(-bound, bound)
            self.att_r.uniform_(-bound, bound)
            if self.edge_dim is not None:
                self.weights_edge.uniform_(-bound, bound)
                self.att_e.uniform_(-bound, bound)

    def _edge_scores(self, edge_attr, inputInfo):
        """ee [nnz, heads] of the layer's edge features, or None for a layer without them."""
        if self.edge_dim is None:
            if edge_attr is not None:
                raise ValueError("GATConv: edge_attr given to a layer built without edge_dim")
            return None
        if edge_attr is None:
            raise ValueError(f"GATConv(edge_dim={self.edge_dim}): forward needs edge_attr [nnz, {self.edge_dim}]")
        nnz = inputInfo.column_index.numel()
        if edge_attr.dim() != 2 or tuple(edge_attr.shape) != (nnz, self.edge_dim):
            raise ValueError(f"GATConv: edge_attr must be [nnz = {nnz}, edge_dim = {self.edge_dim}] in the order of column_index "
                             f"(got {tuple(edge_attr.shape)})")
        if edge_attr.dtype != torch.float32 or _x16_dtype(edge_attr) is not None:
            raise TypeError("GATConv with edge features computes in float32 only: 16-bit features and torch.autocast are not "
                            f"supported (got {edge_attr.dtype}{', inside torch.autocast' if edge_attr.dtype == torch.float32 else ''})")
        M = (self.weights_edge.view(self.edge_dim, self.heads, self.out_dim) * self.att_e).sum(-1)      # [edge_dim, heads]
        return torch.mm(edge_attr, M)

    def forward(self, X, inputInfo, rng_seed=None, edge_attr=None, return_attention_weights=False):
        block = _is_block(inputInfo)
        drop = self.training and self.attn_drop > 0.0
        if block:
            if not self.fused:
                _refuse_block(inputInfo, "GATConv(fused=False)")
            if X.dtype != torch.float32 or _x16_dtype(X) is not None:
                raise TypeError("GATConv on a SampledBlock computes in float32 only: 16-bit features and torch.autocast are not "
                                f"supported (got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
            X = _block_features(X, inputInfo, "GATConv")
        ee = self._edge_scores(edge_attr, inputInfo)
        if ee is not None and (X.dtype != torch.float32 or _x16_dtype(X) is not None):
            raise TypeError("GATConv with edge features computes in float32 only: 16-bit features and torch.autocast are not "
                            f"supported (got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        H = torch.mm(X, self.weights)
        Hh = H.view(X.shape[0], self.heads, self.out_dim)
        n = inputInfo.num_dst if block else X.shape[0]      # rows of the result
        el = ((Hh[:n] if block else Hh) * self.att_l).sum(-1)      # [N, heads] ([num_dst, heads]): destination side
        er = (Hh * self.att_r).sum(-1)          # [N, heads] ([num_src, heads]): source side
        weights = None
        if self.fused and drop:
            seed = _step_seed(self, rng_seed)
            if ee is not None:
                Y = GATEdgeAttention.apply(H, el, er, ee, inputInfo, self.negative_slope, self.attn_drop, seed)
            else:
                Y = GATAttention.apply(H, el, er, inputInfo, self.negative_slope, self.attn_drop, seed)
        elif self.fused:
            if ee is not None:
                Y = GATEdgeAttention.apply(H, el, er, ee, inputInfo, self.negative_slope)
            else:
                Y = GATAttention.apply(H, el, er, inputInfo, self.negative_slope)
        else:
            rows, ci = inputInfo.edge_rows(), inputInfo.column_index
            z = el.index_select(0, rows) + er.index_select(0, ci)
            if ee is not None:
                z = z + ee
            s = torch.nn.functional.leaky_relu(z, self.negative_slope)
            alpha = EdgeSoftmax.apply(s.t().contiguous(), inputInfo.row_pointers)      # [heads, nnz]
            if return_attention_weights:
                weights = alpha.detach().t().contiguous()
            if drop:
                alpha = torch.nn.functional.dropout(alpha, self.attn_drop, training=True)
            Y = EdgeWeightedAggregate.apply(H, alpha, inputInfo)
        if self.fused and return_attention_weights:
            weights = _fused_attention_weights(H, el, er, ee, inputInfo, self.negative_slope)
        if not (self.concat or self.heads == 1):
            Y = Y.view(n, self.heads, self.out_dim).mean(1)
        return (Y, weights) if return_attention_weights else Y


def _fused_attention_weights(H, el, er, ee, info, negative_slope):
    """alpha [nnz, heads] of the fused attention (libgnna gnna_gat_alpha_f32), edge for edge from el, er, ee and the log-sum-exp
    of the rows.  The autograd Functions keep their lse to themselves, so this asks the forward entry for it once more (without
    dropout: lse is that of the undropped scores) -- the price of the option, a second forward pass."""
    with torch.no_grad():
        H, el, er = H.detach(), el.detach().contiguous(), er.detach().contiguous()
        graph = (info.row_pointers, info.column_index, info.partPtr, info.part2Node, info.partSize, float(negative_slope))
        if ee is None:
            lse = GNNA.gat_forward(H, el, er, *graph)[1]
        else:
            ee = ee.detach().contiguous()
            lse = GNNA.gat_edge_forward(H, el, er, ee, *graph)[1]
        return GNNA.gat_alpha(el, er, ee, lse, info.row_pointers, info.column_index, float(negative_slope))


class GATv2Attention(Function):
    """The attention of a GATv2 layer ("dynamic" attention, Brody et al.) in one fused call per direction (libgnna
    gnna_gatv2_forward_f32 / gnna_gatv2_backward_f32, include/gnna_gatv2.h):
    ``GATv2Attention.apply(Hs, Hd, att, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0) -> Y`` with Hs [N, heads * F] (the
    source side and the message), Hd [N, heads * F] (the destination side), att [heads, F] and
    Y[i, h] = sum_e alpha(e, h) k Hs[col(e), h], alpha = softmax over row i of z = sum_d att[h, d] leaky_relu(Hs[col(e), h, d] +
    Hd[i, h, d]).  The non-linearity sits inside the dot product, so the score cannot be made from two node-sized scalars as in
    GATAttention: every kernel recomputes z from the row it gathers and the row's own Hd piece.  No [nnz] tensor is made, saved or
    cached (saved: Hs, Hd, att, lse, Y -- all node-sized).  Returns (dHs, dHd, d_att).  Hs and Hd may be the same tensor (shared
    weights): autograd adds the two gradients.

    `inputInfo` is a graph, a ``directed`` graph or a sampling.SampledBlock (Hs [num_src, heads * F], Hd [num_dst, heads * F],
    Y [num_dst, heads * F]); ``transposed()`` / ``require_symmetric`` are handled exactly as in GATAttention.  attn_drop / rng_seed:
    the mask rule of GATAttention (include/gnna_ext.h), recomputed in every pass; attn_drop = 0 is the plain function."""

    @staticmethod
    def forward(ctx, Hs, Hd, att, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0):
        info = inputInfo
        attn_drop, rng_seed = _drop_args("GATv2Attention", attn_drop, rng_seed)
        for t, name in ((Hs, "Hs"), (Hd, "Hd"), (att, "att")):
            if t.dtype != torch.float32:
                raise TypeError(f"GATv2Attention: float32 only (got {name}: {t.dtype})")
        if att.dim() != 2 or Hs.dim() != 2 or Hd.dim() != 2 or Hs.shape[1] != Hd.shape[1] or att.numel() != Hs.shape[1]:
            raise ValueError(f"GATv2Attention: Hs [num_src, heads * F], Hd [num_dst, heads * F] and att [heads, F] expected (got "
                             f"{tuple(Hs.shape)}, {tuple(Hd.shape)} and {tuple(att.shape)})")
        if _is_block(info):
            Hs = _block_features(Hs, info, "GATv2Attention")
            if Hd.shape[0] != info.num_dst:
                raise ValueError(f"GATv2Attention on a SampledBlock: Hd must be [num_dst = {info.num_dst}, heads * F] "
                                 f"(got {tuple(Hd.shape)})")
        att = _packed(att)
        Y, lse = GNNA.gatv2_forward(Hs, Hd, att, info.row_pointers, info.column_index, info.partPtr, info.part2Node, info.partSize,
                                    float(negative_slope), attn_drop, rng_seed)
        ctx.info, ctx.negative_slope, ctx.attn_drop, ctx.rng_seed = info, float(negative_slope), attn_drop, rng_seed
        ctx.save_for_backward(Hs, Hd, att, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        Hs, Hd, att, lse, Y = ctx.saved_tensors
        info = ctx.info
        if not any(ctx.needs_input_grad[:3]):
            return _grads(ctx)
        transposed = _transposed_args(info, backward_structure(info, require_symmetric=True))
        return _grads(ctx, GNNA.gatv2_backward(Hs, Hd, att, lse, Y, dY, info.row_pointers, info.column_index, info.partPtr,
                                               info.part2Node, info.partSize, ctx.negative_slope, ctx.attn_drop, ctx.rng_seed,
                                               transposed))


class GATv2Conv(Module):
    """GATv2 ("How Attentive are Graph Attention Networks?"): Hs = X W_l, Hd = X W_r; per head h,
    z[e] = <att[h], leaky_relu(Hs_h[col(e)] + Hd_h[row(e)])>, alpha = edge softmax of z over every row, Y_h = A_alpha Hs_h.  Heads
    are concatenated (concat=True, [N, heads * out]) or averaged ([N, out]).  share_weights: W_r is W_l (no second parameter), so
    Hd = Hs.  fused=True (the default): the attention runs on GATv2Attention -- no per-edge tensor, one call for all heads.
    fused=False is the composed path: t and z are [nnz, heads * out]-sized torch work (index_select, add, leaky_relu, dot), then
    EdgeSoftmax, torch dropout and EdgeWeightedAggregate; it exists to be compared with, and its memory is why it is not the default.
    With fused=True `inputInfo` may be a sampling.SampledBlock: X is [num_src, in], Hs covers all num_src rows and Hd is
    X[:num_dst] W_r (with share_weights: the first num_dst rows of Hs); fused=False refuses a block.  float32 only.
    attn_drop, ``forward(..., rng_seed=...)`` and ``last_rng_seed`` are GATConv's."""

    def __init__(self, input_dim, output_dim, heads=1, concat=True, negative_slope=0.2, share_weights=False, attn_drop=0.0,
                 fused=True):
        super().__init__()
        self.attn_drop = float(attn_drop)
        if not 0.0 <= self.attn_drop < 1.0:
            raise ValueError(f"GATv2Conv: attn_drop must be in [0, 1) (got {attn_drop})")
        if int(heads) < 1 or int(output_dim) < 1:
            raise ValueError(f"GATv2Conv: heads and output_dim must be >= 1 (got {heads}, {output_dim})")
        self.last_rng_seed = None
        self.heads, self.out_dim, self.concat, self.negative_slope = int(heads), int(output_dim), bool(concat), float(negative_slope)
        self.share_weights, self.fused = bool(share_weights), bool(fused)
        self.W_l = Parameter(torch.empty(input_dim, self.heads * self.out_dim))
        if self.share_weights:
            self.register_parameter("W_r", None)
        else:
            self.W_r = Parameter(torch.empty(input_dim, self.heads * self.out_dim))
        self.att = Parameter(torch.empty(self.heads, self.out_dim))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.out_dim)
        with torch.no_grad():
            self.W_l.uniform_(-bound, bound)
            if self.W_r is not None:
                self.W_r.uniform_(-bound, bound)
            self.att.uniform_(-bound, bound)

    def forward(self, X, inputInfo, rng_seed=None):
        block = _is_block(inputInfo)
        drop = self.training and self.attn_drop > 0.0
        if block and not self.fused:
            _refuse_block(inputInfo, "GATv2Conv(fused=False)")
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("GATv2Conv computes in float32 only: 16-bit features and torch.autocast are not "
                            f"supported (got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        if block:
            X = _block_features(X, inputInfo, "GATv2Conv")
        n = inputInfo.num_dst if block else X.shape[0]      # rows of the result
        Hs = torch.mm(X, self.W_l)
        if self.share_weights:
            Hd = Hs[:n] if block else Hs
        else:
            Hd = torch.mm(X[:n] if block else X, self.W_r)
        if self.fused:
            if drop:
                Y = GATv2Attention.apply(Hs, Hd, self.att, inputInfo, self.negative_slope, self.attn_drop,
                                         _step_seed(self, rng_seed))
            else:
                Y = GATv2Attention.apply(Hs, Hd, self.att, inputInfo, self.negative_slope)
        else:
            rows, ci = inputInfo.edge_rows(), inputInfo.column_index
            t = torch.nn.functional.leaky_relu(Hs.index_select(0, ci) + Hd.index_select(0, rows), self.negative_slope)
            z = (t.view(-1, self.heads, self.out_dim) * self.att).sum(-1)              # [nnz, heads]
            alpha = EdgeSoftmax.apply(z.t().contiguous(), inputInfo.row_pointers)      # [heads, nnz]
            if drop:
                alpha = torch.nn.functional.dropout(alpha, self.attn_drop, training=True)
            Y = EdgeWeightedAggregate.apply(Hs, alpha, inputInfo)
        if self.concat or self.heads == 1:
            return Y
        return Y.view(n, self.heads, self.out_dim).mean(1)


class DotAttention(Function):
    """Scaled dot-product attention over the edges of a graph -- the attention of graph transformers (TransformerConv / UniMP,
    DotGatConv, the inner step of HGT and GPS layers) -- in one fused call per direction (libgnna gnna_dot_attn_forward_f32 /
    gnna_dot_attn_backward_f32, include/gnna_dotattn.h):
    ``DotAttention.apply(Q, K, V, inputInfo, heads, scale=None, attn_drop=0.0, rng_seed=0) -> Y`` with Q [N, heads * F] (the
    queries of the destination rows), K and V [N, heads * F] (the keys and the messages of the source rows) and
    Y[i, h] = sum_e alpha(e, h) k V[col(e), h], alpha = softmax over row i of z = scale * <Q[i, h], K[col(e), h]>; scale defaults to
    1 / sqrt(F), which is why the op is told `heads`.  Every kernel recomputes z from the rows it gathers; no [nnz] tensor is made,
    saved or cached (saved: Q, K, V, lse, Y -- all node-sized).  Returns (dQ, dK, dV).  Q, K and V may be row-strided views
    (column slices of one projection matrix): they are passed with their strides, not copied.

    `inputInfo` is a graph, a ``directed`` graph or a sampling.SampledBlock (Q [num_dst, heads * F], K and V [num_src, heads * F],
    Y [num_dst, heads * F]); ``transposed()`` / ``require_symmetric`` are handled exactly as in GATv2Attention.  attn_drop /
    rng_seed: the mask rule of GATAttention (include/gnna_ext.h), recomputed in every pass; attn_drop = 0 is the plain function."""

    @staticmethod
    def forward(ctx, Q, K, V, inputInfo, heads, scale=None, attn_drop=0.0, rng_seed=0):
        info = inputInfo
        heads = int(heads)
        attn_drop, rng_seed = _drop_args("DotAttention", attn_drop, rng_seed)
        for t, name in ((Q, "Q"), (K, "K"), (V, "V")):
            if t.dtype != torch.float32:
                raise TypeError(f"DotAttention: float32 only (got {name}: {t.dtype})")
        if Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or K.shape[1] != Q.shape[1] or V.shape != K.shape or heads < 1 or \
                Q.shape[1] % heads != 0:
            raise ValueError(f"DotAttention: Q [num_dst, heads * F], K and V [num_src, heads * F] with heads = {heads} expected (got "
                             f"{tuple(Q.shape)}, {tuple(K.shape)} and {tuple(V.shape)})")
        scale = 1.0 / math.sqrt(Q.shape[1] // heads) if scale is None else float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"DotAttention: scale must be finite (got {scale})")
        if _is_block(info):
            K = _block_features(K, info, "DotAttention")
            if V.shape[0] != info.num_src or Q.shape[0] != info.num_dst:
                raise ValueError(f"DotAttention on a SampledBlock: Q must be [num_dst = {info.num_dst}, heads * F] and V "
                                 f"[num_src = {info.num_src}, heads * F] (got {tuple(Q.shape)} and {tuple(V.shape)})")
        Y, lse = GNNA.dot_attn_forward(Q, K, V, heads, info.row_pointers, info.column_index, info.partPtr, info.part2Node,
                                       info.partSize, scale, attn_drop, rng_seed)
        ctx.info, ctx.heads, ctx.scale, ctx.attn_drop, ctx.rng_seed = info, heads, scale, attn_drop, rng_seed
        ctx.save_for_backward(Q, K, V, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        Q, K, V, lse, Y = ctx.saved_tensors
        info = ctx.info
        if not any(ctx.needs_input_grad[:3]):
            return _grads(ctx)
        transposed = _transposed_args(info, backward_structure(info, require_symmetric=True))
        return _grads(ctx, GNNA.dot_attn_backward(Q, K, V, ctx.heads, lse, Y, dY, info.row_pointers, info.column_index, info.partPtr,
                                                  info.part2Node, info.partSize, ctx.scale, ctx.attn_drop, ctx.rng_seed, transposed))


class TransformerConv(Module):
    """The graph transformer layer ("Masked Label Prediction: Unified Message Passing Model", PyG's TransformerConv without edge
    features, biases or the beta gate): [Q | K | V] = X W with one weight [in, 3 * heads * out] and one torch.mm; per head h,
    z[e] = <Q_h[row(e)], K_h[col(e)]> / sqrt(out), alpha = edge softmax of z over every row, Y_h = A_alpha V_h.  Heads are
    concatenated (concat=True, [N, heads * out]) or averaged ([N, out]); root_weight adds the skip connection X W_skip.  Q, K and V
    are handed on as column slices of the product, never copied.  fused=True (the default, for memory, not as a speed claim): the
    attention runs on DotAttention -- no per-edge tensor, one call for all heads.  fused=False is the composed path: Q[rows] and
    K[cols] are [nnz, heads * out]-sized torch work (index_select, product, sum), then EdgeSoftmax, torch dropout and
    EdgeWeightedAggregate; it exists to be compared with.  With fused=True `inputInfo` may be a sampling.SampledBlock: X is
    [num_src, in], K and V cover all num_src rows, Q is the first num_dst rows and the skip connection reads X[:num_dst];
    fused=False refuses a block.  float32 only.  attn_drop, ``forward(..., rng_seed=...)`` and ``last_rng_seed`` are GATConv's."""

    def __init__(self, input_dim, output_dim, heads=1, concat=True, root_weight=True, attn_drop=0.0, fused=True):
        super().__init__()
        self.attn_drop = float(attn_drop)
        if not 0.0 <= self.attn_drop < 1.0:
            raise ValueError(f"TransformerConv: attn_drop must be in [0, 1) (got {attn_drop})")
        if int(heads) < 1 or int(output_dim) < 1:
            raise ValueError(f"TransformerConv: heads and output_dim must be >= 1 (got {heads}, {output_dim})")
        self.last_rng_seed = None
        self.heads, self.out_dim, self.concat = int(heads), int(output_dim), bool(concat)
        self.root_weight, self.fused = bool(root_weight), bool(fused)
        self.weights = Parameter(torch.empty(input_dim, 3 * self.heads * self.out_dim))
        if self.root_weight:
            self.W_skip = Parameter(torch.empty(input_dim, self.heads * self.out_dim if self.concat else self.out_dim))
        else:
            self.register_parameter("W_skip", None)
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.out_dim)
        with torch.no_grad():
            self.weights.uniform_(-bound, bound)
            if self.W_skip is not None:
                self.W_skip.uniform_(-bound, bound)

    def forward(self, X, inputInfo, rng_seed=None):
        block = _is_block(inputInfo)
        drop = self.training and self.attn_drop > 0.0
        if block and not self.fused:
            _refuse_block(inputInfo, "TransformerConv(fused=False)")
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("TransformerConv computes in float32 only: 16-bit features and torch.autocast are not "
                            f"supported (got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        if block:
            X = _block_features(X, inputInfo, "TransformerConv")
        n = inputInfo.num_dst if block else X.shape[0]      # rows of the result
        W = self.heads * self.out_dim
        P = torch.mm(X, self.weights)                       # [num_src, 3 * heads * out]: Q | K | V
        Q, K, V = P[:n, :W], P[:, W:2 * W], P[:, 2 * W:]
        if self.fused:
            if drop:
                Y = DotAttention.apply(Q, K, V, inputInfo, self.heads, None, self.attn_drop, _step_seed(self, rng_seed))
            else:
                Y = DotAttention.apply(Q, K, V, inputInfo, self.heads)
        else:
            rows, ci = inputInfo.edge_rows(), inputInfo.column_index
            qk = Q.index_select(0, rows) * K.index_select(0, ci)                       # [nnz, heads * out]
            z = qk.view(-1, self.heads, self.out_dim).sum(-1) / math.sqrt(self.out_dim)
            alpha = EdgeSoftmax.apply(z.t().contiguous(), inputInfo.row_pointers)      # [heads, nnz]
            if drop:
                alpha = torch.nn.functional.dropout(alpha, self.attn_drop, training=True)
            Y = EdgeWeightedAggregate.apply(V.contiguous(), alpha, inputInfo)
        if not (self.concat or self.heads == 1):
            Y = Y.view(n, self.heads, self.out_dim).mean(1)
        if self.W_skip is not None:
            Y = Y + torch.mm(X[:n] if block else X, self.W_skip)
        return Y


# ---- graph-level readout: one row per graph of a batch (batching.GraphBatch) ------------------------------------------------
POOL_MODES = ("sum", "mean", "max", "min")


def _graph_pointers_of(batch, device):
    """graph_pointers (int32 [G + 1] on `device`) of a batching.GraphBatch, or the tensor itself."""
    gp = getattr(batch, "graph_pointers", batch)
    if not isinstance(gp, torch.Tensor) or gp.dtype != torch.int32 or gp.dim() != 1 or gp.numel() < 1:
        raise TypeError("a readout takes a GraphBatch or its graph_pointers, an int32 tensor [num_graphs + 1] (an unsorted "
                        "`batch` vector is not supported: the rows of a graph must be contiguous)")
    return gp.to(device).contiguous()


class SegmentPool(Function):
    """``SegmentPool.apply(X, graph_pointers, want_sum, want_max, want_min, mean) -> (sum, max, min)``: the statistics over the rows
    [graph_pointers[g], graph_pointers[g + 1]) of X for every graph g, each [G, F], from ONE read of X (libgnna
    gnna_segment_pool_ld_f32); None for a statistic that was not asked for.  `mean` turns the sum into the mean.  A graph without
    rows gives 0.  The op saves the winning rows argmax / argmin [G, F] and graph_pointers -- nothing of the size of X.

    Backward: one pass that writes every row of dX once (libgnna gnna_segment_pool_backward_ld_f32): a row gets the gradient of its
    graph's sum (over the rows of the graph with `mean`) plus those of the max / min elements it won; ties go to the smallest row.
    The gradient of an output that was not used is not read, and nothing runs when X needs no gradient.  The same bits on every
    run.  float32 only."""

    @staticmethod
    def forward(ctx, X, graph_pointers, want_sum=True, want_max=False, want_min=False, mean=False):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("SegmentPool computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        if X.dim() != 2:
            raise ValueError(f"SegmentPool: X must be [rows, F] (got {tuple(X.shape)})")
        ctx.set_materialize_grads(False)
        gp = _graph_pointers_of(graph_pointers, X.device)
        s, mx, amx, mn, amn = GNNA.segment_pool(_laid_out(X), gp, bool(want_sum), bool(want_max), bool(want_min), bool(mean))
        ctx.save_for_backward(gp, amx, amn)
        ctx.num_rows, ctx.mean, ctx.width = X.shape[0], bool(mean), X.shape[1]
        return s, mx, mn

    @staticmethod
    def backward(ctx, d_sum, d_max, d_min):
        nothing = (None,) * 6
        if not ctx.needs_input_grad[0] or (d_sum is None and d_max is None and d_min is None):
            return nothing
        gp, amx, amn = ctx.saved_tensors
        if gp.numel() == 1:                                  # a batch without graphs: every row is a row of no graph
            return (torch.zeros(ctx.num_rows, ctx.width, dtype=torch.float32, device=gp.device),) + nothing[1:]
        dX = GNNA.segment_pool_backward(_laid_out(d_sum), _laid_out(d_max), amx if d_max is not None else None, _laid_out(d_min),
                                        amn if d_min is not None else None, gp, ctx.num_rows, ctx.mean)
        return (dX,) + nothing[1:]


def global_add_pool(X, batch):
    """[G, F]: the sum of the rows of every graph of `batch` (a batching.GraphBatch or its graph_pointers)."""
    return SegmentPool.apply(X, batch, True, False, False, False)[0]


def global_mean_pool(X, batch):
    """[G, F]: the mean of the rows of every graph; 0 for a graph without rows."""
    return SegmentPool.apply(X, batch, True, False, False, True)[0]


def global_max_pool(X, batch):
    """[G, F]: the element-wise maximum over the rows of every graph; 0 for a graph without rows."""
    return SegmentPool.apply(X, batch, False, True, False, False)[1]


def global_min_pool(X, batch):
    """[G, F]: the element-wise minimum over the rows of every graph; 0 for a graph without rows."""
    return SegmentPool.apply(X, batch, False, False, True, False)[2]


def _batch_vector(batch, device):
    """(graph_pointers as int64, G, the `batch` vector -- the graph of every row that has one --, the first such row): what the
    compositions from torch ops index by."""
    gp = _graph_pointers_of(batch, device).long()
    G = gp.numel() - 1
    rows = getattr(batch, "batch", None)
    if rows is None or rows.device != device:
        rows = torch.repeat_interleave(torch.arange(G, device=device), gp[1:] - gp[:-1])
    return gp, G, rows, int(gp[0]) if G else 0


def _composed_readout(X, batch, modes):
    """The same statistics from torch ops on the `batch` vector (index_add_, scatter_reduce): the timing baseline and a second
    opinion.  It makes an [N] index tensor (an [N, F] one for the extrema) and fills before it adds."""
    gp, G, rows, lo = _batch_vector(batch, X.device)
    counts = (gp[1:] - gp[:-1]).clamp(min=0)
    Xg = X[lo: lo + rows.numel()]                          # rows of no graph lie before the first and after the last graph
    out = []
    for mode in modes:
        if mode in ("sum", "mean"):
            s = torch.zeros(G, X.shape[1], dtype=X.dtype, device=X.device).index_add_(0, rows, Xg)
            out.append(s if mode == "sum" else s / counts.clamp(min=1).to(X.dtype).unsqueeze(1))
        else:
            idx = rows.unsqueeze(1).expand_as(Xg)
            r = torch.zeros(G, X.shape[1], dtype=X.dtype, device=X.device).scatter_reduce(0, idx, Xg, "amax" if mode == "max" else "amin",
                                                                                           include_self=False)
            out.append(r)
    return out


class Readout(Module):
    """``Readout(modes=("sum",), fused=True)(X, batch) -> [G, F * len(modes)]``: the chosen statistics -- some of "sum", "mean",
    "max", "min" -- of the rows of every graph of `batch` (a batching.GraphBatch or its graph_pointers), side by side in the order of
    `modes`.  fused=True takes all of them from ONE call of SegmentPool, one read of X ("mean" next to "sum" is the sum times
    1 / rows, [G, F] arithmetic).  fused=False is the composition from torch ops (index_add_, scatter_reduce), kept as the timing
    baseline and as a second opinion.  float32 only."""

    def __init__(self, modes=("sum",), fused=True):
        super().__init__()
        modes = (modes,) if isinstance(modes, str) else tuple(modes)
        if not modes or [m for m in modes if m not in POOL_MODES] or len(set(modes)) != len(modes):
            raise ValueError(f"modes must name some of {POOL_MODES}, each once (got {modes!r})")
        self.modes, self.fused = modes, bool(fused)

    def forward(self, X, batch):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("Readout computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        if not self.fused:
            parts = _composed_readout(X, batch, self.modes)
            return parts[0] if len(parts) == 1 else torch.cat(parts, 1)
        both = "sum" in self.modes and "mean" in self.modes
        s, mx, mn = SegmentPool.apply(X, batch, "sum" in self.modes or "mean" in self.modes, "max" in self.modes, "min" in self.modes,
                                      "mean" in self.modes and not both)
        parts = []
        for mode in self.modes:
            if mode == "mean" and both:
                gp = _graph_pointers_of(batch, X.device)
                parts.append(s * (1.0 / (gp[1:] - gp[:-1]).clamp(min=1).float()).unsqueeze(1))
            else:
                parts.append({"sum": s, "mean": s, "max": mx, "min": mn}[mode])
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)


# ---- attention readout: the softmax-weighted sum of the rows of every graph ---------------------------------------------------
def _gate_2d(X, gate, what):
    """`gate` as [N, 1] or [N, F]: a score per row ([N] or [N, 1]) or per element ([N, F])."""
    g2 = gate.unsqueeze(1) if gate.dim() == 1 else gate
    if g2.dim() != 2 or g2.shape[0] != X.shape[0] or g2.shape[1] not in (1, X.shape[1]):
        raise ValueError(f"{what}: gate must be [rows], [rows, 1] or [rows, F] for X [rows, F] = {tuple(X.shape)} "
                         f"(got {tuple(gate.shape)})")
    return g2


class SegmentAttentionPool(Function):
    """``SegmentAttentionPool.apply(X, gate, batch) -> Y [G, F]``: attention pooling over the rows of every graph of `batch` (a
    batching.GraphBatch or its graph_pointers), Y[g] = sum over the rows r of graph g of softmax_r(gate[r]) * X[r], from ONE read of
    X and of the gate (libgnna gnna_segment_attn_pool_ld_f32).  `gate` is [N] or [N, 1] (a score per row) or [N, F] (a score per
    element, a softmax per column); it may be X itself or a view of it.  A graph without rows gives 0.  Finite scores of any size
    are safe: exp is only taken of a score minus a running maximum.

    The op saves X, the gate, Y, the log-sum-exp [G, 1 or F] and graph_pointers; no alpha tensor and no [N, F] temporary exists in
    either pass.  Backward: one pass (libgnna gnna_segment_attn_pool_backward_ld_f32) that writes dX = alpha * dY[g] and
    d_gate = alpha * dY[g] * (X - Y[g]) (summed over the columns for a score per row), each only if it is needed.  The same bits on
    every run.  float32 only."""

    @staticmethod
    def forward(ctx, X, gate, graph_pointers):
        for t in (X, gate):
            if t.dtype != torch.float32 or _x16_dtype(t) is not None:
                raise TypeError("SegmentAttentionPool computes in float32 only: 16-bit features and torch.autocast are not supported "
                                f"(got {t.dtype}{', inside torch.autocast' if t.dtype == torch.float32 else ''})")
        if X.dim() != 2:
            raise ValueError(f"SegmentAttentionPool: X must be [rows, F] (got {tuple(X.shape)})")
        g2 = _gate_2d(X, gate, "SegmentAttentionPool")
        ctx.set_materialize_grads(False)
        gp = _graph_pointers_of(graph_pointers, X.device)
        Xl, gl = _laid_out(X), _laid_out(g2)
        Y, lse = GNNA.segment_attn_pool(Xl, gl, gp)
        ctx.save_for_backward(Xl, gl, Y, lse, gp)
        ctx.gate_shape = tuple(gate.shape)
        return Y

    @staticmethod
    def backward(ctx, dY):
        need_x, need_gate = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if dY is None or not (need_x or need_gate):
            return None, None, None
        X, gate, Y, lse, gp = ctx.saved_tensors
        if gp.numel() == 1:                                  # a batch without graphs: every row is a row of no graph
            return (torch.zeros_like(X) if need_x else None, torch.zeros(ctx.gate_shape, dtype=torch.float32, device=X.device)
                    if need_gate else None, None)
        dX, dG = GNNA.segment_attn_pool_backward(X, gate, lse, Y, _laid_out(dY), gp, need_x, need_gate)
        return dX, None if dG is None else dG.view(ctx.gate_shape), None


def global_attention_pool(X, gate, batch):
    """[G, F]: the rows of every graph of `batch` weighted by the softmax of `gate` ([N], [N, 1] or [N, F]) over the graph's rows;
    0 for a graph without rows."""
    return SegmentAttentionPool.apply(X, gate, batch)


def _composed_attention_readout(V, gate, batch):
    """The same readout from torch ops on the `batch` vector (scatter_reduce amax, exp, index_add_, a division, a product,
    index_add_): the timing baseline and a second opinion.  It makes several [N, F]-sized temporaries."""
    gp, G, rows, lo = _batch_vector(batch, V.device)
    g2 = _gate_2d(V, gate, "AttentionalReadout")
    Vg, sg = V[lo: lo + rows.numel()], g2[lo: lo + rows.numel()]
    m = torch.full((G, sg.shape[1]), float("-inf"), dtype=V.dtype, device=V.device)
    m = m.scatter_reduce(0, rows.unsqueeze(1).expand_as(sg), sg.detach(), "amax", include_self=True)
    e = torch.exp(sg - m[rows])
    l = torch.zeros(G, sg.shape[1], dtype=V.dtype, device=V.device).index_add_(0, rows, e)
    return torch.zeros(G, V.shape[1], dtype=V.dtype, device=V.device).index_add_(0, rows, (e / l[rows]) * Vg)


class AttentionalReadout(Module):
    """``AttentionalReadout(gate_nn, nn=None, fused=True)(X, batch) -> [G, F']``: the learned readout of gated graph networks
    (PyG's GlobalAttention / AttentionalAggregation): gate = gate_nn(X), one score per row ([N, 1]) or per element ([N, F']);
    V = nn(X) if `nn` is given, else X; Y[g] = sum over the rows r of graph g of softmax_r(gate[r]) * V[r].  fused=True is ONE call
    of SegmentAttentionPool: one read of V and of the gate, no alpha tensor.  fused=False is the composition from torch ops
    (scatter_reduce, exp, index_add_), kept as the timing baseline and as a second opinion.  float32 only."""

    def __init__(self, gate_nn, nn=None, fused=True):
        super().__init__()
        self.gate_nn, self.nn, self.fused = gate_nn, nn, bool(fused)

    def forward(self, X, batch):
        if X.dtype != torch.float32 or _x16_dtype(X) is not None:
            raise TypeError("AttentionalReadout computes in float32 only: 16-bit features and torch.autocast are not supported "
                            f"(got {X.dtype}{', inside torch.autocast' if X.dtype == torch.float32 else ''})")
        gate = self.gate_nn(X)
        V = X if self.nn is None else self.nn(X)
        if not self.fused:
            return _composed_attention_readout(V, gate, batch)
        return SegmentAttentionPool.apply(V, gate, batch)


# ---- hierarchical pooling: the best-scoring rows of every graph, the induced sub-batch, and the way back ----------------------
def _f32_only(t, who):
    if t.dtype != torch.float32 or _x16_dtype(t) is not None:
        raise TypeError(f"{who} computes in float32 only: 16-bit features and torch.autocast are not supported "
                        f"(got {t.dtype}{', inside torch.autocast' if t.dtype == torch.float32 else ''})")


class SelectRows(Function):
    """``SelectRows.apply(X, scale, selection) -> X' [N', F]``: the rows a ``GraphBatch.coarsen`` kept, X'[i] = scale[perm[i]] *
    X[perm[i]] (libgnna gnna_gather_rows_scale_ld_f32, one pass, one multiplication per element); `scale` is a float32 [N] or
    None (a plain gather), `selection` the TopKSelection of coarsen.

    Backward: one pass over the rows of X (libgnna gnna_gather_rows_scale_backward_ld_f32) that writes every element of dX =
    scale * dX'[new_id] and of d_scale = <dX'[new_id], X> once, zeros for the rows that were dropped -- no zero-fill, no
    index_add_.  The op saves new_id [N], X only when scale needs a gradient and scale only when X does: nothing of the size of X
    beyond X itself.  The same bits on every run.  float32 only."""

    @staticmethod
    def forward(ctx, X, scale, selection):
        _f32_only(X, "SelectRows")
        if X.dim() != 2 or X.shape[0] != selection.num_nodes:
            raise ValueError(f"SelectRows: X must be [{selection.num_nodes}, F] (got {tuple(X.shape)})")
        if scale is not None:
            _f32_only(scale, "SelectRows")
            if scale.numel() != X.shape[0]:
                raise ValueError(f"SelectRows: scale must hold one factor per row of X ({X.shape[0]}; got {tuple(scale.shape)})")
        ctx.scale_shape = None if scale is None else tuple(scale.shape)
        if scale is not None:
            scale = _packed(scale.reshape(-1))
        ctx.set_materialize_grads(False)
        Xl = _laid_out(X)
        need_x, need_scale = ctx.needs_input_grad[0], scale is not None and ctx.needs_input_grad[1]
        ctx.save_for_backward(selection.new_id, Xl if need_scale else None, scale if need_x else None)
        return GNNA.gather_rows_scale(Xl, selection.perm, scale)

    @staticmethod
    def backward(ctx, dY):
        need_x, need_scale = ctx.needs_input_grad[0], ctx.scale_shape is not None and ctx.needs_input_grad[1]
        if dY is None or not (need_x or need_scale):
            return None, None, None
        new_id, X, scale = ctx.saved_tensors
        dX, dS = GNNA.gather_rows_scale_backward(_laid_out(dY), new_id, X, scale, need_x, need_scale)
        return dX, None if dS is None else dS.view(ctx.scale_shape), None


class UnpoolRows(Function):
    """``UnpoolRows.apply(X_small, selection) -> [N, F]``: the rows of X_small back at the rows they were selected from, zeros
    elsewhere (the unpooling of a Graph U-Net), in the one pass of gnna_gather_rows_scale_backward_ld_f32 without a zero-fill;
    the backward is the plain gather."""

    @staticmethod
    def forward(ctx, X_small, selection):
        _f32_only(X_small, "unpool")
        if X_small.dim() != 2 or X_small.shape[0] != selection.perm.numel():
            raise ValueError(f"unpool: X_small must be [{selection.perm.numel()}, F] (got {tuple(X_small.shape)})")
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(selection.perm)
        return GNNA.gather_rows_scale_backward(_laid_out(X_small), selection.new_id, None, None, True, False)[0]

    @staticmethod
    def backward(ctx, dY):
        if dY is None or not ctx.needs_input_grad[0]:
            return None, None
        perm, = ctx.saved_tensors
        return GNNA.gather_rows_scale(_laid_out(dY), perm, None), None


def unpool(X_small, selection):
    """[N, F]: the rows of `X_small` [N', F] placed back at the rows `selection` (GraphBatch.coarsen) took them from, zeros for
    the rows that were dropped."""
    return UnpoolRows.apply(X_small, selection)


def _order_key(score):
    """int64 [N]: keys that order like the float32 `score` in the library's total order (-0 below +0, a NaN with a clear sign bit
    above +inf, one with the sign bit set below -inf) -- gnna_keys.h from torch ops."""
    b = score.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b + 0x80000000)


def _composed_coarsen(batch, score, ratio=None, k=None):
    """``GraphBatch.coarsen`` from torch ops, the same rows under the same tie rule: two stable sorts over the whole batch (by
    key, then by graph), boolean masks over the rows and the edges, cumulative sums for the new ids and row pointers, and the
    partition built again from the new row pointers.  The timing baseline and a second opinion; graph_pointers must ascend."""
    from .batching import GraphBatch, TopKSelection
    if (ratio is None) == (k is None):
        raise ValueError("coarsen takes exactly one of ratio and k")
    dev, N = score.device, batch.num_nodes
    gp, G, rows, lo = _batch_vector(batch, dev)
    sizes = (gp[1:] - gp[:-1]).clamp(min=0)
    if k is not None:
        keep_n = sizes.clamp(max=int(k))
    else:
        keep_n = torch.minimum(sizes, torch.ceil(float(ratio) * sizes.double()).long())
    key = _order_key(score.detach().reshape(-1))[lo: lo + rows.numel()]
    by_key = torch.sort(key, descending=True, stable=True).indices            # equal keys stay in row order
    by_graph = torch.sort(rows[by_key], stable=True).indices                   # then graph by graph, best first
    order = by_key[by_graph]
    g_sorted = rows[order]
    rank = torch.arange(order.numel(), device=dev) - (gp[:-1] - lo)[g_sorted]
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    mask[lo + order[rank < keep_n[g_sorted]]] = True
    perm = mask.nonzero().reshape(-1)
    new_id = torch.where(mask, torch.cumsum(mask, 0) - 1, torch.full((N,), -1, dtype=torch.int64, device=dev))
    new_gp = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    new_gp[1:] = torch.cumsum(keep_n, 0)
    e_rows, ci = batch.edge_rows().long(), batch.column_index.long()
    inside = (ci >= 0) & (ci < N)
    alive = mask[e_rows] & inside & mask[ci.clamp(0, max(N - 1, 0))] if N > 0 else torch.zeros_like(inside)
    edge_ids = alive.nonzero().reshape(-1)
    new_ci = new_id[ci[edge_ids]]
    counts = torch.zeros(perm.numel(), dtype=torch.int64, device=dev).index_add_(0, new_id[e_rows[edge_ids]], torch.ones_like(edge_ids))
    new_rp = torch.zeros(perm.numel() + 1, dtype=torch.int64, device=dev)
    new_rp[1:] = torch.cumsum(counts, 0)
    small = GraphBatch(new_rp.to(torch.int32), new_ci.to(torch.int32), new_gp.to(torch.int32), partSize=batch.partSize,
                       dimWorker=batch.dimWorker, warpPerBlock=batch.warpPerBlock, directed=batch.directed)
    return small, TopKSelection(perm.to(torch.int32), new_id.to(torch.int32), edge_ids.to(torch.int32), N)


_GATES = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, None: None}


class _ScorePooling(Module):
    """What TopKPooling and SAGPooling share: the gate, the selection and the scaled gather, fused or composed."""

    def __init__(self, ratio, k, multiplier, nonlinearity, fused):
        super().__init__()
        if nonlinearity not in _GATES:
            raise ValueError(f"nonlinearity must be \"tanh\", \"sigmoid\" or None (got {nonlinearity!r})")
        if k is None and not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f"ratio must be in (0, 1] (got {ratio!r})")
        if k is not None and int(k) < 1:
            raise ValueError(f"k must be >= 1 (got {k!r})")
        self.ratio, self.k = (None if k is not None else float(ratio)), (None if k is None else int(k))
        self.multiplier, self.nonlinearity, self.fused = float(multiplier), nonlinearity, bool(fused)

    def _pool(self, X, score, batch):
        gate = score if self.nonlinearity is None else _GATES[self.nonlinearity](score)
        scale = gate if self.multiplier == 1.0 else self.multiplier * gate
        carries = getattr(batch, "edge_attr", None) is not None        # edge features follow the coarsening (edgeconv.GINEConv, CFConv)
        if self.fused:
            small, sel = batch.coarsen(score, ratio=self.ratio, k=self.k, want_edge_ids=carries)
            if carries:
                batch.carry_edge_attr(small, sel)
            perm = sel.perm.long()
            return SelectRows.apply(X, scale, sel), small, sel, gate[perm]
        small, sel = _composed_coarsen(batch, score, ratio=self.ratio, k=self.k)
        if carries:
            batch.carry_edge_attr(small, sel)
        perm = sel.perm.long()
        return scale[perm].unsqueeze(1) * X[perm], small, sel, gate[perm]


class TopKPooling(_ScorePooling):
    """``TopKPooling(in_channels, ratio=0.5, k=None, multiplier=1.0, nonlinearity="tanh", fused=True)(X, batch) -> (X', new_batch,
    selection, gate[perm])``: the top-k pooling of Graph U-Nets on a batching.GraphBatch.  score = (X @ w) / ||w|| with a learned
    w [in_channels]; every graph keeps its min(n, ceil(ratio * n)) -- or min(n, k) -- best-scoring rows (the library's total order,
    ties to the smaller row, rows kept in row order); gate = nonlinearity(score) ("tanh", "sigmoid" or None) and X' = multiplier *
    gate[perm] * X[perm].  The rows are chosen by the score itself, which a monotone gate orders alike but for the ties its
    saturation makes.  The score and the gate are node-sized torch arithmetic.  fused=True: ONE library call builds the coarsened
    batch on the device (GraphBatch.coarsen) and SelectRows gathers and scales in one pass, with a one-pass backward.  fused=False
    is the same function composed from torch ops (sorts, masks, index_add_, a partition built again), kept as the timing baseline
    and as a second opinion; it selects the same rows.  float32 only."""

    def __init__(self, in_channels, ratio=0.5, k=None, multiplier=1.0, nonlinearity="tanh", fused=True):
        super().__init__(ratio, k, multiplier, nonlinearity, fused)
        self.weight = Parameter(torch.empty(int(in_channels)))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.weight.numel())
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)

    def forward(self, X, batch):
        _f32_only(X, "TopKPooling")
        # (a one-row linear map, not torch.mv: rocBLAS's gemv takes 25 ms for the weight gradient of 2.6 M rows of 64 floats where
        # the GEMM path takes 2.5 -- profiles/topk_pool/README.md)
        score = torch.nn.functional.linear(X, self.weight.unsqueeze(0)).reshape(-1) / self.weight.norm(p=2)
        return self._pool(X, score, batch)


class SAGPooling(_ScorePooling):
    """``SAGPooling(in_channels, ratio=0.5, k=None, GNN=GCNConv, nonlinearity="tanh", fused=True)(X, batch) -> (X', new_batch,
    selection, gate[perm])``: self-attention graph pooling -- TopKPooling whose score comes from one conv layer of the library at
    output width 1 on the batch, ``GNN(in_channels, 1)(X, batch)``; X' = gate[perm] * X[perm].  fused as in TopKPooling."""

    def __init__(self, in_channels, ratio=0.5, k=None, GNN=GCNConv, nonlinearity="tanh", fused=True):
        super().__init__(ratio, k, 1.0, nonlinearity, fused)
        self.gnn = GNN(int(in_channels), 1)

    def forward(self, X, batch):
        _f32_only(X, "SAGPooling")
        return self._pool(X, self.gnn(X, batch).reshape(-1), batch)


# ---- per-graph normalisation: GraphNorm on a batch of graphs -------------------------------------------------------------------
def _norm_param(t, F, device, what):
    """A per-column parameter as the library takes it: float32 [F] on `device`, contiguous; None stays None (the default)."""
    if t is None:
        return None
    if t.dtype != torch.float32 or tuple(t.shape) != (F,) or t.device != device:
        raise ValueError(f"{what} must be a float32 tensor [{F}] on {device} (got {t.dtype} {tuple(t.shape)} on {t.device})")
    return t.contiguous()


class SegmentNorm(Function):
    """``SegmentNorm.apply(X, graph_pointers, weight, bias, alpha, eps) -> Y like X``: per-graph normalisation (GraphNorm).  Over
    the rows of graph g (n rows), per column: mean, var = (1/n) sum (x - alpha mean)^2, Y = weight (x - alpha mean) /
    sqrt(var + eps) + bias (libgnna gnna_segment_norm_ld_f32: one read of X for the centred moments -- merged pairwise, never from
    sums of x^2 --, one more for the rows).  weight / bias / alpha are [F] or None for 1 / 0 / 1; a row of no graph gets 0, a
    one-row graph with alpha = 1 gives bias.  The op saves X, mean and rstd [G, F], the parameters and graph_pointers -- nothing
    else of the size of X.

    Backward: one pass over dY and X for A = sum dY and B = sum dY xhat per graph, one pass that writes every row of dX once
    (libgnna gnna_segment_norm_backward_ld_f32; skipped when X needs no gradient); the parameter gradients are [G, F] arithmetic on
    A, B, mean and rstd.  The same bits on every run.  float32 only."""

    @staticmethod
    def forward(ctx, X, graph_pointers, weight=None, bias=None, alpha=None, eps=1e-5):
        _f32_only(X, "SegmentNorm")
        if X.dim() != 2:
            raise ValueError(f"SegmentNorm: X must be [rows, F] (got {tuple(X.shape)})")
        if not (float(eps) > 0.0 and math.isfinite(float(eps))):
            raise ValueError(f"SegmentNorm: eps must be finite and > 0 (got {eps!r})")
        gp = _graph_pointers_of(graph_pointers, X.device)
        F = X.shape[1]
        w, b, a = (_norm_param(t, F, X.device, name) for t, name in ((weight, "weight"), (bias, "bias"), (alpha, "alpha")))
        Xl = _laid_out(X)
        Y, mean, rstd = GNNA.segment_norm(Xl, gp, w, b, a, float(eps))
        ctx.save_for_backward(Xl, mean, rstd, gp, *(t for t in (w, a) if t is not None))
        ctx.has_weight, ctx.has_alpha = w is not None, a is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        need_x, need_w, need_b, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        if not (need_x or need_w or need_b or need_a):
            return (None,) * 6
        X, mean, rstd, gp = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        w = rest.pop(0) if ctx.has_weight else None
        a = rest.pop(0) if ctx.has_alpha else None
        dX, A, B = GNNA.segment_norm_backward(_laid_out(dY), X, mean, rstd, gp, w, a, bool(need_x))
        dW = B.sum(0) if need_w else None
        dB = A.sum(0) if need_b else None
        dA = None
        if need_a:
            mr = mean * rstd
            t = mr * (A - (1.0 - a) * mr * B)
            dA = -(t if w is None else t * w).sum(0)
        return dX, None, dW, dB, dA, None


def _composed_graph_norm(X, batch, weight, bias, alpha, eps):
    """The same function from torch ops on the `batch` vector (index_add_, indexing, a division, a square root): the timing
    baseline and a second opinion.  It makes several [N, F]-sized temporaries."""
    gp, G, rows, lo = _batch_vector(batch, X.device)
    n = rows.numel()
    Xg = X[lo: lo + n]
    cnt = (gp[1:] - gp[:-1]).clamp(min=1).to(X.dtype).unsqueeze(1)
    mean = torch.zeros(G, X.shape[1], dtype=X.dtype, device=X.device).index_add_(0, rows, Xg) / cnt
    xc = Xg - (mean if alpha is None else alpha * mean)[rows]
    var = torch.zeros(G, X.shape[1], dtype=X.dtype, device=X.device).index_add_(0, rows, xc * xc) / cnt
    y = xc / torch.sqrt(var + eps)[rows]
    if weight is not None:
        y = y * weight
    if bias is not None:
        y = y + bias
    return torch.nn.functional.pad(y, (0, 0, lo, X.shape[0] - lo - n))          # rows of no graph get 0


def graph_norm(x, batch, weight=None, bias=None, mean_scale=None, eps=1e-5):
    """GraphNorm of the rows of every graph of `batch` (a batching.GraphBatch or its graph_pointers), one fused call:
    weight * (x - mean_scale * mean) / sqrt(var + eps) + bias with the mean and the variance of (x - mean_scale * mean) per graph and
    column; weight / bias / mean_scale are [F] or None for 1 / 0 / 1 (mean_scale=None: instance normalisation)."""
    return SegmentNorm.apply(x, batch, weight, bias, mean_scale, eps)


class GraphNorm(Module):
    """``GraphNorm(channels, eps=1e-5, mean_scale=True, affine=True, fused=True)(x, batch) -> like x``: the normalisation of GraphNorm
    (Cai et al., ICML 2021; PyG's nn.GraphNorm) on a batching.GraphBatch or its graph_pointers: per graph and column,
    weight * (x - mean_scale * mean) / sqrt(var + eps) + bias, var the variance of (x - mean_scale * mean).  Parameters `weight`
    (ones), `bias` (zeros) and `mean_scale` (ones): PyG's names and initial values.  mean_scale=False fixes the scale of the mean at 1
    (PyG's InstanceNorm on a batch), affine=False leaves weight and bias out.  There are no running statistics: training and
    evaluation compute the same function.  fused=True is ONE call of SegmentNorm; fused=False composes the same function from
    torch ops on the `batch` vector, kept as the timing baseline and as a second opinion.  float32 only."""

    def __init__(self, channels, eps=1e-5, mean_scale=True, affine=True, fused=True):
        super().__init__()
        if not (float(eps) > 0.0 and math.isfinite(float(eps))):
            raise ValueError(f"eps must be finite and > 0 (got {eps!r})")
        self.channels, self.eps, self.fused = int(channels), float(eps), bool(fused)
        self.weight = Parameter(torch.ones(self.channels)) if affine else None
        self.bias = Parameter(torch.zeros(self.channels)) if affine else None
        self.mean_scale = Parameter(torch.ones(self.channels)) if mean_scale else None

    def reset_parameters(self):
        with torch.no_grad():
            for t, v in ((self.weight, 1.0), (self.bias, 0.0), (self.mean_scale, 1.0)):
                if t is not None:
                    t.fill_(v)

    def forward(self, x, batch):
        _f32_only(x, "GraphNorm")
        if x.dim() != 2 or x.shape[1] != self.channels:
            raise ValueError(f"GraphNorm({self.channels}): x must be [rows, {self.channels}] (got {tuple(x.shape)})")
        if not self.fused:
            return _composed_graph_norm(x, batch, self.weight, self.bias, self.mean_scale, self.eps)
        return SegmentNorm.apply(x, batch, self.weight, self.bias, self.mean_scale, self.eps)

"""``GATAttentionRows``: the fused GAT attention by kernels that own the rows they write (include/gnna_gat_rows.h).  Re-exported as
``ops.GATAttentionRows``; ``ops.GATConv(..., fused="rows")`` runs on it."""
import torch
from torch.autograd import Function

from .structure import backward_structure


class GATAttentionRows(Function):
    """GATAttention by kernels that own the rows they write (libgnna gnna_gat_forward_rows_f32 / gnna_gat_backward_rows_f32,
    include/gnna_gat_rows.h): ``GATAttentionRows.apply(H, el, er, inputInfo, negative_slope) -> Y``, the same function and the
    same saved tensors (H, el, er, lse, Y -- all node-sized).  No partition is read, nothing is added with atomics and the order
    of every sum is fixed by the structure: two runs give the same bits, and the calls are accepted under
    ``_lib.set_tuning(deterministic=1)``, which GATAttention's are not.  The forward makes the softmax online, in ONE pass over
    column_index.  Full graphs, ``directed`` graphs and sampling.SampledBlocks as GATAttention: the backward's source-side pass
    walks ``structure.backward_structure`` (the structure itself once it is established to be symmetric, else the transposed one).
    No attention dropout and no per-edge score term: those stay on GATAttention / GATEdgeAttention."""

    @staticmethod
    def forward(ctx, H, el, er, inputInfo, negative_slope):
        info = inputInfo
        if _ops._is_block(info):
            H = _ops._block_features(H, info, "GATAttentionRows")
            if er.dim() != 2 or er.shape[0] != info.num_src or el.dim() != 2 or el.shape[0] != info.num_dst or \
                    el.shape[1] != er.shape[1]:
                raise ValueError(f"GATAttentionRows on a SampledBlock: el must be [num_dst = {info.num_dst}, heads] and er "
                                 f"[num_src = {info.num_src}, heads] (got {tuple(el.shape)} and {tuple(er.shape)})")
        if any(t.dtype != torch.float32 for t in (H, el, er)):
            raise TypeError(f"GATAttentionRows: float32 only (got {H.dtype}, {el.dtype}, {er.dtype})")
        el, er = _ops._packed(el), _ops._packed(er)
        Y, lse = _ops.GNNA.gat_forward_rows(H, el, er, info.row_pointers, info.column_index, float(negative_slope))
        ctx.info, ctx.negative_slope = info, float(negative_slope)
        ctx.save_for_backward(H, el, er, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        H, el, er, lse, Y = ctx.saved_tensors
        info = ctx.info
        need = list(ctx.needs_input_grad[:3])
        if not any(need):
            return _ops._grads(ctx)
        t = backward_structure(info, require_symmetric=True)
        return _ops._grads(ctx, _ops.GNNA.gat_backward_rows(H, el, er, lse, Y, dY, info.row_pointers, info.column_index,
                                                            t.row_pointers, t.column_index, ctx.negative_slope, need))


from . import ops as _ops  # noqa: E402  (at the end: ops imports this module at its own end, whichever of the two is imported first)

"""``GATv2AttentionRows``: the fused GATv2 attention by kernels that own the rows they write (include/gnna_gatv2_rows.h).
Re-exported as ``ops.GATv2AttentionRows``; ``ops.GATv2Conv(..., fused="rows")`` runs on it."""
import torch
from torch.autograd import Function

from .structure import backward_structure


class GATv2AttentionRows(Function):
    """GATv2Attention by kernels that own the rows they write (libgnna gnna_gatv2_forward_rows_f32 /
    gnna_gatv2_backward_rows_f32, include/gnna_gatv2_rows.h):
    ``GATv2AttentionRows.apply(Hs, Hd, att, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0) -> Y``, the same function, the
    same mask rule (the two drop the same edges for the same seed) and the same saved tensors (Hs, Hd, att, lse, Y -- all
    node-sized).  No partition is read, nothing is added with atomics -- the gradient of att included, which is summed from one
    partial per workgroup in a fixed order -- and the order of every sum is fixed by the structure: two runs give the same bits,
    and the calls are accepted under ``_lib.set_tuning(deterministic=1)``, which GATv2Attention's are not.  The forward makes the
    softmax online, in ONE pass that gathers Hs once per edge.  Full graphs, ``directed`` graphs and sampling.SampledBlocks as
    GATv2Attention: the backward's source-side pass walks ``structure.backward_structure`` (the structure itself once it is
    established to be symmetric, else the transposed one), and only the gradients that are needed are made.  Hs and Hd may be the
    same tensor (shared weights): autograd adds the two gradients."""

    @staticmethod
    def forward(ctx, Hs, Hd, att, inputInfo, negative_slope, attn_drop=0.0, rng_seed=0):
        info = inputInfo
        attn_drop, rng_seed = _ops._drop_args("GATv2AttentionRows", attn_drop, rng_seed)
        for t, name in ((Hs, "Hs"), (Hd, "Hd"), (att, "att")):
            if t.dtype != torch.float32:
                raise TypeError(f"GATv2AttentionRows: float32 only (got {name}: {t.dtype})")
        if att.dim() != 2 or Hs.dim() != 2 or Hd.dim() != 2 or Hs.shape[1] != Hd.shape[1] or att.numel() != Hs.shape[1]:
            raise ValueError(f"GATv2AttentionRows: Hs [num_src, heads * F], Hd [num_dst, heads * F] and att [heads, F] expected (got "
                             f"{tuple(Hs.shape)}, {tuple(Hd.shape)} and {tuple(att.shape)})")
        if _ops._is_block(info):
            Hs = _ops._block_features(Hs, info, "GATv2AttentionRows")
            if Hd.shape[0] != info.num_dst:
                raise ValueError(f"GATv2AttentionRows on a SampledBlock: Hd must be [num_dst = {info.num_dst}, heads * F] "
                                 f"(got {tuple(Hd.shape)})")
        att = _ops._packed(att)
        Y, lse = _ops.GNNA.gatv2_forward_rows(Hs, Hd, att, info.row_pointers, info.column_index, float(negative_slope), attn_drop,
                                              rng_seed)
        ctx.info, ctx.negative_slope, ctx.attn_drop, ctx.rng_seed = info, float(negative_slope), attn_drop, rng_seed
        ctx.save_for_backward(Hs, Hd, att, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        Hs, Hd, att, lse, Y = ctx.saved_tensors
        info = ctx.info
        need = list(ctx.needs_input_grad[:3])
        if not any(need):
            return _ops._grads(ctx)
        t = backward_structure(info, require_symmetric=True)
        return _ops._grads(ctx, _ops.GNNA.gatv2_backward_rows(Hs, Hd, att, lse, Y, dY, info.row_pointers, info.column_index,
                                                              t.row_pointers, t.column_index, ctx.negative_slope, ctx.attn_drop,
                                                              ctx.rng_seed, need))


from . import ops as _ops  # noqa: E402  (at the end: ops imports this module at its own end, whichever of the two is imported first)

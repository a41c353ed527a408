"""``DotAttentionRows``: the fused dot-product graph attention by kernels that own the rows they write (include/gnna_dot_rows.h).
Re-exported as ``ops.DotAttentionRows``; ``ops.TransformerConv(..., fused="rows")`` runs on it."""
import math

import torch
from torch.autograd import Function

from .structure import backward_structure


class DotAttentionRows(Function):
    """DotAttention by kernels that own the rows they write (libgnna gnna_dot_attn_forward_rows_f32 /
    gnna_dot_attn_backward_rows_f32, include/gnna_dot_rows.h):
    ``DotAttentionRows.apply(Q, K, V, inputInfo, heads, scale=None, attn_drop=0.0, rng_seed=0) -> Y``, the same function, the same
    mask rule (the two drop the same edges for the same seed) and the same saved tensors (Q, K, V, lse, Y -- all node-sized, the
    slices as they came).  No partition is read, nothing is added with atomics and the order of every sum is fixed by the
    structure: two runs give the same bits, and the calls are accepted under ``_lib.set_tuning(deterministic=1)``, which
    DotAttention's are not.  The forward makes the softmax online, in ONE pass that gathers K and V once each.  Full graphs,
    ``directed`` graphs and sampling.SampledBlocks as DotAttention: the backward's source-side pass walks
    ``structure.backward_structure`` (the structure itself once it is established to be symmetric, else the transposed one), and
    only the gradients that are needed are made."""

    @staticmethod
    def forward(ctx, Q, K, V, inputInfo, heads, scale=None, attn_drop=0.0, rng_seed=0):
        info = inputInfo
        heads = int(heads)
        attn_drop, rng_seed = _ops._drop_args("DotAttentionRows", attn_drop, rng_seed)
        # float32, or all three bfloat16 / all three float16 (the x16 entries: fp32 accumulation, Y and the gradients in that dtype)
        x16 = Q.dtype in _ops._X16
        for t, name in ((Q, "Q"), (K, "K"), (V, "V")):
            if t.dtype != (Q.dtype if x16 else torch.float32):
                raise TypeError(f"DotAttentionRows: float32, or Q, K and V all bfloat16 or all float16 (got {name}: {t.dtype}"
                                f"{', Q: ' + str(Q.dtype) if x16 else ''})")
        if Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or K.shape[1] != Q.shape[1] or V.shape != K.shape or heads < 1 or \
                Q.shape[1] % heads != 0:
            raise ValueError(f"DotAttentionRows: Q [num_dst, heads * F], K and V [num_src, heads * F] with heads = {heads} expected "
                             f"(got {tuple(Q.shape)}, {tuple(K.shape)} and {tuple(V.shape)})")
        scale = 1.0 / math.sqrt(Q.shape[1] // heads) if scale is None else float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"DotAttentionRows: scale must be finite (got {scale})")
        if _ops._is_block(info):
            K = _ops._block_features(K, info, "DotAttentionRows", x16)
            if V.shape[0] != info.num_src or Q.shape[0] != info.num_dst:
                raise ValueError(f"DotAttentionRows on a SampledBlock: Q must be [num_dst = {info.num_dst}, heads * F] and V "
                                 f"[num_src = {info.num_src}, heads * F] (got {tuple(Q.shape)} and {tuple(V.shape)})")
        forward = _ops.GNNA.dot_attn_forward_rows_x16 if x16 else _ops.GNNA.dot_attn_forward_rows
        Y, lse = forward(Q, K, V, heads, info.row_pointers, info.column_index, scale, attn_drop, rng_seed)      # (lse: float32)
        ctx.info, ctx.heads, ctx.scale, ctx.attn_drop, ctx.rng_seed = info, heads, scale, attn_drop, rng_seed
        ctx.save_for_backward(Q, K, V, lse, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        Q, K, V, lse, Y = ctx.saved_tensors
        info = ctx.info
        need = list(ctx.needs_input_grad[:3])
        if not any(need):
            return _ops._grads(ctx)
        t = backward_structure(info, require_symmetric=True)
        backward = _ops.GNNA.dot_attn_backward_rows_x16 if Q.dtype in _ops._X16 else _ops.GNNA.dot_attn_backward_rows
        return _ops._grads(ctx, backward(Q, K, V, ctx.heads, lse, Y, dY.to(Q.dtype), info.row_pointers, info.column_index,
                                         t.row_pointers, t.column_index, ctx.scale, ctx.attn_drop, ctx.rng_seed, need))


from . import ops as _ops  # noqa: E402  (at the end: ops imports this module at its own end, whichever of the two is imported first)

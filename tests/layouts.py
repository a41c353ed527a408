"""Strided layouts of operands and of incoming gradients for the autograd Functions of ops.py (checker side only: plain torch,
no library call; runs on whatever device its tensors are on).

``relayout(t, kind)`` returns a tensor equal in value to the 2-D ``t`` with the strides of ``kind`` ([n, W] elements):

    contiguous      (W, 1)      as given (the control)
    column_block    (W + 3, 1)  columns [1, 1 + W) of a NaN-filled [n, W + 3] buffer: a leading dimension, rows that start off
                                a 16-byte boundary, and padding a kernel must neither read into its result nor write
    column_major    (1, n)      as given (``lin.weight.t()``; a product with a column-major operand)
    inner_stride_2  (2 W, 2)    as given (every other element of a [n, 2 W] buffer whose other elements are NaN)
    row_broadcast   (0, 1)      every row equal to row 0 of t (``emb.expand(n, F)``; the gradient of a sum readout): the caller
                                gives the reference ``materialised(t, kind)``
    full_broadcast  (0, 0)      every element equal to t[0, 0] (the gradient of ``Y.sum()``)

An [n, 1] operand takes the same kinds ((1, 1), (4, 1), (2, 2), (0, 1), (0, 0); column_major does not differ from contiguous
there).  A 1-D operand takes ``contiguous`` and ``inner_stride_2`` (every other element), a 1-D gradient also ``full_broadcast``
((0,), the gradient of a sum); a [heads, nnz] operand is 2-D: its ``column_major`` is the transposed (edge-major) form.

``grad_layout(Y, kind)`` is the identity whose backward hands ``relayout(dZ, kind)`` on, so that the Function that made Y receives
that layout as its incoming gradient.  The two broadcast kinds are made the way models make them (``layout_loss``)."""
import torch
from torch.autograd import Function

KINDS = ("contiguous", "column_block", "column_major", "inner_stride_2", "row_broadcast", "full_broadcast")
PAD = 3                     # columns a column_block buffer is wider by; the block starts at column 1


def expected_strides(shape, kind):
    """The strides ``relayout`` gives a tensor of `shape` (1-D or 2-D)."""
    if len(shape) == 1:
        return {"contiguous": (1,), "inner_stride_2": (2,), "full_broadcast": (0,)}[kind]
    n, W = shape
    return {"contiguous": (W, 1), "column_block": (W + PAD, 1), "column_major": (1, n), "inner_stride_2": (2 * W, 2),
            "row_broadcast": (0, 1), "full_broadcast": (0, 0)}[kind]


def kinds_for(t):
    """The kinds that differ from one another for an operand of t's shape."""
    if t.dim() == 1:
        return ("contiguous", "inner_stride_2")
    if t.shape[1] == 1:
        return tuple(k for k in KINDS if k != "column_major")
    return KINDS


def materialised(t, kind):
    """A contiguous tensor with the values ``relayout(t, kind)`` has: what the reference is evaluated on."""
    if kind == "row_broadcast":
        return t[:1].expand_as(t).contiguous()
    if kind == "full_broadcast":
        return (t[:1] if t.dim() == 1 else t[:1, :1]).expand_as(t).contiguous()
    return t.contiguous()


def relayout(t, kind, keep=None):
    """`t` (1-D or 2-D) in the layout `kind`.  keep: a list that receives the NaN-padded buffer of a ``column_block`` or
    ``inner_stride_2`` result, for ``padding_intact``."""
    t = t.detach()
    nan = float("nan")
    if t.dim() == 1:
        if kind == "contiguous":
            out = t.contiguous().clone()
        elif kind == "inner_stride_2":
            buf = torch.full((2 * t.numel(),), nan, dtype=t.dtype, device=t.device)
            out = buf[::2]
            out.copy_(t)
            if keep is not None:
                keep.append((buf, out))
        elif kind == "full_broadcast":
            out = t[0].clone().expand(t.numel())
        else:
            raise ValueError(f"a 1-D operand has no layout {kind!r}")
    else:
        n, W = t.shape
        if kind == "contiguous":
            out = t.contiguous().clone()
        elif kind == "column_block":
            buf = torch.full((n, W + PAD), nan, dtype=t.dtype, device=t.device)
            out = buf[:, 1:1 + W]
            out.copy_(t)
            if keep is not None:
                keep.append((buf, out))
        elif kind == "column_major":
            out = t.t().contiguous().clone().t()
        elif kind == "inner_stride_2":
            buf = torch.full((n, 2 * W), nan, dtype=t.dtype, device=t.device)
            out = buf[:, ::2]
            out.copy_(t)
            if keep is not None:
                keep.append((buf, out))
        elif kind == "row_broadcast":
            out = t[0].contiguous().clone().unsqueeze(0).expand(n, W)
        elif kind == "full_broadcast":
            out = t[0, 0].clone().expand(n, W)
        else:
            raise ValueError(f"unknown layout {kind!r}")
    # (sizes of 1 leave a stride free: as_strided pins it, the memory read is the same)
    want = expected_strides(tuple(t.shape), kind)
    if tuple(out.stride()) != want:
        out = out.as_strided(out.shape, want, out.storage_offset())
    return out


def padding_intact(kept):
    """Every element of the kept buffers outside the view is still NaN, and the view itself holds none."""
    for buf, view in kept:
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
        inside_view = inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset())
        inside_view.fill_(True)
        if not bool(torch.isnan(buf[~inside]).all()) or bool(torch.isnan(buf[inside]).any()):
            return False
    return True


class _GradLayout(Function):
    @staticmethod
    def forward(ctx, Y, kind, keep):
        ctx.kind, ctx.keep = kind, keep
        return Y.view_as(Y)

    @staticmethod
    def backward(ctx, dZ):
        return relayout(dZ, ctx.kind, ctx.keep), None, None


def grad_layout(Y, kind, keep=None):
    """Y itself; in the backward pass, the gradient that reaches whatever made Y has the layout `kind` (and dZ's values for the
    kinds that are no broadcast)."""
    return _GradLayout.apply(Y, kind, keep)


def record_arrival(Y, into):
    """A tensor hook on Y that appends the strides of the gradient that arrives for it."""
    Y.register_hook(lambda g: into.append(tuple(g.stride())))


def layout_loss(Y, kind, wgt, keep=None):
    """(loss, dY): a scalar whose backward pass hands Y's producer a gradient in the layout `kind`, and the values of that
    gradient (contiguous, Y's dtype).  `wgt` is a tensor like Y.  The broadcast kinds arise the way they do in models:
    ``Y.sum()`` and the sum readout ``(Y.sum(0) * w).sum()`` with w = wgt[0]; ``cat_block`` is the column block that
    ``torch.cat([Y, other], 1)`` hands back."""
    if kind == "full_broadcast":
        return Y.sum(), torch.ones_like(wgt)
    if kind == "row_broadcast":
        w = wgt[0].contiguous()
        return (Y.sum(0) * w).sum(), w.unsqueeze(0).expand_as(wgt).contiguous()
    if kind == "cat_block":
        other = torch.zeros(Y.shape[0], PAD, dtype=Y.dtype, device=Y.device)
        wide = torch.cat([wgt, torch.ones_like(other)], 1)
        return (torch.cat([Y, other], 1) * wide).sum(), wgt.contiguous()
    return (grad_layout(Y, kind, keep) * wgt).sum(), wgt.contiguous()


def arrival_strides(shape, kind):
    """The strides of the gradient that ``layout_loss`` makes arrive."""
    if kind == "cat_block":
        return (shape[1] + PAD, 1)
    return expected_strides(tuple(shape), kind)

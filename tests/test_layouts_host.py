"""tests/layouts.py on the CPU: every layout has the strides and the values it names, and the constructions models use (a sum, a
sum readout, a concatenation, a product with a column-major operand) hand a backward pass the strides test_ops_layouts_gpu.py
relies on -- seen by a probe Function, so that a change in torch cannot quietly turn those cases into contiguous ones."""
import pytest
import torch
from torch.autograd import Function

import layouts as L

N, W = 7, 5


def _t(*shape, seed=1):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class _Probe(Function):
    """Identity that records the strides of the gradient its backward is handed."""
    seen = []

    @staticmethod
    def forward(ctx, X):
        return X.view_as(X)

    @staticmethod
    def backward(ctx, dY):
        _Probe.seen.append(tuple(dY.stride()))
        return dY


def _probe(loss_of, shape=(N, W)):
    X = _t(*shape).requires_grad_()
    _Probe.seen.clear()
    loss_of(_Probe.apply(X)).backward()
    assert len(_Probe.seen) == 1
    return _Probe.seen[0], X.grad


@pytest.mark.parametrize("shape", [(N, W), (N, 1)], ids=["wide", "one_column"])
@pytest.mark.parametrize("kind", L.KINDS)
def test_relayout_strides_and_values(kind, shape):
    t = _t(*shape)
    keep = []
    r = L.relayout(t, kind, keep)
    assert r.shape == t.shape and tuple(r.stride()) == L.expected_strides(shape, kind)
    assert torch.equal(r, L.materialised(t, kind))
    if kind == "row_broadcast":
        assert torch.equal(r, t[:1].expand(*shape))
    elif kind == "full_broadcast":
        assert torch.equal(r, t[0, 0].expand(*shape))
    else:
        assert torch.equal(r, t)
    assert r.data_ptr() != t.data_ptr(), "a layout never aliases the tensor it was made from"
    if kind in ("column_block", "inner_stride_2"):
        buf, view = keep[0]
        assert buf.shape == ((shape[0], shape[1] + L.PAD) if kind == "column_block" else (shape[0], 2 * shape[1]))
        assert int(torch.isnan(buf).sum()) == buf.numel() - t.numel() and L.padding_intact(keep)
        if kind == "column_block":
            assert (r.data_ptr() - buf.data_ptr()) == t.element_size(), "the block starts at column 1: off a 16-byte boundary"
        buf[0, 0 if kind == "column_block" else 1] = 0.0
        assert not L.padding_intact(keep), "a write into the padding shows"
    else:
        assert keep == []


def test_the_kinds_of_an_operand():
    assert L.kinds_for(_t(N, W)) == L.KINDS
    assert "column_major" not in L.kinds_for(_t(N, 1)) and len(L.kinds_for(_t(N, 1))) == 5
    assert L.kinds_for(_t(N)) == ("contiguous", "inner_stride_2")


def test_relayout_of_a_vector_and_of_per_edge_values():
    v = _t(9)
    keep = []
    r = L.relayout(v, "inner_stride_2", keep)
    assert tuple(r.stride()) == (2,) and torch.equal(r, v) and L.padding_intact(keep)
    assert tuple(L.relayout(v, "contiguous").stride()) == (1,)
    w = _t(3, 11)                                             # [heads, nnz]
    assert tuple(L.relayout(w, "column_major").stride()) == (1, 3) and torch.equal(L.relayout(w, "column_major"), w)
    assert tuple(L.relayout(w, "inner_stride_2").stride()) == (22, 2)


@pytest.mark.parametrize("kind", L.KINDS + ("cat_block",))
def test_layout_loss_delivers_the_layout_and_the_values(kind):
    wgt = _t(N, W, seed=2)
    keep = []
    box = {}

    def loss_of(Y):
        loss, box["dY"] = L.layout_loss(Y, kind, wgt, keep)
        return loss

    strides, grad = _probe(loss_of)
    assert strides == L.arrival_strides((N, W), kind)
    assert torch.equal(grad, box["dY"]) and box["dY"].is_contiguous()
    if kind == "row_broadcast":
        assert torch.equal(box["dY"], wgt[:1].expand(N, W))
    elif kind == "full_broadcast":
        assert torch.equal(box["dY"], torch.ones(N, W))
    else:
        assert torch.equal(box["dY"], wgt)
    assert L.padding_intact(keep) and (len(keep) == 1) == (kind in ("column_block", "inner_stride_2"))


def test_record_arrival_sees_what_the_producer_gets():
    X = _t(N, W).requires_grad_()
    Y = _Probe.apply(X)
    seen = []
    L.record_arrival(Y, seen)
    _Probe.seen.clear()
    (L.grad_layout(Y, "column_major") * _t(N, W, seed=3)).sum().backward()
    assert seen == [(1, N)] == _Probe.seen


def test_the_natural_constructions():
    """The table of the issue: what ordinary model code downstream of Y hands Y's backward."""
    w = _t(W, seed=4)
    assert _probe(lambda Y: Y.sum())[0] == (0, 0)
    assert _probe(lambda Y: (Y.sum(0) * w).sum())[0] == (0, 1)
    other = _t(N, 4, seed=5)
    assert _probe(lambda Y: (torch.cat([Y, other], 1) ** 2).sum())[0] == (W + 4, 1)
    wide = _t(N, W + 4, seed=6).requires_grad_()
    assert _probe(lambda Y: (Y * wide[:, :W].detach()).sum() + 0 * wide.sum())[0] == (W, 1)          # (the control: contiguous)
    # a slice of Y downstream: the gradient is a zero-padded full tensor, contiguous; a slice UPSTREAM hands back a block
    assert _probe(lambda Y: (Y[:, :3] ** 2).sum())[0] == (W, 1)
    col_major = _t(W, N, seed=7).t()                       # strides (1, N)
    mask = (_t(N, W, seed=8) > 0).float()
    # g * mask keeps the layout of its column-major operand: what d_output * (Y > 0) does inside a backward
    g = col_major * mask
    assert tuple(g.stride()) == (1, N)
    assert _probe(lambda Y: (L.grad_layout(Y, "column_major") * mask).sum())[0] == (1, N)
    # forward operands
    emb = _t(W, seed=9)
    assert tuple(emb.expand(N, W).stride()) == (0, 1)
    assert tuple(wide[:, 1:1 + W].stride()) == (W + 4, 1)
    assert tuple(torch.nn.Linear(W, 3).weight.t().stride()) == (1, W)

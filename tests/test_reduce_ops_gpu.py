"""NeighborMax / NeighborMin / NeighborMean, SAGEConv and the `sage` driver model on the GPU, against fp64 torch on the CPU.

torch's amax / amin gradient splits a tied extreme evenly and this library sends it to the first edge, so every comparison of a
max / min gradient runs on inputs whose reference has no tied extreme (asserted), and one hand-made case pins the tie rule."""
import re

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib
from reduce_ref import _agg64, _no_ties, _rows_of
from util import assert_close_f64, make_case

pytestmark = pytest.mark.gpu

GRAPHS = {"uniform": (3000, 40000), "powerlaw": (3000, 60000)}


class _Info:
    """The slice of decider.inputProperty the operators read."""

    def __init__(self, row_pointers, column_index, partSize=32):
        from gnnadvisor_osdi21_amd.decider import inputProperty
        self.row_pointers, self.column_index = row_pointers.cuda(), column_index.cuda()
        self.degrees = _lib.degrees(row_pointers.cpu()).cuda()
        self.partSize, self.dimWorker, self.warpPerBlock = partSize, 32, 4
        self.partPtr, self.part2Node = [t.cuda() for t in _lib.build_part(partSize, row_pointers.cpu())]
        self._edge_arrays = lambda: inputProperty._edge_arrays(self)
        self.inv_row_counts = lambda: inputProperty.inv_row_counts(self)


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_neighbor_ops_forward_and_input_gradient(kind, d):
    from gnnadvisor_osdi21_amd.ops import NeighborMax, NeighborMean, NeighborMin
    n, e = GRAPHS[kind]
    g, X, _, _ = make_case(n, e, d, 32, seed=3, kind=kind)
    info = _Info(g.row_pointers, g.column_index)
    G = torch.randn(n, d, generator=torch.Generator().manual_seed(5))
    for op, how in ((NeighborMax, "amax"), (NeighborMin, "amin"), (NeighborMean, "mean")):
        X64 = X.double().requires_grad_(True)
        if how != "mean":
            assert _no_ties(X64.detach(), g.row_pointers, g.column_index, how), "the reference has a tied extreme: torch splits it"
        ref = _agg64(X64, g.row_pointers, g.column_index, how)
        (ref * G.double()).sum().backward()
        Xd = X.cuda().requires_grad_(True)
        Y = op.apply(Xd, info)
        (Y * G.cuda()).sum().backward()
        if how == "mean":
            scale_y = _agg64(X.double().abs(), g.row_pointers, g.column_index, "mean")
            Xa = X.double().abs().requires_grad_(True)
            (_agg64(Xa, g.row_pointers, g.column_index, "mean") * G.double().abs()).sum().backward()
            scale_g = Xa.grad
            assert_close_f64(Y.detach().cpu().numpy(), ref.detach().numpy(), scale=scale_y.numpy(), what=f"{how} forward")
        else:
            assert torch.equal(Y.detach().cpu().double(), ref.detach()), f"{how} forward is not exact"
            Xa = X.double().requires_grad_(True)             # the same routing of the gradient, on |G|: the sum of |terms|
            (_agg64(Xa, g.row_pointers, g.column_index, how) * G.double().abs()).sum().backward()
            scale_g = Xa.grad
        assert_close_f64(Xd.grad.cpu().numpy(), X64.grad.numpy(), scale=scale_g.numpy(), what=f"{how} dX {kind} D={d}")


def test_tied_gradient_goes_to_the_earlier_edge():
    from gnnadvisor_osdi21_amd.ops import NeighborMax, NeighborMin
    # row 0 has the neighbours 1, 2, 3 (positions 0, 1, 2); rows 1..3 have the neighbour 0
    rp = torch.tensor([0, 3, 4, 5, 6], dtype=torch.int32)
    ci = torch.tensor([1, 2, 3, 0, 0, 0], dtype=torch.int32)
    info = _Info(rp, ci, partSize=2)                          # row 0 is split over two groups
    X = torch.tensor([[0., 0.], [5., -1.], [5., -1.], [4., -1.]], device="cuda", requires_grad=True)
    G = torch.tensor([[1., 10.], [0., 0.], [0., 0.], [0., 0.]], device="cuda")
    Y = NeighborMax.apply(X, info)
    assert torch.equal(Y[0].detach().cpu(), torch.tensor([5., -1.]))
    (Y * G).sum().backward()
    # column 0: nodes 1 and 2 tie at 5 -> all of it to node 1; column 1: all three tie at -1 -> node 1
    assert torch.equal(X.grad.cpu(), torch.tensor([[0., 0.], [1., 10.], [0., 0.], [0., 0.]]))
    X.grad = None
    Y = NeighborMin.apply(X, info)
    assert torch.equal(Y[0].detach().cpu(), torch.tensor([4., -1.]))
    (Y * G).sum().backward()
    assert torch.equal(X.grad.cpu(), torch.tensor([[0., 0.], [0., 10.], [0., 0.], [1., 0.]]))


def test_directed_graph_gradient():
    """A structure that is NOT symmetric: NeighborMax's backward needs no reverse edges and still matches fp64."""
    from gnnadvisor_osdi21_amd.ops import NeighborMax
    n, d = 500, 16
    rs = np.random.RandomState(4)
    key = np.unique(rs.randint(0, n, size=6000).astype(np.int64) * n + rs.randint(0, n, size=6000))
    rows, cols = key // n, key % n
    A = np.zeros((n, n), dtype=bool)
    A[rows, cols] = True
    assert (A != A.T).any()
    rp = torch.zeros(n + 1, dtype=torch.int32)
    rp[1:] = torch.from_numpy(np.cumsum(np.bincount(rows, minlength=n))).int()
    ci = torch.from_numpy(cols.astype(np.int32))
    info = _Info(rp, ci)
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(6))
    G = torch.randn(n, d, generator=torch.Generator().manual_seed(7))
    X64 = X.double().requires_grad_(True)
    assert _no_ties(X64.detach(), rp, ci, "amax")
    ref = _agg64(X64, rp, ci, "amax")
    (ref * G.double()).sum().backward()
    Xd = X.cuda().requires_grad_(True)
    Y = NeighborMax.apply(Xd, info)
    (Y * G.cuda()).sum().backward()
    assert torch.equal(Y.detach().cpu().double(), ref.detach())
    Xa = X.double().requires_grad_(True)
    (_agg64(Xa, rp, ci, "amax") * G.double().abs()).sum().backward()
    assert_close_f64(Xd.grad.cpu().numpy(), X64.grad.numpy(), scale=Xa.grad.numpy(), what="directed dX")


def _sage64(X, Ws, Wn, b, rp, ci, how, relu, G, Y_got):
    """fp64 SAGEConv and the gradients of sum(Y * G), written out (the aggregation's own gradient through torch's
    scatter_reduce), with the sum of |terms| of every result.  A ReLU pre-activation that cancels to within 1e-5 of its sum
    of |terms| has no defined sign in fp32: there the mask follows the sign the path under test computed (util.py)."""
    X = X.clone().requires_grad_(True)
    N = _agg64(X, rp, ci, how)
    Z = X.detach() @ Ws + N.detach() @ Wn + (b if b is not None else 0)
    Na = _agg64(X.detach().abs(), rp, ci, how).abs() if how == "mean" else N.detach().abs()
    Za = X.detach().abs() @ Ws.abs() + Na @ Wn.abs() + (b.abs() if b is not None else 0)
    mask = torch.ones_like(Z)
    if relu:
        mask = (Z > 0).double()
        amb = Z.abs() <= 1e-5 * Za
        mask = torch.where(amb, (Y_got > 0).double(), mask)
    Y = Z * mask
    dZ, dZa = G * mask, G.abs()
    N.backward(dZ @ Wn.t())
    dX = X.grad + dZ @ Ws.t()
    Xa = X.detach().clone().requires_grad_(True) if how != "mean" else X.detach().abs().requires_grad_(True)
    _agg64(Xa, rp, ci, how).backward(dZa @ Wn.abs().t())
    dXa = Xa.grad + dZa @ Ws.abs().t()
    res = dict(Y=(Y, Za), dX=(dX, dXa), dWs=(X.detach().t() @ dZ, X.detach().abs().t() @ dZa),
               dWn=(N.detach().t() @ dZ, Na.t() @ dZa))
    if b is not None:
        res["db"] = (dZ.sum(0), dZa.sum(0))
    return res


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("fin,fout", [(100, 16), (16, 100), (64, 64)], ids=["narrow", "widen", "square"])
@pytest.mark.parametrize("how", ["mean", "max", "min"])
def test_sage_conv(how, fin, fout, relu, bias):
    from gnnadvisor_osdi21_amd.ops import SAGEConv
    g, X, _, _ = make_case(3000, 60000, fin, 32, seed=3, kind="powerlaw")
    rp, ci = g.row_pointers, g.column_index
    info = _Info(rp, ci)
    torch.manual_seed(11)
    conv = SAGEConv(fin, fout, aggregator=how, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.uniform_(-0.5, 0.5)
    conv = conv.cuda()
    if how == "mean" and fin == 100:
        assert conv._update_first(X.cuda().requires_grad_(True))     # the narrowing layer aggregates X W_neigh
    tref = {"mean": "mean", "max": "amax", "min": "amin"}[how]
    if how != "mean":
        assert _no_ties(X.double(), rp, ci, tref)
    Xd = X.cuda().requires_grad_(True)
    Y = conv(Xd, info, relu=relu)
    G = torch.randn(3000, fout, generator=torch.Generator().manual_seed(12))
    (Y * G.cuda()).sum().backward()
    ref = _sage64(X.double(), conv.weights_self.detach().double().cpu(), conv.weights_neigh.detach().double().cpu(),
                  conv.bias.detach().double().cpu() if bias else None, rp, ci, tref, relu, G.double(), Y.detach().cpu())
    got = dict(Y=Y.detach(), dX=Xd.grad, dWs=conv.weights_self.grad, dWn=conv.weights_neigh.grad)
    if bias:
        got["db"] = conv.bias.grad
    for name, (r, scale) in ref.items():
        assert_close_f64(got[name].cpu().numpy(), r.detach().numpy(), scale=scale.detach().numpy(),
                         what=f"SAGEConv {how} {fin}->{fout} relu={relu} bias={bias}: {name}")


def test_sage_conv_refuses_16_bit_and_autocast():
    from gnnadvisor_osdi21_amd.ops import SAGEConv
    g, X, _, _ = make_case(300, 3000, 16, 32, seed=3)
    info = _Info(g.row_pointers, g.column_index)
    conv = SAGEConv(16, 8, aggregator="max").cuda()
    with pytest.raises(TypeError, match="float32"):
        conv(X.cuda().bfloat16(), info)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(TypeError, match="float32"):
            conv(X.cuda(), info)
    with pytest.raises(ValueError):
        SAGEConv(16, 8, aggregator="median")


# ---- driver -----------------------------------------------------------------------------------------------------------

def _drive(capsys, extra):
    from gnnadvisor_osdi21_amd import main as driver
    torch.manual_seed(0)
    rc = driver.main(["--synthetic", "cora-like", "--model", "sage", "--verbose_mode", "True", "--num_epoches", "30"] + extra)
    out = capsys.readouterr().out
    assert rc == 0
    assert re.search(r"Time \(ms\): (\d+\.\d{3})", out)
    first = re.search(r"# first loss: (\S+)", out)
    final = float(re.search(r"# final loss: (\S+)", out).group(1))
    return (float(first.group(1)) if first else None), final


@pytest.mark.parametrize("agg", ["max", "mean"])
def test_driver_sage_trains(capsys, agg):
    first, final = _drive(capsys, ["--aggregator", agg])
    print(f"{agg}: first loss {first}, final loss {final}")
    assert np.isfinite(final) and final < first


@pytest.mark.parametrize("agg", ["max", "mean"])
def test_driver_sage_under_a_captured_epoch(capsys, agg):
    """--hip_graph True: 10 eager steps and 30 replays of the captured step against 40 eager steps from the same seed.  The
    forward of max is exact; scatter_arg's float atomics and the dense products reorder sums, hence the 1e-3."""
    _, eager = _drive(capsys, ["--aggregator", agg])
    _, graphed = _drive(capsys, ["--aggregator", agg, "--hip_graph", "True"])
    print(f"{agg}: eager final loss {eager}, captured final loss {graphed}")
    assert np.isfinite(graphed)
    if agg == "max":
        assert abs(graphed - eager) <= 1e-3 * abs(eager)

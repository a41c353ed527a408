"""bfloat16 / float16 features through the GNNAdvisor module, the autograd ops and the driver.

Reference: fp64 (dense adjacency, the 16-bit inputs converted exactly).  Aggregation outputs use the bound of
tests/test_x16_gpu.py: |err| <= 1e-4 * max(1, sum |coef * x|) + u * |ref| with u = 2^-8 (bf16) / 2^-11 (fp16)."""
import re

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph, load_extension

pytestmark = pytest.mark.gpu
GNNA = load_extension()
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}


class _Info:
    """The attributes of a decider.inputProperty the ops read."""

    def __init__(self, g, partSize=32):
        pp, p2n = _lib.build_part(partSize, g.row_pointers)
        self.row_pointers, self.column_index, self.degrees = g.row_pointers.cuda(), g.column_index.cuda(), g.degrees.cuda()
        self.partPtr, self.part2Node = pp.cuda(), p2n.cuda()
        self.partSize, self.dimWorker, self.warpPerBlock = partSize, 32, 4


def _sym_graph(n=1500, nnz=30000, seed=3):
    g = graph.uniform_graph(n, nnz, seed=seed)
    A = torch.zeros(n, n, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(n), (g.row_pointers[1:] - g.row_pointers[:-1]).long())
    A[rows, g.column_index.long()] = 1.0
    assert torch.equal(A, A.t()), "the generators make symmetric graphs"
    return g, A.cuda()


def _close(got, ref, scale, what):
    u = UNIT[got.dtype]
    err = (got.double() - ref).abs()
    tol = 1e-4 * scale.clamp(min=1.0) + u * ref.abs()
    worst = float((err / tol).nan_to_num(nan=float("inf")).max())
    print(f"{what}: worst err / tol = {worst:.3f}")
    assert not (~(err <= tol)).any(), f"{what}: worst err / tol {worst:.3f}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_module_aggregate_ld_accepts_16_bit_input(dtype):
    """GNNA.aggregate_ld routes bf16 / fp16 input to gnna_agg_ld_x16: default output dtype = the input's, out_dtype=float32 on
    request; the fresh 16-bit output is poisoned like the fp32 ones; float32 input takes today's path and refuses out_dtype."""
    g, A = _sym_graph()
    info = _Info(g)
    X = torch.randn(g.num_nodes, 41, generator=torch.Generator().manual_seed(1)).to(dtype).cuda()
    deg = info.degrees if dtype == torch.bfloat16 else info.degrees / info.degrees.max()
    for mode, M in ((0, A), (1, deg.double()[:, None] * A * deg.double()[None, :]), (2, 0.25 * A)):
        ref, scale = M @ X.double(), M.abs() @ X.double().abs()
        Y = GNNA.aggregate_ld(mode, X, info.column_index, deg, 0.25, info.partPtr, info.part2Node, 32)
        assert Y.dtype == dtype
        _close(Y, ref, scale, f"module {dtype} mode={mode}")
        Y32 = GNNA.aggregate_ld(mode, X, info.column_index, deg, 0.25, info.partPtr, info.part2Node, 32, out_dtype=torch.float32)
        assert Y32.dtype == torch.float32
        _close(Y32, ref, scale, f"module {dtype} mode={mode} fp32 out")
        R = GNNA.aggregate_ld(mode, X, info.column_index, deg, 0.25, info.partPtr, info.part2Node, 32, relu=True)
        _close(R, ref.clamp(min=0), scale, f"module {dtype} mode={mode} relu")
    Xf = X.float()
    Yf = GNNA.aggregate_ld(0, Xf, info.column_index, None, 1.0, info.partPtr, info.part2Node, 32)
    assert Yf.dtype == torch.float32 and torch.equal(Yf, _lib.agg_ld(0, Xf, info.column_index, info.partPtr, info.part2Node, g.num_nodes, 32))
    with pytest.raises(RuntimeError, match="out_dtype"):
        GNNA.aggregate_ld(0, Xf, info.column_index, None, 1.0, info.partPtr, info.part2Node, 32, out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="float32"):
        GNNA.SAG(X, info.row_pointers, info.column_index, info.degrees, info.partPtr, info.part2Node, 32, 32, 4)


def test_scatter_and_gather_16_bit_forward_and_backward():
    from gnnadvisor_osdi21_amd.ops import ScatterAndGather
    g, A = _sym_graph()
    info = _Info(g)
    X = torch.randn(g.num_nodes, 64, generator=torch.Generator().manual_seed(2)).bfloat16().cuda().requires_grad_()
    W = torch.randn(g.num_nodes, 64, generator=torch.Generator().manual_seed(3)).bfloat16().cuda()
    Y = ScatterAndGather.apply(X, info)
    assert Y.dtype == torch.bfloat16
    _close(Y.detach(), A @ X.detach().double(), A @ X.detach().double().abs(), "SAG forward")
    (Y * W).sum().backward()
    assert X.grad.dtype == torch.bfloat16
    _close(X.grad, A @ W.double(), A @ W.double().abs(), "SAG dX")


def _net(kind, fin, hid, ncls):
    from gnnadvisor_osdi21_amd.ops import GCNConv, GINConv
    Conv = GCNConv if kind == "gcn" else GINConv
    torch.manual_seed(5)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.c2 = Conv(fin, hid), Conv(hid, ncls)

        def forward(self, x, info):
            return self.c2(self.c1(x, info, relu=True), info)
    return Net().cuda()


def _reference(kind, A, deg, X, W1, W2, wgt):
    """fp64 two-layer network y = L2(relu(L1(x))), loss = sum(y * wgt): (loss, dX, y)."""
    M = deg.double()[:, None] * A * deg.double()[None, :] if kind == "gcn" else 0.5 * A
    X = X.double().requires_grad_()
    W1, W2 = W1.double(), W2.double()
    H = torch.relu(M @ (X @ W1))
    y = M @ (H @ W2)
    loss = (y * wgt.double()).sum()
    loss.backward()
    return float(loss.detach()), X.grad, y.detach()


def _sparse_baseline(kind, A, deg, X, W1, W2, wgt, dtype):
    """The same model through torch.sparse.mm with `dtype` storage (the baseline a user would otherwise run): its loss.
    This torch build has no bfloat16 torch.sparse.mm: the COO form raises NotImplementedError ("addmm_sparse_cuda" not
    implemented for 'BFloat16') and the CSR form ends the process inside the sparse library.  So the baseline runs
    torch.sparse.mm's float32 kernel on the bf16 operands (exact upcast) and rounds each product to `dtype`: a bf16 model
    whose sparse product accumulates in fp32 -- no bf16 sparse kernel can be more accurate, so the comparison is not easier
    than the one against a native bf16 kernel would be."""
    M = (deg.double()[:, None] * A * deg.double()[None, :] if kind == "gcn" else 0.5 * A)
    Ms = M.to(dtype).float().to_sparse()
    Xh, W1h, W2h = X.to(dtype), W1.to(dtype), W2.to(dtype)
    H = torch.relu(torch.sparse.mm(Ms, (Xh @ W1h).float()).to(dtype))
    y = torch.sparse.mm(Ms, (H @ W2h).float()).to(dtype)
    return float((y.double() * wgt.double()).sum())


@pytest.mark.parametrize("how", ["autocast", "cast"])
@pytest.mark.parametrize("kind", ["gcn", "gin"])
def test_two_layer_network_bf16(kind, how):
    """Two-layer GCN / GIN in bf16 -- under torch.autocast (fp32 parameters and inputs) and as a model cast to bf16 -- forward
    and dX against the fp64 dense reference.  The loss error is compared with the error of the same model run through
    torch.sparse.mm in bf16: ours must be no worse than 2 x that baseline (the summation order differs).  Measured on MI355X,
    |loss - fp64| ours vs. the baseline (_sparse_baseline: what it is on this torch build): GCN 1.006 vs. 0.654 (fp64 loss
    -3.618e4), GIN 4.63 vs. 4.91 (fp64 loss -2.581e4); the same figures under autocast and for the cast model."""
    g, A = _sym_graph()
    info = _Info(g)
    fin, hid, ncls = 48, 64, 16
    net = _net(kind, fin, hid, ncls)
    gen = torch.Generator().manual_seed(7)
    X = torch.randn(g.num_nodes, fin, generator=gen).cuda()
    wgt = torch.rand(g.num_nodes, ncls, generator=gen).cuda()
    # bf16-representable inputs and weights, so that both ways of running see the numbers the fp64 reference sees
    X = X.bfloat16().float()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.bfloat16().float())
    if kind == "gcn":
        info.degrees = (info.degrees / info.degrees.max()).contiguous()     # keeps two layers of sqrt-degree products O(1)
    W1, W2 = net.c1.weights.detach().clone(), net.c2.weights.detach().clone()
    ref_loss, ref_dX, ref_y = _reference(kind, A, info.degrees, X, W1, W2, wgt)
    if how == "autocast":
        Xin = X.clone().requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = net(Xin, info)
        assert y.dtype == torch.bfloat16
        assert net.c1.weights.dtype == torch.float32
    else:
        net = net.bfloat16()
        Xin = X.bfloat16().requires_grad_()
        y = net(Xin, info)
        assert y.dtype == torch.bfloat16
    loss = (y.float() * wgt).sum()
    loss.backward()
    assert Xin.grad.dtype == Xin.dtype and net.c1.weights.grad.dtype == net.c1.weights.dtype
    assert torch.isfinite(Xin.grad).all() and torch.isfinite(net.c1.weights.grad).all() and torch.isfinite(net.c2.weights.grad).all()
    ours = abs(float(loss) - ref_loss)
    base = abs(_sparse_baseline(kind, A, info.degrees, X, W1, W2, wgt, torch.bfloat16) - ref_loss)
    print(f"{kind} {how}: |loss - fp64| ours {ours:.4e}, torch.sparse.mm bf16 {base:.4e}, fp64 loss {ref_loss:.6e}")
    assert ours <= 2.0 * base, (ours, base)
    # forward and dX agree with fp64 to what bf16 intermediates allow: every layer rounds its activations to bf16, so the
    # error of an element is bounded by a few units of bf16 roundoff of the magnitudes that enter it
    M = (info.degrees.double()[:, None] * A * info.degrees.double()[None, :]) if kind == "gcn" else 0.5 * A
    mag_y = M @ (torch.relu(M @ (X.double().abs() @ W1.double().abs())) @ W2.double().abs())
    assert ((y.double() - ref_y).abs() <= 8 * 2.0 ** -8 * mag_y.clamp(min=1e-30) + 1e-4).all()
    mag_dx = (M @ ((M @ (wgt.double() @ W2.double().abs().t())) @ W1.double().abs().t()))
    assert ((Xin.grad.double() - ref_dX).abs() <= 8 * 2.0 ** -8 * mag_dx + 1e-4).all()


def test_first_layer_aggregation_inside_the_network_meets_the_bound():
    """The aggregation output of layer 1 (GCN order: agg(X W), ReLU fused) as the op computes it, against fp64 on the bf16
    product it was given: the bound of the library-level tests."""
    from gnnadvisor_osdi21_amd.ops import GCNConv
    g, A = _sym_graph()
    info = _Info(g)
    torch.manual_seed(1)
    conv = GCNConv(48, 64).cuda().bfloat16()
    X = torch.randn(g.num_nodes, 48, generator=torch.Generator().manual_seed(2)).bfloat16().cuda()
    Y = conv(X, info, relu=True)
    XW = torch.mm(X, conv.weights.detach())
    M = info.degrees.double()[:, None] * A * info.degrees.double()[None, :]
    _close(Y.detach(), (M @ XW.double()).clamp(min=0), M @ XW.double().abs(), "GCNConv layer")


def test_autocast_is_refused_today_for_nothing_else():
    """Outside autocast and with fp32 tensors the layers take exactly the fp32 Functions."""
    from gnnadvisor_osdi21_amd import ops
    g, _A = _sym_graph()
    info = _Info(g)
    conv = ops.GCNConv(16, 8).cuda()
    X = torch.randn(g.num_nodes, 16, generator=torch.Generator().manual_seed(2)).cuda()
    assert ops._x16_dtype(X) is None
    Y = conv(X, info)
    assert Y.dtype == torch.float32 and Y.grad_fn.name().startswith("GNNAFunctionBackward")


def test_driver_trains_in_bfloat16(capsys):
    """main.py --dtype bfloat16 --synthetic ... runs and its loss decreases."""
    from gnnadvisor_osdi21_amd import main as driver
    rc = driver.main(["--synthetic", "cora-like", "--dim", "96", "--hidden", "16", "--classes", "7", "--model", "gcn",
                      "--num_epoches", "40", "--dtype", "bfloat16", "--verbose_mode", "True"])
    out = capsys.readouterr().out
    assert rc == 0
    first = float(re.search(r"# first loss: (\d+\.\d+)", out).group(1))
    final = float(re.search(r"# final loss: (\d+\.\d+)", out).group(1))
    print(f"bf16 GCN on cora-like: loss {first:.4f} -> {final:.4f}")
    assert np.isfinite(final) and final < first
    assert re.search(r"Time \(ms\): \d+\.\d{3}", out)

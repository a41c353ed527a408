"""NeighborStats and PNAConv on the GPU, against fp64 torch on the CPU.

The reference is the CENTRED definition: mean = sum x / c, var = sum (x - mean)^2 / c (never negative, so no clamp),
std = sqrt(var + eps), c = max(count, 1); max / min as in test_reduce_ops_gpu.py, on inputs without a tied extreme (asserted).
Its gradients come from fp64 autograd.  Features are unit-scale randn (make_case's).

Bounds, all of the project's form 1e-4 * max(1, sum of |terms|):
  mean   scale = the row's mean of |x|;
  std    |std - std64| <= 1e-4 * max(1, 3 * m2 / (std64 + sqrt(eps))), m2 the row's mean of x^2: the 1e-4 bound on sum and sumsq
         carried through var = q / c - (s / c)^2 and the square root;
  dX     per source row j, the sum over the rows i that list j of |g_mean| / c + |g_std| * (|x_j| + mean_i |x|) / (c * std64),
         plus the routed |g_max| and |g_min|."""
import types

import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, ops
from gnnadvisor_osdi21_amd.sampling import NeighborSampler
from util import assert_close_f64, make_case

from pna_ref import EPS, _bounds, _no_ties, _stats64, _zeros
from test_reduce_ops_gpu import _Info, _rows_of

pytestmark = pytest.mark.gpu

NAMES = ("mean", "std", "max", "min")


def _check(info, X, rows, src, n_out, seed=5, given=NAMES, what=""):
    """forward of all four and dX for gradients into `given`, against fp64 within the bounds -> dX (device)."""
    X64 = X.double().requires_grad_(True)
    assert _no_ties(X64.detach(), rows, src, n_out), "the reference has a tied extreme: torch splits its gradient"
    ref = _stats64(X64, rows, src, n_out)
    gen = torch.Generator().manual_seed(seed)
    grads = [torch.randn(n_out, X.shape[1], generator=gen).double() if k in given else None for k in NAMES]
    sum((y * g).sum() for y, g in zip(ref, grads) if g is not None).backward()
    Xd = X.cuda().requires_grad_(True)
    got = ops.NeighborStats.apply(Xd, info, EPS)
    sum((y * g.float().cuda()).sum() for y, g in zip(got, grads) if g is not None).backward()
    mean, std, mx, mn = [t.detach().cpu().double() for t in got]
    mabs, std_tol, dx_scale = _bounds(X64.detach(), rows, src, n_out, grads, ref[1].detach())
    assert_close_f64(mean.numpy(), ref[0].detach().numpy(), scale=mabs.numpy(), what=f"{what} mean")
    err = (std - ref[1].detach()).abs()
    print(f"{what}: std worst error / bound {float((err / std_tol).max()):.4f}")
    assert bool((err <= std_tol).all()), f"{what} std: max err {float(err.max()):.3e}, worst ratio to the bound {float((err / std_tol).max()):.3f}"
    assert torch.equal(mx, ref[2].detach()) and torch.equal(mn, ref[3].detach()), f"{what}: max / min are not exact"
    dx_err = (Xd.grad.cpu().double() - X64.grad).abs() / (1e-4 * dx_scale.clamp(min=1.0))
    print(f"{what}: dX worst error / bound {float(dx_err.max()):.4f}")
    assert_close_f64(Xd.grad.cpu().numpy(), X64.grad.numpy(), scale=dx_scale.numpy(), what=f"{what} dX")
    return Xd.grad


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_symmetric_graph(kind, d):
    n, e = (3000, 40000) if kind == "uniform" else (3000, 60000)
    g, X, _, _ = make_case(n, e, d, 32, seed=3, kind=kind)
    info = _Info(g.row_pointers, g.column_index)
    _check(info, X, _rows_of(g.row_pointers), g.column_index.long(), n, what=f"{kind} D={d}")


def _directed_structure(n=500, edges=6000):
    rs = np.random.RandomState(4)
    key = np.unique(rs.randint(0, n, size=edges).astype(np.int64) * n + rs.randint(0, n, size=edges))
    rows, cols = key // n, key % n
    A = np.zeros((n, n), dtype=bool)
    A[rows, cols] = True
    assert (A != A.T).any()
    rp = torch.zeros(n + 1, dtype=torch.int32)
    rp[1:] = torch.from_numpy(np.cumsum(np.bincount(rows, minlength=n))).int()
    return rp, torch.from_numpy(cols.astype(np.int32))


def _directed_info(rp, ci):
    """A decider.inputProperty on the device with ``directed`` set: its backward passes run on transposed()."""
    from gnnadvisor_osdi21_amd.decider import inputProperty
    n = rp.numel() - 1
    ds = types.SimpleNamespace(num_nodes=n, avg_degree=ci.numel() / n, avg_edgeSpan=n / 3, num_features=16)
    info = inputProperty(rp.cuda(), ci.cuda(), _lib.degrees(rp).cuda(), 32, 32, 4, hiddenDim=16, dataset_obj=ds)
    info.partPtr, info.part2Node = [t.cuda() for t in _lib.build_part(32, rp)]
    info.directed = True
    return info


def test_directed_graph():
    rp, ci = _directed_structure()
    info = _directed_info(rp, ci)
    X = torch.randn(500, 16, generator=torch.Generator().manual_seed(6))
    _check(info, X, _rows_of(rp), ci.long(), 500, what="directed")


def _block(fanout=5):
    g, _, _, _ = make_case(3000, 60000, 1, 32, seed=3, kind="powerlaw")
    bundle = types.SimpleNamespace(row_pointers=g.row_pointers.cuda(), column_index=g.column_index.cuda(), partSize=32)
    seeds = torch.arange(0, 3000, 3, dtype=torch.int32).cuda()
    blocks, _ = NeighborSampler(bundle, [fanout]).sample(seeds, 11)
    return blocks[0]


def test_sampled_block():
    block = _block()
    assert block.num_src > block.num_dst
    X = torch.randn(block.num_src, 16, generator=torch.Generator().manual_seed(7))
    rp, ci = block.row_pointers.cpu(), block.column_index.cpu()
    got = ops.NeighborStats.apply(X.cuda(), block)
    assert all(t.shape == (block.num_dst, 16) for t in got)
    _check(block, X, _rows_of(rp), ci.long(), block.num_dst, what="block")


def test_degree_one_duplicate_edges_and_an_empty_row():
    # row 0: one edge; row 1: two edges that name the same source; row 2: no edge; row 3: three different sources
    rp = torch.tensor([0, 1, 3, 3, 6], dtype=torch.int32)
    ci = torch.tensor([2, 3, 3, 0, 1, 2], dtype=torch.int32)
    info = _directed_info(rp, ci)
    X = torch.randn(4, 8, generator=torch.Generator().manual_seed(8))
    rows, src = _rows_of(rp), ci.long()
    X64 = X.double().requires_grad_(True)
    ref = _stats64(X64, rows, src, 4)
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(4, 8, generator=gen).double() for _ in range(2)] + [None, None]     # (row 1's extreme is tied)
    sum((y * g).sum() for y, g in zip(ref, grads) if g is not None).backward()
    Xd = X.cuda().requires_grad_(True)
    mean, std, mx, mn = ops.NeighborStats.apply(Xd, info, EPS)
    (mean * grads[0].float().cuda() + std * grads[1].float().cuda()).sum().backward()
    mabs, std_tol, dx_scale = _bounds(X64.detach(), rows, src, 4, grads, ref[1].detach())
    err = (std.detach().cpu().double() - ref[1].detach()).abs()
    assert bool((err <= std_tol).all())
    assert bool(((std.detach().cpu().double()[:3] - EPS ** 0.5).abs() <= std_tol[:3]).all())       # rows 0, 1, 2: std = sqrt(eps)
    assert torch.isfinite(Xd.grad).all()
    assert_close_f64(Xd.grad.cpu().numpy(), X64.grad.numpy(), scale=dx_scale.numpy(), what="hand-made dX")
    for t in (mean, mx, mn):
        assert float(t[2].detach().abs().max()) == 0.0
    assert torch.equal(mx[1].cpu(), X[3]) and torch.equal(mn[0].cpu(), X[2])


def test_gradient_skipping():
    g, X, _, _ = make_case(3000, 60000, 16, 32, seed=3, kind="powerlaw")
    rows, src = _rows_of(g.row_pointers), g.column_index.long()
    rp, ci = _directed_structure()
    info = _directed_info(rp, ci)
    Xs = torch.randn(500, 16, generator=torch.Generator().manual_seed(6)).cuda()
    # an input that needs no gradient builds no transposed structure
    out = ops.NeighborStats.apply(Xs, info)
    assert all(not t.requires_grad for t in out) and info._edge_arrays().get("transposed") is None
    W = torch.ones(16, 1, device="cuda", requires_grad=True)
    (sum(out) @ W).sum().backward()
    assert W.grad is not None and info._edge_arrays().get("transposed") is None
    # gradients into some outputs only = zero gradients into the others (within the bound of the gradients given)
    sym = _Info(g.row_pointers, g.column_index)
    for given in (("std",), ("mean", "max"), ("min",)):
        part = _check(sym, X, rows, src, 3000, given=given, what=f"only {given}")
        Xd = X.cuda().requires_grad_(True)
        got = ops.NeighborStats.apply(Xd, sym, EPS)
        gen = torch.Generator().manual_seed(5)
        gs = [torch.randn(3000, 16, generator=gen).double() if k in given else None for k in NAMES]
        sum((y * (g.float().cuda() if g is not None else torch.zeros_like(y))).sum() for y, g in zip(got, gs)).backward()
        _, _, scale = _bounds(X.double(), rows, src, 3000, gs, _stats64(X.double(), rows, src, 3000)[1])
        assert_close_f64(part.cpu().numpy(), Xd.grad.cpu().double().numpy(), rtol=2e-4, scale=scale.numpy(), what=f"only {given} vs zeros")
    # the statistics wanted: the others are None and their kernels' outputs are not computed
    mean, std, mx, mn = ops.NeighborStats.apply(X.cuda(), sym, EPS, ("std", "min"))
    assert mean is None and mx is None and std is not None and mn is not None


def _pna64(conv, X, rows, src, n_out, G, relu_from=None):
    """fp64 PNAConv (centred statistics) and the gradients of sum(Y * G) by autograd, with the sum of |terms| of every result:
    the same network on |X|, |W|, |b| with every statistic replaced by a bound of its magnitude and |G| flowing back."""
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in conv.named_parameters()}
    delta = float(conv.delta)
    Xr = X.double().requires_grad_(True)
    stats = dict(zip(NAMES, _stats64(Xr, rows, src, n_out, conv.eps)))
    c = torch.bincount(rows, minlength=n_out).clamp(min=1).double().unsqueeze(1)
    logd = torch.log(c + 1)
    scale_of = {"identity": torch.ones_like(logd), "amplification": logd / delta, "attenuation": delta / logd}

    def net(x, st, par):
        A = torch.cat([st[a] for a in conv.aggregators], 1)
        Y = x[:n_out] @ par["weights_self"]
        for k, s in enumerate(conv.scalers):
            Y = Y + scale_of[s] * (A @ par[f"weights_scaler.{k}"])
        return Y + par["bias"] if "bias" in par else Y
    Y = net(Xr, stats, p)
    (Y * G).sum().backward()
    ref = dict(Y=Y.detach(), dX=Xr.grad, **{k: v.grad for k, v in p.items()})
    # the |.|-network: mean|x| bounds |mean|, max|x| bounds |max| and |min|, sqrt(mean x^2 + eps) bounds std
    pa = {k: v.detach().abs().requires_grad_(True) for k, v in p.items()}
    Xa = X.double().abs().requires_grad_(True)
    Ga = Xa[src]
    mabs = _zeros(n_out, Xa).index_add(0, rows, Ga) / c
    amax = _zeros(n_out, Xa).scatter_reduce(0, rows[:, None].expand_as(Ga), Ga, reduce="amax", include_self=False)
    rms = torch.sqrt(_zeros(n_out, Xa).index_add(0, rows, Ga ** 2) / c + conv.eps)
    Ya = net(Xa, {"mean": mabs, "std": rms, "max": amax, "min": amax}, pa)
    (Ya * G.abs()).sum().backward()
    scale = dict(Y=Ya.detach(), dX=Xa.grad, **{k: v.grad for k, v in pa.items()})
    return ref, scale


# the gradient of std w.r.t. x_j is (x_j - mean) / (c std): its |.|-bound needs 1 / std, which the |.|-network above does not
# carry; the dX scale of the layer adds the NeighborStats bound for the gradients that reach the statistics
def _pna_dx_scale(conv, X, rows, src, n_out, G):
    p = {k: v.detach().double().cpu().abs() for k, v in conv.named_parameters()}
    c = torch.bincount(rows, minlength=n_out).clamp(min=1).double().unsqueeze(1)
    logd = torch.log(c + 1)
    delta = float(conv.delta)
    scale_of = {"identity": torch.ones_like(logd), "amplification": logd / delta, "attenuation": delta / logd}
    F = X.shape[1]
    dA = sum((scale_of[s] * G.abs()) @ p[f"weights_scaler.{k}"].t() for k, s in enumerate(conv.scalers))
    grads = [dA[:, i * F:(i + 1) * F] for i in range(len(conv.aggregators))]
    by_name = dict(zip(conv.aggregators, grads))
    std64 = _stats64(X.double(), rows, src, n_out, conv.eps)[1]
    _, _, stat_scale = _bounds(X.double(), rows, src, n_out, [by_name.get(k) for k in NAMES], std64)
    self_term = torch.zeros_like(stat_scale)                 # (a block's self term reads its first num_dst source rows)
    self_term[:n_out] = G.abs() @ p["weights_self"].t()
    return stat_scale + self_term


CONFIGS = {
    "all-computed-delta": dict(),
    "all-given-delta-bias": dict(delta=2.5, bias=True),
    "subset": dict(aggregators=("std", "max"), scalers=("attenuation",), bias=True),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_pna_conv(config):
    fin, fout = 16, 24
    g, X, _, _ = make_case(3000, 60000, fin, 32, seed=3, kind="powerlaw")
    rows, src = _rows_of(g.row_pointers), g.column_index.long()
    info = _Info(g.row_pointers, g.column_index)
    assert _no_ties(X.double(), rows, src, 3000)
    torch.manual_seed(11)
    conv = ops.PNAConv(fin, fout, **CONFIGS[config])
    if conv.bias is not None:
        with torch.no_grad():
            conv.bias.uniform_(-0.5, 0.5)
    conv = conv.cuda()
    Xd = X.cuda().requires_grad_(True)
    Y = conv(Xd, info)
    if "delta" in CONFIGS[config]:
        assert float(conv.delta) == 2.5
    else:
        c = torch.bincount(rows, minlength=3000).clamp(min=1).double()
        assert float(conv.delta) == pytest.approx(float(torch.log(c + 1).mean()), rel=1e-5)
        assert ops.PNAConv.delta_of(info) == pytest.approx(float(conv.delta), rel=1e-6)
    G = torch.randn(3000, fout, generator=torch.Generator().manual_seed(12)).double()
    (Y * G.float().cuda()).sum().backward()
    ref, scale = _pna64(conv, X, rows, src, 3000, G)
    scale["dX"] = _pna_dx_scale(conv, X, rows, src, 3000, G)
    got = dict(Y=Y.detach(), dX=Xd.grad, **{k: v.grad for k, v in conv.named_parameters()})
    assert set(got) == set(ref)
    for name in ref:
        err = (got[name].cpu().double() - ref[name]).abs() / (1e-4 * scale[name].clamp(min=1.0))
        print(f"PNAConv {config} {name}: worst error / bound {float(err.max()):.4f}")
        assert_close_f64(got[name].cpu().numpy(), ref[name].numpy(), scale=scale[name].numpy(), what=f"PNAConv {config}: {name}")
    # relu=True is relu(layer): a second run (its sums meet in another order), held to relu of the reference -- the clamp moves
    # nothing by more than the layer's own error
    Yr = conv(Xd.detach(), info, relu=True)
    assert float(Yr.min()) == 0.0
    assert_close_f64(Yr.detach().cpu().numpy(), torch.relu(ref["Y"]).numpy(), scale=scale["Y"].numpy(), what=f"PNAConv {config}: relu")


def test_pna_conv_on_a_block_and_what_it_refuses():
    block = _block()
    torch.manual_seed(13)
    conv = ops.PNAConv(16, 8, delta=1.7).cuda()
    X = torch.randn(block.num_src, 16, generator=torch.Generator().manual_seed(14))
    rows, src = _rows_of(block.row_pointers.cpu()), block.column_index.cpu().long()
    assert _no_ties(X.double(), rows, src, block.num_dst)
    Xd = X.cuda().requires_grad_(True)
    Y = conv(Xd, block)
    assert Y.shape == (block.num_dst, 8)
    G = torch.randn(block.num_dst, 8, generator=torch.Generator().manual_seed(15)).double()
    (Y * G.float().cuda()).sum().backward()
    ref, scale = _pna64(conv, X, rows, src, block.num_dst, G)
    scale["dX"] = _pna_dx_scale(conv, X, rows, src, block.num_dst, G)
    got = dict(Y=Y.detach(), dX=Xd.grad, **{k: v.grad for k, v in conv.named_parameters()})
    for name in ref:
        assert_close_f64(got[name].cpu().numpy(), ref[name].numpy(), scale=scale[name].numpy(), what=f"PNAConv on a block: {name}")
    with pytest.raises(TypeError, match="float32 only"):
        conv.bfloat16()(X.cuda().bfloat16(), block)
    conv = conv.float()
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(TypeError, match="float32 only"):
        conv(X.cuda(), block)
    with pytest.raises(TypeError, match="float32 only"):
        ops.NeighborStats.apply(X.cuda().half(), block)

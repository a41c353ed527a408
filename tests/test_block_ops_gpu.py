"""The GraphSAGE operators on sampled blocks, against fp64 dense autograd on the [num_dst x num_src] matrix of the block.
Bound (tests/util.py): |got - ref| <= 1e-4 * max(1, sum of |terms|); the sum of |terms| of every output and gradient is the same
network evaluated on |X|, |W| and |weights of the loss| (every coefficient of the network is non-negative)."""
import functools
import types

import numpy as np
import pytest
import torch

import sampling_ref as ref
from gnnadvisor_osdi21_amd import _lib, ops
from gnnadvisor_osdi21_amd.sampling import NeighborSampler, SampledBlock
from util import assert_close_f64

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_graph():
    rp, ci = ref.shared_graph()
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


def bundle(partSize=32):
    rp, ci = device_graph()
    return types.SimpleNamespace(row_pointers=rp, column_index=ci, partSize=partSize)


def dense_of(block):
    """float64 [num_dst, num_src]: how often every source appears in every destination row (duplicate edges count)."""
    rp, ci = block.row_pointers.cpu().long(), block.column_index.cpu().long()
    rows = torch.repeat_interleave(torch.arange(block.num_dst), rp[1:] - rp[:-1])
    A = torch.zeros(block.num_dst, block.num_src, dtype=torch.float64)
    A.index_put_((rows, ci), torch.ones(len(ci), dtype=torch.float64), accumulate=True)
    return A


def extreme_sources(block, X64, op):
    """[num_dst, F] local source id that supplies every element of the max / min (-1: the row has no edges)."""
    rp, ci = block.row_pointers.cpu().long(), block.column_index.cpu().long()
    out = torch.full((block.num_dst, X64.shape[1]), -1, dtype=torch.long)
    for i in range(block.num_dst):
        cols = ci[rp[i]: rp[i + 1]]
        if len(cols):
            vals = X64[cols]
            out[i] = cols[vals.argmax(0) if op == "max" else vals.argmin(0)]
    return out


def reference_layer(block, aggregator, X, Ws, Wn, picked=None):
    """fp64 SAGEConv on a block from dense pieces; differentiable in X, Ws, Wn."""
    if aggregator == "mean":
        A = dense_of(block)
        N = (A / A.sum(1, keepdim=True).clamp(min=1)) @ X
    else:
        N = X.gather(0, picked.clamp(min=0)) * (picked >= 0)
    return X[:block.num_dst] @ Ws + N @ Wn


def grads_of(fn, tensors, wgt):
    leaves = [t.clone().requires_grad_(True) for t in tensors]
    Y = fn(*leaves)
    (Y * wgt).sum().backward()
    return [Y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("widths", [(4, 3), (41, 64), (64, 16)])
@pytest.mark.parametrize("aggregator", ["mean", "max", "min"])
def test_sageconv_on_one_block(aggregator, widths):
    fin, fout = widths
    b = bundle()
    seeds = torch.from_numpy(ref.seed_sets()[65]).cuda()
    block = SampledBlock.sample(b.row_pointers, b.column_index, seeds, 5, 77, partSize=32)
    assert block.num_dst == 65 and block.directed
    gen = torch.Generator().manual_seed(fin * 100 + fout)
    X = torch.randn(block.num_src, fin, generator=gen)          # continuous draws: no two candidates of a max / min are equal
    wgt = torch.rand(65, fout, generator=gen) + 0.5
    conv = ops.SAGEConv(fin, fout, aggregator=aggregator).cuda()
    Xd = X.cuda().requires_grad_(True)
    Y = conv(Xd, block)
    assert Y.shape == (65, fout)
    (Y * wgt.cuda()).sum().backward()
    got = [Y.detach(), Xd.grad, conv.weights_self.grad, conv.weights_neigh.grad]

    X64, Ws, Wn = X.double(), conv.weights_self.detach().cpu().double(), conv.weights_neigh.detach().cpu().double()
    picked = None if aggregator == "mean" else extreme_sources(block, X64, aggregator)
    fn = lambda x, ws, wn: reference_layer(block, aggregator, x, ws, wn, picked)
    want = grads_of(fn, (X64, Ws, Wn), wgt.double())
    scale = grads_of(fn, (X64.abs(), Ws.abs(), Wn.abs()), wgt.double())
    for name, g, w, s in zip(("out", "dX", "dW_self", "dW_neigh"), got, want, scale):
        assert_close_f64(g.cpu().numpy(), w.numpy(), what=f"{aggregator} {widths} {name}", scale=s.numpy())


def test_first_layer_builds_no_transpose():
    b = bundle()
    block = SampledBlock.sample(b.row_pointers, b.column_index, torch.from_numpy(ref.seed_sets()[64]).cuda(), 5, 3, partSize=32)
    conv = ops.SAGEConv(8, 4).cuda()
    conv(torch.randn(block.num_src, 8, device="cuda"), block).sum().backward()      # X needs no gradient
    assert block._transposed is None and conv.weights_neigh.grad is not None


@pytest.mark.parametrize("aggregator", ["mean", "max"])
def test_full_block_agrees_with_the_full_graph(aggregator):
    rp, ci = device_graph()
    n = rp.numel() - 1
    block = SampledBlock.sample(rp, ci, torch.arange(n, dtype=torch.int32, device="cuda"), -1, 5, partSize=32)
    assert torch.equal(block.src_nodes, torch.arange(n, dtype=torch.int32, device="cuda"))
    assert torch.equal(block.column_index, ci) and torch.equal(block.row_pointers, rp)
    pp, p2n = _lib.build_part(32, rp.cpu())
    counts = (rp[1:] - rp[:-1]).clamp(min=1).float()
    info = types.SimpleNamespace(row_pointers=rp, column_index=ci, degrees=torch.ones(n, device="cuda"), partPtr=pp.int().cuda(),
                                 part2Node=p2n.int().cuda(), partSize=32, dimWorker=32, warpPerBlock=4,
                                 inv_row_counts=lambda: 1.0 / counts)
    conv = ops.SAGEConv(16, 8, aggregator=aggregator).cuda()
    X = torch.randn(n, 16, device="cuda")
    with torch.no_grad():
        want, got = conv(X, info), conv(X, block)
    assert_close_f64(got.cpu().numpy(), want.double().cpu().numpy(), what=f"full block, {aggregator}")


def test_sampler_chains_blocks_and_a_two_layer_model_matches_dense_autograd():
    sampler = NeighborSampler(bundle(), [5, 3])
    seeds = torch.from_numpy(ref.seed_sets()[65]).cuda()
    blocks, input_nodes = sampler.sample(seeds, 9)
    assert len(blocks) == 2 and blocks[1].num_dst == 65
    assert blocks[0].num_dst == blocks[1].num_src
    assert torch.equal(blocks[0].src_nodes[:blocks[0].num_dst], blocks[1].src_nodes)
    assert input_nodes is blocks[0].src_nodes
    # hop l uses rng_seed + l
    rp, ci = ref.shared_graph()
    last = ref.sample_block(rp, ci, ref.seed_sets()[65], 3, 9 + 1)
    first = ref.sample_block(rp, ci, last["src_nodes"], 5, 9 + 0)
    assert (blocks[1].column_index.cpu().numpy() == last["column_index"]).all()
    assert (blocks[0].src_nodes.cpu().numpy() == first["src_nodes"]).all()

    gen = torch.Generator().manual_seed(21)
    X = torch.randn(blocks[0].num_src, 8, generator=gen)
    wgt = torch.rand(65, 4, generator=gen) + 0.5
    conv1, conv2 = ops.SAGEConv(8, 16).cuda(), ops.SAGEConv(16, 4).cuda()
    Xd = X.cuda().requires_grad_(True)
    Y = conv2(conv1(Xd, blocks[0]), blocks[1])
    (Y * wgt.cuda()).sum().backward()
    got = [Y.detach(), Xd.grad, conv1.weights_self.grad, conv1.weights_neigh.grad, conv2.weights_self.grad, conv2.weights_neigh.grad]
    params = [p.detach().cpu().double() for p in (conv1.weights_self, conv1.weights_neigh, conv2.weights_self, conv2.weights_neigh)]

    def fn(x, a, b_, c, d):
        return reference_layer(blocks[1], "mean", reference_layer(blocks[0], "mean", x, a, b_), c, d)
    want = grads_of(fn, [X.double()] + params, wgt.double())
    scale = grads_of(fn, [X.double().abs()] + [p.abs() for p in params], wgt.double())
    for name, g, w, s in zip(("out", "dX", "dW1_self", "dW1_neigh", "dW2_self", "dW2_neigh"), got, want, scale):
        assert_close_f64(g.cpu().numpy(), w.numpy(), what=f"two layers, {name}", scale=s.numpy())


def test_twenty_blocks_one_after_another():
    rp, ci = device_graph()
    n = rp.numel() - 1
    X = torch.randn(n, 8, device="cuda")
    rng = np.random.default_rng(5)
    before = None
    for k in range(21):
        seeds = torch.from_numpy(rng.permutation(n)[:500].astype(np.int32)).cuda()
        block = SampledBlock.sample(rp, ci, seeds, 5, 1000 + k, partSize=32)
        Xb = X.index_select(0, block.src_nodes)
        Y = ops.ScatterAndGather.apply(Xb, block)
        brp = block.row_pointers.long()
        rows = torch.repeat_interleave(torch.arange(500, device="cuda"), brp[1:] - brp[:-1])
        want = torch.zeros(500, 8, dtype=torch.float64, device="cuda").index_add_(0, rows, Xb.double()[block.column_index.long()])
        assert_close_f64(Y.cpu().numpy(), want.cpu().numpy(), what=f"block {k}")
        del block, Y, Xb                                         # the next block may get this one's addresses
        if k == 0:
            before = _lib.runtime_counters()                     # (the first block sized the stream's scratch)
    after = _lib.runtime_counters()
    assert after["launch_frees"] == before["launch_frees"]


def test_other_layers_refuse_a_block():
    b = bundle()
    block = SampledBlock.sample(b.row_pointers, b.column_index, torch.from_numpy(ref.seed_sets()[64]).cuda(), 5, 3, partSize=32)
    X = torch.randn(block.num_src, 8, device="cuda")
    for layer in (ops.GCNConv(8, 4), ops.GINConv(8, 4), ops.GATConv(8, 4)):
        with pytest.raises(TypeError, match="GraphSAGE operators"):
            layer.cuda()(X, block)
    with pytest.raises(TypeError, match="float32"):
        ops.SAGEConv(8, 4).cuda().half()(X.half(), block)

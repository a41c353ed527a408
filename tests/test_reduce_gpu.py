"""gnna_agg_reduce_ld_f32 / gnna_scatter_arg_ld_f32 through _lib, on the GPU.

A max does not round, so values AND positions are compared with torch.equal against a numpy reference on the CPU: per row,
np.argmax / np.argmin over X[column_index[rp[i]:rp[i + 1]]] along axis 0 (first occurrence = smallest position) plus rp[i];
0 and -1 for rows without edges."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph
from util import assert_close_f64, make_case

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 7, 8, 16, 32, 41, 64, 100, 128, 256, 602)
PART_SIZES = (1, 3, 32, 512)
OPS = ((_lib.REDUCE_MAX, "max"), (_lib.REDUCE_MIN, "min"))


def _reference(rp, ci, X, op, rows=None, num_rows=None):
    """(values float32 [R, D], arg int32 [R, D], rows with a tied extreme, rows with edges) for `rows` (default: all)."""
    rp, ci, X = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(X, dtype=np.float32)
    rows = np.arange((len(rp) - 1) if num_rows is None else num_rows) if rows is None else np.asarray(rows)
    vals = np.zeros((len(rows), X.shape[1]), dtype=np.float32)
    arg = np.full((len(rows), X.shape[1]), -1, dtype=np.int32)
    tied = nonempty = 0
    for k, i in enumerate(rows):
        b, e = rp[i], rp[i + 1]
        if e <= b:
            continue
        nonempty += 1
        block = X[ci[b:e]]
        a = block.argmax(0) if op == _lib.REDUCE_MAX else block.argmin(0)
        vals[k] = block[a, np.arange(X.shape[1])]
        arg[k] = a + b
        tied += bool(((block == vals[k]).sum(0) > 1).any())
    return vals, arg, tied, nonempty


def _features(n, d, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "randint":
        return torch.randint(-2, 3, (n, d), generator=gen).float()
    return torch.randn(n, d, generator=gen)


def _check(out, arg, ref_v, ref_a, what):
    assert torch.equal(out.cpu(), torch.from_numpy(ref_v)), f"{what}: values differ"
    if arg is not None:
        assert torch.equal(arg.cpu(), torch.from_numpy(ref_a)), f"{what}: positions differ"


@pytest.mark.parametrize("xkind", ["randn", "randint"])
@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_values_and_positions_are_exact(kind, xkind):
    n, e = (3000, 40000) if kind == "uniform" else (3000, 60000)
    g, _, _, _ = make_case(n, e, 1, 32, seed=3, kind=kind)
    rp, ci = g.row_pointers.numpy(), g.column_index.numpy()
    if kind == "powerlaw":          # rows without edges and one very long row
        deg = np.diff(rp)
        assert (deg == 0).sum() == 18 and deg.max() == 1128
    parts = {ps: [t.cuda() for t in _lib.build_part(ps, g.row_pointers)] for ps in PART_SIZES}
    ci_d = g.column_index.cuda()
    for d in WIDTHS:
        X = _features(n, d, xkind, seed=100 + d)
        Xd = X.cuda()
        for op, name in OPS:
            ref_v, ref_a, tied, nonempty = _reference(rp, ci, X.numpy(), op)
            if xkind == "randint":
                # five values: ties are the rule, so this IS the test of the tie contract
                assert tied > nonempty / 2, f"only {tied} of {nonempty} rows have a tied extreme: the case no longer tests ties"
            for ps in PART_SIZES:
                pp, p2n = parts[ps]
                out, arg = _lib.agg_reduce_ld(op, Xd, ci_d, pp, p2n, ps)
                _check(out, arg, ref_v, ref_a, f"{kind} {xkind} {name} D={d} partSize={ps}")


def _reference_partition(ci, pp, p2n, X, op, n_out):
    """The same reference over a partition AS GIVEN: row r reduces the positions of all its groups [pp[p], pp[p + 1]) (a pair
    with pp[p + 1] <= pp[p] is an empty group); among equal values the smallest position."""
    X = np.asarray(X, dtype=np.float32)
    d = X.shape[1]
    pos_of = {}
    for p, r in enumerate(np.asarray(p2n).tolist()):
        if pp[p + 1] > pp[p]:
            pos_of.setdefault(r, []).append(np.arange(pp[p], pp[p + 1]))
    vals = np.zeros((n_out, d), dtype=np.float32)
    arg = np.full((n_out, d), -1, dtype=np.int32)
    for r, chunks in pos_of.items():
        pos = np.unique(np.concatenate(chunks))
        block = X[ci[pos]]
        a = block.argmax(0) if op == _lib.REDUCE_MAX else block.argmin(0)
        vals[r], arg[r] = block[a, np.arange(d)], pos[a]
    return vals, arg


@pytest.mark.parametrize("d", [64, 7])
@pytest.mark.parametrize("ps", [1, 8])
def test_shuffled_partition_and_reversed_pairs(d, ps):
    """Groups in shuffled order (part2Node permuted with them, rows split over distant groups), plus an empty group and a pair
    of part_pointers that runs backwards: the answer is the reduction over the partition as given."""
    g, _, pp0, p2n0 = make_case(3000, 60000, 1, ps, seed=3, kind="powerlaw")
    P = p2n0.numel()
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(1))
    # a shuffled partition cannot share one pointer array, so every group gets its own [start, end) pair through a
    # column_index that repeats the group's ids in the new order
    lens = (pp0[1:] - pp0[:-1]).long()[perm]
    pp = torch.zeros(P + 1, dtype=torch.int64)
    pp[1:] = torch.cumsum(lens, 0)
    starts = pp0[:-1].long()[perm]
    src = torch.repeat_interleave(starts - pp[:-1], lens) + torch.arange(int(pp[-1]))
    ci_new = g.column_index[src].contiguous()
    p2n = p2n0[perm].clone()
    pp = pp.int()
    # an empty group and a negative range in the middle (the group behind them re-reads 5 positions for its own row)
    mid = P // 2
    cut = int(pp[mid])
    pp = torch.cat([pp[:mid + 1], torch.tensor([cut, cut - 5], dtype=torch.int32), pp[mid + 1:]])
    p2n = torch.cat([p2n[:mid], torch.tensor([5, 6], dtype=torch.int32), p2n[mid:]])
    assert (pp[1:] < pp[:-1]).any() and (pp[1:] == pp[:-1]).any() and not torch.equal(p2n, p2n.sort().values)
    for xkind in ("randint", "randn"):
        X = _features(3000, d, xkind, seed=7)
        for op, name in OPS:
            ref_v, ref_a = _reference_partition(ci_new.numpy(), pp.numpy(), p2n.numpy(), X.numpy(), op, 3000)
            out, arg = _lib.agg_reduce_ld(op, X.cuda(), ci_new.cuda(), pp.cuda(), p2n.cuda(), ps)
            _check(out, arg, ref_v, ref_a, f"shuffled {xkind} {name} D={d} partSize={ps}")


def _hub_graph(n=20000, edges=300000, hub=7, hub_edges=5000, seed=11):
    g = graph.uniform_graph(n, edges, seed=seed)
    rp, ci = g.row_pointers.numpy().astype(np.int64), g.column_index.numpy().astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    extra = np.random.RandomState(seed).choice(n, size=hub_edges, replace=False)
    key = np.unique(np.concatenate([rows * n + ci, hub * n + extra]))
    rows, cols = key // n, key % n
    rp2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp2[1:])
    return torch.from_numpy(rp2.astype(np.int32)), torch.from_numpy(cols.astype(np.int32)), hub


@pytest.mark.parametrize("d", [64, 7])
def test_hub_row_spanning_many_wavefronts(d):
    """partSize 1 over 300 k edges: the library takes 64 groups per wavefront, and the hub row's ~5000 groups span ~80 of them."""
    rp, ci, hub = _hub_graph()
    n = rp.numel() - 1
    assert int(rp[hub + 1] - rp[hub]) > 64 * 1 * 4 and ci.numel() // 64 >= _lib.device_cus() * 16
    pp, p2n = [t.cuda() for t in _lib.build_part(1, rp)]
    for xkind in ("randn", "randint"):
        X = _features(n, d, xkind, seed=21)
        for op, name in OPS:
            ref_v, ref_a, _, _ = _reference(rp.numpy(), ci.numpy(), X.numpy(), op)
            out, arg = _lib.agg_reduce_ld(op, X.cuda(), ci.cuda(), pp, p2n, 1)
            _check(out, arg, ref_v, ref_a, f"hub {xkind} {name} D={d}")


def test_rectangular_strided_null_arg_relu():
    g, _, pp, p2n = make_case(3000, 60000, 1, 32, seed=3, kind="powerlaw")
    rp, ci = g.row_pointers.numpy(), g.column_index.numpy()
    n, n_out = 3000, 1777
    ci_d = g.column_index.cuda()
    # the partition of the first n_out rows only: a shard
    pp_s, p2n_s = [t.cuda() for t in _lib.build_part(32, g.row_pointers[:n_out + 1].contiguous())]
    big = _features(n, 256, "randn", seed=9).cuda()
    X = big[:, 64:128]                                        # a 64-column block of a 256-wide matrix
    assert X.stride(0) == 256 and not X.is_contiguous()
    for op, name in OPS:
        ref_v, ref_a, _, _ = _reference(rp, ci, X.cpu().numpy(), op, num_rows=n_out)
        out_big = torch.full((n_out, 256), float("nan"), device="cuda")
        arg_big = torch.full((n_out, 256), -7, dtype=torch.int32, device="cuda")
        out, arg = _lib.agg_reduce_ld(op, X, ci_d, pp_s, p2n_s, 32, num_out_rows=n_out, out=out_big[:, 128:192],
                                      arg=arg_big[:, 64:128])
        _check(out, arg, ref_v, ref_a, f"rect strided {name}")
        # nothing outside the two blocks was touched
        assert torch.isnan(out_big[:, :128]).all() and torch.isnan(out_big[:, 192:]).all()
        assert (arg_big[:, :64] == -7).all() and (arg_big[:, 128:] == -7).all()
        out2, arg2 = _lib.agg_reduce_ld(op, X, ci_d, pp_s, p2n_s, 32, num_out_rows=n_out, want_arg=False)
        assert arg2 is None
        _check(out2, None, ref_v, ref_a, f"arg = NULL {name}")
        out3, arg3 = _lib.agg_reduce_ld(op, X, ci_d, pp_s, p2n_s, 32, num_out_rows=n_out, relu=True)
        _check(out3, arg3, np.maximum(ref_v, np.float32(0)), ref_a, f"relu {name}")


def test_refusals():
    g, X, pp, p2n = make_case(300, 3000, 16, 32, seed=3)
    Xd, ci, pp, p2n = X.cuda(), g.column_index.cuda(), pp.cuda(), p2n.cuda()
    out = torch.empty(300, 16, device="cuda")
    arg = torch.empty(300, 16, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def call(op=0, ld_in=16, ld_out=16, ld_arg=16, dim=16, flags=0):
        return lib.gnna_agg_reduce_ld_f32(op, Xd.data_ptr(), ld_in, 300, ci.data_ptr(), pp.data_ptr(), p2n.data_ptr(),
                                          out.data_ptr(), ld_out, arg.data_ptr(), ld_arg, 300, dim, p2n.numel(), 32, flags, None)
    INVALID_ARGUMENT, UNSUPPORTED = -1, -3                           # include/gnna.h
    assert call() == 0
    assert call(flags=_lib.ACCUMULATE) == UNSUPPORTED
    for kw in (dict(op=2), dict(op=-1), dict(dim=0), dict(ld_in=15), dict(ld_out=15), dict(ld_arg=15), dict(flags=4)):
        assert call(**kw) == INVALID_ARGUMENT, kw
    assert call(flags=_lib.EPILOGUE_RELU) == 0
    torch.cuda.synchronize()


def test_deterministic_tuning():
    g, X, pp, p2n = make_case(3000, 60000, 64, 32, seed=3, kind="powerlaw")
    Xd, ci, pp, p2n = X.cuda(), g.column_index.cuda(), pp.cuda(), p2n.cuda()
    out0, arg0 = _lib.agg_reduce_ld(_lib.REDUCE_MAX, Xd, ci, pp, p2n, 32)
    try:
        _lib.set_tuning(deterministic=1)
        out1, arg1 = _lib.agg_reduce_ld(_lib.REDUCE_MAX, Xd, ci, pp, p2n, 32)
        assert torch.equal(out0, out1) and torch.equal(arg0, arg1)
        with pytest.raises(_lib.GnnaError, match="deterministic"):
            _lib.scatter_arg_ld(out1, arg1, ci, 3000)
    finally:
        _lib.reset_tuning()
    _lib.scatter_arg_ld(out0, arg0, ci, 3000)
    torch.cuda.synchronize()


def _scatter_f64(go, arg, ci, n_in):
    go, arg, ci = go.double().cpu(), arg.cpu().long(), ci.cpu().long()
    ref = torch.zeros(n_in, go.shape[1], dtype=torch.float64)
    scale = torch.zeros_like(ref)
    cols = torch.arange(go.shape[1]).expand_as(arg)
    m = arg >= 0
    flat = ci[arg[m]] * go.shape[1] + cols[m]
    ref.view(-1).index_add_(0, flat, go[m])
    scale.view(-1).index_add_(0, flat, go[m].abs())
    return ref, scale


@pytest.mark.parametrize("d", [64, 41, 1])
def test_scatter_arg_against_fp64(d):
    g, _, pp, p2n = make_case(3000, 60000, 1, 32, seed=3, kind="powerlaw")
    ci = g.column_index.cuda()
    X = _features(3000, d, "randint", seed=4).cuda()          # ties: hub sources win many rows and receive many adds
    _, arg = _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp.cuda(), p2n.cuda(), 32)
    assert (arg < 0).any() and (arg >= 0).any()               # rows without edges send nothing
    go = torch.randn(3000, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    ref, scale = _scatter_f64(go, arg, ci, 3000)
    assert float(scale.max()) > 20 * float(go.abs().mean())   # some element really is a sum of many terms
    gi = _lib.scatter_arg_ld(go, arg, ci, 3000)
    assert_close_f64(gi.cpu().numpy(), ref.numpy(), scale=scale.numpy(), what=f"scatter_arg D={d}")
    base = torch.randn(3000, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    acc = base.clone()
    same = _lib.scatter_arg_ld(go, arg, ci, 3000, out=acc, accumulate=True)
    assert same is acc
    assert_close_f64(acc.cpu().numpy(), (ref + base.double().cpu()).numpy(), scale=(scale + base.double().abs().cpu()).numpy(),
                     what=f"scatter_arg accumulate D={d}")
    # strided gradient, positions and result: 64-column blocks of wider matrices
    if d == 64:
        go_b = torch.zeros(3000, 256, device="cuda"); go_b[:, 64:128] = go
        arg_b = torch.full((3000, 256), -1, dtype=torch.int32, device="cuda"); arg_b[:, 128:192] = arg
        gi_b = torch.full((3000, 256), float("nan"), device="cuda")
        _lib.scatter_arg_ld(go_b[:, 64:128], arg_b[:, 128:192], ci, 3000, out=gi_b[:, 0:64])
        assert_close_f64(gi_b[:, 0:64].cpu().numpy(), ref.numpy(), scale=scale.numpy(), what="scatter_arg strided")
        assert torch.isnan(gi_b[:, 64:]).all()


def _pair(X, ci, pp, p2n, go, out, arg, gi):
    """reduce + scatter: the forward and backward of one NeighborMax."""
    _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, 32, out=out, arg=arg)
    _lib.scatter_arg_ld(go, arg, ci, X.shape[0], out=gi)


def test_captured_pair_without_warm_up_replayed_with_new_inputs():
    g, _, pp, p2n = make_case(3000, 60000, 1, 32, seed=3, kind="powerlaw")
    ci, pp, p2n = g.column_index.cuda(), pp.cuda(), p2n.cuda()
    n, d = 3000, 64
    X = _features(n, d, "randn", seed=30).cuda()
    # an integer-valued gradient: its sums are exact in fp32 in any order, so the scatter can be compared bit for bit too
    go = torch.randint(-4, 5, (n, d), generator=torch.Generator().manual_seed(31)).float().cuda()
    out, gi = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
    arg = torch.empty(n, d, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=torch.cuda.Stream()):    # a stream that never ran the library: no eager scratch on it
        _pair(X, ci, pp, p2n, go, out, arg, gi)
    for rep in range(3):
        X.copy_(_features(n, d, "randn", seed=40 + rep))
        out.fill_(float("nan")); gi.fill_(float("nan")); arg.fill_(-9)
        gr.replay()
        torch.cuda.synchronize()
        e_out, e_arg = _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, 32)
        e_gi = _lib.scatter_arg_ld(go, e_arg, ci, n)
        ref_v, ref_a, _, _ = _reference(g.row_pointers.numpy(), g.column_index.numpy(), X.cpu().numpy(), _lib.REDUCE_MAX)
        _check(e_out, e_arg, ref_v, ref_a, f"eager, replay {rep}")
        assert torch.equal(out, e_out) and torch.equal(arg, e_arg) and torch.equal(gi, e_gi), f"replay {rep}"


def test_two_graphs_on_the_default_capture_stream_side_by_side():
    g, _, pp, p2n = make_case(3000, 60000, 1, 32, seed=3, kind="powerlaw")
    ci, pp, p2n = g.column_index.cuda(), pp.cuda(), p2n.cuda()
    n, d = 3000, 64
    X0 = _features(n, d, "randn", seed=50).cuda()
    Xs = [X0, 3 - X0]
    go = torch.randint(-4, 5, (n, d), generator=torch.Generator().manual_seed(51)).float().cuda()
    bufs = [(torch.empty(n, d, device="cuda"), torch.empty(n, d, dtype=torch.int32, device="cuda"), torch.empty(n, d, device="cuda"))
            for _ in Xs]
    torch.cuda.synchronize()
    graphs = []
    for X, (out, arg, gi) in zip(Xs, bufs):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):                            # torch's one class-wide capture stream
            _pair(X, ci, pp, p2n, go, out, arg, gi)
        graphs.append(gr)
    torch.cuda.synchronize()
    expect = []
    for X in Xs:
        e_out, e_arg = _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, 32)
        expect.append((e_out, e_arg, _lib.scatter_arg_ld(go, e_arg, ci, n)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(6):
        for out, arg, gi in bufs:
            out.fill_(float("nan")); gi.fill_(float("nan")); arg.fill_(-9)
        torch.cuda.synchronize()
        for s, gr in zip(streams, graphs):
            with torch.cuda.stream(s):
                gr.replay()
        torch.cuda.synchronize()
        for k, ((out, arg, gi), (e_out, e_arg, e_gi)) in enumerate(zip(bufs, expect)):
            assert torch.equal(out, e_out) and torch.equal(arg, e_arg) and torch.equal(gi, e_gi), f"graph {k}, replay {rep}"


def test_reddit_like_full_size():
    g = graph.make_config_graph("reddit-like", device="cuda")
    n, ci = g.num_nodes, g.column_index
    pp, p2n = [t.cuda() for t in _lib.build_part(32, g.row_pointers.cpu())]
    X = torch.randn(n, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    rp_h, ci_h, X_h = g.row_pointers.cpu().numpy(), ci.cpu().numpy(), X.cpu().numpy()
    empty = np.where(np.diff(rp_h) == 0)[0]
    sample = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:4096].numpy()
    rows = np.unique(np.concatenate([sample, empty]))
    for op, name in OPS:
        out, arg = _lib.agg_reduce_ld(op, X, ci, pp, p2n, 32)
        ref_v, ref_a, _, _ = _reference(rp_h, ci_h, X_h, op, rows=rows)
        idx = torch.from_numpy(rows).cuda()
        _check(out[idx], arg[idx], ref_v, ref_a, f"Reddit-like {name}")
        assert not torch.isnan(out).any() and int(arg.min()) >= -1 and int(arg.max()) < ci.numel()

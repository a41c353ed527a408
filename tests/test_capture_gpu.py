"""Captured graphs the way PyTorch callers make them, held to fp64.

The other capture tests own their capture stream and warm it up.  ``torch.cuda.graph(g)`` without ``stream=`` captures every
graph on one class-wide side stream, and ``torch.cuda.make_graphed_callables`` warms up on a throw-away stream and then
captures there with no eager call first.  So: two graphs captured on that one stream and replayed side by side (one case per
user of library scratch: the staged copy of X, the pre-scaled GCN copy, the deterministic schedule's partial rows, the
weight-gradient slabs, SDDMM's staged source side), eager calls on the capture stream next to a replay, a whole GCN -> GIN
model under make_graphed_callables, SDDMM captured on a stream that never ran it, and the full id hash of a packed copy run
from two streams at once.  Outputs are NaN-filled before every replay; every result is compared with fp64."""
import numpy as np
import pytest
import torch

import oracle
from gnnadvisor_osdi21_amd import _lib, decider, graph, load_extension
from util import assert_close_f64, gcn_gin_reference

pytestmark = pytest.mark.gpu

REPLAYS = 12


def _capture_stream():
    """The stream torch.cuda.graph captures on when it is given none (created lazily by torch)."""
    if torch.cuda.graph.default_capture_stream is None:
        torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
    return torch.cuda.graph.default_capture_stream


_HOT = {}


def _hot_graph():
    """Average degree 150 (every source row gathered >= 32 times): D = 17..64 rows are staged, GCN pre-scales."""
    if "g" not in _HOT:
        g = graph.powerlaw_graph(20000, 3_000_000, 3000, seed=71, device="cuda")
        pp, p2n = _lib.build_part(32, g.row_pointers.cpu())
        rp, ci = g.row_pointers.cpu().numpy(), g.column_index.cpu().numpy()
        _HOT["g"] = (g, pp.cuda(), p2n.cuda(), rp, ci)
    return _HOT["g"]


def _features(n, d, seed):
    return torch.randn(n, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _edge_rows(rp):
    return torch.repeat_interleave(torch.arange(len(rp) - 1, device="cuda"), torch.as_tensor(np.diff(rp), device="cuda"))


def _sddmm_f64(A, B, rows, ci):
    """out[e] = <A[row(e)], B[ci[e]]> and its sum of |terms|, in fp64 (chunked on the device)."""
    cl = ci.long()
    ref = torch.empty(cl.numel(), dtype=torch.float64, device="cuda")
    scale = torch.empty_like(ref)
    for c0 in range(0, cl.numel(), 1 << 20):
        a, b = A[rows[c0:c0 + (1 << 20)]].double(), B[cl[c0:c0 + (1 << 20)]].double()
        ref[c0:c0 + (1 << 20)] = (a * b).sum(1)
        scale[c0:c0 + (1 << 20)] = (a.abs() * b.abs()).sum(1)
    return ref.cpu().numpy(), scale.cpu().numpy()


def _case(kind, k):
    """(call(out), out, fp64 reference, scale) of scratch user `kind` for input set k (k = 1: 3 - the inputs of k = 0)."""
    g, pp, p2n, rp, ci = _hot_graph()
    n = g.num_nodes
    flip = (lambda t: 3.0 - t) if k else (lambda t: t)
    if kind in ("stage64", "stage41_pad", "det"):
        d = 41 if kind == "stage41_pad" else 64
        X = flip(_features(n, d, 5 + d))
        out = torch.empty(n, d, device="cuda")
        Xh = X.cpu().numpy()
        ref = oracle.csr_f64(0, Xh, rp, ci)
        scale = oracle.csr_f64(0, np.abs(Xh), rp, ci)
        return (lambda o: _lib.agg_ld(0, X, g.column_index, pp, p2n, n, 32, out=o)), out, ref, scale
    if kind == "gcn_prescale":
        X = flip(_features(n, 64, 9))
        deg = g.degrees.cuda()
        out = torch.empty(n, 64, device="cuda")
        Xh, dh = X.cpu().numpy(), g.degrees.cpu().numpy()
        ref = oracle.csr_f64(1, Xh, rp, ci, dh)
        scale = oracle.csr_f64(1, np.abs(Xh), rp, ci, dh)
        return (lambda o: _lib.agg_gcn(X, g.row_pointers, g.column_index, deg, pp, p2n, out=o)), out, ref, scale
    if kind == "xtg":
        M, K, N = 120000, 64, 48            # 2 tiles, hundreds of row slabs
        X = flip(_features(M, K, 11))
        G = flip(_features(M, N, 12))
        out = torch.empty(K, N, device="cuda")
        Xh, Gh = X.double().cpu().numpy(), G.double().cpu().numpy()
        return (lambda o: _lib.xtg(X, G, out=o)), out, Xh.T @ Gh, np.abs(Xh).T @ np.abs(Gh)
    if kind == "sddmm":
        A = flip(_features(n, 64, 13))
        B = flip(_features(n, 64, 14))
        out = torch.empty(g.column_index.numel(), device="cuda")
        ref, scale = _sddmm_f64(A, B, _edge_rows(rp), g.column_index)
        return (lambda o: _lib.sddmm(A, B, g.column_index, pp, p2n, 32, out=o)), out, ref, scale
    raise AssertionError(kind)


def _tuning(kind, delayed):
    knobs = dict(ids_check_every=1 << 30)
    if kind == "stage41_pad":
        knobs["pad_rows"] = 1
    if kind == "gcn_prescale":
        knobs["gcn_prescale"] = 1
    if kind == "det":
        knobs["deterministic"] = 1
    if delayed:
        knobs["sweep"] = 2                  # the streaming kernel: one long main kernel behind the staging pass
    return knobs


def _replay_ms(gr, reps=3):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gr.replay()
    t0.record()
    for _ in range(reps):
        gr.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def _sleep_cycles_per_ms():
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    t0.record()
    torch.cuda._sleep(2_000_000)
    t1.record()
    torch.cuda.synchronize()
    return 2_000_000 / max(t0.elapsed_time(t1), 1e-3)


@pytest.mark.parametrize("delayed", [False, True], ids=["default", "delayed"])
@pytest.mark.parametrize("kind", ["stage64", "stage41_pad", "gcn_prescale", "det", "xtg", "sddmm"])
def test_two_graphs_on_the_default_capture_stream_replayed_side_by_side(kind, delayed):
    """Two graphs captured with plain torch.cuda.graph(g) -- one capture stream -- over different inputs (X and 3 - X),
    replayed at the same time on two streams: each must read only its own scratch.  `delayed`: the second replay starts
    behind a calibrated sleep, so that its scratch-writing first kernel lands inside the first graph's main kernel."""
    _lib.reset_tuning()
    _lib.set_tuning(**_tuning(kind, delayed))
    try:
        cases = [_case(kind, k) for k in (0, 1)]
        cap = _capture_stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(cap):                 # the warm-up the library used to ask for: eager scratch on that stream
            for call, out, _, _ in cases:
                call(out)
        torch.cuda.synchronize()
        graphs = []
        for call, out, _, _ in cases:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                call(out)
            graphs.append(gr)
        torch.cuda.synchronize()
        delays = [0]
        if delayed:
            per_ms = _sleep_cycles_per_ms()
            ms = _replay_ms(graphs[0])
            delays = [int(per_ms * ms * f) for f in (0.1, 0.25, 0.4, 0.55, 0.7, 0.85)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        first = [None, None]
        for rep in range(REPLAYS):
            for _, out, _, _ in cases:
                out.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                graphs[0].replay()
            with torch.cuda.stream(streams[1]):
                if delays[rep % len(delays)]:
                    torch.cuda._sleep(delays[rep % len(delays)])
                graphs[1].replay()
            torch.cuda.synchronize()
            for k, (_, out, ref, scale) in enumerate(cases):
                got = out.cpu().numpy()
                assert_close_f64(got, ref, scale=scale, what=f"{kind}: graph {k}, side-by-side replay {rep}")
                if kind == "det":                   # the deterministic schedule: every replay bit-identical to the first
                    if first[k] is None:
                        first[k] = got.copy()
                    assert np.array_equal(got, first[k]), f"det: graph {k}, replay {rep} differs from replay 0"
    finally:
        _lib.reset_tuning()


def test_eager_calls_on_the_capture_stream_next_to_a_replay():
    """After a capture, eager calls on the capture stream -- the same shape with other X, then a larger one -- run while the
    graph replays on another stream: the graph keeps its own staged copy, the eager calls theirs."""
    g, pp, p2n, rp, ci = _hot_graph()
    n = g.num_nodes
    big = graph.powerlaw_graph(60000, 6_000_000, 4000, seed=72, device="cuda")
    bpp, bp2n = (t.cuda() for t in _lib.build_part(32, big.row_pointers.cpu()))
    _lib.reset_tuning()
    _lib.set_tuning(sweep=2, ids_check_every=1 << 30)
    try:
        X = _features(n, 64, 21)
        Y = 3.0 - X
        Xb = _features(big.num_nodes, 64, 22)
        ref_x = oracle.csr_f64(0, X.cpu().numpy(), rp, ci)
        ref_y = oracle.csr_f64(0, Y.cpu().numpy(), rp, ci)
        ref_b = oracle.csr_f64(0, Xb.cpu().numpy(), big.row_pointers.cpu().numpy(), big.column_index.cpu().numpy())
        out, oy = torch.empty(n, 64, device="cuda"), torch.empty(n, 64, device="cuda")
        ob = torch.empty(big.num_nodes, 64, device="cuda")
        cap = _capture_stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(cap):
            _lib.agg_ld(0, X, g.column_index, pp, p2n, n, 32, out=out)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            _lib.agg_ld(0, X, g.column_index, pp, p2n, n, 32, out=out)
        side = torch.cuda.Stream()
        for rep in range(REPLAYS):
            for t in (out, oy, ob):
                t.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                gr.replay()
            with torch.cuda.stream(cap):
                _lib.agg_ld(0, Y, g.column_index, pp, p2n, n, 32, out=oy)
                if rep % 3 == 2:
                    _lib.agg_ld(0, Xb, big.column_index, bpp, bp2n, big.num_nodes, 32, out=ob)
            torch.cuda.synchronize()
            assert_close_f64(out.cpu().numpy(), ref_x, what=f"graph next to eager calls, replay {rep}")
            assert_close_f64(oy.cpu().numpy(), ref_y, what=f"eager call next to the replay, {rep}")
            if rep % 3 == 2:
                assert_close_f64(ob.cpu().numpy(), ref_b, what=f"larger eager call next to the replay, {rep}")
    finally:
        _lib.reset_tuning()


class _DS:
    def __init__(self, g, feat):
        self.num_nodes, self.avg_degree, self.avg_edgeSpan = g.num_nodes, g.avg_degree, g.avg_edgeSpan
        self.num_features = feat
        self.reorder_flag = False

    def rabbit_reorder(self):
        pass


def _info(g, feat, hidden, partSize=32):
    GNNA = load_extension()
    ip = decider.inputProperty(g.row_pointers, g.column_index, g.degrees.cuda(), partSize, 32, 4, 100,
                               hiddenDim=hidden, dataset_obj=_DS(g, feat), manual_mode=True)
    ip.decider()
    pp, p2n = GNNA.build_part(ip.partSize, ip.row_pointers)
    ip.row_pointers = ip.row_pointers.cuda(); ip.column_index = ip.column_index.cuda()
    ip.partPtr = pp.int().cuda(); ip.part2Node = p2n.int().cuda()
    return ip.set_hidden()


def test_make_graphed_callables_over_a_gcn_gin_model():
    """GCN -> ReLU -> GIN from ops, hidden 64 on a hot-row graph, wrapped in torch.cuda.make_graphed_callables (warm-up on a
    throw-away stream, capture on torch's side stream, no eager call there): three fresh inputs, out / dF / dW1 / dW2
    against the fp64 network."""
    from gnnadvisor_osdi21_amd import ops
    g = graph.powerlaw_graph(12000, 1_200_000, 2000, seed=73)
    fin, hid, ncls = 40, 64, 16
    info = _info(g, fin, hid)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.c2 = ops.GCNConv(fin, hid), ops.GINConv(hid, ncls)

        def forward(self, X):
            h1 = self.c1(X, info)
            return self.c2(torch.relu(h1), info), h1

    torch.manual_seed(4)
    net = Net().cuda()
    _lib.reset_tuning()
    # (torch's side stream as a fresh process has it: no library call has ever run on it)
    saved_stream, torch.cuda.graph.default_capture_stream = torch.cuda.graph.default_capture_stream, torch.cuda.Stream()
    try:
        sample = torch.randn(g.num_nodes, fin, device="cuda", requires_grad=True)
        gnet = torch.cuda.make_graphed_callables(net, (sample,))
        wgt = torch.linspace(0.5, 1.5, ncls, device="cuda")
        for it in range(3):
            X = torch.randn(g.num_nodes, fin, generator=torch.Generator().manual_seed(100 + it)).cuda().requires_grad_(True)
            net.zero_grad(set_to_none=True)
            y, h1 = gnet(X)
            (y * wgt).sum().backward()
            torch.cuda.synchronize()
            ref = gcn_gin_reference(g, X.detach().cpu(), net.c1.weights.detach().cpu(), net.c2.weights.detach().cpu(), wgt,
                                    H1_got=h1)
            assert ref["ambiguous"] <= 16 + 1e-3 * h1.numel()
            for k, v in (("out", y), ("H1", h1), ("dF", X.grad), ("dW1", net.c1.weights.grad), ("dW2", net.c2.weights.grad)):
                assert_close_f64(v.detach().cpu().numpy(), ref[k][0], what=f"graphed model, input {it}: {k}", scale=ref[k][1])
    finally:
        torch.cuda.graph.default_capture_stream = saved_stream
        _lib.reset_tuning()


def test_sddmm_first_captured_on_a_prepared_graph():
    """A prepared graph, and SDDMM captured on a stream that never ran it (no warm-up): the capture succeeds and the replay
    is the dense formula."""
    g, pp, p2n, rp, ci = _hot_graph()
    n = g.num_nodes
    _lib.reset_tuning()
    A, B = _features(n, 64, 31), _features(n, 64, 32)
    ref, scale = _sddmm_f64(A, B, _edge_rows(rp), g.column_index)
    try:
        _lib.prepare_graph(g.column_index, pp, p2n, n, n, 32, [64])
        out = torch.empty(g.column_index.numel(), device="cuda")
        torch.cuda.synchronize()
        before = _lib.runtime_counters()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=torch.cuda.Stream()):
            _lib.sddmm(A, B, g.column_index, pp, p2n, 32, out=out)
        after = _lib.runtime_counters()
        assert after["capture_scratch"] > before["capture_scratch"], "the staged source side got no scratch of its capture"
        assert after["launch_mallocs"] == before["launch_mallocs"] and after["launch_frees"] == before["launch_frees"]
        for rep in range(3):
            out.fill_(float("nan"))
            gr.replay()
            torch.cuda.synchronize()
            assert_close_f64(out.cpu().numpy(), ref, scale=scale, what=f"captured sddmm, replay {rep}")
    finally:
        _lib.release_graph(g.column_index)
        _lib.reset_tuning()


def test_full_id_hash_from_two_streams_keeps_the_packed_copy_trusted():
    """ids_check_every = 1 on a prepared graph: every call also hashes all of column_index into the packed copy's state.
    32 calls on each of two streams, interleaved without a sync: every result is right and no copy ends up marked
    "never trust again".  Control: a real in-place rewrite of column_index still marks it."""
    g = graph.powerlaw_graph(20000, 2_000_000, 3000, seed=74, device="cuda")
    n = g.num_nodes
    pp, p2n = (t.cuda() for t in _lib.build_part(32, g.row_pointers.cpu()))
    ci = g.column_index.clone()
    rp = g.row_pointers.cpu().numpy()
    _lib.reset_tuning()
    _lib.set_tuning(column_phases=4, ids_check_every=1, sweep=2)
    try:
        _lib.prepare_graph(ci, pp, p2n, n, n, 32, [32])
        X = _features(n, 32, 41)
        ref = oracle.csr_f64(0, X.cpu().numpy(), rp, ci.cpu().numpy())
        outs = [torch.full((n, 32), float("nan"), device="cuda") for _ in range(64)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        c0 = _lib.runtime_counters()
        for i in range(64):
            with torch.cuda.stream(streams[i % 2]):
                _lib.agg_ld(0, X, ci, pp, p2n, n, 32, out=outs[i])
        torch.cuda.synchronize()
        c1 = _lib.runtime_counters()
        assert c1["full_hashes"] - c0["full_hashes"] == 64 and c1["packed_launches"] - c0["packed_launches"] == 64
        for i, o in enumerate(outs):
            assert_close_f64(o.cpu().numpy(), ref, what=f"call {i} (stream {i % 2})")
        assert _lib.debug_untrusted_copies(ci) == 0, "concurrent full hashes marked an unchanged graph's copy untrusted"
        # control: three ids rewritten in place (the samples miss them, the full hash does not)
        cpu_ci = ci.cpu()
        for r in (3, 1717, n - 5):
            b = int(rp[r])
            if int(rp[r + 1]) > b:
                cpu_ci[b] = (int(cpu_ci[b]) + 11) % n
        ci.copy_(cpu_ci.cuda())
        out = _lib.agg_ld(0, X, ci, pp, p2n, n, 32)
        torch.cuda.synchronize()
        assert_close_f64(out.cpu().numpy(), oracle.csr_f64(0, X.cpu().numpy(), rp, cpu_ci.numpy()), what="after the rewrite")
        assert _lib.debug_untrusted_copies(ci) >= 1, "the full hash missed a rewritten column_index"
    finally:
        _lib.release_graph(ci)
        _lib.reset_tuning()

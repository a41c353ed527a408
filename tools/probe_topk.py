#!/usr/bin/env python3
"""Times hierarchical pooling -- GraphBatch.coarsen (gnna_segment_topk_i32), the row gathers of ops.SelectRows and a whole
ops.TopKPooling forward + backward -- against the same function composed from torch ops (fused=False), on the shapes the readout
was timed on, and one graph_main.py epoch with and without --pool topk.

    python tools/probe_topk.py [--shapes small,medium,one] [--dims 64,128] [--reps 10] [--driver 1]

Per shape and width it prints one JSON line: ms per structure call (library / torch composition, alternated in one process,
medians), ms and achieved bytes/s of the two gather kernels next to torch.clone of the same bytes, ms per TopKPooling forward +
backward of both paths and their peak torch memory.  The composition is checked against the library's selection once before
timing.  The parent commit has no path for any of this: the composition is the yardstick (profiles/topk_pool/README.md).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import _lib, graph, graph_main, ops      # noqa: E402
from gnnadvisor_osdi21_amd.batching import GraphDataset              # noqa: E402

SHAPES = {                      # graphs, min nodes, max nodes
    "small": (65536, 8, 72),
    "medium": (64, 35000, 37000),
    "one": (1, 232965, 232965),
}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns, reps, warm=2):
    """Medians of ms per call of every function, the calls alternated."""
    ms = [[] for _ in fns]
    for k in range(reps + warm):
        for i, fn in enumerate(fns):
            t = timed(fn)
            if k >= warm:
                ms[i].append(t)
    return [statistics.median(m) for m in ms]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="small,medium,one")
    p.add_argument("--dims", default="64,128")
    p.add_argument("--ratio", type=float, default=0.5)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--driver", type=int, default=1, help="1: also one graph_main.py epoch with and without --pool topk")
    args = p.parse_args(argv)
    dev = torch.device("cuda")
    for name in args.shapes.split(","):
        G, lo, hi = SHAPES[name]
        rp, ci, gp = graph.small_graphs(G, lo, hi, 4.0, seed=1, device=dev)
        b = GraphDataset(rp, ci, gp).batch(torch.arange(G, device=dev))
        n, nnz = b.num_nodes, int(b.column_index.numel())
        score = torch.randn(n, device=dev)
        small, sel = b.coarsen(score, ratio=args.ratio)
        small_c, sel_c = ops._composed_coarsen(b, score, ratio=args.ratio)
        assert torch.equal(sel.perm, sel_c.perm) and torch.equal(small.column_index, small_c.column_index)
        assert torch.equal(small.partPtr, small_c.partPtr) and torch.equal(small.row_pointers, small_c.row_pointers)
        lib_ms, torch_ms = alternate([lambda: b.coarsen(score, ratio=args.ratio), lambda: ops._composed_coarsen(b, score, ratio=args.ratio)],
                                     args.reps)
        head = {"shape": name, "graphs": G, "num_nodes": n, "nnz": nnz, "kept_rows": small.num_nodes, "kept_edges": int(small.column_index.numel()),
                "ratio": args.ratio, "reps": args.reps}
        print(json.dumps(dict(head, what="structure", coarsen_ms_library=round(lib_ms, 3), coarsen_ms_torch=round(torch_ms, 3),
                              library_faster=lib_ms < torch_ms)), flush=True)
        m = small.num_nodes
        for dim in (int(d) for d in args.dims.split(",")):
            X = torch.randn(n, dim, device=dev)
            gate = torch.rand(n, device=dev)
            dY = torch.randn(m, dim, device=dev)
            out, dX, dS = torch.empty(m, dim, device=dev), torch.empty(n, dim, device=dev), torch.empty(n, device=dev)
            fwd_bytes = 2 * m * dim * 4 + 2 * m * 4
            bwd_bytes = (2 * m + n) * dim * 4 + 3 * n * 4
            clone_f, clone_b = torch.empty(fwd_bytes // 8, device=dev), torch.empty(bwd_bytes // 8, device=dev)
            perm64 = sel.perm.long()
            ms = alternate([lambda: _lib.gather_rows_scale(X, sel.perm, gate, out=out), lambda: clone_f.clone(),
                            lambda: gate[perm64].unsqueeze(1) * X[perm64],
                            lambda: _lib.gather_rows_scale_backward(dY, sel.new_id, X, gate, out={"d_input": dX, "d_scale": dS}),
                            lambda: clone_b.clone()], args.reps)
            layers = {fused: ops.TopKPooling(dim, ratio=args.ratio, fused=fused).to(dev) for fused in (True, False)}
            layers[False].load_state_dict(layers[True].state_dict())
            Xg = X.clone().requires_grad_()

            def step(fused):
                Xg.grad = None
                layers[fused].zero_grad(set_to_none=True)
                y = layers[fused](Xg, b)[0]
                y.sum().backward()

            step_lib, step_torch = alternate([lambda: step(True), lambda: step(False)], args.reps)
            res = dict(head, what="features", dim=dim,
                       gather_ms=round(ms[0], 4), gather_GBps=round(fwd_bytes / ms[0] / 1e6, 1), clone_same_bytes_ms=round(ms[1], 4),
                       clone_GBps=round(fwd_bytes / ms[1] / 1e6, 1), torch_index_mul_ms=round(ms[2], 4),
                       backward_ms=round(ms[3], 4), backward_GBps=round(bwd_bytes / ms[3] / 1e6, 1), clone_bwd_bytes_ms=round(ms[4], 4),
                       clone_bwd_GBps=round(bwd_bytes / ms[4] / 1e6, 1),
                       pooling_fwd_bwd_ms_fused=round(step_lib, 3), pooling_fwd_bwd_ms_composed=round(step_torch, 3),
                       peak_MiB_fused=round(peak_mb(lambda: step(True)), 1), peak_MiB_composed=round(peak_mb(lambda: step(False)), 1),
                       fused_faster=step_lib < step_torch)
            print(json.dumps(res), flush=True)
            del X, gate, dY, out, dX, dS, clone_f, clone_b, Xg, layers
        del b, small, small_c, sel, sel_c, rp, ci, gp, score
        torch.cuda.empty_cache()
    if args.driver:
        base = ["--num_graphs", "4096", "--batch_graphs", "256", "--num_epoches", "3", "--num_layers", "3"]
        res = {"what": "graph_main epoch", "args": " ".join(base)}
        for key, extra in (("no_pool", []), ("pool_topk_fused", ["--pool", "topk"]), ("pool_topk_composed", ["--pool", "topk", "--fused_pool", "False"])):
            seen = {}
            graph_main.main(base + extra, capture=seen)
            res[key + "_epoch_ms"] = round(seen["epoch_ms"], 2)
            res[key + "_final_loss"] = round(seen["final_loss"], 4)
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

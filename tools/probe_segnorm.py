#!/usr/bin/env python3
"""Times per-graph normalisation -- the moments pass (gnna_segment_moments_ld_f32), the forward (gnna_segment_norm_ld_f32) and a
whole ops.GraphNorm forward + backward -- against the same function composed from torch ops (fused=False), the library's own sum
readout of the same X and torch.clone of the bytes each pass must move, on the shapes the readout was timed on; and graph_main.py
epochs with --norm graph, fused and composed.

    python tools/probe_segnorm.py [--shapes small,medium,one] [--dims 64,128] [--reps 10] [--driver 1]

Per shape and width it prints one JSON line: medians of ms per call, the calls alternated in one process; achieved bytes/s of the
forward (3 N D 4 bytes: two reads of X, one write) and of forward + backward (8 N D 4: the forward's three and the backward's
five -- dY and X twice, dX once) next to torch.clone of the same bytes; the peak torch memory of a forward + backward of both paths.
The composition is checked against the fused path once before timing.  The parent commit has no path for any of this: the
composition is the yardstick (profiles/graph_norm/README.md).
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import _lib, graph_main, ops      # noqa: E402

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
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--driver", type=int, default=1, help="1: also graph_main.py epochs without --norm and with --norm graph, fused and composed")
    args = p.parse_args(argv)
    dev = torch.device("cuda")
    for name in args.shapes.split(","):
        G, lo, hi = SHAPES[name]
        sizes = torch.randint(lo, hi + 1, (G,), generator=torch.Generator().manual_seed(1))
        gp = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
        n = int(gp[-1])
        # the batch as the compositions take it: with its `batch` vector made once, as a GraphBatch keeps it
        batch = types.SimpleNamespace(graph_pointers=gp, batch=torch.repeat_interleave(torch.arange(G, device=dev), sizes.to(dev)))
        for dim in (int(d) for d in args.dims.split(",")):
            X = 1.0 + torch.randn(n, dim, device=dev)
            layers = {fused: ops.GraphNorm(dim, fused=fused).to(dev) for fused in (True, False)}
            with torch.no_grad():
                for layer in layers.values():
                    layer.weight.fill_(1.25), layer.bias.fill_(0.5), layer.mean_scale.fill_(0.75)
            w, b, a = layers[True].weight.detach(), layers[True].bias.detach(), layers[True].mean_scale.detach()
            with torch.no_grad():
                diff = float((layers[True](X, batch) - layers[False](X, batch)).abs().max())
            assert diff < 1e-3, diff
            stats = {k: torch.empty(G, dim, device=dev) for k in ("mean", "m2", "rstd", "sum")}
            out = torch.empty(n, dim, device=dev)
            fwd_bytes, both_bytes = 3 * n * dim * 4, 8 * n * dim * 4
            clone_f, clone_b = torch.empty(fwd_bytes // 8, device=dev), torch.empty(both_bytes // 8, device=dev)
            Xg = X.clone().requires_grad_()

            def step(fused):
                Xg.grad = None
                layers[fused].zero_grad(set_to_none=True)
                layers[fused](Xg, batch).sum().backward()

            def forward(fused):
                with torch.no_grad():
                    layers[fused](X, batch)

            ms = alternate([lambda: _lib.segment_moments(X, gp, out=dict(mean=stats["mean"], m2=stats["m2"])),
                            lambda: _lib.segment_pool(X, gp, want=("sum",), out=dict(sum=stats["sum"])),
                            lambda: _lib.segment_norm(X, gp, w, b, a, out=dict(out=out, mean=stats["mean"], rstd=stats["rstd"])),
                            lambda: forward(False), lambda: clone_f.clone(),
                            lambda: step(True), lambda: step(False), lambda: clone_b.clone()], args.reps)
            res = {"shape": name, "graphs": G, "num_nodes": n, "dim": dim, "reps": args.reps, "max_abs_fused_minus_composed": diff,
                   "moments_ms": round(ms[0], 4), "moments_GBps": round(n * dim * 4 / ms[0] / 1e6, 1), "sum_readout_ms": round(ms[1], 4),
                   "forward_ms_fused": round(ms[2], 4), "forward_GBps_fused": round(fwd_bytes / ms[2] / 1e6, 1),
                   "forward_ms_composed": round(ms[3], 4), "clone_forward_bytes_ms": round(ms[4], 4),
                   "clone_forward_GBps": round(fwd_bytes / ms[4] / 1e6, 1),
                   "fwd_bwd_ms_fused": round(ms[5], 4), "fwd_bwd_GBps_fused": round(both_bytes / ms[5] / 1e6, 1),
                   "fwd_bwd_ms_composed": round(ms[6], 4), "clone_fwd_bwd_bytes_ms": round(ms[7], 4),
                   "clone_fwd_bwd_GBps": round(both_bytes / ms[7] / 1e6, 1),
                   "peak_MiB_fused": round(peak_mb(lambda: step(True)), 1), "peak_MiB_composed": round(peak_mb(lambda: step(False)), 1),
                   "fused_faster": ms[5] < ms[6], "moments_slower_than_sum_readout": ms[0] > ms[1]}
            print(json.dumps(res), flush=True)
            del X, Xg, out, stats, clone_f, clone_b, layers
            torch.cuda.empty_cache()
    if args.driver:
        base = ["--num_graphs", "4096", "--batch_graphs", "256", "--num_epoches", "3"]
        res = {"what": "graph_main epoch", "args": " ".join(base)}
        for key, extra in (("no_norm", []), ("norm_graph_fused", ["--norm", "graph"]), ("norm_graph_composed", ["--norm", "graph", "--fused_norm", "False"])):
            seen = {}
            graph_main.main(base + extra, capture=seen)
            res[key + "_epoch_ms"] = round(seen["epoch_ms"], 2)
            res[key + "_final_loss"] = round(seen["final_loss"], 4)
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

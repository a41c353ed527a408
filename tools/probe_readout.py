#!/usr/bin/env python
"""Times the graph-level readout (libgnna gnna_segment_pool_ld_f32 / _backward_ld_f32 through ops.SegmentPool) against the torch
composition on the `batch` vector (index_add_, scatter_reduce) and against torch.clone of the same matrix, in one process.

    python tools/probe_readout.py --workload many-small|few-large|one-segment [--dims 64,128] [--out probe.jsonl]
    python tools/probe_readout.py --driver [--out probe.jsonl]          # graph_main.py epochs on the many-small set

One JSON line per (workload, D), appended to --out.  HIP events, the variants alternated round by round after a warm-up, median
of 5 rounds of 10 calls, ms per call."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import graph_main, ops  # noqa: E402

ROUNDS, CALLS = 5, 10


def graph_pointers(workload):
    g = torch.Generator().manual_seed(1)
    if workload == "many-small":
        sizes = torch.randint(8, 73, (65536,), generator=g)
    elif workload == "few-large":
        sizes = torch.randint(35000, 37001, (64,), generator=g)
    else:
        sizes = torch.tensor([232965])
    gp = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    gp[1:] = torch.cumsum(sizes, 0)
    return gp.to(torch.int32).cuda()


def timed(fns):
    """{name: median ms per call}; the variants take turns round by round."""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / CALLS)
    return {name: round(statistics.median(v), 4) for name, v in ms.items()}


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def probe(workload, D):
    gp = graph_pointers(workload)
    G, N = gp.numel() - 1, int(gp[-1])
    X = torch.randn(N, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    rows = torch.repeat_interleave(torch.arange(G, device="cuda"), (gp[1:] - gp[:-1]).long())
    idx = rows.unsqueeze(1).expand(N, D)
    W = [torch.rand(G, D, device="cuda") for _ in range(3)]
    Xg = X.clone().requires_grad_()

    def composed_sum():
        return torch.zeros(G, D, device="cuda").index_add_(0, rows, X)

    def composed_all(x=X):
        s = torch.zeros(G, D, device="cuda").index_add_(0, rows, x)
        mx = torch.zeros(G, D, device="cuda").scatter_reduce(0, idx, x, "amax", include_self=False)
        mn = torch.zeros(G, D, device="cuda").scatter_reduce(0, idx, x, "amin", include_self=False)
        return s, mx, mn

    def step(forward):
        Xg.grad = None
        s, mx, mn = forward()
        (s * W[0] + mx * W[1] + mn * W[2]).sum().backward()

    fused_step = lambda: step(lambda: ops.SegmentPool.apply(Xg, gp, True, True, True, False))          # noqa: E731
    composed_step = lambda: step(lambda: composed_all(Xg))                                               # noqa: E731
    t = timed({
        "fused_sum": lambda: ops.SegmentPool.apply(X, gp, True, False, False, False),
        "fused_sum_max_min": lambda: ops.SegmentPool.apply(X, gp, True, True, True, False),
        "fused_step": fused_step,
        "composed_sum": composed_sum,
        "composed_sum_max_min": composed_all,
        "composed_step": composed_step,
        "clone": lambda: X.clone(),
    })
    bytes_x = N * D * 4
    rec = dict(workload=workload, D=D, graphs=G, rows=N, ms=t,
               clone_GBps=round(2 * bytes_x / t["clone"] / 1e6, 1),
               fused_sum_GBps=round(bytes_x / t["fused_sum"] / 1e6, 1),
               fused_sum_max_min_GBps=round(bytes_x / t["fused_sum_max_min"] / 1e6, 1),
               peak_MiB=dict(fused_step=peak_mib(fused_step), composed_step=peak_mib(composed_step)))
    return rec


def driver():
    recs = []
    for fused in ("True", "False"):
        for model in ("gin", "gcn"):
            seen = {}
            graph_main.main(["--model", model, "--num_graphs", "65536", "--graph_nodes", "8,72", "--batch_graphs", "4096", "--dim", "32",
                             "--hidden", "64", "--classes", "4", "--readout", "sum,max", "--num_epoches", "3", "--fused_readout", fused],
                            capture=seen)
            recs.append(dict(workload="graph_main many-small", model=model, fused_readout=fused == "True", readout="sum,max",
                             batch_graphs=4096, hidden=64, epoch_ms=round(seen["epoch_ms"], 2), first_loss=round(seen["first_loss"], 4),
                             final_loss=round(seen["final_loss"], 4)))
    return recs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", choices=["many-small", "few-large", "one-segment"])
    p.add_argument("--dims", default="64,128")
    p.add_argument("--driver", action="store_true")
    p.add_argument("--out", default="probe.jsonl")
    args = p.parse_args()
    recs = driver() if args.driver else [probe(args.workload, int(d)) for d in args.dims.split(",")]
    with open(args.out, "a") as f:
        for r in recs:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times the attention readout (libgnna gnna_segment_attn_pool_ld_f32 / _backward_ld_f32 through ops.SegmentAttentionPool) against
two yardsticks measured in the same process: the torch composition on the `batch` vector (scatter_reduce amax, exp, index_add_, a
division, a product, index_add_) and the library's own sum readout (gnna_segment_pool_ld_f32, sum only), which reads the same X
once.

    python tools/probe_attn_readout.py --workload many-small|few-large|one-segment [--dims 64,128] [--out probe.jsonl]
    python tools/probe_attn_readout.py --driver [--out probe.jsonl]     # graph_main.py epochs on the many-small set

One JSON line per (workload, D, gate width), appended to --out.  HIP events, the variants alternated round by round after a
warm-up, median of 5 rounds of 10 calls, ms per call; the spread (min .. max of the rounds) is recorded next to the median."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import graph_main, ops  # noqa: E402
from probe_readout import graph_pointers, peak_mib  # noqa: E402

ROUNDS, CALLS = 5, 10


def timed(fns):
    """{name: (median, min, max) ms per call}; the variants take turns round by round."""
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
    return {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in ms.items()}


def probe(workload, D, gate_width):
    gp = graph_pointers(workload)
    G, N = gp.numel() - 1, int(gp[-1])
    gd = 1 if gate_width == "scalar" else D
    gen = torch.Generator(device="cuda").manual_seed(2)
    X = torch.randn(N, D, device="cuda", generator=gen)
    S = torch.randn(N, gd, device="cuda", generator=gen)
    W = torch.rand(G, D, device="cuda")
    Xg, Sg = X.clone().requires_grad_(), S.clone().requires_grad_()

    def step(forward):
        Xg.grad = Sg.grad = None
        (forward(Xg, Sg) * W).sum().backward()

    fused = lambda x, s: ops.SegmentAttentionPool.apply(x, s, gp)                                       # noqa: E731
    composed = lambda x, s: ops._composed_attention_readout(x, s, gp)                                   # noqa: E731

    def sum_step():
        Xg.grad = None
        (ops.SegmentPool.apply(Xg, gp, True, False, False, False)[0] * W).sum().backward()

    t = timed({
        "fused": lambda: fused(X, S),
        "composed": lambda: composed(X, S),
        "sum_readout": lambda: ops.SegmentPool.apply(X, gp, True, False, False, False),
        "fused_step": lambda: step(fused),
        "composed_step": lambda: step(composed),
        "sum_readout_step": sum_step,
    })
    bytes_read = N * (D + gd) * 4
    return dict(workload=workload, D=D, gate=gate_width, graphs=G, rows=N, ms_median_min_max=t,
                fused_GBps=round(bytes_read / t["fused"][0] / 1e6, 1), sum_readout_GBps=round(N * D * 4 / t["sum_readout"][0] / 1e6, 1),
                fused_over_sum_readout=round(t["fused"][0] / t["sum_readout"][0], 2), gate_traffic=round((D + gd) / D, 3),
                composed_over_fused=round(t["composed"][0] / t["fused"][0], 1),
                composed_step_over_fused_step=round(t["composed_step"][0] / t["fused_step"][0], 1),
                peak_MiB=dict(fused_step=peak_mib(lambda: step(fused)), composed_step=peak_mib(lambda: step(composed)),
                              sum_readout_step=peak_mib(sum_step)))


def driver():
    recs = []
    for attention in ("scalar", "none"):
        for fused in ("True", "False"):
            seen = {}
            graph_main.main(["--model", "gin", "--num_graphs", "65536", "--graph_nodes", "8,72", "--batch_graphs", "4096", "--dim", "32",
                             "--hidden", "64", "--classes", "4", "--readout", "sum", "--attention_readout", attention, "--num_epoches", "3",
                             "--fused_readout", fused], capture=seen)
            recs.append(dict(workload="graph_main many-small", model="gin", fused_readout=fused == "True", readout="sum",
                             attention_readout=attention, batch_graphs=4096, hidden=64, epoch_ms=round(seen["epoch_ms"], 2),
                             first_loss=round(seen["first_loss"], 4), final_loss=round(seen["final_loss"], 4)))
    return recs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", choices=["many-small", "few-large", "one-segment"])
    p.add_argument("--dims", default="64,128")
    p.add_argument("--driver", action="store_true")
    p.add_argument("--out", default="probe.jsonl")
    args = p.parse_args()
    recs = driver() if args.driver else [probe(args.workload, int(d), w) for d in args.dims.split(",") for w in ("scalar", "channel")]
    with open(args.out, "a") as f:
        for r in recs:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

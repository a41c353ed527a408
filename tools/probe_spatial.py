#!/usr/bin/env python3
"""Times graph construction from coordinates (_lib.radius_graph -> gnna_radius_graph_f32) against the same rule composed from torch
ops on the GPU (spatial.composed_radius_graph), the bare scan + partition tail on the same row pointers, and the share of a
graph_main.py --model schnet step that graph construction takes.

    python tools/probe_spatial.py [--shapes small,sets,cloud] [--reps 7] [--big_reps 3] [--small_graphs 65536] [--driver True]

Shapes (dim = 3, uniform points, density 1 per unit volume so that a cutoff r sees about 4.19 r^3 neighbours away from a face):
  small   65,536 point sets of 8 - 72 points (the shape of graph_main.py), cutoff for about 4 and about 16 neighbours
  sets    64 sets of about 36,000 points
  cloud   one set of 232,965 points
each without a cap, with max_neighbors = 32, and as a kNN graph with k = 16.  One JSON line per (shape, setting): medians after two
warm-up calls, wall-clock with a device synchronisation around every call (the call's own read-back is inside), the peak device
memory of one call above what was allocated before it, the edges, and the pair evaluations per second of the two passes
(2 * sum n_g^2 / time: the select passes of a cap are not counted as work, so a capped setting shows a lower rate).  The torch
composition runs where its [G, n_max, n_max] tensors fit (a guess of 40 bytes per element against the free memory); the line says
so where they do not.  Nothing is started after a step that fails."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="small,sets,cloud")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--big_reps", type=int, default=3)
    p.add_argument("--small_graphs", type=int, default=65536)
    p.add_argument("--driver", default="True")
    args = p.parse_args()
    import torch
    from gnnadvisor_osdi21_amd import _lib, spatial
    dev = torch.device("cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def measure(fn, reps):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(reps):
            ms, out = timed(fn)
            times.append(ms)
            del out
        return statistics.median(times), (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    def cloud(sizes, seed):
        g = torch.Generator()
        g.manual_seed(seed)
        sizes = torch.as_tensor(sizes, dtype=torch.int64)
        gp = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
        gp[1:] = torch.cumsum(sizes, 0)
        side = sizes.double() ** (1.0 / 3.0)                                   # density 1
        which = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
        pos = (torch.rand(int(gp[-1]), 3, generator=g, dtype=torch.float64) * side[which, None]).float()
        return pos.to(dev), gp.to(torch.int32).to(dev), sizes

    def radius_for(neighbours):
        return (neighbours / (4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)

    shapes = {}
    if "small" in args.shapes:
        g = torch.Generator()
        g.manual_seed(1)
        shapes["small"] = (cloud(torch.randint(8, 73, (args.small_graphs,), generator=g), 2), args.reps)
    if "sets" in args.shapes:
        g = torch.Generator()
        g.manual_seed(3)
        shapes["sets"] = (cloud(torch.randint(35000, 37001, (64,), generator=g), 4), args.big_reps)
    if "cloud" in args.shapes:
        shapes["cloud"] = (cloud([232965], 5), args.big_reps)

    for name, ((pos, gp, sizes), reps) in shapes.items():
        pairs = float((sizes.double() ** 2).sum())
        n_max = int(sizes.max())
        settings = [("r4", radius_for(4), None), ("r16", radius_for(16), None), ("r16_cap32", radius_for(16) * 1.4, 32),
                    ("knn16", math.inf, 16)]
        if name != "small":
            settings = settings[1:]
        for label, radius, cap in settings:
            ms, peak = measure(lambda: _lib.radius_graph(pos, gp, radius, cap, partSize=32), reps)
            res = _lib.radius_graph(pos, gp, radius, cap, partSize=32)
            line = {"shape": name, "setting": label, "rows": int(pos.shape[0]), "sets": int(sizes.numel()), "radius": radius,
                    "max_neighbors": cap, "edges": res["num_edges"], "call_ms": round(ms, 3), "call_peak_mib": round(peak, 1),
                    "pair_evals_per_s": round(2 * pairs / (ms * 1e-3), 0)}
            # the floor: the scan + partition tail on the same row pointers
            rp = res["row_pointers"]
            tail_ms, _ = measure(lambda: _lib.build_part_device(32, rp), reps)
            line["tail_ms"] = round(tail_ms, 3)
            need = 40.0 * sizes.numel() * n_max * n_max
            free = torch.cuda.mem_get_info()[0]
            if need < 0.8 * free:
                got = spatial.composed_radius_graph(pos, gp, radius, cap)
                assert torch.equal(got[1], res["column_index"]) and torch.equal(got[0], rp), "the composition disagrees"
                del got
                cms, cpeak = measure(lambda: spatial.composed_radius_graph(pos, gp, radius, cap), reps)
                line.update(composed_ms=round(cms, 3), composed_peak_mib=round(cpeak, 1))
            else:
                line["composed"] = "does not fit: about %.0f GiB of [G, n_max, n_max] tensors, %.0f GiB free" % (need / 2 ** 30, free / 2 ** 30)
            del res, rp
            print(json.dumps(line), flush=True)

    if args.driver == "True":
        base = [sys.executable, "-m", "gnnadvisor_osdi21_amd.graph_main", "--model", "schnet", "--num_graphs", "4096", "--batch_graphs", "256",
                "--cutoff", "%.4f" % radius_for(16), "--num_epoches", "5", "--verbose_mode", "True"]
        for fused in ("True", "False"):
            run = subprocess.run(base + ["--fused_graph", fused], capture_output=True, text=True, timeout=600,
                                 cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            if run.returncode != 0:
                print(run.stderr[-2000:])
                return 1
            out = run.stdout
            epoch_ms = float(out.split("Time (ms): ")[1].split()[0])
            graph_ms = float(out.split("# graph construction: ")[1].split()[0])
            print(json.dumps({"driver": "schnet", "fused_graph": fused == "True", "epoch_ms": epoch_ms, "graph_ms_per_epoch": graph_ms,
                              "share": round(graph_ms / epoch_ms, 4), "steps_per_epoch": 16}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

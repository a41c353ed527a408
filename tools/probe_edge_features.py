#!/usr/bin/env python3
"""Times edge-feature message passing -- edgeconv.EdgeFeatureSum forward and forward + backward, fused against the same function
composed from torch ops, in GINE's mode (add, relu) and CFConv's (mul, none) -- and each kernel pass of include/gnna_edgefeat.h
against torch.clone of the bytes the pass must move; then graph_main.py --model gine epochs, fused and composed.

    python tools/probe_edge_features.py [--shapes small,amazon] [--dims 64,128] [--reps 7] [--driver 1] [--kernels_only 0]

Per shape, width and mode it prints one JSON line: median, min and max of ms per call, the calls alternated in one process after two
warm-up rounds; the peak torch memory of a forward + backward of both paths; per pass the kernel's ms, its byte floor and the ms of
torch.clone of a buffer of half that size (a clone reads and writes it: the same bytes moved).  The byte floors, with
B = 4 * dim bytes per row, nnz edges, N destination and M source rows:

    forward   nnz * B (E) + nnz * B (the gathered rows of X) + N * B (out)
    d_edge    nnz * B (d_edge) + N * B (dY) + what the mask or the product needs: nnz * B (gathered X) if mul or relu, nnz * B (E) if relu
    d_input   nnz * B (the gathered rows of dY) + M * B (d_input) + nnz * B (E) if mul or relu + M * B (x) if relu

The gathered rows are counted as memory traffic although many are served by the L2: the floor is what a kernel without any reuse
would move, so a share above 100 % of clone is possible where rows are reused.  --kernels_only 1 times the passes alone through
``_lib`` (no torch extension: the library named by GNNA_LIB is the only one loaded), which is how the thresholds of
gnna_edgefeat.hip were compared (profiles/edge_features/README.md).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import _lib, graph      # noqa: E402

MODES = (("add", "relu"), ("mul", "none"))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns, reps, warm=2):
    """(median, min, max) of ms per call of every function, the calls alternated."""
    ms = [[] for _ in fns]
    for k in range(reps + warm):
        for i, fn in enumerate(fns):
            t = timed(fn)
            if k >= warm:
                ms[i].append(t)
    return [(round(statistics.median(m), 4), round(min(m), 4), round(max(m), 4)) for m in ms]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def structure(name, dev):
    """(row_pointers, column_index with global ids, graph_pointers) on the device."""
    if name == "small":                                               # the readout's shape: 65,536 graphs of 8 .. 72 nodes
        rp, ci, gp = graph.small_graphs(65536, 8, 72, 4.0, seed=1)
        rows = torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long())
        which = torch.bucketize(rows, gp[1:].long(), right=True)
        ci = (ci.long() + gp.long()[which]).to(torch.int32)
        return rp.to(dev), ci.to(dev), gp.to(dev)
    g = graph.make_config_graph("amazon0505-like")
    n = g.num_nodes
    return g.row_pointers.to(dev), g.column_index.to(dev), torch.tensor([0, n], dtype=torch.int32, device=dev)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="small,amazon")
    p.add_argument("--dims", default="64,128")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--driver", type=int, default=1, help="1: also graph_main.py --model gine epochs, fused and composed")
    p.add_argument("--kernels_only", type=int, default=0, help="1: the three passes through _lib alone")
    args = p.parse_args(argv)
    dev = torch.device("cuda")
    for name in args.shapes.split(","):
        rp, ci, gp = structure(name, dev)
        n, nnz = rp.numel() - 1, ci.numel()
        t_rp, t_ci, t_pos = _lib.transpose_csr(rp, ci)
        deg = (rp[1:] - rp[:-1]).float()
        for dim in (int(d) for d in args.dims.split(",")):
            gen = torch.Generator(device=dev).manual_seed(dim)
            X = torch.randn(n, dim, device=dev, generator=gen)
            E = torch.randn(nnz, dim, device=dev, generator=gen)
            dY = torch.randn(n, dim, device=dev, generator=gen)
            out, dX, dE = torch.empty(n, dim, device=dev), torch.empty(n, dim, device=dev), torch.empty(nnz, dim, device=dev)
            row = 4 * dim
            for combine, act in MODES:
                c, a = {"add": _lib.EDGE_ADD, "mul": _lib.EDGE_MUL}[combine], {"none": _lib.EDGE_ACT_NONE, "relu": _lib.EDGE_ACT_RELU}[act]
                mul, relu = combine == "mul", act == "relu"
                floors = {"forward": 2 * nnz * row + n * row,
                          "d_edge": nnz * row + n * row + (nnz * row if mul or relu else 0) + (nnz * row if relu else 0),
                          "d_input": nnz * row + n * row + (nnz * row if mul or relu else 0) + (n * row if relu else 0)}
                clones = {k: torch.empty(v // 8, device=dev) for k, v in floors.items()}
                passes = {"forward": lambda: _lib.agg_edge_feat(X, E, rp, ci, combine=c, act=a, out=out),
                          "d_edge": lambda: _lib.agg_edge_feat_backward(X, E, dY, rp, ci, combine=c, act=a, want_dx=False, dE=dE),
                          "d_input": lambda: _lib.agg_edge_feat_backward(X, E, dY, rp, ci, t_rp, t_ci, t_pos, combine=c, act=a,
                                                                         want_de=False, dX=dX)}
                fns = [f for k in passes for f in (passes[k], (lambda b: (lambda: b.clone()))(clones[k]))]
                ms = alternate(fns, args.reps)
                res = {"shape": name, "num_nodes": n, "nnz": nnz, "mean_degree": round(float(deg.mean()), 2), "max_degree": int(deg.max()),
                       "dim": dim, "combine": combine, "act": act, "reps": args.reps, "lib": os.path.basename(_lib.LIB_PATH)}
                for i, k in enumerate(passes):
                    kern, clone = ms[2 * i], ms[2 * i + 1]
                    res[k] = {"ms": kern, "floor_MB": round(floors[k] / 1e6, 1), "GBps": round(floors[k] / kern[0] / 1e6, 1),
                              "clone_ms": clone, "share_of_clone": round(clone[0] / kern[0], 3)}
                del clones
                if not args.kernels_only:
                    from gnnadvisor_osdi21_amd.batching import GraphBatch
                    from gnnadvisor_osdi21_amd.edgeconv import EdgeFeatureSum, composed_edge_feature_sum
                    info = GraphBatch(rp, ci, gp, directed=True)
                    info.transposed().perm                                 # built once, before timing, as a training loop has it
                    Xg, Eg = X.clone().requires_grad_(), E.clone().requires_grad_()
                    run = {True: lambda: EdgeFeatureSum.apply(Xg, Eg, info, combine, act),
                           False: lambda: composed_edge_feature_sum(Xg, Eg, info, combine, act)}

                    def forward(fused):
                        with torch.no_grad():
                            run[fused]()

                    def step(fused):
                        Xg.grad = Eg.grad = None
                        (run[fused]() * dY).sum().backward()

                    with torch.no_grad():
                        diff = float((run[True]() - run[False]()).abs().max())
                    assert diff < 1e-2, diff
                    ms = alternate([lambda: forward(True), lambda: forward(False), lambda: step(True), lambda: step(False)], args.reps)
                    res.update({"max_abs_fused_minus_composed": diff, "forward_ms_fused": ms[0], "forward_ms_composed": ms[1],
                                "fwd_bwd_ms_fused": ms[2], "fwd_bwd_ms_composed": ms[3],
                                "peak_MiB_fused": round(peak_mb(lambda: step(True)), 1),
                                "peak_MiB_composed": round(peak_mb(lambda: step(False)), 1),
                                "fused_step_faster": ms[2][0] < ms[3][0], "fused_forward_faster": ms[0][0] < ms[1][0]})
                    del Xg, Eg, info
                print(json.dumps(res), flush=True)
                torch.cuda.empty_cache()
            del X, E, dY, out, dX, dE
            torch.cuda.empty_cache()
    if args.driver and not args.kernels_only:
        from gnnadvisor_osdi21_amd import graph_main
        base = ["--model", "gine", "--edge_dim", "8", "--num_graphs", "4096", "--batch_graphs", "256", "--num_epoches", "3"]
        res = {"what": "graph_main epoch", "args": " ".join(base)}
        for key, extra in (("fused", []), ("composed", ["--fused_edge", "False"])):
            seen = {}
            graph_main.main(base + extra, capture=seen)
            res[key + "_epoch_ms"] = round(seen["epoch_ms"], 2)
            res[key + "_final_loss"] = round(seen["final_loss"], 4)
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

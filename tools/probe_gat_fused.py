"""Fused against composed GAT attention on the Reddit-like graph (profiles/gat_fused/):

    python tools/probe_gat_fused.py [--reps 5] [--rounds 5] [--graph reddit-like] [--configs 1x64,4x16] [--memory 1,4,8]

Forward + backward of the attention alone -- from (H, el, er) to (dH, d_el, d_er); the dense X W is on neither side -- as
ops.GATAttention runs it ("fused") and as GATConv composes it from index_select, leaky_relu, EdgeSoftmax and
EdgeWeightedAggregate ("composed"), in ONE process, the two alternated round by round, ms per step from HIP events, minimum
over the rounds.  --memory: peak torch memory of one step of either path at those head counts (dim 64 / heads).
Kernel times: the same command under `rocprofv3 --kernel-trace --stats` in a run of its own.  One JSON line per variant."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import _lib, graph  # noqa: E402


class Info:
    """The slice of decider.inputProperty the attention ops read."""

    def __init__(self, g, partSize):
        from gnnadvisor_osdi21_amd.decider import inputProperty
        self.row_pointers, self.column_index, self.partSize = g.row_pointers.cuda(), g.column_index.cuda(), partSize
        self.partPtr, self.part2Node = [t.cuda() for t in _lib.build_part(partSize, g.row_pointers.cpu())]
        self._edge_arrays = lambda: inputProperty._edge_arrays(self)
        self.reverse_edges = lambda: inputProperty.reverse_edges(self)
        self.edge_rows = lambda: inputProperty.edge_rows(self)


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def steps(info, heads, dim, seed=1):
    from gnnadvisor_osdi21_amd.ops import EdgeSoftmax, EdgeWeightedAggregate, GATAttention
    n = info.row_pointers.numel() - 1
    gen = torch.Generator(device="cuda").manual_seed(seed)
    H = torch.randn(n, heads * dim, device="cuda", generator=gen).requires_grad_()
    el = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    er = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    G = torch.randn(n, heads * dim, device="cuda", generator=gen)

    def fused():
        Y = GATAttention.apply(H, el, er, info, 0.2)
        return torch.autograd.grad(Y, (H, el, er), G)

    def composed():
        rows, ci = info.edge_rows(), info.column_index
        s = torch.nn.functional.leaky_relu(el.index_select(0, rows) + er.index_select(0, ci), 0.2)
        alpha = EdgeSoftmax.apply(s.t().contiguous(), info.row_pointers)
        Y = EdgeWeightedAggregate.apply(H, alpha, info)
        return torch.autograd.grad(Y, (H, el, er), G)

    return {"fused": fused, "composed": composed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="reddit-like")
    ap.add_argument("--configs", default="1x64,4x16", help="heads x dim, comma separated")
    ap.add_argument("--memory", default="1,4,8", help="head counts for the peak-memory lines ('' = none)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", choices=["", "fused", "composed"])
    args = ap.parse_args()
    g = graph.make_config_graph(args.graph, device="cuda")
    info = Info(g, args.partSize)
    n, nnz = g.num_nodes, info.column_index.numel()
    head = dict(graph=args.graph, nodes=n, edges=nnz, partSize=args.partSize, reps=args.reps, rounds=args.rounds)
    for cfg in [c for c in args.configs.split(",") if c]:
        heads, dim = [int(v) for v in cfg.split("x")]
        variants = {k: f for k, f in steps(info, heads, dim).items() if args.only in ("", k)}
        for fn in variants.values():          # warm-up: the symmetry check, per-edge arrays of the composed path, plans, scratch
            timed(fn, 1)
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn, args.reps))
        for k, v in ms.items():
            print(json.dumps(dict(head, heads=heads, dim=dim, variant=k, ms_per_step=round(min(v), 4),
                                  ms_rounds=[round(x, 4) for x in v])), flush=True)
        if len(ms) == 2:
            print(json.dumps(dict(head, heads=heads, dim=dim, variant="fused / composed",
                                  ratio=round(min(ms["fused"]) / min(ms["composed"]), 4), condition="<= 1")), flush=True)
    for heads in [int(v) for v in args.memory.split(",") if v]:
        dim = max(1, 64 // heads)
        for k, fn in steps(info, heads, dim).items():
            if args.only not in ("", k):
                continue
            timed(fn, 1)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            timed(fn, 1)
            peak = torch.cuda.max_memory_allocated() - before
            print(json.dumps(dict(head, heads=heads, dim=dim, variant=k + " peak memory", peak_mib=round(peak / 2 ** 20, 1),
                                  one_nnz_float_array_mib=round(nnz * 4 / 2 ** 20, 1))), flush=True)
            del fn
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

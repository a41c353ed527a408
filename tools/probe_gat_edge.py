"""Fused GAT attention with a per-edge score term against the plain fused attention and the composed path on the Reddit-like
graph (profiles/gat_edge/):

    python tools/probe_gat_edge.py [--reps 5] [--rounds 5] [--graph reddit-like] [--configs 1x64,4x16]

Forward + backward of the attention alone, ms per step from HIP events, three paths alternated round by round in ONE process,
minimum over the rounds:
    edge      ops.GATEdgeAttention: from (H, el, er, ee) to (dH, d_el, d_er, d_ee)         -- the new entries
    plain     ops.GATAttention: from (H, el, er) to (dH, d_el, d_er)                       -- unchanged code; the cost of the term
    composed  index_select + leaky_relu + EdgeSoftmax + EdgeWeightedAggregate with ee added to the score, to the same four gradients
Conditions: edge <= composed on every shape where composed runs; edge / plain is reported, not gated.  Then the peak torch
memory of one step of `edge` and `composed`.  Kernel times: the same command under `rocprofv3 --kernel-trace --stats` in a run of
its own.  One JSON line per variant."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gnnadvisor_osdi21_amd import graph  # noqa: E402
from probe_gat_fused import Info, timed  # noqa: E402


def steps(info, heads, dim, seed=1):
    from gnnadvisor_osdi21_amd.ops import EdgeSoftmax, EdgeWeightedAggregate, GATAttention, GATEdgeAttention
    n, nnz = info.row_pointers.numel() - 1, info.column_index.numel()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    H = torch.randn(n, heads * dim, device="cuda", generator=gen).requires_grad_()
    el = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    er = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    ee = torch.randn(nnz, heads, device="cuda", generator=gen).requires_grad_()
    G = torch.randn(n, heads * dim, device="cuda", generator=gen)

    def edge():
        Y = GATEdgeAttention.apply(H, el, er, ee, info, 0.2)
        return torch.autograd.grad(Y, (H, el, er, ee), G)

    def plain():
        Y = GATAttention.apply(H, el, er, info, 0.2)
        return torch.autograd.grad(Y, (H, el, er), G)

    def composed():
        rows, ci = info.edge_rows(), info.column_index
        s = torch.nn.functional.leaky_relu(el.index_select(0, rows) + er.index_select(0, ci) + ee, 0.2)
        alpha = EdgeSoftmax.apply(s.t().contiguous(), info.row_pointers)
        Y = EdgeWeightedAggregate.apply(H, alpha, info)
        return torch.autograd.grad(Y, (H, el, er, ee), G)

    return {"edge": edge, "plain": plain, "composed": composed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="reddit-like")
    ap.add_argument("--configs", default="1x64,4x16", help="heads x dim, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--skip", default="", help="comma list of paths to leave out (composed: where it does not fit in memory)")
    args = ap.parse_args()
    g = graph.make_config_graph(args.graph, device="cuda")
    info = Info(g, args.partSize)
    n, nnz = g.num_nodes, info.column_index.numel()
    head = dict(graph=args.graph, nodes=n, edges=nnz, partSize=args.partSize, reps=args.reps, rounds=args.rounds)
    skip = set(args.skip.split(","))
    for cfg in [c for c in args.configs.split(",") if c]:
        heads, dim = [int(v) for v in cfg.split("x")]
        variants = {k: f for k, f in steps(info, heads, dim).items() if k not in skip}
        for fn in variants.values():          # warm-up: the symmetry check, the reverse-edge map, per-edge arrays, plans, scratch
            timed(fn, 1)
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn, args.reps))
        for k, v in ms.items():
            print(json.dumps(dict(head, heads=heads, dim=dim, variant=k, ms_per_step=round(min(v), 4),
                                  ms_rounds=[round(x, 4) for x in v])), flush=True)
        if "edge" in ms and "composed" in ms:
            print(json.dumps(dict(head, heads=heads, dim=dim, variant="edge / composed",
                                  ratio=round(min(ms["edge"]) / min(ms["composed"]), 4), condition="<= 1")), flush=True)
        if "edge" in ms and "plain" in ms:
            print(json.dumps(dict(head, heads=heads, dim=dim, variant="edge / plain",
                                  ratio=round(min(ms["edge"]) / min(ms["plain"]), 4), condition="reported")), flush=True)
        for k in ("edge", "composed"):
            if k not in variants:
                continue
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            timed(variants[k], 1)
            peak = torch.cuda.max_memory_allocated() - before
            print(json.dumps(dict(head, heads=heads, dim=dim, variant=k + " peak memory", peak_mib=round(peak / 2 ** 20, 1),
                                  one_nnz_x_heads_float_array_mib=round(nnz * heads * 4 / 2 ** 20, 1))), flush=True)
        del variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

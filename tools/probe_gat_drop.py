"""Attention dropout in the fused GAT attention against the plain fused call and against the composed path with torch's dropout
on alpha, on the Reddit-like graph (profiles/gat_dropout/):

    python tools/probe_gat_drop.py [--reps 5] [--rounds 7] [--graph reddit-like] [--configs 1x64,4x16] [--attn_drop 0.6]

Forward + backward of the attention alone -- from (H, el, er) to (dH, d_el, d_er) -- in ONE process, the variants alternated round
by round, ms per step from HIP events, median over the rounds (min and max beside it: the spread):
  plain     ops.GATAttention without dropout (gnna_gat_forward_f32 / gnna_gat_backward_f32: the entries as they were)
  drop      ops.GATAttention with attn_drop (gnna_gat_forward_drop_f32 / gnna_gat_backward_drop_f32), a new seed every step
  composed  index_select, leaky_relu, EdgeSoftmax, torch.nn.functional.dropout on alpha, EdgeWeightedAggregate
then the peak torch memory of one step of each.  One JSON line per variant and per ratio (drop / plain, drop / composed)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import graph  # noqa: E402
from probe_gat_fused import Info, timed  # noqa: E402


def steps(info, heads, dim, attn_drop, seed=1):
    from gnnadvisor_osdi21_amd.ops import EdgeSoftmax, EdgeWeightedAggregate, GATAttention
    n = info.row_pointers.numel() - 1
    gen = torch.Generator(device="cuda").manual_seed(seed)
    H = torch.randn(n, heads * dim, device="cuda", generator=gen).requires_grad_()
    el = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    er = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    G = torch.randn(n, heads * dim, device="cuda", generator=gen)
    drawn = [0]

    def plain():
        Y = GATAttention.apply(H, el, er, info, 0.2)
        return torch.autograd.grad(Y, (H, el, er), G)

    def drop():
        drawn[0] += 1
        Y = GATAttention.apply(H, el, er, info, 0.2, attn_drop, 0x5EED + drawn[0])
        return torch.autograd.grad(Y, (H, el, er), G)

    def composed():
        rows, ci = info.edge_rows(), info.column_index
        s = torch.nn.functional.leaky_relu(el.index_select(0, rows) + er.index_select(0, ci), 0.2)
        alpha = EdgeSoftmax.apply(s.t().contiguous(), info.row_pointers)
        alpha = torch.nn.functional.dropout(alpha, attn_drop, training=True)
        Y = EdgeWeightedAggregate.apply(H, alpha, info)
        return torch.autograd.grad(Y, (H, el, er), G)

    return {"plain": plain, "drop": drop, "composed": composed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="reddit-like")
    ap.add_argument("--configs", default="1x64,4x16", help="heads x dim, comma separated")
    ap.add_argument("--attn_drop", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", help="comma list of variants ('' = all)")
    args = ap.parse_args()
    only = [v for v in args.only.split(",") if v]
    g = graph.make_config_graph(args.graph, device="cuda")
    info = Info(g, args.partSize)
    n, nnz = g.num_nodes, info.column_index.numel()
    head = dict(graph=args.graph, nodes=n, edges=nnz, partSize=args.partSize, attn_drop=args.attn_drop, reps=args.reps,
                rounds=args.rounds)
    for cfg in [c for c in args.configs.split(",") if c]:
        heads, dim = [int(v) for v in cfg.split("x")]
        variants = {k: f for k, f in steps(info, heads, dim, args.attn_drop).items() if not only or k in only}
        for fn in variants.values():          # warm-up: the symmetry check, per-edge arrays of the composed path, scratch
            timed(fn, 1)
        ms = {k: [] for k in variants}
        for r in range(args.rounds):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]          # alternate who goes first
            for k in order:
                ms[k].append(timed(variants[k], args.reps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            print(json.dumps(dict(head, heads=heads, dim=dim, variant=k, ms_per_step=round(med[k], 4), ms_min=round(min(v), 4),
                                  ms_max=round(max(v), 4), ms_rounds=[round(x, 4) for x in v])), flush=True)
        for a, b in (("drop", "plain"), ("drop", "composed")):
            if a in med and b in med:
                print(json.dumps(dict(head, heads=heads, dim=dim, variant=f"{a} / {b}", ratio=round(med[a] / med[b], 4))), flush=True)
        for k, fn in variants.items():
            timed(fn, 1)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            timed(fn, 1)
            peak = torch.cuda.max_memory_allocated() - before
            print(json.dumps(dict(head, heads=heads, dim=dim, variant=k + " peak memory", peak_mib=round(peak / 2 ** 20, 1),
                                  one_nnz_float_array_mib=round(nnz * 4 / 2 ** 20, 1))), flush=True)
        del variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

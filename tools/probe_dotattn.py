"""Fused dot-product attention against the composed path and against the fused GATv2 and GAT (v1) attention at the same shape
(profiles/dot_attention/):

    python tools/probe_dotattn.py [--reps 3] [--rounds 5] [--graph reddit-like] [--configs 1x64,4x16] [--only fused,v2,v1]

Forward + backward of the attention alone -- from (Q, K, V) to (dQ, dK, dV) -- in ONE process, the variants alternated round by
round after a warm-up step, ms per step from HIP events, median over the rounds (min and max beside it: the spread):
  fused     ops.DotAttention (gnna_dot_attn_forward_f32 / gnna_dot_attn_backward_f32), Q, K and V as column slices of one
            [N, 3 * heads * dim] matrix -- the layer's normal path
  composed  index_select of Q and K, product, sum, EdgeSoftmax, EdgeWeightedAggregate: [nnz, heads * dim] tensors
  v2        ops.GATv2Attention at the same shape: the yardstick for the row traffic (the dot forward makes three row gathers per
            edge where v2 makes two, the backward four where v2 makes three)
  v1        ops.GATAttention at the same shape (two row gathers in the forward, two in the backward)
then the peak torch memory of one step of each.  `composed` is skipped, and its size arithmetic printed, when three of its
per-edge tensors exceed --composed_limit_gib (default 60: Q[rows], K[cols] and their product are alive at the peak; the Reddit-like
graph at 64 floats per row needs 3 x 27.3 GiB in the forward and more in the backward and is skipped; a smaller graph runs it).  The passes one by one: run under `rocprofv3 --kernel-trace --stats` with --only fused.  One JSON line per variant and per
ratio."""
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


def steps(info, heads, dim, seed=1):
    from gnnadvisor_osdi21_amd.ops import DotAttention, EdgeSoftmax, EdgeWeightedAggregate, GATAttention, GATv2Attention
    n = info.row_pointers.numel() - 1
    W = heads * dim
    gen = torch.Generator(device="cuda").manual_seed(seed)
    P = torch.randn(n, 3 * W, device="cuda", generator=gen).requires_grad_()
    Hs = torch.randn(n, W, device="cuda", generator=gen).requires_grad_()
    Hd = torch.randn(n, W, device="cuda", generator=gen).requires_grad_()
    att = ((torch.rand(heads, dim, device="cuda", generator=gen) * 2 - 1) / dim ** 0.5).requires_grad_()
    el = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    er = torch.randn(n, heads, device="cuda", generator=gen).requires_grad_()
    G = torch.randn(n, W, device="cuda", generator=gen)

    def fused():
        Y = DotAttention.apply(P[:, :W], P[:, W:2 * W], P[:, 2 * W:], info, heads)
        return torch.autograd.grad(Y, (P,), G)

    def composed():
        rows, ci = info.edge_rows(), info.column_index
        qk = P[:, :W].index_select(0, rows) * P[:, W:2 * W].index_select(0, ci)
        z = qk.view(-1, heads, dim).sum(-1) / dim ** 0.5
        alpha = EdgeSoftmax.apply(z.t().contiguous(), info.row_pointers)
        Y = EdgeWeightedAggregate.apply(P[:, 2 * W:].contiguous(), alpha, info)
        return torch.autograd.grad(Y, (P,), G)

    def v2():
        Y = GATv2Attention.apply(Hs, Hd, att, info, 0.2)
        return torch.autograd.grad(Y, (Hs, Hd, att), G)

    def v1():
        Y = GATAttention.apply(Hs, el, er, info, 0.2)
        return torch.autograd.grad(Y, (Hs, el, er), G)

    return {"fused": fused, "composed": composed, "v2": v2, "v1": v1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="reddit-like")
    ap.add_argument("--configs", default="1x64,4x16", help="heads x dim, comma separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", help="comma list of variants ('' = all)")
    ap.add_argument("--composed_limit_gib", type=float, default=60.0,
                    help="skip `composed` when three [nnz, heads * dim] float tensors (Q[rows], K[cols], their product) exceed this")
    args = ap.parse_args()
    only = [v for v in args.only.split(",") if v]
    g = graph.make_config_graph(args.graph, device="cuda")
    info = Info(g, args.partSize)
    n, nnz = g.num_nodes, info.column_index.numel()
    head = dict(graph=args.graph, nodes=n, edges=nnz, partSize=args.partSize, reps=args.reps, rounds=args.rounds)
    for cfg in [c for c in args.configs.split(",") if c]:
        heads, dim = [int(v) for v in cfg.split("x")]
        variants = {k: f for k, f in steps(info, heads, dim).items() if not only or k in only}
        per_edge_gib = nnz * heads * dim * 4 / 2 ** 30
        if "composed" in variants and 3 * per_edge_gib > args.composed_limit_gib:
            del variants["composed"]
            print(json.dumps(dict(head, heads=heads, dim=dim, variant="composed", skipped="its per-edge tensors exceed --composed_limit_gib",
                                  one_edge_tensor_gib=round(per_edge_gib, 1), tensors_alive_at_the_peak=3)), flush=True)
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
        for a, b in (("fused", "composed"), ("fused", "v2"), ("fused", "v1")):
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

#!/usr/bin/env python3
"""Times one mini-batch step of a two-layer GAT on sampled blocks -- sample + forward + backward -- with the fused attention
(ops.GATConv(fused=True) -> gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32) against the same layers with the attention
composed from torch ops on the block (index_select, a scatter-softmax over the rows, index_add_), on the Reddit-like and
products-like graphs.

    python tools/probe_gat_blocks.py [--graphs reddit-like,products-like] [--scale 1.0] [--seeds 1024] [--fanout 25,10]
                                     [--heads 4] [--hidden 16] [--reps 7] [--dim 64]

Both paths share the sampler, the weights and the batches and alternate in one process; per graph one JSON line is printed:
medians of the step (ms), the share of the fused step spent in sample(), and the peak torch memory of one step of each path.
The two paths are compared once before timing (outputs within 1e-4 of max|ref|).  Condition (profiles/gat_blocks/README.md):
the fused step is no slower than the composed one on both graphs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import graph, ops                      # noqa: E402
from gnnadvisor_osdi21_amd.sampling import NeighborSampler       # noqa: E402


def composed_gat(conv, X, block):
    """GATConv's function on a block from torch ops: per-edge scores, softmax over every destination row, weighted sum."""
    n_src, n_dst, heads, out = block.num_src, block.num_dst, conv.heads, conv.out_dim
    H = torch.mm(X, conv.weights)
    Hh = H.view(n_src, heads, out)
    el = (Hh[:n_dst] * conv.att_l).sum(-1)
    er = (Hh * conv.att_r).sum(-1)
    rp = block.row_pointers.long()
    rows = torch.repeat_interleave(torch.arange(n_dst, device=X.device), rp[1:] - rp[:-1])
    cl = block.column_index.long()
    s = F.leaky_relu(el.index_select(0, rows) + er.index_select(0, cl), conv.negative_slope)        # [nnz, heads]
    m = torch.full((n_dst, heads), -float("inf"), device=X.device).scatter_reduce(0, rows[:, None].expand_as(s), s.detach(),
                                                                                 reduce="amax")
    ex = torch.exp(s - m.index_select(0, rows))
    den = torch.zeros(n_dst, heads, device=X.device).index_add_(0, rows, ex)
    alpha = ex / den.index_select(0, rows)
    Y = torch.zeros(n_dst, heads, out, device=X.device).index_add_(0, rows, alpha[:, :, None] * Hh.index_select(0, cl))
    return Y.view(n_dst, heads * out) if conv.concat or heads == 1 else Y.mean(1)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", default="reddit-like,products-like")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanout", default="25,10")
    p.add_argument("--heads", type=int, default=4)
    p.add_argument("--hidden", type=int, default=16)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--dim", type=int, default=64)
    args = p.parse_args(argv)
    assert args.reps >= 5, "medians of at least 5 repetitions"
    fanouts = [int(f) for f in args.fanout.split(",")]
    dev = torch.device("cuda")
    for name in args.graphs.split(","):
        cfg = graph.CONFIGS[name]
        n, edges = max(64, int(cfg["num_nodes"] * args.scale)), int(cfg["num_edges"] * args.scale)
        g = graph.powerlaw_graph(n, edges, min(cfg["max_degree"], n - 1), seed=cfg["seed"])
        info = argparse.Namespace(row_pointers=g.row_pointers.to(dev), column_index=g.column_index.to(dev), partSize=32)
        sampler = NeighborSampler(info, fanouts)
        X = torch.randn(n, args.dim, device=dev)
        y = torch.randint(0, cfg["classes"], (n,), device=dev)
        torch.manual_seed(1)
        conv1 = ops.GATConv(args.dim, args.hidden, heads=args.heads, fused=True).to(dev)
        conv2 = ops.GATConv(args.hidden * args.heads, cfg["classes"], heads=1, fused=True).to(dev)
        params = list(conv1.parameters()) + list(conv2.parameters())
        gen = torch.Generator().manual_seed(1)
        batches = [torch.randperm(n, generator=gen)[: args.seeds].int().to(dev) for _ in range(args.reps + 2)]

        def forward(fused, x, blks):
            if fused:
                return conv2(F.elu(conv1(x, blks[0])), blks[1])
            return composed_gat(conv2, F.elu(composed_gat(conv1, x, blks[0])), blks[1])

        def step(fused, seeds, k):
            blks, inputs = sampler.sample(seeds, 100 + 2 * k)
            for q in params:
                q.grad = None
            out = forward(fused, X.index_select(0, inputs), blks)
            F.cross_entropy(out, y.index_select(0, seeds)).backward()

        # the two paths compute the same function
        blks, inputs = sampler.sample(batches[0], 7)
        with torch.no_grad():
            a, b = forward(True, X.index_select(0, inputs), blks), forward(False, X.index_select(0, inputs), blks)
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), "fused and composed outputs differ"
        edges_0, edges_1 = int(blks[0].column_index.numel()), int(blks[1].column_index.numel())
        src_0 = blks[0].num_src
        del blks, a, b

        fused_ms, comp_ms, sample_ms = [], [], []
        for k, seeds in enumerate(batches):
            s = timed(lambda: sampler.sample(seeds, 100 + 2 * k))
            order = (True, False) if k % 2 == 0 else (False, True)        # alternate which path goes first
            t = {f: timed(lambda f=f: step(f, seeds, k)) for f in order}
            if k >= 2:                                                      # two warm-up rounds
                fused_ms.append(t[True]), comp_ms.append(t[False]), sample_ms.append(s)
        peak_fused = peak_of(lambda: step(True, batches[-1], 0))
        peak_comp = peak_of(lambda: step(False, batches[-1], 0))
        res = {"graph": name, "num_nodes": n, "nnz": int(info.column_index.numel()), "seeds": args.seeds, "fanouts": fanouts,
               "heads": args.heads, "hidden": args.hidden, "block0_src": src_0, "block0_edges": edges_0, "block1_edges": edges_1,
               "step_ms_fused": round(statistics.median(fused_ms), 3), "step_ms_composed": round(statistics.median(comp_ms), 3),
               "sample_ms": round(statistics.median(sample_ms), 3), "reps": args.reps,
               "peak_bytes_fused": int(peak_fused), "peak_bytes_composed": int(peak_comp)}
        res["sampling_share_of_fused_step"] = round(res["sample_ms"] / res["step_ms_fused"], 3)
        res["fused_no_slower"] = res["step_ms_fused"] <= res["step_ms_composed"]
        print(json.dumps(res), flush=True)
        del g, info, sampler, X, y
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())

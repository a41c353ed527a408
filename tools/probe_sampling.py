#!/usr/bin/env python3
"""Times device-side neighbor sampling (sampling.NeighborSampler -> gnna_sample_neighbors_i32) against the same rule composed
from torch ops on the GPU, and a mini-batch GraphSAGE step, on the Reddit-like and products-like graphs.

    python tools/probe_sampling.py [--graphs reddit-like,products-like] [--scale 1.0] [--seeds 1024] [--fanout 25,10] [--reps 10]

Per graph it prints one JSON line: ms per sample() call (library / torch composition, alternated in one process, medians),
ms per mini-batch step (sample + gather + forward + backward + Adam) and the share of the step spent sampling.  The torch
composition builds the keys of the seeds' rows in a padded [S, max degree] matrix, takes topk, sorts the picks and relabels
with unique -- it is checked against the library's block once before timing.  Conditions (profiles/sampling/README.md): the
library call is faster than the composition on both graphs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import graph, ops                      # noqa: E402
from gnnadvisor_osdi21_amd.sampling import NeighborSampler       # noqa: E402

M63 = (1 << 63) - 1


def _i64(v):
    """A 64-bit pattern as the int64 torch computes with (wrapping arithmetic)."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _lsr(z, k):
    """Logical shift right of int64 bit patterns."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def torch_keys(rng_seed, e):
    z = _i64(rng_seed) + _i64(0x9E3779B97F4A7C15) * (e + 1)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def torch_block(rp, ci, seeds, fanout, rng_seed):
    """The rule from torch ops: -> (blk_rp, edge ids, local column ids, src_nodes)."""
    s = seeds.long()
    start, deg = rp[s].long(), (rp[s + 1] - rp[s]).long()
    width = int(deg.max()) if s.numel() else 0
    slot = torch.arange(width, device=rp.device)
    valid = slot[None, :] < deg[:, None]
    e = start[:, None] + slot[None, :]
    take = deg.clamp(max=fanout) if fanout > 0 else deg
    if fanout > 0 and width > fanout:
        # unsigned order of the keys = signed order after flipping the top bit; padding sorts last
        keys = torch_keys(rng_seed, e) ^ _i64(1 << 63)
        keys = torch.where(valid, keys, torch.full_like(keys, M63))
        idx = keys.topk(fanout, dim=1, largest=False).indices
        picked = torch.zeros_like(valid).scatter_(1, idx, True) & valid
        picked = torch.where((deg <= fanout)[:, None], valid, picked)
    else:
        picked = valid
    eid = e[picked]                                                # row-major: rows in order, positions increasing
    blk_rp = torch.zeros(s.numel() + 1, dtype=torch.long, device=rp.device)
    blk_rp[1:] = take.cumsum(0)
    cols = ci[eid].long()
    n = rp.numel() - 1
    is_seed = torch.zeros(n, dtype=torch.bool, device=rp.device)
    is_seed[s] = True
    others = torch.unique(cols[~is_seed[cols]])
    src = torch.cat([s, others])
    local = torch.empty(n, dtype=torch.long, device=rp.device)
    local[src] = torch.arange(src.numel(), device=rp.device)
    return blk_rp, eid, local[cols], src


def torch_sample(rp, ci, seeds, fanouts, rng_seed):
    out, dst = [], seeds
    for layer in reversed(range(len(fanouts))):
        blk = torch_block(rp, ci, dst, fanouts[layer], rng_seed + layer)
        out.append(blk)
        dst = blk[3].int()
    return out[::-1]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", default="reddit-like,products-like")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanout", default="25,10")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--dim", type=int, default=64)
    args = p.parse_args(argv)
    fanouts = [int(f) for f in args.fanout.split(",")]
    dev = torch.device("cuda")
    for name in args.graphs.split(","):
        cfg = graph.CONFIGS[name]
        n, edges = max(64, int(cfg["num_nodes"] * args.scale)), int(cfg["num_edges"] * args.scale)
        g = graph.powerlaw_graph(n, edges, min(cfg["max_degree"], n - 1), seed=cfg["seed"])
        info = argparse.Namespace(row_pointers=g.row_pointers.to(dev), column_index=g.column_index.to(dev), partSize=32)
        rp, ci = info.row_pointers, info.column_index
        sampler = NeighborSampler(info, fanouts)
        X = torch.randn(n, args.dim, device=dev)
        y = torch.randint(0, cfg["classes"], (n,), device=dev)
        conv1, conv2 = ops.SAGEConv(args.dim, cfg["hidden"]).to(dev), ops.SAGEConv(cfg["hidden"], cfg["classes"]).to(dev)
        opt = torch.optim.Adam(list(conv1.parameters()) + list(conv2.parameters()), lr=0.01)
        gen = torch.Generator().manual_seed(1)
        batches = [torch.randperm(n, generator=gen)[: args.seeds].int().to(dev) for _ in range(args.reps + 2)]

        # the composition computes the library's block
        blocks, _ = sampler.sample(batches[0], 7)
        mine = torch_sample(rp, ci, batches[0], fanouts, 7)
        for b, m in zip(blocks, mine):
            assert torch.equal(b.row_pointers.long(), m[0]) and torch.equal(b.column_index.long(), m[2])
            assert torch.equal(b.src_nodes.long(), m[3])

        def step(seeds, k):
            blks, inputs = sampler.sample(seeds, 100 + 2 * k)
            opt.zero_grad()
            out = conv2(conv1(X.index_select(0, inputs), blks[0], relu=True), blks[1])
            loss = torch.nn.functional.cross_entropy(out, y.index_select(0, seeds))
            loss.backward()
            opt.step()

        lib_ms, torch_ms, step_ms = [], [], []
        for k, seeds in enumerate(batches):
            a = timed(lambda: sampler.sample(seeds, 100 + 2 * k))
            b = timed(lambda: torch_sample(rp, ci, seeds, fanouts, 100 + 2 * k))
            c = timed(lambda: step(seeds, k))
            if k >= 2:                                              # two warm-up rounds
                lib_ms.append(a), torch_ms.append(b), step_ms.append(c)
        res = {"graph": name, "num_nodes": n, "nnz": int(ci.numel()), "seeds": args.seeds, "fanouts": fanouts,
               "sample_ms_library": round(statistics.median(lib_ms), 3), "sample_ms_torch": round(statistics.median(torch_ms), 3),
               "step_ms": round(statistics.median(step_ms), 3), "reps": args.reps}
        res["sampling_share_of_step"] = round(res["sample_ms_library"] / res["step_ms"], 3)
        res["library_faster"] = res["sample_ms_library"] < res["sample_ms_torch"]
        print(json.dumps(res), flush=True)
        del g, info, sampler, X, rp, ci
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())

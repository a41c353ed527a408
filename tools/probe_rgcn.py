#!/usr/bin/env python3
"""Times the relation-typed aggregation (gnna_agg_typed_expand_ld_f32 and its two backward passes) against the same math
composed from the entries the library had before, on the Reddit-like and products-like graphs.

    python tools/probe_rgcn.py [--graphs reddit-like,products-like] [--scale 1.0] [--dim 64] [--relations 8] [--bases 4] [--reps 7]

Per graph it prints one JSON line with medians over alternated repetitions (ms) and the peak device memory of one step (MiB
above what the inputs hold):

  expand_ms            the fused forward alone: T = expand(X)
  fused_ms             fused forward + backward: expand, contract over the transposed structure, coef grad
  composed_ms          the yardstick -- forward: B calls of gnna_agg_edge_ld_f32 with w_b = n * C[t, b] built in torch;
                       backward: B edge-weighted calls over the transpose (weights read through its perm) plus B
                       gnna_sddmm_ld_f32 calls with index_add_ by type
  fused_peak_mib / composed_peak_mib

Both paths are compared once before timing.  Condition (profiles/rgcn/README.md): fused_ms < composed_ms and
fused_peak_mib < composed_peak_mib on both graphs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnadvisor_osdi21_amd import _lib, graph                                      # noqa: E402
from gnnadvisor_osdi21_amd.relational import RelationalGraph, synthetic_edge_types  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", default="reddit-like,products-like")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--relations", type=int, default=8)
    p.add_argument("--bases", type=int, default=4)
    p.add_argument("--reps", type=int, default=7)
    args = p.parse_args(argv)
    dev = torch.device("cuda")
    D, R, B, ps = args.dim, args.relations, args.bases, 32
    for name in args.graphs.split(","):
        cfg = graph.CONFIGS[name]
        n, edges = max(64, int(cfg["num_nodes"] * args.scale)), int(cfg["num_edges"] * args.scale)
        g = graph.powerlaw_graph(n, edges, min(cfg["max_degree"], n - 1), seed=cfg["seed"])
        pp, p2n = _lib.build_part(ps, g.row_pointers)
        info = argparse.Namespace(row_pointers=g.row_pointers.to(dev), column_index=g.column_index.to(dev), partSize=ps,
                                  partPtr=pp.to(dev), part2Node=p2n.to(dev))
        t_rp, t_ci, perm = _lib.transpose_csr(info.row_pointers, info.column_index)
        t_pp, t_p2n = _lib.build_part_device(ps, t_rp)
        tg = argparse.Namespace(row_pointers=t_rp, column_index=t_ci, partPtr=t_pp, part2Node=t_p2n, partSize=ps,
                                perm=perm.clamp_(min=0))
        info.transposed = lambda tg=tg: tg
        rel = RelationalGraph(info, synthetic_edge_types(info.row_pointers, info.column_index, R, seed=1), R)
        rel.transposed()
        ci, ety, nrm, perm64 = info.column_index, rel.edge_type.long(), rel.edge_norm, tg.perm.long()
        gen = torch.Generator().manual_seed(1)
        X = torch.randn(n, D, generator=gen).to(dev)
        C = torch.randn(R, B, generator=gen).to(dev)
        G = torch.randn(n, B * D, generator=gen).to(dev)

        def fused_forward():
            return rel.expand(X, C)

        def fused_step():
            return rel.expand(X, C), rel.contract(G, C), rel.coef_grad(X, G)

        def composed_step():
            T = torch.empty(n, B * D, device=dev)
            for b in range(B):
                w = nrm * C[:, b].index_select(0, ety)
                _lib.agg_edge(X, ci, w, info.partPtr, info.part2Node, n, ps, out=T[:, b * D:(b + 1) * D])
            dX = torch.empty(n, D, device=dev)
            dC = torch.zeros(R, B, device=dev)
            for b in range(B):
                w = (nrm * C[:, b].index_select(0, ety)).index_select(0, perm64)
                _lib.agg_edge(G[:, b * D:(b + 1) * D], t_ci, w, t_pp, t_p2n, n, ps, out=dX, accumulate=b > 0)
                s = _lib.sddmm(G[:, b * D:(b + 1) * D], X, ci, info.partPtr, info.part2Node, ps)
                dC[:, b].index_add_(0, ety, s * nrm)
            return T, dX, dC

        # both paths compute the same thing (fp32 sums in another order)
        for got, want, what in zip(fused_step(), composed_step(), ("T", "dX", "dC")):
            err = float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))
            assert err < 1e-3, f"{name}: fused and composed {what} differ ({err:.2e} of the largest value)"

        expand_ms, fused_ms, composed_ms = [], [], []
        for k in range(args.reps + 2):
            a, b, c = timed(fused_forward), timed(fused_step), timed(composed_step)
            if k >= 2:                                                # two warm-up rounds
                expand_ms.append(a), fused_ms.append(b), composed_ms.append(c)
        res = {"graph": name, "num_nodes": n, "nnz": int(ci.numel()), "dim": D, "relations": R, "bases": B, "reps": args.reps,
               "expand_ms": round(statistics.median(expand_ms), 3), "fused_ms": round(statistics.median(fused_ms), 3),
               "composed_ms": round(statistics.median(composed_ms), 3),
               "fused_ms_min_max": [round(min(fused_ms), 3), round(max(fused_ms), 3)],
               "composed_ms_min_max": [round(min(composed_ms), 3), round(max(composed_ms), 3)],
               "fused_peak_mib": round(peak_mib(fused_step), 1), "composed_peak_mib": round(peak_mib(composed_step), 1)}
        res["fused_faster"] = res["fused_ms"] < res["composed_ms"]
        res["fused_smaller"] = res["fused_peak_mib"] < res["composed_peak_mib"]
        print(json.dumps(res), flush=True)
        del g, info, tg, rel, X, G, ci, ety, nrm, perm64, t_rp, t_ci, t_pp, t_p2n, perm
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The one-gather softmax aggregation against what a caller had before and against the library's other gathers, in ONE process
(profiles/softmax_agg/):

    python tools/probe_softmax_agg.py [--graphs reddit-like,products-like] [--dims 64,128] [--reps 5] [--rounds 5]
                                      [--composed-on amazon0505-like] [--only VARIANT,...] [--out profiles/softmax_agg/probe.jsonl]

Per graph and width, fp32, on a prepared graph (gnna_prepare_graph, as main.py prepares it), ms per call:
  softmax_fwd            gnna_agg_softmax_ld_f32 without sq (NeighborSoftmax's forward with a fixed temperature);
  softmax_fwd_sq         the same with sq (a learnt temperature);
  softmax_step           ops.NeighborSoftmax forward + backward for X (a fixed temperature): the forward gather, the pack pass and
                         the backward gather;
  softmax_step_learn     the same with a learnt temperature: sq in the forward, dt in node-sized torch arithmetic;
  sag_fwd / sag_step     gnna_agg_ld_f32 (the neighbor sum on the library's schedule for the prepared graph) once / twice: what a
                         sum aggregator costs for the forward / for forward + backward at that width;
  stats_moments, stats   gnna_agg_stats_ld_f32 for sum and sumsq / for all four statistics: the other one-gather kernel;
  composed_fwd, composed_step, composed_step_learn
                         SoftmaxAggregation(fused=False), the composition from torch ops with [nnz, F] tensors -- only on the
                         graphs named by --composed-on (a step keeps several [nnz, F] tensors alive).
The variants are alternated round by round after a warm-up; ms from HIP events, the median over the rounds.  *_step variants also
report peak_mib: torch.cuda.max_memory_allocated of one step above what was allocated before it.  One JSON line per variant,
printed and appended to --out; softmax lines carry vs_sag / vs_stats / vs_composed = softmax / other (below 1: the softmax entry
is faster)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import _lib, graph, ops  # noqa: E402

RATIOS = {"softmax_fwd": (("vs_sag", "sag_fwd"), ("vs_stats", "stats_moments"), ("vs_composed", "composed_fwd")),
          "softmax_fwd_sq": (("vs_sag", "sag_fwd"), ("vs_stats", "stats_moments")),
          "softmax_step": (("vs_sag", "sag_step"), ("vs_composed", "composed_step")),
          "softmax_step_learn": (("vs_sag", "sag_step"), ("vs_composed", "composed_step_learn"))}


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="reddit-like,products-like")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--composed-on", default="amazon0505-like", help="graphs on which the torch composition is timed as well")
    ap.add_argument("--only", default="", help="time these variants alone (a comma list)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_agg", "probe.jsonl"))
    args = ap.parse_args()
    dims = [int(d) for d in args.dims.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = open(args.out, "a")
    for name in args.graphs.split(","):
        g = graph.make_config_graph(name, device="cuda")
        n, nnz, ps = g.num_nodes, g.column_index.numel(), args.partSize
        rp, ci = g.row_pointers.cuda(), g.column_index
        pp, p2n = [t.cuda() for t in _lib.build_part(ps, g.row_pointers.cpu())]
        _lib.prepare_graph(ci, pp, p2n, n, n, ps, dims)
        info = types.SimpleNamespace(row_pointers=rp, column_index=ci, degrees=None, partPtr=pp, part2Node=p2n, partSize=ps,
                                     dimWorker=32, warpPerBlock=4, directed=False)
        for D in dims:
            gen = torch.Generator(device="cuda").manual_seed(1)
            X = torch.randn(n, D, device="cuda", generator=gen)
            G = torch.randn(n, D, device="cuda", generator=gen)
            t = torch.ones(1, device="cuda")
            bufs = [torch.empty(n, D, device="cuda") for _ in range(4)]
            i32 = [torch.empty(n, D, dtype=torch.int32, device="cuda") for _ in range(2)]
            stats_out = dict(sum=bufs[0], sumsq=bufs[1], max=bufs[2], min=bufs[3], argmax=i32[0], argmin=i32[1])

            def step(fused, learn):
                agg = ops.SoftmaxAggregation(t=1.0, learn=learn, fused=fused).cuda()
                Xr = X.detach().requires_grad_(True)

                def run():
                    Xr.grad = None
                    agg.zero_grad(set_to_none=True)
                    (agg(Xr, info) * G).sum().backward()
                return run

            def sag():
                _lib.agg_ld(0, X, ci, pp, p2n, n, ps, out=bufs[0])

            def sag_twice():
                _lib.agg_ld(0, X, ci, pp, p2n, n, ps, out=bufs[0])
                _lib.agg_ld(0, G, ci, pp, p2n, n, ps, out=bufs[1])

            composed = ops.SoftmaxAggregation(t=1.0, fused=False).cuda()

            def composed_fwd():
                with torch.no_grad():
                    composed(X, info)

            variants = {
                "softmax_fwd": lambda: _lib.agg_softmax(X, t, rp, ci, n, out=bufs[0], lse=bufs[1]),
                "softmax_fwd_sq": lambda: _lib.agg_softmax(X, t, rp, ci, n, out=bufs[0], lse=bufs[1], sq=bufs[2]),
                "softmax_step": step(True, False),
                "softmax_step_learn": step(True, True),
                "sag_fwd": sag,
                "sag_step": sag_twice,
                "stats_moments": lambda: _lib.agg_stats_ld(X, ci, pp, p2n, n, ps, want=("sum", "sumsq"), out=stats_out),
                "stats": lambda: _lib.agg_stats_ld(X, ci, pp, p2n, n, ps, out=stats_out),
            }
            if name in args.composed_on.split(","):
                variants.update(composed_fwd=composed_fwd, composed_step=step(False, False), composed_step_learn=step(False, True))
            if args.only:
                variants = {k: variants[k] for k in args.only.split(",")}
            for fn in variants.values():      # warm-up: plans, packed copies, scratch, clocks
                timed(fn, 2)
            ms = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn, args.reps))
            head = dict(graph=name, nodes=n, edges=nnz, dim=D, partSize=ps, reps=args.reps, rounds=args.rounds)
            med = {k: statistics.median(v) for k, v in ms.items()}
            for k, v in ms.items():
                rec = dict(head, variant=k, ms_per_call=round(med[k], 4), ms_rounds=[round(x, 4) for x in v])
                if k.endswith(("_step", "_step_learn")) and k != "sag_step":
                    rec["peak_mib"] = round(peak_mib(variants[k]), 1)
                for key, other in RATIOS.get(k, ()):
                    if other in med:
                        rec[key] = round(med[k] / med[other], 4)
                line = json.dumps(rec)
                print(line, flush=True)
                sink.write(line + "\n")
                sink.flush()
            del X, G, bufs, i32, stats_out, variants
            torch.cuda.empty_cache()
        _lib.release_graph(ci)
        del g, ci, rp, pp, p2n, info
        torch.cuda.empty_cache()
    sink.close()


if __name__ == "__main__":
    main()

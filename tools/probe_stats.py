"""The four neighbor statistics from one gather against the composition a caller had before, in ONE process (profiles/pna/):

    python tools/probe_stats.py [--graphs reddit-like,products-like] [--dims 64,128] [--reps 10] [--rounds 5] [--only VARIANT]
                                [--out profiles/pna/probe.jsonl]

Per graph and width, on a prepared graph (gnna_prepare_graph, as main.py prepares it):
  fused            gnna_agg_stats_ld_f32: sum, sumsq, max + argmax, min + argmin in one call;
  composed         what the older entries need for the same six results: gnna_agg_ld_f32 (sum) on X, X * X into an [N, D]
                   temporary and gnna_agg_ld_f32 on it, gnna_agg_reduce_ld_f32 max with arg, the same with min;
  fused_moments    the fused call for sum and sumsq alone;     composed_moments: the two sums and X * X;
  fused_extrema    the fused call for max and min with arg;    composed_extrema: the two reduce calls.
The variants are alternated round by round after a warm-up; ms per call from HIP events, the median over the rounds.  One JSON
line per variant, printed and appended to --out; fused lines carry vs_composed = fused / composed (below 1: the fused call is
faster).  Kernel times: the same command under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import _lib, graph  # noqa: E402

PAIRS = {"fused": "composed", "fused_moments": "composed_moments", "fused_extrema": "composed_extrema"}


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="reddit-like,products-like")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", help="time this variant alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pna", "probe.jsonl"))
    args = ap.parse_args()
    dims = [int(d) for d in args.dims.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = open(args.out, "a")
    for name in args.graphs.split(","):
        g = graph.make_config_graph(name, device="cuda")
        n, nnz, ps = g.num_nodes, g.column_index.numel(), args.partSize
        ci = g.column_index
        pp, p2n = [t.cuda() for t in _lib.build_part(ps, g.row_pointers.cpu())]
        _lib.prepare_graph(ci, pp, p2n, n, n, ps, dims)
        for D in dims:
            X = torch.randn(n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            f32 = {k: torch.empty(n, D, device="cuda") for k in ("sum", "sumsq", "max", "min", "sq")}
            i32 = {k: torch.empty(n, D, dtype=torch.int32, device="cuda") for k in ("argmax", "argmin")}
            outs = {k: f32[k] for k in ("sum", "sumsq", "max", "min")}
            outs.update(i32)

            def composed_moments():
                _lib.agg_ld(0, X, ci, pp, p2n, n, ps, out=f32["sum"])
                torch.mul(X, X, out=f32["sq"])
                _lib.agg_ld(0, f32["sq"], ci, pp, p2n, n, ps, out=f32["sumsq"])

            def composed_extrema():
                _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, ps, out=f32["max"], arg=i32["argmax"])
                _lib.agg_reduce_ld(_lib.REDUCE_MIN, X, ci, pp, p2n, ps, out=f32["min"], arg=i32["argmin"])

            def composed():
                composed_moments()
                composed_extrema()

            variants = {
                "fused": lambda: _lib.agg_stats_ld(X, ci, pp, p2n, n, ps, out=outs),
                "composed": composed,
                "fused_moments": lambda: _lib.agg_stats_ld(X, ci, pp, p2n, n, ps, want=("sum", "sumsq"), out=outs),
                "composed_moments": composed_moments,
                "fused_extrema": lambda: _lib.agg_stats_ld(X, ci, pp, p2n, n, ps, want=("max", "min"), out=outs),
                "composed_extrema": composed_extrema,
            }
            if args.only:
                variants = {args.only: variants[args.only]}
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
                if PAIRS.get(k) in med:
                    rec["vs_composed"] = round(med[k] / med[PAIRS[k]], 4)
                line = json.dumps(rec)
                print(line, flush=True)
                sink.write(line + "\n")
                sink.flush()
            del X, f32, i32, outs
            torch.cuda.empty_cache()
        _lib.release_graph(ci)
        del g, ci, pp, p2n
        torch.cuda.empty_cache()
    sink.close()


if __name__ == "__main__":
    main()

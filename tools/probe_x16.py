"""16-bit storage against fp32 on the same graph, in ONE process (profiles/x16/):

    python tools/probe_x16.py [--graphs reddit-like,products-like] [--dims 64,128] [--reps 20] [--rounds 5] [--only VARIANT]

Per graph and width, unweighted SAG on a prepared graph (gnna_prepare_graph + gnna_prepare_x16, as main.py prepares it): the fp32
call gnna_agg_ld_f32 -- the yardstick -- and gnna_agg_ld_x16 on bfloat16 / float16 features with 16-bit and with fp32 output.
The variants are alternated round by round after a warm-up; ms per call from HIP events, the median over the rounds.
Kernel times: the same command under `rocprofv3 --kernel-trace --stats` in a run of its own; L2 requests per edge: a separate
`rocprofv3 --pmc` run with --only.  One JSON line per variant."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import _lib, graph  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", help="time this variant alone (counter runs)")
    args = ap.parse_args()
    dims = [int(d) for d in args.dims.split(",")]
    for name in args.graphs.split(","):
        g = graph.make_config_graph(name, device="cuda")
        n, nnz, ps = g.num_nodes, g.column_index.numel(), args.partSize
        ci = g.column_index
        pp, p2n = [t.cuda() for t in _lib.build_part(ps, g.row_pointers.cpu())]
        _lib.prepare_graph(ci, pp, p2n, n, n, ps, dims)
        _lib.prepare_x16(n, n, dims)
        for D in dims:
            X = torch.randn(n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            Xb, Xh = X.bfloat16(), X.half()
            o32 = torch.empty(n, D, device="cuda")
            ob, oh = torch.empty_like(Xb), torch.empty_like(Xh)
            variants = {
                "fp32": lambda: _lib.agg_ld(0, X, ci, pp, p2n, n, ps, out=o32),
                "bf16_out_bf16": lambda: _lib.agg_ld_x16(0, Xb, ci, pp, p2n, n, ps, out=ob),
                "bf16_out_fp32": lambda: _lib.agg_ld_x16(0, Xb, ci, pp, p2n, n, ps, out=o32),
                "fp16_out_fp16": lambda: _lib.agg_ld_x16(0, Xh, ci, pp, p2n, n, ps, out=oh),
                "fp16_out_fp32": lambda: _lib.agg_ld_x16(0, Xh, ci, pp, p2n, n, ps, out=o32),
            }
            if args.only:
                variants = {args.only: variants[args.only]}
            for fn in variants.values():      # warm-up: plans, packed copies, scratch, clocks
                timed(fn, 3)
            ms = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn, args.reps))
            head = dict(graph=name, nodes=n, edges=nnz, dim=D, partSize=ps, reps=args.reps, rounds=args.rounds)
            med = {k: statistics.median(v) for k, v in ms.items()}
            for k, v in ms.items():
                rec = dict(head, variant=k, ms_per_call=round(med[k], 4), ms_rounds=[round(x, 4) for x in v])
                if "fp32" in med and k != "fp32":
                    rec["vs_fp32"] = round(med[k] / med["fp32"], 4)
                print(json.dumps(rec), flush=True)
        _lib.release_graph(ci)
        del g, ci, pp, p2n
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

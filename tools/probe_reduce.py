"""Max / min neighbor reduction against the SAG call on the same graph, in ONE process (profiles/neighbor_reduce/):

    python tools/probe_reduce.py [--graphs reddit-like,products-like] [--dims 64,128] [--reps 10] [--rounds 5] [--only VARIANT]
                                 [--out profiles/neighbor_reduce/probe.jsonl]

Per graph and width, on a prepared graph (gnna_prepare_graph, as main.py prepares it):
  sag              gnna_agg_ld_f32 mode 0, the yardstick: the same gather, whatever kernel the library picks for it;
  sag_stream       the same call held to the streaming kernel (gnna_tuning.sweep = 2), the like-for-like line;
  reduce_max_arg   gnna_agg_reduce_ld_f32 max with arg;      reduce_max_noarg: with arg = NULL;
  scatter_arg      gnna_scatter_arg_ld_f32 on the positions of reduce_max_arg;
  torch_amax       what a caller had before: X[column_index] + scatter_reduce("amax") on the GPU (nnz x D floats of temporary;
                   an allocation failure is recorded instead of a time).
The variants are alternated round by round after a warm-up; ms per call from HIP events, the median over the rounds.  One JSON
line per variant, printed and appended to --out.  Kernel times: the same command under `rocprofv3 --kernel-trace --stats` in a
run of its own."""
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", help="time this variant alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_reduce", "probe.jsonl"))
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
        rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (g.row_pointers[1:] - g.row_pointers[:-1]).long().cuda())
        for D in dims:
            X = torch.randn(n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            out, gi = torch.empty(n, D, device="cuda"), torch.empty(n, D, device="cuda")
            arg = torch.empty(n, D, dtype=torch.int32, device="cuda")
            _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, ps, out=out, arg=arg)

            def sag_stream():
                _lib.set_tuning(sweep=2)
                try:
                    _lib.agg_ld(0, X, ci, pp, p2n, n, ps, out=out)
                finally:
                    _lib.reset_tuning()

            def torch_amax():
                src = X[ci.long()]
                torch.zeros(n, D, device="cuda").scatter_reduce_(0, rows[:, None].expand_as(src), src, reduce="amax", include_self=False)

            variants = {
                "sag": lambda: _lib.agg_ld(0, X, ci, pp, p2n, n, ps, out=out),
                "sag_stream": sag_stream,
                "reduce_max_arg": lambda: _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, ps, out=out, arg=arg),
                "reduce_max_noarg": lambda: _lib.agg_reduce_ld(_lib.REDUCE_MAX, X, ci, pp, p2n, ps, out=out, want_arg=False),
                "scatter_arg": lambda: _lib.scatter_arg_ld(X, arg, ci, n, out=gi),
                "torch_amax": torch_amax,
            }
            if args.only:
                variants = {args.only: variants[args.only]}
            failed = {}
            for k, fn in list(variants.items()):      # warm-up: plans, packed copies, scratch, clocks
                try:
                    timed(fn, 2)
                except torch.OutOfMemoryError as e:
                    failed[k] = str(e).splitlines()[0]
                    del variants[k]
                    torch.cuda.empty_cache()
            ms = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn, args.reps if k != "torch_amax" else max(1, args.reps // 5)))
            head = dict(graph=name, nodes=n, edges=nnz, dim=D, partSize=ps, reps=args.reps, rounds=args.rounds)
            med = {k: statistics.median(v) for k, v in ms.items()}
            recs = [dict(head, variant=k, ms_per_call=round(med[k], 4), ms_rounds=[round(x, 4) for x in v]) for k, v in ms.items()]
            recs += [dict(head, variant=k, ms_per_call=None, failed=why) for k, why in failed.items()]
            for rec in recs:
                if rec["ms_per_call"] is not None:
                    for base in ("sag", "sag_stream", "torch_amax"):
                        if base in med and rec["variant"] != base:
                            rec["vs_" + base] = round(rec["ms_per_call"] / med[base], 4)
                line = json.dumps(rec)
                print(line, flush=True)
                sink.write(line + "\n")
                sink.flush()
            del X, out, gi, arg
            torch.cuda.empty_cache()
        _lib.release_graph(ci)
        del g, ci, pp, p2n, rows
        torch.cuda.empty_cache()
    sink.close()


if __name__ == "__main__":
    main()

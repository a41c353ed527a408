"""The rows form of the fused GATv2 attention against the atomic fused path (profiles/gatv2_rows/):

    python tools/probe_gatv2_rows.py [--graphs reddit-like,products-like,amazon0505-like] [--configs 1x64,4x16] [--reps 5] [--rounds 5]

The attention alone, from (Hs, Hd, att): "forward" is the forward call, "step" forward + backward to (dHs, dHd, d_att), as
ops.GATv2Attention ("atomic") and ops.GATv2AttentionRows ("rows") run them, in ONE process, the two alternated round by round, ms
from HIP events, median / smallest / largest round.  Then the backward of the rows form by what is asked of it -- dHd alone (the
destination side walking the edges), dHd and d_att (the same with the workgroups' partials and the finishing kernel), dHs alone
(the destination side without an edge walk, for the records, and the source side) -- the peak torch memory of one step of either,
and how far the outputs of the two are apart (relative to the largest |element|).  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gnnadvisor_osdi21_amd import graph  # noqa: E402
from probe_gat_fused import Info, timed  # noqa: E402

SPLIT = {"dHd (destination side)": [False, True, False], "dHd + d_att (destination side, partials, finish)": [False, True, True],
         "dHs (records, source side)": [True, False, False], "all three": [True, True, True]}


def variants(info, heads, dim, seed=1):
    from gnnadvisor_osdi21_amd.ops import GNNA, GATv2Attention, GATv2AttentionRows
    n = info.row_pointers.numel() - 1
    gen = torch.Generator(device="cuda").manual_seed(seed)
    Hs, Hd = [torch.randn(n, heads * dim, device="cuda", generator=gen).requires_grad_() for _ in range(2)]
    att = ((torch.rand(heads, dim, device="cuda", generator=gen) * 2 - 1) / dim ** 0.5).requires_grad_()
    G = torch.randn(n, heads * dim, device="cuda", generator=gen)
    out = {}
    for name, op in (("atomic", GATv2Attention), ("rows", GATv2AttentionRows)):
        def forward(op=op):
            with torch.no_grad():
                return op.apply(Hs, Hd, att, info, 0.2)

        def step(op=op):
            return torch.autograd.grad(op.apply(Hs, Hd, att, info, 0.2), (Hs, Hd, att), G)
        out[name] = {"forward": forward, "step": step}
    with torch.no_grad():
        Y, lse = GNNA.gatv2_forward_rows(Hs, Hd, att, info.row_pointers, info.column_index, 0.2)
    split = {k: (lambda need=need: GNNA.gatv2_backward_rows(Hs.detach(), Hd.detach(), att.detach(), lse, Y, G, info.row_pointers,
                                                            info.column_index, info.row_pointers, info.column_index, 0.2, 0.0, 0, need))
             for k, need in SPLIT.items()}
    return out, split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="reddit-like,products-like,amazon0505-like")
    ap.add_argument("--configs", default="1x64,4x16", help="heads x dim, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for name in args.graphs.split(","):
        g = graph.make_config_graph(name, device="cuda")
        info = Info(g, 32)
        head = dict(graph=name, nodes=g.num_nodes, edges=info.column_index.numel(), reps=args.reps, rounds=args.rounds)
        for cfg in args.configs.split(","):
            heads, dim = [int(v) for v in cfg.split("x")]
            v, split = variants(info, heads, dim)
            a, r = [(v[k]["forward"](),) + v[k]["step"]() for k in ("atomic", "rows")]      # (also the warm-up: symmetry check, scratch)
            apart = [float((x - y).abs().max() / x.abs().max()) for x, y in zip(a, r)]
            print(json.dumps(dict(head, heads=heads, dim=dim, figure="rows vs atomic, max |difference| / max |element| of (Y, dHs, "
                                  "dHd, d_att)", values=[float("%.3g" % x) for x in apart])), flush=True)
            del a, r
            for what in ("forward", "step"):
                ms = {k: [] for k in v}
                for _ in range(args.rounds):
                    for k in v:
                        ms[k].append(timed(v[k][what], args.reps))
                for k, t in ms.items():
                    print(json.dumps(dict(head, heads=heads, dim=dim, what=what, variant=k, ms_median=round(statistics.median(t), 4),
                                          ms_min=round(min(t), 4), ms_max=round(max(t), 4))), flush=True)
                print(json.dumps(dict(head, heads=heads, dim=dim, what=what, variant="rows / atomic",
                                      ratio_of_medians=round(statistics.median(ms["rows"]) / statistics.median(ms["atomic"]), 4))), flush=True)
            for k, call in split.items():
                call()
                t = [timed(call, args.reps) for _ in range(args.rounds)]
                print(json.dumps(dict(head, heads=heads, dim=dim, what="rows backward, asked for " + k,
                                      ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))), flush=True)
            for k in v:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                timed(v[k]["step"], 1)
                print(json.dumps(dict(head, heads=heads, dim=dim, variant=k, figure="peak torch memory of one step, MiB",
                                      peak_mib=round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))), flush=True)
            del v, split
            torch.cuda.empty_cache()
        del info, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

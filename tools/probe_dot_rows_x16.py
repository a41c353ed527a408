"""The rows form of the fused dot-product attention on bf16 / fp16 storage against the same on fp32 (profiles/dot_rows_x16/):

    python tools/probe_dot_rows_x16.py [--graphs reddit-like,products-like,amazon0505-like] [--configs 1x64,4x16] [--reps 5] [--rounds 5]

The attention alone, from (Q, K, V): "forward" is the forward call, "step" forward + backward to (dQ, dK, dV), as
ops.DotAttentionRows runs them on float32, bfloat16 and float16 leaves, in ONE process, the three alternated round by round, ms from
HIP events, median / smallest / largest round.  Then the peak torch memory of one step of each, and how far the 16-bit outputs are
from the fp32 ones (relative to the largest |element|; the inputs of the 16-bit runs are the rounded fp32 inputs).  One JSON line
per figure.  (The fp32 kernels are those of gnna_dot_rows.hip, whose object code this feature leaves as it was.)"""
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

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def variants(info, heads, dim, seed=1):
    from gnnadvisor_osdi21_amd.ops import DotAttentionRows
    n = info.row_pointers.numel() - 1
    gen = torch.Generator(device="cuda").manual_seed(seed)
    base = [torch.randn(n, heads * dim, device="cuda", generator=gen) for _ in range(4)]
    out = {}
    for name, dtype in DTYPES.items():
        Q, K, V = [t.to(dtype).requires_grad_() for t in base[:3]]
        G = base[3].to(dtype)

        def forward(Q=Q, K=K, V=V):
            with torch.no_grad():
                return DotAttentionRows.apply(Q, K, V, info, heads)

        def step(Q=Q, K=K, V=V, G=G):
            return torch.autograd.grad(DotAttentionRows.apply(Q, K, V, info, heads), (Q, K, V), G)
        out[name] = {"forward": forward, "step": step}
    return out


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
            v = variants(info, heads, dim)
            res = {k: (v[k]["forward"](),) + v[k]["step"]() for k in v}         # (also the warm-up: symmetry check, scratch)
            for k in ("bf16", "fp16"):
                apart = [float((x - y.float()).abs().max() / x.abs().max()) for x, y in zip(res["fp32"], res[k])]
                print(json.dumps(dict(head, heads=heads, dim=dim, figure=f"{k} vs fp32, max |difference| / max |element| of (Y, dQ, dK, "
                                      "dV)", values=[float("%.3g" % x) for x in apart])), flush=True)
            del res
            for what in ("forward", "step"):
                ms = {k: [] for k in v}
                for _ in range(args.rounds):
                    for k in v:
                        ms[k].append(timed(v[k][what], args.reps))
                for k, t in ms.items():
                    print(json.dumps(dict(head, heads=heads, dim=dim, what=what, variant=k, ms_median=round(statistics.median(t), 4),
                                          ms_min=round(min(t), 4), ms_max=round(max(t), 4))), flush=True)
                for k in ("bf16", "fp16"):
                    print(json.dumps(dict(head, heads=heads, dim=dim, what=what, variant=f"{k} / fp32",
                                          ratio_of_medians=round(statistics.median(ms[k]) / statistics.median(ms["fp32"]), 4))), flush=True)
            for k in v:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                timed(v[k]["step"], 1)
                print(json.dumps(dict(head, heads=heads, dim=dim, variant=k, figure="peak torch memory of one step, MiB",
                                      peak_mib=round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))), flush=True)
            del v
            torch.cuda.empty_cache()
        del info, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Edge-attention measurements on the Reddit-like graph (profiles/edge_attention/):

    python tools/probe_edge_attention.py [--reps 20] [--dim 64] [--graph reddit-like] [--only agg|softmax]

* the edge-weighted aggregation (gnna_agg_edge_ld_f32) against SAG, the per-edge GCN form (gcn_prescale = 2, same streaming
  kernel) and torch.sparse.mm on a CSR tensor with values -- in ONE process, the variants alternated round by round, on a
  prepared graph (as main.py prepares it), ms per call from HIP events;
* the edge softmax, forward and backward, per head.
Kernel times: the same command under `rocprofv3 --kernel-trace --stats` in a run of its own.  One JSON line per variant."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import _lib, graph, load_extension  # noqa: E402


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
    ap.add_argument("--graph", default="reddit-like")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--partSize", type=int, default=32)
    ap.add_argument("--only", default="", choices=["", "agg", "softmax"])
    args = ap.parse_args()
    GNNA = load_extension()
    g = graph.make_config_graph(args.graph, device="cuda")
    n, nnz, D, ps = g.num_nodes, g.column_index.numel(), args.dim, args.partSize
    rp, ci = g.row_pointers, g.column_index
    pp, p2n = [t.cuda() for t in _lib.build_part(ps, rp.cpu())]
    deg = g.degrees.cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n, D, device="cuda", generator=gen)
    w = torch.rand(nnz, device="cuda", generator=gen)
    head = dict(graph=args.graph, nodes=n, edges=nnz, dim=D, partSize=ps, reps=args.reps, rounds=args.rounds)
    if args.only in ("", "agg"):
        _lib.prepare_graph(ci, pp, p2n, n, n, ps, [D])
        A = torch.sparse_csr_tensor(rp.long(), ci.long(), w, size=(n, n))
        out = torch.empty(n, D, device="cuda")

        variants = {
            "sag": lambda: GNNA.aggregate_ld(0, X, ci, None, 1.0, pp, p2n, ps, out),
            "gcn_per_edge": lambda: GNNA.aggregate_ld(1, X, ci, deg, 1.0, pp, p2n, ps, out),     # (timed under gcn_prescale = 2)
            "edge_weighted": lambda: GNNA.aggregate_edge(X, ci, w, pp, p2n, ps, out),
            "torch_sparse_mm": lambda: torch.sparse.mm(A, X),
        }
        def run(k, fn, reps):
            if k == "gcn_per_edge":
                _lib.set_tuning(gcn_prescale=2)
            try:
                return timed(fn, reps)
            finally:
                _lib.reset_tuning()
        for k, fn in variants.items():    # warm-up: plans, packed copies, scratch
            run(k, fn, 2)
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(run(k, fn, args.reps))
        for k, v in ms.items():
            print(json.dumps(dict(head, variant=k, ms_per_call=min(v), ms_rounds=[round(x, 4) for x in v])), flush=True)
        ratio = min(ms["edge_weighted"]) / min(ms["gcn_per_edge"])
        print(json.dumps(dict(head, variant="edge_weighted / gcn_per_edge", ratio=round(ratio, 4), target=1.10)), flush=True)
    if args.only in ("", "softmax"):
        s = torch.randn(nnz, device="cuda", generator=gen) * 10
        dp = torch.randn(nnz, device="cuda", generator=gen)
        p = GNNA.edge_softmax(s, rp)
        fwd = [timed(lambda: GNNA.edge_softmax(s, rp), args.reps) for _ in range(args.rounds)]
        bwd = [timed(lambda: GNNA.edge_softmax_backward(p, dp, rp), args.reps) for _ in range(args.rounds)]
        print(json.dumps(dict(head, variant="edge_softmax_forward_per_head", ms_per_call=min(fwd), target_ms=0.4)), flush=True)
        print(json.dumps(dict(head, variant="edge_softmax_backward_per_head", ms_per_call=min(bwd), target_ms=0.4)), flush=True)


if __name__ == "__main__":
    main()

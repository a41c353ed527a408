#!/usr/bin/env python3
"""Times the subgraph sampler (sampling.SaintRWSampler -> gnna_random_walk_i32 + gnna_induced_subgraph_i32) against the same two
rules composed from torch ops on the GPU, and a GraphSAINT training step, on the Reddit-like and products-like graphs.

    python tools/probe_saint.py [--graphs reddit-like,products-like] [--scale 1.0] [--roots 2000] [--walk_length 2] [--reps 10]
                                [--timeout 900]

One child process per graph, each under its own time limit; after a child that fails or runs out of time nothing more is started.
Per graph the child prints one JSON line (medians after two warm-up rounds, the library call and the torch composition alternated
in one process, wall-clock with a device synchronisation around every call):

  (a) ms per random_walk call / per torch composition of the walk rule (per step: two row-pointer gathers, the splitmix64 key in
      int64 bit patterns, the high half of key * d from two 32-bit halves, one column gather) -- checked to give the library's walks
      before it is timed;
  (b) ms per induced_subgraph call / per torch composition (a new_id table, a mask over ALL edges, nonzero, bincount + cumsum,
      build_part_device; the row of every edge is built once outside the timing) -- checked equal before it is timed;
  (c) ms per training step (roots, walk, subgraph, gather x and y, two SAGEConv layers forward and backward, Adam) and the share
      of it that is sampling -- to be read beside the --fanout 25,10 figures of profiles/sampling/;
  (d) the positions one call's fill pass visits (the degree sum of the kept rows): over the fill kernels' time from a kernel
      trace of `--child NAME --only subgraph` it gives the fill pass's edges/s.
Conditions (profiles/saint/README.md): (a) and (b) are faster than their compositions on both graphs.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M32 = (1 << 32) - 1


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


def torch_walk(rp, ci, roots, walk_length, rng_seed):
    """The walk rule from torch ops (valid roots, a consistent CSR): -> (walks [R, L + 1], edge_ids [R, L]) int64."""
    import torch
    n, R, L = rp.numel() - 1, roots.numel(), walk_length
    v = roots.long()
    w = torch.arange(R, device=rp.device)
    walks, eids = [v], []
    for t in range(L):
        lo = rp[v].long()
        d = rp[v + 1].long() - lo
        key = torch_keys(rng_seed, w * L + t)
        # floor(key * d / 2^64) from the two 32-bit halves of the key (d < 2^31: no product leaves 63 bits)
        j = ((_lsr(key, 32) * d) + _lsr((key & M32) * d, 32)) >> 32
        e = (lo + j).clamp(max=ci.numel() - 1)
        c = ci[e].long()
        move = (d > 0) & (c >= 0) & (c < n)
        v = torch.where(move, c, v)
        walks.append(v)
        eids.append(torch.where(move, e, torch.full_like(e, -1)))
    return torch.stack(walks, 1), (torch.stack(eids, 1) if L else torch.zeros(R, 0, dtype=torch.long, device=rp.device))


def torch_subgraph(rp, ci, rows, ids, partSize):
    """The subgraph rule from torch ops, edge-parallel: -> (S, sub_rp, sub_ci, edge ids, partPtr, part2Node)."""
    import torch
    from gnnadvisor_osdi21_amd import _lib
    n = rp.numel() - 1
    mark = torch.zeros(n, dtype=torch.bool, device=rp.device)
    mark[ids[ids >= 0].long()] = True
    S = mark.nonzero().flatten()
    new_id = torch.full((n,), -1, dtype=torch.long, device=rp.device)
    new_id[S] = torch.arange(S.numel(), device=rp.device)
    keep = mark[rows] & mark[ci.long()]                             # a mask over all edges
    eid = keep.nonzero().flatten()
    sub_ci = new_id[ci[eid].long()]
    sub_rp = torch.zeros(S.numel() + 1, dtype=torch.long, device=rp.device)
    sub_rp[1:] = torch.bincount(new_id[rows[eid]], minlength=S.numel()).cumsum(0)
    pp, p2n = _lib.build_part_device(partSize, sub_rp.int())
    return S, sub_rp, sub_ci, eid, pp, p2n


def child(args):
    import torch
    from gnnadvisor_osdi21_amd import _lib, graph, ops
    from gnnadvisor_osdi21_amd.sampling import SaintRWSampler

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    name, dev = args.child, torch.device("cuda")
    cfg = graph.CONFIGS[name]
    n, edges = max(64, int(cfg["num_nodes"] * args.scale)), int(cfg["num_edges"] * args.scale)
    g = graph.powerlaw_graph(n, edges, min(cfg["max_degree"], n - 1), seed=cfg["seed"])
    info = argparse.Namespace(row_pointers=g.row_pointers.to(dev), column_index=g.column_index.to(dev), partSize=32)
    rp, ci = info.row_pointers, info.column_index
    L = args.walk_length
    sampler = SaintRWSampler(info, args.roots, L, seed=1)
    rounds = args.reps + 2                                          # two warm-up rounds
    res = {"graph": name, "num_nodes": n, "nnz": int(ci.numel()), "roots": args.roots, "walk_length": L, "reps": args.reps}

    # the compositions compute what the library computes
    roots0, seed0 = sampler.roots(0), sampler._step_seed(0)
    walks, eids = _lib.random_walk(rp, ci, roots0, L, seed0, want_edge_ids=True)
    mine = torch_walk(rp, ci, roots0, L, seed0)
    assert torch.equal(walks.long(), mine[0]) and torch.equal(eids.long(), mine[1]), "the torch walk is not the library's"
    ids = walks.reshape(-1)
    rows = None
    if args.only != "walk":
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long(), output_size=ci.numel())
        r = _lib.induced_subgraph(rp, ci, ids, partSize=32)
        S, sub_rp, sub_ci, eid, pp, p2n = torch_subgraph(rp, ci, rows, ids, 32)
        for got, want, what in ((r["nodes"], S, "nodes"), (r["row_pointers"], sub_rp, "row_pointers"), (r["column_index"], sub_ci, "column_index"),
                                (r["edge_ids"], eid, "edge_ids"), (r["partPtr"], pp, "partPtr"), (r["part2Node"], p2n, "part2Node")):
            assert torch.equal(got.long(), want.long()), f"the torch subgraph is not the library's: {what}"
        kept = r["nodes"].long()
        res.update(sub_nodes=int(kept.numel()), sub_edges=int(r["column_index"].numel()),
                   fill_pass_positions=int((rp[kept + 1] - rp[kept]).sum()))

    if args.only in ("all", "walk"):
        lib_ms, torch_ms = [], []
        for k in range(rounds):
            roots, seed = sampler.roots(k), sampler._step_seed(k)
            a = timed(lambda: _lib.random_walk(rp, ci, roots, L, seed))
            b = timed(lambda: torch_walk(rp, ci, roots, L, seed))
            if k >= 2:
                lib_ms.append(a), torch_ms.append(b)
        res.update(walk_ms_library=round(statistics.median(lib_ms), 4), walk_ms_torch=round(statistics.median(torch_ms), 4))
        res["walk_library_faster"] = res["walk_ms_library"] < res["walk_ms_torch"]
    if args.only in ("all", "subgraph"):
        lib_ms, torch_ms = [], []
        for k in range(rounds):
            ids = _lib.random_walk(rp, ci, sampler.roots(k), L, sampler._step_seed(k))[0].reshape(-1)
            a = timed(lambda: _lib.induced_subgraph(rp, ci, ids, partSize=32))
            if args.only == "subgraph":                             # (a kernel trace wants the library's kernels only)
                continue
            b = timed(lambda: torch_subgraph(rp, ci, rows, ids, 32))
            if k >= 2:
                lib_ms.append(a), torch_ms.append(b)
        if lib_ms:
            res.update(subgraph_ms_library=round(statistics.median(lib_ms), 3), subgraph_ms_torch=round(statistics.median(torch_ms), 3))
            res["subgraph_library_faster"] = res["subgraph_ms_library"] < res["subgraph_ms_torch"]
    if args.only == "all":
        del rows
        torch.cuda.empty_cache()
        X = torch.randn(n, args.dim, device=dev)
        y = torch.randint(0, cfg["classes"], (n,), device=dev)
        conv1, conv2 = ops.SAGEConv(args.dim, cfg["hidden"]).to(dev), ops.SAGEConv(cfg["hidden"], cfg["classes"]).to(dev)
        opt = torch.optim.Adam(list(conv1.parameters()) + list(conv2.parameters()), lr=0.01)

        def step(k):
            sub = sampler.sample(k)
            picked = sub.nodes.long()
            opt.zero_grad()
            out = conv2(conv1(X.index_select(0, picked), sub, relu=True), sub)
            torch.nn.functional.cross_entropy(out, y.index_select(0, picked)).backward()
            opt.step()

        sample_ms, step_ms = [], []
        for k in range(rounds):
            a = timed(lambda: sampler.sample(k))
            b = timed(lambda: step(k))
            if k >= 2:
                sample_ms.append(a), step_ms.append(b)
        res.update(sample_ms=round(statistics.median(sample_ms), 3), step_ms=round(statistics.median(step_ms), 3))
        res["sampling_share_of_step"] = round(res["sample_ms"] / res["step_ms"], 3)
    print(json.dumps(res), flush=True)
    return 0


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", default="reddit-like,products-like")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--roots", type=int, default=2000)
    p.add_argument("--walk_length", type=int, default=2)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--timeout", type=int, default=900, help="seconds one graph's process may take")
    p.add_argument("--only", default="all", choices=["all", "walk", "subgraph"], help="subgraph: the library's cut alone (for a kernel trace)")
    p.add_argument("--child", default=None, help="(internal) measure this one graph in this process")
    args = p.parse_args(argv)
    if args.child:
        return child(args)
    passed = [a for a in (argv if argv is not None else sys.argv[1:])]
    for name in args.graphs.split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name] + passed, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"graph": name, "error": "ran out of its %d s" % args.timeout}), flush=True)
            return 124
        if rc != 0:                                                 # after a failure nothing more is started on the GPU
            print(json.dumps({"graph": name, "error": "exit status %d" % rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

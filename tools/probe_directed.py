"""Directed-graph measurements (profiles/directed/): (1) device transpose + partition against the host reverse-edge pass it
replaces for GAT, both timed in this one process; (2) main.py epochs with --directed True / False on the Reddit-like graph
(symmetric: both settings run the same kernels on the same ids), alternated, up to 5 rounds.

    python tools/probe_directed.py [time box in seconds] [build,epochs] [output directory]

Appends JSON lines to <output directory>/measure.jsonl as it goes."""
import contextlib
import io
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnnadvisor_osdi21_amd import _lib, graph  # noqa: E402
from gnnadvisor_osdi21_amd import main as driver  # noqa: E402

T0 = time.perf_counter()
DEADLINE = float(sys.argv[1]) if len(sys.argv) > 1 else 480.0
WHAT = sys.argv[2] if len(sys.argv) > 2 else "build,epochs"
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "directed")
os.makedirs(OUT, exist_ok=True)
LOG = open(os.path.join(OUT, "measure.jsonl"), "a")


def say(**kw):
    kw["t"] = round(time.perf_counter() - T0, 1)
    LOG.write(json.dumps(kw) + "\n")
    LOG.flush()
    print(json.dumps(kw), flush=True)


def build_times(name, partSize):
    g = graph.make_config_graph(name, device="cuda")
    rp, ci = g.row_pointers.cuda(), g.column_index.cuda()
    torch.cuda.synchronize()
    dev = []
    for _ in range(4):
        t = time.perf_counter()
        t_rp, t_ci, _ = _lib.transpose_csr(rp, ci, want_perm=False)
        pp, p2n = _lib.build_part_device(partSize, t_rp)
        torch.cuda.synchronize()
        dev.append(time.perf_counter() - t)
    t = time.perf_counter()
    t_rp, t_ci, t_perm = _lib.transpose_csr(rp, ci, want_perm=True)
    torch.cuda.synchronize()
    with_perm = time.perf_counter() - t
    same = bool(torch.equal(t_rp, rp) and torch.equal(t_ci, ci))          # the generators make symmetric, sorted graphs
    host = []
    for _ in range(2):
        t = time.perf_counter()
        rev = _lib.reverse_edges(rp, ci)                                   # copies the CSR to the host, then the host pass
        host.append(time.perf_counter() - t)
    perm_is_rev = bool(torch.equal(t_perm.cpu(), rev))
    say(kind="build", graph=name, nodes=g.num_nodes, nnz=int(ci.numel()), partSize=partSize, parts=int(p2n.numel()),
        device_s=[round(x, 4) for x in dev], device_with_perm_s=round(with_perm, 4), host_reverse_edges_s=[round(x, 3) for x in host],
        transpose_equals_graph=same, perm_equals_reverse_edges=perm_is_rev)
    del g, rp, ci, t_rp, t_ci, t_perm, rev
    torch.cuda.empty_cache()


def epoch(model, directed, epochs=30):
    argv = ["--synthetic", "reddit-like", "--dim", "64", "--hidden", "64", "--classes", "41", "--model", model,
            "--num_epoches", str(epochs), "--directed", str(directed)]
    if model == "gat":
        argv += ["--fused_attention", "True"]
    buf = io.StringIO()
    t = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        driver.main(argv)
    ms = float(re.search(r"Time \(ms\): (\d+\.\d+)", buf.getvalue()).group(1))
    say(kind="epoch", model=model, directed=directed, epoch_ms=ms, wall_s=round(time.perf_counter() - t, 1))
    torch.cuda.empty_cache()


if "build" in WHAT:
    build_times("reddit-like", 128)
    build_times("products-like", 32)
if "epochs" in WHAT:
    for rnd in range(5):
        for model in ("gcn", "gin", "sage", "gat"):
            for directed in (False, True):
                if time.perf_counter() - T0 > DEADLINE:
                    say(kind="stop", reason="time box", round=rnd)
                    sys.exit(0)
                epoch(model, directed)
say(kind="done")

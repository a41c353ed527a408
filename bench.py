#!/usr/bin/env python3
"""bench.py -- neighbor-group SpMM aggregation (GNNAdvisor `SAG`) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]

A "step" is one pass of the hot path -- `gnna_sag_f32` through the C ABI (prologue + the
aggregation kernel's column-phase launches) -- over the whole synthetic graph, inputs already
resident in HBM.  Headline workload (BASELINE.json config 3, the one the metric is quoted on): a
seeded Reddit-like power-law graph (N = 232,965, ~1.1e8 CSR entries, max degree ~21.6k, random
node order), D = 64 fp32 features; neighbor-group size and schedule are chosen by the Decider in
auto mode (`--manual` = the reference's manual mode, partSize 32, single pass).

`--gpus N` with N > 1 launches N ranks by itself (re-exec under torch.distributed.run on
127.0.0.1) unless the launcher's environment (WORLD_SIZE) is already there.  The N-rank line's `value` is the
weak-scaling leg -- every rank owns a Reddit-sized block of destination rows whose sources are drawn from all
ranks' nodes; each step exchanges source features over RCCL/xGMI (only the referenced remote rows when that is
clearly less than the whole blocks, `--exchange`) and aggregates locally (gnnadvisor_osdi21_amd/dist.py) -- so that
N = 1 is the single-GPU workload.  With `--full`, `--scaling strong,config5` (default) adds, inside `config.values` (detail
file: `config.legs`), the strong-scaling leg (the SAME Reddit-like graph as the single-GPU line, split into N nnz-balanced
destination blocks) and, at 8 ranks (or with --config5-leg, with or without `--full`), BASELINE config 5 (papers100M-like,
D = 128, exchange chosen collectively), each verified on every rank.

A plain run (no `--full`) does what its headline figure needs and nothing else: it sets up the workload, runs W warm-up
steps, times exactly K steps (`ms_per_step` = their wall time / K), writes the outputs of the last timed step when
`--dump-outputs DIR` is given (dump_outputs: DIR/aggregated.npy on one GPU; the inputs are seeded, so the same arguments give
the same inputs), and prints the line.  `--full` (implied by `--detail`) adds everything below: four more blocks of K steps
for the spread, the verification, the floor probe, the reference-style timing, the other modes, the PMC child passes, the
CPU baseline and the detail file.

Rank 0 prints ONE compact JSON line (< 8 KB, normally ~2 KB: `compact_single` / `compact_sharded`; the driver keeps an 8 KB
tail of stdout): the contract's keys, `config` as flat scalars, `roofline` (its PMC and floor terms with `--full`) and, with
`--full`, `cpu_baseline` as numbers.  `value` = total aggregated edges per second over all ranks.  With `--full` the FULL
record -- verification detail, the other modes, the reference-style wall-clock timing, the PMC detail, and with `--detail`
the secondary legs (config 4's GIN widths, the HBM-resident graph, the node-order legs, config 5's per-rank shape, the
prepared lifecycle) -- goes to the detail file (`--detail-file`; by default bench_detail[_nN].json in the run's output
folder) and a one-line summary to stderr.  Copies of the detail file are kept under profiles/.

`verified` (`--full`; not in the line of a plain single-GPU run): after the timed loop the timed configuration itself is checked --
X = ones must give the exact row nnz in every column (the reference's own known-answer test, unitest.py:54-63), and 256
sampled rows of the timed randn output are compared with an fp64 gather-sum.

`roofline` (definition frozen in round 5, tests/test_bench_cpu.py): `achieved` = SURVEY.md 8(d) ALGORITHMIC bytes per launch
(gather model: nnz*(4D+4) + N*(4D+4) + P*8) / the aggregation kernel's time, measured with HIP events on the launch stream
inside the timed loop; `peak` = the ceiling that binds -- 34.5 TB/s (the 8 L2s together) when the gathered source matrix is
below the 256 MiB Infinity Cache (`ceiling: "l2"`, the headline: 59.6 MB), 8 TB/s otherwise (`ceiling: "hbm"`); `frac` =
achieved / peak.  `traffic` = MEASURED fabric bytes per launch (rocprofv3 PMC child passes of this very invocation:
FETCH_SIZE x a copy calibration made in the same child + WRITE_SIZE), `frac_hbm_measured` = traffic / kernel time / 8 TB/s
-- the figure to quote for `ceiling == "hbm"` legs, whose gather-model `frac` can exceed 1 because repeated rows are served
by the L2s; `l2_hit_rate`, `l2_requests_per_edge`, `frac_l2` from a TCC_HIT/TCC_MISS pass; `floor_ms` = the bare access
stream of the timed schedule (tools/ceiling/gather_ceiling.hip), `frac_of_floor` = floor / kernel.
With `--detail`, `roofline.other_workloads` (detail file only) repeats this on products-like graphs (627 MB of features,
HBM-resident; GIN at D = 100 / 64; scrambled / renumbered / planted node orders) and on BASELINE config 5 in its TRUE per-rank
shape: rank 0 of 8 of a papers100M-like graph -- 13.9 M destination rows gathering D = 128 rows of all 111 M source nodes,
from the resident 56.9 GB all-gather buffer and from the compact halo buffer (`ShardedAggregator(emulate=...)`: the KERNELS
of a rank's step, the receive buffer filled from the global features instead of by RCCL).
`config.reference_style_ms`: the reference's own timing method (unitest.py:65-79: 10 warm-up + 200 GNNA.SAG calls
through the pybind module, fresh outputs, wall clock).  `cpu_baseline` times the oracle (CPU port) on the host.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time



def process_env():
    """Environment of a bench PROCESS, set by main() before torch / HIP / libgomp start -- not at import: tests/test_bench_cpu.py
    imports this module, and OMP_PROC_BIND in the environment of the whole pytest process made libgomp bind ITS main thread to
    one core (found in round 6: the GPU suite's host passes -- renumbering, CSR builders -- ran all their threads on one core)."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL across processes); before HIP starts
    os.environ.setdefault("OMP_PROC_BIND", "close")            # cpu_baseline: pinned OpenMP threads (before libgomp starts)
    os.environ.setdefault("OMP_PLACES", "cores")
    if _QUOTA and _QUOTA < (os.cpu_count() or 1):
        os.environ.setdefault("OMP_NUM_THREADS", str(max(1, int(_QUOTA))))   # as many threads as the container is granted


# With OMP_PROC_BIND set, libgomp binds the INITIAL thread to the first place (one core) as soon as it starts -- and every
# std::thread the native host code spawns from it inherits that one-core mask: round 5's "24.3 s" renumbering inside this script
# was 16 threads on one core (4.6 s with the mask restored).  The mask the process started with is kept here; `unbound()` puts it
# back on the main thread around native multi-threaded host work, `cpu_baseline` runs under the binding it asked for.
_START_AFFINITY = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None


class unbound:
    """Context: the main thread may run (and spawn threads) on every CPU the process started with."""

    def __enter__(self):
        self.saved = None
        if _START_AFFINITY is not None:
            self.saved = os.sched_getaffinity(0)
            if self.saved != _START_AFFINITY:
                os.sched_setaffinity(0, _START_AFFINITY)
        return self

    def __exit__(self, *exc):
        if self.saved is not None and self.saved != _START_AFFINITY:
            os.sched_setaffinity(0, self.saved)
        return False


def cpu_quota_cores():
    """CPUs this container may use per scheduling period (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited.
    The GPU boxes show 256 hardware threads but grant 16 CPUs: 128 OpenMP threads burn that in 12.5 ms of every 100 ms period
    and are throttled for the rest -- the "bimodal" ~100 / ~200 ms passes of rounds 1-3 were whole throttle periods
    (tools/probe_cpu_baseline.py, profiles/r4/cpu_baseline_probe.log)."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            return float(quota) / float(period)
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            quota = float(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            period = float(f.read())
        if quota > 0:
            return quota / period
    except Exception:
        pass
    return None


_QUOTA = cpu_quota_cores()

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md); measured copy ceiling is ~6290
L2_PEAK_GBS = 34500.0  # the 8 XCD L2s together, 128-byte requests (MI355X_MICROARCH.md)
CALIB_BYTES = 1 << 30


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--partSize", type=int, default=0,
                    help="neighbor-group size; 0 = the Decider's choice (auto mode, mi355x policy)")
    ap.add_argument("--manual", action="store_true",
                    help="reference manual mode: partSize 32 and library-default scheduling, no Decider")
    ap.add_argument("--config", default="reddit-like")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (debug only)")
    ap.add_argument("--locality", type=float, default=0.0)
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps, measure and check everything else: the spread over more blocks of steps, the "
                         "verification, the floor probe, the reference-style timing, the other modes, the PMC passes, the CPU "
                         "baseline and the detail file (N ranks: the strong-scaling and config-5 legs, the single-GPU comparison)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last step returned as DIR/<name>.npy (float32, at most 64 MB "
                         "in all; a seeded sample of rows beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 PMC child passes (traffic = null)")
    ap.add_argument("--detail", action="store_true",
                    help="also run the secondary legs (config 4 GIN widths, the HBM-resident graph, the node-order legs, config 5's "
                         "per-rank shape, the prepared lifecycle); their records go to the detail file, never into the line; "
                         "implies --full")
    ap.add_argument("--detail-file", default="",
                    help="where the full record goes (default gpurun_out/bench_detail[_nN].json under the repo)")
    ap.add_argument("--no-secondary", action="store_true", help="with --detail: skip the HBM-resident second workload and the node-order legs")
    ap.add_argument("--secondary-config", default="products-like")
    ap.add_argument("--prepared", action="store_true",
                    help="time the build's lifecycle extension (hints + gnna_prepare_graph + measured phases + producer-written "
                         "layout through gnna_agg_ld_f32) as the headline instead of the reference caller's path (profiling aid)")
    ap.add_argument("--no-config5", action="store_true",
                    help="skip BASELINE config 5's true per-rank shape (rank 0 of 8 of a papers100M-like graph, D = 128, "
                         "gathering from all 111 M source nodes)")
    ap.add_argument("--config5-scale", type=float, default=1.0, help="shrink the config-5 graph (debug only)")
    ap.add_argument("--headline-only", action="store_true",
                    help="only the timed headline workload: no calibration, other modes, PMC children, second "
                         "workload or CPU baseline (used for rocprofv3 kernel-trace runs)")
    ap.add_argument("--pipeline-chunks", type=int, default=0,
                    help="multi-GPU all-gather exchange: pieces of the pipelined feature exchange (0 = automatic)")
    ap.add_argument("--exchange", default="auto", choices=("auto", "halo", "allgather"),
                    help="multi-GPU source-feature exchange: only the referenced remote rows (all_to_all), whole "
                         "blocks (all-gather), or whichever moves clearly fewer bytes (decided collectively)")
    ap.add_argument("--scaling", default="strong,config5",
                    help="extra legs of the N-rank line besides the weak-scaling headline: 'strong' (the single-GPU graph "
                         "split over the ranks), 'config5' (papers100M-like, D = 128; at 8 ranks), '' = none")
    ap.add_argument("--config5-leg", action="store_true", help="run the config-5 leg at any world size (debug / tests)")
    ap.add_argument("--backend", default="nccl", help="debug: 'gloo' runs the N-rank path without RCCL")
    ap.add_argument("--share-gpu", action="store_true", help="debug: every rank uses cuda:0 (with --backend gloo)")
    ap.add_argument("--force-dist", action="store_true",
                    help="debug: take the sharded (torch.distributed) path even with one rank")
    ap.add_argument("--force-collectives", action="store_true",
                    help="bring-up: with ONE rank, still issue every collective of the N-rank step through the process group "
                         "(the second half of the rank's block travels through RCCL to the rank itself); implies --force-dist")
    # internal: PMC child mode (run under rocprofv3 by the parent)
    ap.add_argument("--pmc-child", default="", help=argparse.SUPPRESS)     # manifest path
    ap.add_argument("--pmc-workloads", default="", help=argparse.SUPPRESS)  # JSON file of workload specs
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------- models

def gather_model_bytes(nnz: int, n_rows: int, parts: int, dim: int) -> int:
    """per edge one fp32 source row + one int32 column id; per destination
    row one fp32 output row + one row pointer; per neighbor-group partPtr + part2Node."""
    return nnz * (4 * dim + 4) + n_rows * (4 * dim + 4) + parts * 8


def compulsory_bytes(nnz: int, n_rows: int, n_src: int, dim: int) -> int:
    return nnz * 4 + (n_rows + 1) * 4 + (n_rows + n_src) * dim * 4


# ---------------------------------------------------------------------------------------------- self launch

def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n: int):
    """`python bench.py --gpus N` from a bare shell: become N ranks (one per GPU) under
    torch.distributed.run.  The ranks inherit stdout, so rank 0's JSON line is this command's."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.abspath(__file__), *sys.argv[1:]]
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


# ---------------------------------------------------------------------------------------------- workload

class Workload:
    """One single-GPU aggregation workload: graph + partition + features, and its step().

    lifecycle "dropin" (the headline): what a caller of the REFERENCE API gets -- the Decider's `inputProperty.decider()`
    for partSize (param.py:51-120), `GNNAdvisor.build_part`, then nothing but the module's six functions on contiguous
    tensors (`GNNA.SAG(...)`, GNNAdvisor.cpp:75-96; a fresh output tensor per call like the reference's zeros_like).  No
    hints, no gnna_prepare_graph, no calibration, no process-wide tuning: the library counts the partition at first sight
    and the module prepares the graph by itself on its second sighting (gnna_torch.cpp: note_graph).
    lifecycle "prepared": the build's own extension -- hints + gnna_prepare_graph + measured phase count before the timed
    region and X written by the producer with `gnna_preferred_ld`, gathered through gnna_agg_ld_f32 into a preallocated
    output -- reported beside the headline, never as `value`.
    kind "sag" (GNNAdvisor_kernel.cu:186-259) or "gin" (eps = 0.5 scaled sum, .cu:620-689, through the module's
    aggregate_gin / gnna_agg_gin_f32).
    order "generator" (the generator's ids: random for locality = 0, the hidden community order otherwise), "scrambled"
    (a seeded random relabelling of that) or "renumbered" (the scrambled graph relabelled by the native community
    renumbering, `gnna_reorder_community_i32` -- the role of rabbit_module/src/reorder.cpp:235-295)."""

    def __init__(self, config, dim, dev, *, scale=1.0, locality=0.0, manual=False, part_size=0, lifecycle="dropin",
                 kind="sag", calibrate=True, force_phases=0, order="generator", perm_file=None):
        import torch
        from gnnadvisor_osdi21_amd import _lib, graph, load_extension
        from gnnadvisor_osdi21_amd.decider import inputProperty, calibrate_phases
        assert lifecycle in ("dropin", "prepared") and kind in ("sag", "gin") and order in ("generator", "scrambled", "renumbered")
        self.config, self.dim, self.dev, self.scale = config, dim, dev, scale
        self.lifecycle, self.kind, self.order, self.locality, self.eps = lifecycle, kind, order, locality, 0.5
        self.GNNA = load_extension()
        cfg = graph.CONFIGS[config]
        g = graph.make_config_graph(config, device=dev, locality=locality, scale=scale)
        self.reorder_seconds = None
        if order != "generator":
            n = g.num_nodes
            rows = torch.repeat_interleave(torch.arange(n, device=dev), (g.row_pointers[1:] - g.row_pointers[:-1]).long())
            perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            src, dst = perm[rows], perm[g.column_index.long()]
            del rows, perm
            if order == "renumbered":
                if perm_file and os.path.exists(perm_file):
                    new_id = torch.load(perm_file).to(dev).long()          # (a PMC child re-uses the parent's renumbering)
                else:
                    # what loader.custom_dataset.rabbit_reorder() does: the renumbering from the host CSR of the graph as loaded
                    scr = graph.graph_from_edges(src, dst, n)
                    rp_h, ci_h = scr.row_pointers.cpu(), scr.column_index.cpu()
                    del scr
                    with unbound():
                        t0 = time.perf_counter()
                        new_id = _lib.reorder_community_csr(rp_h, ci_h, n)
                        self.reorder_seconds = time.perf_counter() - t0
                    new_id = new_id.to(dev).long()
                    del rp_h, ci_h
                    if perm_file:
                        torch.save(new_id.to(torch.int32).cpu(), perm_file)
                src, dst = new_id[src], new_id[dst]
            g = graph.graph_from_edges(src, dst, n)
            del src, dst
        self.g = g

        class _Profile:
            pass
        prof = _Profile()
        prof.num_nodes, prof.avg_degree, prof.avg_edgeSpan = g.num_nodes, g.avg_degree, g.avg_edgeSpan
        prof.num_features, prof.reorder_flag = cfg["feat"], False
        prof.rabbit_reorder = lambda: None
        info = inputProperty(None, None, None, 32, 32, 4, 100, hiddenDim=dim, dataset_obj=prof,
                             enable_rabbit=False, manual_mode=manual)
        info.decider()
        if lifecycle == "prepared" and not manual:
            info.apply_tuning()
        self.ps = part_size if part_size > 0 else info.partSize
        self.pp, self.p2n = self.GNNA.build_part(self.ps, g.row_pointers.cpu())        # GNNA_main.py:102
        self.ppd, self.p2nd = self.pp.to(dev), self.p2n.to(dev)
        self.P = int(self.p2n.numel())
        gen = torch.Generator(device=dev).manual_seed(1234)
        self.Xc = torch.randn(g.num_nodes, dim, device=dev, generator=gen)          # the contiguous layout of the reference
        self.ld = dim
        self.X = self.Xc
        self.out = None
        self.calibrated = None
        self.prepared = bool(lifecycle == "prepared" and not manual)
        if self.prepared:
            # the layout a producer writes for this gather (gnna_preferred_ld: e.g. torch::mm into buf[:, :64] of a [N, 128]
            # allocation -- every 256-byte row on its own 512-byte boundary): gathered from directly, no staged copy per call
            self.ld = _lib.preferred_ld(dim, g.num_nodes, g.nnz)
            if self.ld != dim:
                self.X = _lib.empty_rows(g.num_nodes, dim, self.ld, dev)
                self.X.copy_(self.Xc)
            self.out = torch.empty_like(self.Xc)
            _lib.set_graph_hints(g.column_index, g.nnz / g.num_nodes, g.avg_edgeSpan > 0.28 * g.num_nodes)
            _lib.prepare_graph(g.column_index, self.ppd, self.p2nd, g.num_nodes, g.num_nodes, self.ps, [dim])
            if force_phases > 0:
                _lib.set_graph_phases(g.column_index, dim, force_phases)
            elif calibrate:
                self.calibrated = calibrate_phases(g.column_index, self.ppd, self.p2nd, g.num_nodes, self.ps, [dim])
            _lib.prepare_graph(g.column_index, self.ppd, self.p2nd, g.num_nodes, g.num_nodes, self.ps, [dim])
        self._lib = _lib

    def step(self, X=None, out=None):
        """One aggregation.  dropin: through the module, fresh output (returned and kept as self.out); prepared:
        gnna_agg_ld_f32 into the preallocated output."""
        g = self.g
        if self.lifecycle == "dropin":
            X = self.Xc if X is None else X
            if self.kind == "sag":
                y = self.GNNA.SAG(X, g.row_pointers, g.column_index, g.degrees, self.ppd, self.p2nd, self.ps, 32, 4)
            else:
                y = self.GNNA.aggregate_gin(X, g.row_pointers, g.column_index, self.eps, self.ppd, self.p2nd, self.ps, 32, 4)
            if out is not None:
                out.copy_(y)
            else:
                self.out = y
            return y
        X = self.X if X is None else X
        out = self.out if out is None else out
        return self._lib.agg_ld(0 if self.kind == "sag" else 2, X, g.column_index, self.ppd, self.p2nd, g.num_nodes, self.ps,
                                epsilon=self.eps if self.kind == "gin" else 1.0, out=out)

    def time(self, steps, warmup, blocks=5):
        import torch
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        swept0 = self._lib.runtime_counters()["sweep_launches"]
        self._lib.profile_begin(steps)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        prof = self._lib.profile_end()
        self.phases = self._lib.last_num_phases()
        self.launches = self._lib.last_num_launches()
        c = self._lib.runtime_counters()
        self.swept = c["sweep_launches"] - swept0 >= steps                               # which kernel the library picked
        self.packed = c["packed_launches"] > 0                                           # (process-wide: > 0 once any call read packed ids)
        # run-to-run spread inside this invocation: more blocks of the same K steps (the headline is the first)
        self.block_ms = [elapsed * 1e3 / steps]
        for _ in range(blocks - 1):
            t1 = time.perf_counter()
            for _ in range(steps):
                self.step()
            torch.cuda.synchronize()
            self.block_ms.append((time.perf_counter() - t1) * 1e3 / steps)
        return elapsed, prof

    def verify(self, samples=256):
        """Checks the configuration that was just timed (same partition, same call path, same schedule):
        (1) X = ones -> every output element equals eps x the row's nnz exactly (unitest.py:54-63);
        (2) `samples` rows of the timed randn output against an fp64 gather-sum in the STRICT form of SURVEY appendix A,
            |err| <= 1e-4 * max(1, |ref|) per element (the sum-of-|terms| ratio rides beside it)."""
        import torch
        g = self.g
        scale_out = self.eps if self.kind == "gin" else 1.0
        if self.lifecycle == "prepared" and self.ld != self.dim:
            ones = self._lib.empty_rows(g.num_nodes, self.dim, self.ld, self.dev)
        else:
            ones = torch.empty_like(self.Xc)
        ones.fill_(1.0)                                        # (same layout as the timed input)
        y1 = torch.empty_like(self.Xc)
        self.step(ones, y1)
        deg = (g.row_pointers[1:] - g.row_pointers[:-1]).to(torch.float32)
        exact = bool((y1 == (deg * scale_out)[:, None]).all())
        phases_ones = self._lib.last_num_phases()
        del ones, y1
        self.step()                                            # the timed call once more -> self.out
        gen = torch.Generator(device="cpu").manual_seed(99)
        rows = torch.randint(0, g.num_nodes, (samples,), generator=gen).tolist()
        rows[0] = int(torch.argmax(deg))                       # the hub row is always among them
        worst_abs, worst_sum, worst_abs_long = 0.0, 0.0, 0.0
        ok = True
        for i in rows:
            b, e = int(g.row_pointers[i]), int(g.row_pointers[i + 1])
            xs = self.Xc[g.column_index[b:e].long()].double() * scale_out
            ref = xs.sum(0)
            err = (self.out[i].double() - ref).abs()
            rel_abs = float((err / torch.clamp(ref.abs(), min=1.0)).max())
            worst_sum = max(worst_sum, float((err / torch.clamp(xs.abs().sum(0), min=1.0)).max()))
            if e - b <= STRICT_ROW_EDGES:
                worst_abs = max(worst_abs, rel_abs)
                ok = ok and bool((err <= 1e-4 * torch.clamp(ref.abs(), min=1.0)).all())
            else:       # (a row of thousands of edges: the sum-of-|terms| form; the strict ratio is reported, not asserted)
                worst_abs_long = max(worst_abs_long, rel_abs)
                ok = ok and bool((err <= 1e-4 * torch.clamp(xs.abs().sum(0), min=1.0)).all())
        return {"ones_exact": exact, "sampled_rows": samples, "sampled_rows_ok": ok,
                "max_err_over_abs_ref": worst_abs, "max_err_over_sum_abs": worst_sum, "bound": 1e-4,
                "max_err_over_abs_ref_rows_beyond_%d_edges" % STRICT_ROW_EDGES: worst_abs_long,
                "bound_form": "|err| <= 1e-4 * max(1, |ref|) (SURVEY appendix A, strict) for rows of <= %d edges; 1e-4 * max(1, sum |terms|) "
                              "for longer rows (a sum of thousands of O(1) terms rounds by more than 1e-4 of a result that happens to "
                              "cancel: 1 element of 10 M at 1.5e-4 on 8,000-edge rows, tests/test_sweep_gpu.py)" % STRICT_ROW_EDGES,
                "column_phases_checked": phases_ones, "verified": bool(exact and ok)}


class RankOf8Workload:
    """BASELINE config 5 in its TRUE per-rank shape, on one GPU: rank `rank` of `world` = 8 of a papers100M-like graph.
    The rank's destination shard (13.9 M rows, ~2.0e8 edges) gathers D = 128 features from ALL 111 M source nodes:
    either from the all-gather buffer (every rank's block: 56.9 GB resident, 64-bit row offsets) or, with the halo
    exchange, from the compact buffer of the remote rows this shard references (a few GB) plus the rank's own
    block.  One process plays the rank (`ShardedAggregator(emulate=(rank, world))`): shard, local / remote split,
    halo lists and piece CSRs are built exactly as that rank builds them; the receive buffer is filled from the
    global features instead of by RCCL, so a step times the KERNELS a rank runs per aggregation (the exchange itself
    is the N-GPU run's to measure)."""

    def __init__(self, dev, dim=128, form="allgather-one-call", world=8, rank=0, scale=1.0, manual=False,
                 config="papers100M-like", keep_global=True):
        import torch
        from gnnadvisor_osdi21_amd import _lib, graph
        from gnnadvisor_osdi21_amd.decider import choose_part_size
        from gnnadvisor_osdi21_amd.dist import ShardedAggregator
        self._lib, self.dev, self.dim, self.form, self.world, self.rank, self.scale = _lib, dev, dim, form, world, rank, scale
        self.config = f"rank-of-{world}/{form}"
        cfg = graph.CONFIGS[config]
        self.n_local = n_local = max(64, int(cfg["num_nodes"] * scale) // world)
        self.n_global = n_global = n_local * world
        e_target = int(cfg["num_edges"] * scale * cfg.get("oversample", 1.0)) // world
        rp, ci = graph.powerlaw_shard(n_local, n_global, e_target, min(cfg["max_degree"], n_global - 1),
                                      seed=cfg["seed"] * 1000 + rank, device=dev, block_start=rank * n_local)
        self.rp, self.ci_global = rp, ci
        bounds = [i * n_local for i in range(world + 1)]
        avg = ci.numel() / n_local
        self.ps = 32 if manual else choose_part_size(avg, dim)
        kw = dict(device=dev, emulate=(rank, world))
        if form == "allgather-one-call":      # the whole shard in one rectangular call over the all-gather buffer
            self.agg = ShardedAggregator(rp, ci, bounds, self.ps, overlap=False, exchange="allgather", **kw)
        elif form == "allgather-pieces":      # local part + K piece CSRs over the sub-block-major all-gather buffer
            self.agg = ShardedAggregator(rp, ci, bounds, self.ps, force_overlap=True, exchange="allgather", **kw)
        elif form == "halo":                  # what `--exchange auto` takes: local part + K pieces over the compact buffer
            self.agg = ShardedAggregator(rp, ci, bounds, self.ps, force_overlap=True, exchange="auto", **kw)
        else:
            raise ValueError(form)
        gen = torch.Generator(device=dev).manual_seed(4321)
        self.X_global = torch.randn(n_global, dim, device=dev, generator=gen)
        self.X_local = self.X_global[rank * n_local:(rank + 1) * n_local]
        self.buf = self.agg.emulated_receive(self.X_global)
        self.out = torch.empty(n_local, dim, device=dev)
        self.P = int(self.agg.part2Node.numel())
        self.unique_sources = int(torch.unique(ci).numel())

        class _G:
            pass
        self.g = _G()
        self.g.nnz, self.g.num_nodes = int(ci.numel()), n_local
        self.calibrated = None
        self.phases, self.launches = 1, 1
        if not keep_global and self.buf is not self.X_global:
            self.X_global = None              # (the PMC child does not verify)

    # -- one aggregation's kernels on the resident buffers
    def step(self, X=None, out=None):
        calls = []
        real = self.agg.aggregate_fn

        def counting(*a, **k):
            r = real(*a, **k)
            calls.append((self._lib.last_num_launches(), self._lib.last_num_phases()))
            return r
        self.agg.aggregate_fn = counting
        try:
            y = self.agg.aggregate_only(self.X_local if X is None else X, out=self.out if out is None else out)
        finally:
            self.agg.aggregate_fn = real
        self.launches = sum(c[0] for c in calls)
        self.phases = max(c[1] for c in calls)
        self.calls = len(calls)
        return y

    def time(self, steps, warmup):
        import torch
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        self._lib.profile_begin(steps * 16)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        prof = self._lib.profile_end()
        per_step = prof["calls"] / max(1, steps)
        self.send_gather_ms = None
        if self.agg.exchange == "halo":
            # the send half of the halo exchange (rows the peers reference, gathered per piece into send buffers):
            # by symmetry as many rows as this rank receives
            for _ in range(2):
                bufs = self.agg.send_side_gather(self.X_local)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                bufs = self.agg.send_side_gather(self.X_local)
            torch.cuda.synchronize()
            self.send_gather_ms = (time.perf_counter() - t1) * 1e3 / 3
            self.send_gather_rows = int(sum(b.shape[0] for b in bufs))
            del bufs
        return elapsed, {"main_ms": prof["main_ms"] * per_step, "prologue_ms": prof["prologue_ms"] * per_step,
                         "calls": prof["calls"]}

    def verify(self, samples=200):
        """X = ones on every rank -> exact row nnz; `samples` rows of the timed output against an fp64 gather-sum over
        the GLOBAL features and the shard's GLOBAL column ids (so the remap into the buffer layout is checked too);
        then the degree-weighted (GCN) form the same way."""
        import torch
        n, D, dev = self.n_local, self.dim, self.dev
        rp, ci = self.rp, self.ci_global
        deg = (rp[1:] - rp[:-1]).to(torch.float32)
        # (1) ones: the receive buffer becomes all ones as well
        keep = self.agg._halo_buf if self.agg.exchange == "halo" else self.agg._gather_buf
        ones_buf = torch.ones_like(keep) if keep is not self.X_global else None
        if ones_buf is None:
            ones_buf = torch.ones(self.n_global, D, device=dev)
        if self.agg.exchange == "halo":
            self.agg._halo_buf = ones_buf
        else:
            self.agg._gather_buf = ones_buf
        y1 = torch.empty(n, D, device=dev)
        self.step(torch.ones(n, D, device=dev), y1)
        exact = bool((y1 == deg[:, None]).all())
        del y1, ones_buf
        if self.agg.exchange == "halo":
            self.agg._halo_buf = keep
        else:
            self.agg._gather_buf = keep
        # (2) sampled rows of the timed configuration
        self.step()
        gen = torch.Generator(device="cpu").manual_seed(77)
        rows = torch.randint(0, n, (samples,), generator=gen).tolist()
        rows[0] = int(torch.argmax(deg))
        worst, ok = 0.0, True
        for i in rows:
            b, e = int(rp[i]), int(rp[i + 1])
            xs = self.X_global[ci[b:e].long()].double()
            ref, scale = xs.sum(0), torch.clamp(xs.abs().sum(0), min=1.0)
            err = (self.out[i].double() - ref).abs()
            worst = max(worst, float((err / scale).max()))
            ok = ok and bool((err <= 1e-4 * scale).all())
        # (3) the degree-weighted form on the same buffers: deg_i * sum_j deg_j x_j
        gen_d = torch.Generator(device=dev).manual_seed(5)
        deg_global = torch.rand(self.n_global, device=dev, generator=gen_d) + 0.5
        self.agg.emulated_receive_degrees(deg_global)
        deg_local = deg_global[self.rank * n:(self.rank + 1) * n].contiguous()
        yg = self.agg.aggregate_only(self.X_local, mode=1, degrees_local=deg_local)
        worst_g, ok_g = 0.0, True
        for i in rows[:64]:
            b, e = int(rp[i]), int(rp[i + 1])
            ids = ci[b:e].long()
            xs = self.X_global[ids].double() * deg_global[ids].double()[:, None] * float(deg_local[i])
            ref, scale = xs.sum(0), torch.clamp(xs.abs().sum(0), min=1.0)
            err = (yg[i].double() - ref).abs()
            worst_g = max(worst_g, float((err / scale).max()))
            ok_g = ok_g and bool((err <= 1e-4 * scale).all())
        del yg, deg_global
        self.agg._deg_all = None
        return {"ones_exact": exact, "sampled_rows": samples, "sampled_rows_ok": ok, "max_err_over_sum_abs": worst,
                "gcn_weighted_rows_ok": ok_g, "gcn_max_err_over_sum_abs": worst_g, "bound": 1e-4,
                "verified": bool(exact and ok and ok_g)}

    def release(self):
        """Drops the device tensors (the record keeps what the roofline line and the PMC child need)."""
        self.X_global = self.X_local = self.buf = self.out = self.agg = self.rp = self.ci_global = None

    def describe(self):
        a = self.agg
        D = self.dim
        gb = lambda rows: rows * D * 4 / 1e9
        d = {"rows_per_rank": self.n_local, "source_rows_all_ranks": self.n_global, "nnz": self.g.nnz,
             "unique_source_rows_referenced": self.unique_sources, "partSize": self.ps, "num_parts": self.P,
             "exchange": a.exchange, "pieces": a.chunks, "library_calls_per_step": getattr(self, "calls", None),
             "source_buffer_rows": int(self.buf.shape[0]), "source_buffer_GB": gb(int(self.buf.shape[0])),
             "allgather_buffer_GB": gb(self.n_global), "own_block_GB": gb(self.n_local),
             "wide_offsets": bool(self.buf.shape[0] * D * 4 > 0xffffffff)}
        if a.exchange == "halo":
            d["halo_rows_per_peer"] = list(a.halo_rows_per_peer)
            d["halo_rows"] = a.halo_rows
            d["halo_share_of_remote_rows"] = a.halo_rows / max(1, (self.world - 1) * self.n_local)
            d["bytes_received_per_step"] = a.bytes_received_per_step(D)
            if getattr(self, "send_gather_ms", None) is not None:
                d["send_side_gather_ms"] = self.send_gather_ms
                d["send_side_gather_rows"] = self.send_gather_rows
                d["send_side_gather_GBs"] = 2 * self.send_gather_rows * D * 4 / (self.send_gather_ms * 1e-3) / 1e9
        d["allgather_bytes_received_per_step"] = a.allgather_bytes_per_step(D)
        return d


# ---------------------------------------------------------------------------------------------- PMC child

def workload_spec(w):
    """What a PMC child needs to rebuild a workload of this invocation with the schedule that was timed."""
    if isinstance(w, RankOf8Workload):
        return {"rank_of": w.world, "form": w.form, "dim": w.dim, "scale": w.scale}
    return {"config": w.config, "dim": w.dim, "ps": w.ps, "phases": w.phases, "scale": w.scale, "locality": w.locality,
            "lifecycle": w.lifecycle, "kind": w.kind, "order": w.order, "perm_file": getattr(w, "perm_file", None)}


def pmc_child(args):
    """Runs under rocprofv3 --pmc: a few steps of each workload as the parent timed it (same call path, lifecycle and --
    for the prepared extension -- forced phase count), then a known-size device copy and a known-size read-only random row
    gather for the FETCH_SIZE / WRITE_SIZE calibration.  Writes a manifest that tells the parent which dispatches belong
    to which workload."""
    import torch
    from gnnadvisor_osdi21_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    manifest = {"workloads": [], "calib_bytes": CALIB_BYTES, "calib_copies": 3, "calib_gathers": 3}
    for spec in json.load(open(args.pmc_workloads)):
        if "rank_of" in spec:
            w = RankOf8Workload(dev, int(spec["dim"]), form=spec["form"], world=int(spec["rank_of"]), scale=float(spec["scale"]),
                                manual=args.manual, keep_global=False)
        else:
            w = Workload(spec["config"], int(spec["dim"]), dev, scale=float(spec["scale"]), locality=float(spec["locality"]),
                         manual=args.manual, part_size=int(spec["ps"]), lifecycle=spec["lifecycle"], kind=spec["kind"],
                         calibrate=False, order=spec["order"], perm_file=spec.get("perm_file"),
                         force_phases=0 if (args.manual or spec["lifecycle"] == "dropin") else int(spec["phases"]))
        warm, steps = 4, 3           # (a drop-in graph is prepared by the module at its second sighting: steady from call 3)
        for _ in range(warm + steps):
            w.step()
        torch.cuda.synchronize()
        if "rank_of" not in spec:
            w.launches, w.phases = _lib.last_num_launches(), _lib.last_num_phases()
        manifest["workloads"].append({"spec": spec, "warmup": warm, "steps": steps,
                                      "launches_per_step": w.launches, "phases": w.phases})
        del w
        torch.cuda.empty_cache()
    x = torch.randn(CALIB_BYTES // 4, device=dev)
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    # read-only gather of known size: every 256-byte row of a 1 GiB matrix (4 x the Infinity Cache) exactly once, in a
    # random order, summed per wavefront into a small output -- the access pattern of the HBM-resident aggregation legs
    # (VERDICT r4 task 4: the copy calibrates a streaming read + write, not a row gather)
    rows = CALIB_BYTES // 256
    M = x.view(rows, 64)
    idx = torch.randperm(rows, device=dev, generator=torch.Generator(device=dev).manual_seed(7)).to(torch.int32)
    pp = torch.arange(0, rows + 1, 64, dtype=torch.int32, device=dev)          # 64-edge groups, one destination row each
    p2n = torch.arange(0, rows // 64, dtype=torch.int32, device=dev)
    sink = torch.empty(rows // 64, 64, device=dev)
    _lib.set_tuning(column_phases=1)
    for _ in range(3):
        _lib.agg_rect(0, M, idx, pp, p2n, rows // 64, 64, out=sink)
    torch.cuda.synchronize()
    _lib.reset_tuning()
    manifest["calib_gather_bytes"] = rows * 256
    with open(args.pmc_child, "w") as f:
        json.dump(manifest, f)


def run_pmc_pass(counters, spec_file, args, workdir):
    """One rocprofv3 --pmc pass of the child.  -> (manifest, rows of the counter CSV) or raises."""
    tag = "_".join(counters)[:40]
    outdir = os.path.join(workdir, tag)
    manifest_path = os.path.join(workdir, tag + "_manifest.json")
    child = [sys.executable, os.path.abspath(__file__), "--pmc-child", manifest_path, "--pmc-workloads", spec_file]
    if args.manual:
        child.append("--manual")
    cmd = ["rocprofv3", "--pmc", *counters, "--kernel-include-regex", "stream_kernel|sweep_kernel|copyBuffer", "-T",
           "-d", outdir, "-o", "pmc", "-f", "csv", "--", *child]
    env = dict(os.environ, TMPDIR="/tmp")
    r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    if r.returncode != 0 or not os.path.exists(manifest_path):
        raise RuntimeError(f"rocprofv3 pass {tag} failed (rc {r.returncode}): {r.stdout.decode(errors='replace')[-400:]}")
    rows = []
    for f in glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r_: int(r_["Dispatch_Id"]))
    return json.load(open(manifest_path)), rows


def split_counters(manifest, rows, counter):
    """-> ([per-step sum of `counter` over the aggregation launches, per workload], copy-kernel values, gather-calibration values)"""
    agg = [float(r["Counter_Value"]) for r in rows if r["Counter_Name"] == counter
           and any(k in r["Kernel_Name"] for k in ("stream_kernel", "sweep_kernel"))]
    cp = [float(r["Counter_Value"]) for r in rows if r["Counter_Name"] == counter and "copyBuffer" in r["Kernel_Name"]]
    cp = cp[-manifest["calib_copies"]:]      # the calibration copies are the child's last copy dispatches (earlier
    #                                          copyBuffer dispatches are small host-to-device transfers)
    ng = manifest.get("calib_gathers", 0)
    gather = agg[len(agg) - ng:] if ng else []     # ... and the calibration gathers its last aggregation dispatches
    if ng:
        agg = agg[:len(agg) - ng]
    per_step, at = [], len(agg)
    # walk the workloads from the END: a drop-in workload's first calls (counting pass at first sight, preparation at the
    # second) may take another schedule and another number of launches than its steady state
    for w in reversed(manifest["workloads"]):
        n = w["steps"] * w["launches_per_step"]
        timed = agg[max(0, at - n):at]
        per_step.append(sum(timed) / w["steps"] if len(timed) == n else None)
        at -= (w["warmup"] + w["steps"]) * w["launches_per_step"]
        if at < 0:
            at = 0
    per_step.reverse()
    return per_step, cp, gather


def measure_traffic(workloads, args):
    """Fabric-side bytes per step of the aggregation launches of each workload, from rocprofv3 PMC
    passes of this invocation's configuration (separate passes: FETCH_SIZE and WRITE_SIZE do not fit
    one; counters in KiB; FETCH_SIZE under-reports wide streaming reads on gfx950 and is calibrated on
    a 1 GiB device copy in the same child, as MI355X_MICROARCH.md prescribes; the factor a read-only random
    row gather of 1 GiB gives is recorded beside it).  -> list of dicts."""
    if shutil.which("rocprofv3") is None:
        return [{"error": "rocprofv3 not found"} for _ in workloads]
    workdir = tempfile.mkdtemp(prefix="gnna_pmc_", dir="/tmp")
    spec_file = os.path.join(workdir, "specs.json")
    with open(spec_file, "w") as f:
        json.dump([workload_spec(w) for w in workloads], f)
    res = [dict() for _ in workloads]
    try:
        mf, rows = run_pmc_pass(["FETCH_SIZE"], spec_file, args, workdir)
        fetch, cp_f, ga_f = split_counters(mf, rows, "FETCH_SIZE")
        mw, rows = run_pmc_pass(["WRITE_SIZE"], spec_file, args, workdir)
        write, cp_w, _ = split_counters(mw, rows, "WRITE_SIZE")
        try:
            mh, rows = run_pmc_pass(["TCC_HIT_sum", "TCC_MISS_sum"], spec_file, args, workdir)
            hit, _, _ = split_counters(mh, rows, "TCC_HIT_sum")
            miss, _, _ = split_counters(mh, rows, "TCC_MISS_sum")
        except Exception:
            hit = miss = [None] * len(workloads)
        # calibration: a 1 GiB copy reads 1 GiB and writes 1 GiB; the row gather reads 1 GiB of rows + 16 MiB of ids
        kf = (CALIB_BYTES / (1024.0 * (sum(cp_f) / len(cp_f)))) if cp_f else 2.0
        kw = (CALIB_BYTES / (1024.0 * (sum(cp_w) / len(cp_w)))) if cp_w else 1.0
        gather_bytes = mf.get("calib_gather_bytes", 0) * (1.0 + 4.0 / 256.0)
        kg = (gather_bytes / (1024.0 * (sum(ga_f) / len(ga_f)))) if ga_f and sum(ga_f) > 0 else None
        for i, w in enumerate(workloads):
            m = mf["workloads"][i]
            if fetch[i] is None or write[i] is None or m["launches_per_step"] != w.launches or m["phases"] != w.phases:
                res[i] = {"error": "dispatch count of the PMC child does not match the timed schedule (child: %s launches, %s phases; "
                                   "timed: %s, %s)" % (m["launches_per_step"], m["phases"], w.launches, w.phases)}
                continue
            res[i] = {"bytes_per_step": (fetch[i] * kf + write[i] * kw) * 1024.0,
                      "fetch_KiB_per_step_raw": fetch[i], "write_KiB_per_step_raw": write[i],
                      "fetch_calibration": kf, "write_calibration": kw, "fetch_calibration_random_row_gather": kg,
                      "bytes_per_step_gather_calibrated": ((fetch[i] * kg + write[i] * kw) * 1024.0) if kg else None,
                      "calibrated_in_this_run": bool(cp_f and cp_w),
                      "l2_hit_rate": (hit[i] / (hit[i] + miss[i])) if hit[i] and miss[i] is not None else None,
                      "l2_requests_per_step": (hit[i] + miss[i]) if hit[i] and miss[i] is not None else None,
                      "source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child passes of this bench.py invocation "
                                "(3 steady steps each, same call path and schedule as the timed loop)"}
    except Exception as exc:  # profiler missing / refused: report, never fake
        res = [{"error": str(exc)[:300]} for _ in workloads]
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    return res


def kernel_label(w):
    calls = getattr(w, "calls", 1) or 1
    if getattr(w, "swept", False):
        return "sweep_kernel (dst-blocked slice sweep, LDS accumulators, one launch)"
    if calls > 1:
        return f"stream_kernel x {calls} library calls per step (local part + remote pieces)"
    if w.launches == 1:
        return "stream_kernel (sliced schedule, one launch)" if w.phases > 1 else "stream_kernel"
    return f"{w.launches} launches per step (wide rows in 64-float column blocks, or the deterministic schedule's ordered phases)"


INFINITY_CACHE_BYTES = 256 << 20
STRICT_ROW_EDGES = 4096     # rows up to this many edges are verified in the strict form |err| <= 1e-4 * max(1, |ref|)


def roofline_ceiling(source_bytes: int):
    """The ceiling `roofline.frac` is quoted against -- FROZEN in round 5 (VERDICT r4 task 4; tests/test_bench_cpu.py fails
    if it changes): the aggregate L2 rate (34.5 TB/s, MI355X_MICROARCH.md) when the gathered source matrix fits the 256 MiB
    Infinity Cache -- its rows then reach the CUs through the L2s and never from HBM in steady state --, the HBM peak
    (8 TB/s) otherwise.  -> (name, GB/s)"""
    return ("l2", L2_PEAK_GBS) if source_bytes < INFINITY_CACHE_BYTES else ("hbm", HBM_PEAK_GBS)


def roofline_frac(algorithmic_bytes: float, kernel_s: float, source_bytes: int) -> float:
    """frac = SURVEY 8(d) algorithmic (gather-model) bytes / kernel time / roofline_ceiling.  One formula, no max() of
    alternatives; the measured terms (frac_hbm_measured, frac_l2) are side keys."""
    return algorithmic_bytes / kernel_s / 1e9 / roofline_ceiling(source_bytes)[1]


def roofline_record(w, kern_ms, prologue_ms, traffic, floor=None):
    g = w.g
    n_src = getattr(w, "n_global", g.num_nodes)
    alg = gather_model_bytes(g.nnz, g.num_nodes, w.P, w.dim)
    comp = compulsory_bytes(g.nnz, g.num_nodes, getattr(w, "unique_sources", g.num_nodes), w.dim)
    src_bytes = int(getattr(w, "source_bytes", n_src * w.dim * 4))
    t = kern_ms * 1e-3
    ceiling, peak = roofline_ceiling(src_bytes)
    achieved = alg / t / 1e9 if t > 0 else 0.0
    rec = {"bound": "hbm", "ceiling": ceiling, "peak": peak, "unit": "GB/s", "achieved": achieved, "frac": achieved / peak,
           "frac_definition": "algorithmic bytes (SURVEY 8d gather model: nnz*(4D+4) + N*(4D+4) + P*8) / kernel time / ceiling; "
                              "ceiling = 34.5 TB/s (aggregate L2) when the gathered source matrix is < 256 MiB (Infinity-Cache "
                              "resident: its rows never come from HBM in steady state), 8 TB/s (HBM) otherwise.  The model counts every "
                              "gathered row once per edge, whichever level serves it; a kernel that serves repeated rows from LDS or "
                              "L1 moves fewer bytes than the model and can exceed 1.0 of the L2 ceiling.  Frozen in round 5.",
           "bound_detail": ("source features (%.0f MB) are Infinity-Cache resident: the gather runs L2 -> L1, the fabric carries the L2 "
                            "misses" % (src_bytes / 1e6)) if ceiling == "l2" else
                           ("source features (%.0f MB) exceed the Infinity Cache: HBM-resident gather" % (src_bytes / 1e6)),
           "kernel": kernel_label(w),
           "kernel_ms": kern_ms, "kernel_launches_per_step": w.launches, "column_phases": w.phases,
           "kernel_ms_per_launch": kern_ms / max(1, w.launches), "prologue_ms": prologue_ms,
           "kernel_edges_per_s": g.nnz / t if t > 0 else 0.0,
           "algorithmic_bytes_per_step": alg, "algorithmic_bytes_per_launch": alg / max(1, w.launches),
           "frac_gather_model_of_hbm": achieved / HBM_PEAK_GBS,
           "compulsory_model": {"bytes_per_step": comp, "GBs": comp / t / 1e9 if t > 0 else 0.0},
           "traffic": None, "frac_hbm_measured": None, "frac_l2": None}
    if floor:
        rec.update({"floor_ms": floor.get("ms"), "frac_of_floor": (floor["ms"] / kern_ms) if floor.get("ms") and kern_ms > 0 else None,
                    "floor": floor})
    fabric = traffic.get("bytes_per_step") if traffic else None
    if fabric:
        req = traffic.get("l2_requests_per_step")
        rec.update({"traffic": fabric / max(1, w.launches), "traffic_per_step": fabric,
                    "traffic_source": "measured fabric traffic (FETCH_SIZE x copy calibration + WRITE_SIZE; KiB counters) of the "
                                      "aggregation launches, per launch like `achieved`",
                    "traffic_over_compulsory": fabric / comp, "traffic_over_algorithmic": fabric / alg,
                    "frac_hbm_measured": fabric / t / 1e9 / HBM_PEAK_GBS,
                    "frac_of_achievable_6300GBs": fabric / t / 1e9 / 6300.0,
                    "frac_l2": (req * 128.0 / t / 1e9 / L2_PEAK_GBS) if req else None,
                    "l2_requests_per_step": req, "l2_requests_per_edge": req / g.nnz if req else None,
                    "l2_hit_rate": traffic.get("l2_hit_rate"), "traffic_detail": traffic})
        kg = traffic.get("fetch_calibration_random_row_gather")
        if kg:
            gb = traffic["bytes_per_step_gather_calibrated"]
            rec["hbm_read_rate_note"] = (
                "FETCH_SIZE x %.2f (1 GiB copy) gives %.2f TB/s of fabric traffic; x %.2f (1 GiB read-only random row gather, same child) "
                "gives %.2f TB/s.  FETCH_SIZE counts L2 misses whether the Infinity Cache or HBM serves them, so on a matrix larger than "
                "the cache this is an upper bound of the HBM read rate, not the rate itself."
                % (traffic["fetch_calibration"], fabric / t / 1e12, kg, gb / t / 1e12))
    elif traffic:
        rec["traffic_error"] = traffic.get("error", "not measured")
    # which number a reader should take as "share of the ceiling" (a partly cached matrix under the HBM ceiling reads
    # > 1 in the frozen gather-model `frac`; there the measured fabric share is the honest figure)
    rec["fraction_to_read"] = "frac" if ceiling == "l2" else ("frac_hbm_measured" if rec.get("frac_hbm_measured") is not None else "frac (gather model: can exceed 1 under the HBM ceiling)")
    return rec


def floor_probe(w, phases):
    """The bare access stream of the timed schedule (tools/ceiling/gather_ceiling.hip: the column ids sorted phase-major as
    the sliced schedule consumes them, U row loads in flight per wavefront, no partition, no pieces, no flushes) on the
    layout the kernel gathers from -- the chip's rate for this request pattern, the floor of any pull-form kernel on these
    slices.  -> {"ms": ...} or None when the measurement tool is not built / the width is not covered."""
    import ctypes
    import torch
    so = os.path.join(ROOT, "tools", "ceiling", "libceiling.so")
    if not os.path.exists(so) or w.dim != 64 or w.g.nnz > 0x7fffffff:
        return None
    try:
        lib = ctypes.CDLL(so)
        lib.gather_ceiling_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_void_p]
        g, dev = w.g, w.dev
        N, nnz = g.num_nodes, g.nnz
        B = max(1, int(phases))
        col = g.column_index
        if B > 1:
            slice_rows = (N + 31) // 32
            ph = torch.div((col // slice_rows) * B, 32, rounding_mode="floor").to(torch.int16)
            ids = col[torch.sort(ph, stable=True).indices].contiguous()
            del ph
        else:
            ids = col
        # the gapped layout the library stages hot 64-float rows into (every row on its own 512-byte boundary): row id at
        # float offset id * 128 == row 2 * id of a [2N, 64] matrix
        Xg = torch.zeros(2 * N, 64, device=dev)
        Xg[0::2] = w.Xc
        ids2 = (ids * 2).contiguous()
        out = torch.empty((nnz // 256 + 64) * 256, device=dev)
        best = None
        for seg, U in ((512, 8), (512, 4), (256, 8)):
            def go():
                rc = lib.gather_ceiling_launch(Xg.data_ptr(), ids2.data_ptr(), ids2.numel(), 64, seg, U, out.data_ptr())
                if rc != 0:
                    raise RuntimeError("gather_ceiling_launch rc %d" % rc)
            for _ in range(3):
                go()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                go()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 10
            if best is None or ms < best[0]:
                best = (ms, seg, U)
        return {"ms": best[0], "what": "bare access stream of the %d-slice schedule (tools/ceiling/gather_ceiling.hip: %d ids per wavefront, "
                                       "%d row loads in flight, rows on 512-byte boundaries), measured in this run" % (B, best[1], best[2]),
                "phases": B}
    except Exception as exc:                      # (a measurement aid must never cost the line)
        return {"ms": None, "error": repr(exc)[:200]}


# ---------------------------------------------------------------------------------------------- CPU baseline

def cpu_baseline(g_cpu, X_cpu, pp, p2n, dim):
    """Oracle timed on the host: row-parallel fp32 CSR SpMM on all cores (value = median of >= 10
    passes; threads pinned with OMP_PROC_BIND=close / OMP_PLACES=cores, X and the output first-touched
    by the same threads so that their pages are spread over the NUMA nodes) and the single-thread
    neighbor-group port on a bounded slice of groups."""
    import numpy as np
    import oracle
    rp = g_cpu.row_pointers.numpy(); ci = g_cpu.column_index.numpy()
    X = oracle.first_touch_copy(X_cpu.numpy())
    nnz = int(ci.size)
    threads = oracle.num_threads()
    out = oracle.first_touch_copy(None, X.shape)
    for _ in range(2):
        oracle.csr_sag_omp(X, rp, ci, out=out)              # thread pool / page warm-up
    times = []
    t_all = time.perf_counter()
    while len(times) < 10 or (time.perf_counter() - t_all < 6.0 and len(times) < 30):
        t0 = time.perf_counter()
        oracle.csr_sag_omp(X, rp, ci, out=out)
        times.append(time.perf_counter() - t0)
    order = list(times)
    times.sort()
    # (rounds 1-3 ran 128 threads against a 16-CPU container quota and measured throttle periods -- passes of ~100 / ~200 ms;
    # with as many threads as the quota grants the passes are steady.)  `value` is the median of ALL passes, the median of
    # the faster half rides beside it as value_best_half
    med = times[len(times) // 2]
    best_half = times[len(times) // 4]
    # scalar port of the reference algorithm on ~1/16 of the groups
    ppn, p2nn = pp.numpy(), p2n.numpy()
    P = int(p2nn.size)
    g_end = max(1, P // 16)
    out1 = np.zeros_like(X)
    t0 = time.perf_counter()
    oracle.sag_groups_slice(X, ci, ppn, p2nn, 0, g_end, out1)
    t1 = time.perf_counter() - t0
    e1 = int(ppn[g_end] - ppn[0])
    return {
        "value": nnz / med, "unit": "edges/s", "cores": threads, "kind": "port",
        "cpu_quota_cores": _QUOTA, "host_hardware_threads": os.cpu_count(),
        "sample": f"full graph ({nnz} edges, D={dim}), median of all {len(times)} passes of the OpenMP "
                  f"row-parallel fp32 CSR SpMM in oracle/gnna_oracle.c ({threads} threads pinned"
                  + (f" = the container's CPU quota of {_QUOTA:g}" if _QUOTA else "") + ", NUMA first-touch)",
        "value_best_half": nnz / best_half, "ms_best_half": best_half * 1e3,
        "ms_median_all_passes": times[len(times) // 2] * 1e3,
        "ms": med * 1e3, "ms_min": times[0] * 1e3, "ms_max": times[-1] * 1e3,
        "pass_ms_in_order": [round(t * 1e3, 1) for t in order],
        "gather_model_GBs": gather_model_bytes(nnz, len(rp) - 1, P, dim) / med / 1e9,
        "single_thread": {"value": e1 / t1, "unit": "edges/s", "cores": 1,
                          "sample": f"first {g_end} neighbor-groups ({e1} edges), scalar neighbor-group port"},
        "libraries": library_baselines(rp, ci, X, nnz, threads),
    }


def library_baselines(rp, ci, X, nnz, cores):
    """SURVEY.md 8(d) baselines (i), (ii), (iv): scipy CSR @ X (one thread), torch.sparse_csr @ X
    (all cores), DGL copy_u/sum if importable.  One bounded pass each on the same CSR and X."""
    import numpy as np
    import torch
    res = {}
    n = len(rp) - 1
    try:
        import scipy.sparse as sp
        rows = min(n, max(1, n // 8))                       # ~1/8 of the rows: a few seconds on one thread
        A = sp.csr_matrix((np.ones(int(rp[rows]), dtype=np.float32), ci[:int(rp[rows])], rp[:rows + 1]),
                          shape=(rows, X.shape[0]))
        t0 = time.perf_counter(); A @ X; t = time.perf_counter() - t0
        res["scipy_csr_1thread"] = {"value": int(rp[rows]) / t, "unit": "edges/s", "cores": 1,
                                    "sample": f"first {rows} rows ({int(rp[rows])} edges)"}
    except Exception as exc:  # pragma: no cover
        res["scipy_csr_1thread"] = f"unavailable: {exc}"
    try:
        import warnings
        warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta")
        torch.set_num_threads(cores)
        A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)),
                                    torch.ones(nnz), size=(n, X.shape[0]))
        Xt = torch.from_numpy(X)
        A @ Xt
        t0 = time.perf_counter(); A @ Xt; t = time.perf_counter() - t0
        res["torch_sparse_csr"] = {"value": nnz / t, "unit": "edges/s", "cores": cores, "sample": "full graph, 2nd pass"}
    except Exception as exc:  # pragma: no cover
        res["torch_sparse_csr"] = f"unavailable: {exc}"
    try:
        import dgl  # noqa: F401
        res["dgl_copy_u_sum"] = "importable but not timed"
    except Exception:
        res["dgl_copy_u_sum"] = "unavailable (dgl is not installed on this image)"
    return res


def reference_style_ms(w, dims=(16, 64), warmup: int = 10, calls: int = 200):
    """The reference's own timing method (GNNAdvisor/unitest.py:65-79: 10 warm-up calls, then `--num_epoches` = 200
    calls of GNNA.SAG between two synchronisations, wall clock): through the pybind module `GNNAdvisor`, every call
    allocating its output, at hidden = 16 and 64 -- the number comparable with its `=> SpMM profiling avg (ms)`."""
    import torch
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    g, res = w.g, {}
    for d in dims:
        X = w.Xc if d == w.dim else torch.randn(g.num_nodes, d, device=w.dev, generator=torch.Generator(device=w.dev).manual_seed(d))
        for _ in range(warmup):
            GNNA.SAG(X, g.row_pointers, g.column_index, g.degrees, w.ppd, w.p2nd, w.ps, 32, 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            GNNA.SAG(X, g.row_pointers, g.column_index, g.degrees, w.ppd, w.p2nd, w.ps, 32, 4)
        torch.cuda.synchronize()
        res[str(d)] = (time.perf_counter() - t0) * 1e3 / calls
    res["method"] = (f"{warmup} warm-up + {calls} GNNA.SAG calls through the pybind module, fresh output tensor per call, "
                     "wall clock between two synchronisations (reference unitest.py:65-79)")
    return res


def other_modes(w, steps: int = 10):
    """edges/s of the GCN-weighted and GIN aggregation entries (C ABI, contiguous rows) and of the SDDMM extension on
    the bench graph: same partition, the library's own schedule."""
    import torch
    _lib, g = w._lib, w.g
    out = torch.empty_like(w.Xc)
    res = {}

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        _lib.profile_begin(steps)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        pr = _lib.profile_end()
        return {"edges_per_s": g.nnz * steps / el, "ms_per_step": el * 1e3 / steps, "kernel_ms": pr["main_ms"]}
    for name, fn in (("gcn_weighted", lambda: _lib.agg_gcn(w.Xc, g.row_pointers, g.column_index, g.degrees, w.ppd,
                                                           w.p2nd, w.ps, 32, 4, out=out)),
                     ("gin_eps", lambda: _lib.agg_gin(w.Xc, g.row_pointers, g.column_index, 0.5, w.ppd, w.p2nd,
                                                      w.ps, 32, 4, out=out))):
        res[name + "_edges_per_s"] = timed(fn)["edges_per_s"]
    # SDDMM over the same partition (build-defined; north_star names it next to the aggregation): edge_out[e] = <A[row(e)], X[col(e)]>
    try:
        edge_out = torch.empty(g.nnz, dtype=torch.float32, device=w.Xc.device)
        sd = timed(lambda: _lib.sddmm(out, w.Xc, g.column_index, w.ppd, w.p2nd, w.ps, out=edge_out))
        res["sddmm"] = dict(edges_per_s=sd["edges_per_s"], ms_per_step=sd["ms_per_step"],
                            what="gnna_sddmm_f32 on the bench graph, contiguous rows, same partition (wall clock, %d calls)" % steps)
        del edge_out
    except Exception as exc:                      # (an extra figure must never cost the headline line)
        res["sddmm"] = {"error": repr(exc)[:200]}
    return res


# ---------------------------------------------------------------------------------------------- --dump-outputs
DUMP_LIMIT_BYTES = 64 * 1000 * 1000     # all files of one --dump-outputs together
DUMP_SAMPLE_SEED = 20211104


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """What the timed path returned in its last step -> `out_dir`/<name>.npy, float32, rows as they came back.  An array
    larger than its share of `limit` is written as a fixed, seeded sample of its rows (the same rows for the same shape),
    with the sampled row ids beside it as <name>_rows.npy (float64), so that two builds can be compared row for row."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    share = limit // max(1, len(arrays)) - 4096                          # (room for the .npy headers)
    for name, t in arrays.items():
        t = t.detach()
        rows = t.shape[0] if t.dim() else 1
        row_bytes = max(1, t.numel() // max(1, rows)) * 4
        if rows * row_bytes <= share:
            np.save(os.path.join(out_dir, name + ".npy"), t.float().cpu().numpy())
            continue
        k = max(1, share // (row_bytes + 8))
        ids = torch.randperm(rows, generator=torch.Generator().manual_seed(DUMP_SAMPLE_SEED))[:k].sort().values
        np.save(os.path.join(out_dir, name + ".npy"), t[ids.to(t.device)].float().cpu().numpy())
        np.save(os.path.join(out_dir, name + "_rows.npy"), ids.numpy().astype(np.float64))


# ---------------------------------------------------------------------------------------------- the line
LINE_LIMIT = 8000       # the driver keeps an 8 KB tail of stdout: a longer line cannot be parsed (round 5's was 34.7 KB)
LINE_TARGET = 4096


def _clean(v, digits=7):
    """Strict JSON for the line: no NaN / Infinity tokens, floats to `digits` significant figures."""
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None
        return float("%.*g" % (digits, v))
    if isinstance(v, dict):
        return {str(k): _clean(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_clean(x, digits) for x in v]
    return str(v)


def _pick(src, keys):
    return {k: src.get(k) for k in keys if src.get(k) is not None or k in ("traffic", "vs_baseline")}


def compact_roofline(r):
    """The roofline object of the line: numbers and short tokens only (definitions live in DESIGN.md 4)."""
    out = _pick(r, ("bound", "ceiling", "peak", "unit", "achieved", "frac"))
    label = str(r.get("kernel", ""))
    out["kernel"] = label.split(" (")[0] if label else None
    out.update(_pick(r, ("kernel_ms", "kernel_launches_per_step", "column_phases", "prologue_ms", "traffic", "frac_hbm_measured",
                         "l2_hit_rate", "l2_requests_per_edge", "frac_l2", "traffic_over_compulsory", "floor_ms", "frac_of_floor",
                         "library_calls_per_step")))
    out["algorithmic_bytes"] = r.get("algorithmic_bytes_per_launch", r.get("algorithmic_bytes_per_step"))
    comp = r.get("compulsory_model") or {}
    if comp.get("bytes_per_step") is not None:
        out["compulsory_bytes"] = comp["bytes_per_step"]
    if r.get("traffic") is None and r.get("traffic_error"):
        out["traffic_error"] = str(r["traffic_error"])[:120]
    if r.get("l2_hit_rate") is not None:
        out["frac_note"] = "gather model; L2 hit %.2f" % r["l2_hit_rate"]
    return out


def compact_single(rec, detail_file=None):
    """The ONE line of a single-GPU run: the contract's keys, `config` as flat scalars, `roofline` and `cpu_baseline` as
    numbers.  Everything else of `rec` stays in the detail file."""
    c = rec.get("config", {})
    line = _pick(rec, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data", "verified"))
    cfg = {"workload": c.get("workload"), "num_nodes": c.get("num_nodes_per_gpu"), "nnz": c.get("nnz_per_gpu"), "dim": c.get("dim"),
           "partSize": c.get("partSize"), "num_parts": c.get("num_parts_per_gpu"), "feature_MB": c.get("feature_MB"),
           "parallelism": c.get("parallelism"),
           "call": "GNNA.SAG (pybind module, reference signature, fresh output)" if "pybind" in str(c.get("call", ""))
                   else "gnna_agg_ld_f32 (C ABI, prepared lifecycle)",
           "decider": "manual" if str(c.get("decider", "")).startswith("manual") else "auto/mi355x",
           "column_phases": c.get("column_phases_used"), "build_id": c.get("build_id")}
    cfg.update(_pick(c, ("ms_per_step_min", "ms_per_step_median", "ms_per_step_max", "reference_style_ms_hidden64",
                         "reference_style_ms_hidden16", "gcn_weighted_value", "gin_value", "sddmm_value", "prepared_value")))
    ver = c.get("verification") or {}
    cfg.update({"ones_exact": ver.get("ones_exact"), "sampled_rows_ok": ver.get("sampled_rows_ok"),
                "max_err_over_abs_ref": ver.get("max_err_over_abs_ref")})
    if detail_file:
        cfg["detail_file"] = detail_file
    line["config"] = {k: v for k, v in cfg.items() if v is not None}
    line["roofline"] = compact_roofline(rec.get("roofline", {}))
    cb = rec.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "ms", "ms_min", "ms_max"))
        line["cpu_baseline"]["sample"] = "full graph, D=%s, median of %s passes of the OpenMP CSR SpMM in oracle/gnna_oracle.c, %s pinned threads" % (
            c.get("dim"), len(cb.get("pass_ms_in_order") or []) or "all", cb.get("cores"))
        lib = cb.get("libraries") or {}
        for key, short in (("torch_sparse_csr", "torch_sparse_csr_value"), ("scipy_csr_1thread", "scipy_1thread_value")):
            if isinstance(lib.get(key), dict):
                line["cpu_baseline"][short] = lib[key].get("value")
        line["cpu_baseline"]["dgl"] = "unavailable" if "unavailable" in str(lib.get("dgl_copy_u_sum", "unavailable")) else "importable"
    return _clean(line)


def compact_sharded(rec, detail_file=None):
    """The ONE line of an N-rank run: headline (weak-scaling leg), the per-leg values, who counted the ranks."""
    c = rec.get("config", {})
    line = _pick(rec, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data", "verified"))
    cfg = _pick(c, ("workload", "num_nodes_per_gpu", "nnz_per_gpu", "dim", "partSize", "num_parts_per_gpu", "source_nodes",
                    "world_size", "backend", "rccl_world_size", "communicator_ranks_counted", "parallelism", "exchange", "exchange_requested",
                    "exchange_only_ms", "aggregate_only_ms", "exchange_GBs_per_rank", "bytes_received_per_rank_per_step",
                    "allgather_bytes_per_rank_per_step", "decider", "force_collectives", "build_id"))
    cfg["parallelism"] = str(cfg.get("parallelism", ""))[:120]
    if c.get("values"):
        cfg["values"] = {n: _pick(v, ("value", "ms_per_step", "scaling", "verified", "exchange")) for n, v in c["values"].items()}
    if c.get("failed_legs"):
        cfg["failed_legs"] = {n: str(v)[:120] for n, v in c["failed_legs"].items()}
    if c.get("exchange_timed"):
        cfg["exchange_timed"] = _pick(c["exchange_timed"], ("allgather_ms", "halo_ms", "chosen"))
    if c.get("single_gpu_line"):
        cfg["single_gpu_value"] = c["single_gpu_line"].get("value")
        cfg["sharded_over_single"] = c["single_gpu_line"].get("sharded_over_single")
    if detail_file:
        cfg["detail_file"] = detail_file
    line["config"] = cfg
    line["roofline"] = compact_roofline(rec.get("roofline", {}))
    return _clean(line)


def emit(rec, result_fd, compact, args, suffix=""):
    """Full record -> the detail file (with --full or --detail-file; and a short summary on stderr); the compact line -> the
    saved stdout."""
    path = args.detail_file or os.path.join(ROOT, "gpurun_out", "bench_detail%s.json" % suffix)
    shown = None
    if args.detail_file or args.full:
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                json.dump(_clean(rec, 9), f, indent=1)
            shown = os.path.relpath(path, ROOT)
        except OSError as exc:                               # (a read-only tree must not cost the line)
            print(f"# bench.py: detail file not written ({exc})", file=sys.stderr)
    line = compact(rec, shown)
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    if len(text) >= LINE_LIMIT:                              # never print a line the driver cannot read: shed the optional keys
        for key in ("cpu_baseline", "config"):
            sub = line.get(key, {})
            for k in [k for k in sub if k not in ("value", "unit", "cores", "kind", "workload", "nnz", "dim", "partSize")]:
                sub.pop(k)
        text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(text) < LINE_LIMIT, len(text)
    r = line.get("roofline", {})
    print("# bench.py: %.4g %s, %.4f ms/step, verified %s; %s %.4f ms, frac %.3f of %s; line %d chars; detail: %s"
          % (line.get("value") or 0, line.get("unit"), line.get("ms_per_step") or 0, line.get("verified"), r.get("kernel"),
             r.get("kernel_ms") or 0, r.get("frac") or 0, r.get("ceiling", r.get("bound")), len(text), shown), file=sys.stderr, flush=True)
    os.write(result_fd, (text + "\n").encode())


# ---------------------------------------------------------------------------------------------- single GPU

def leg_record(w, elapsed, prof, steps, check, traffic, what):
    """One secondary workload of the single-GPU line: value, verification, roofline."""
    g = w.g
    rec = {"workload": what, "value": g.nnz * steps / elapsed, "unit": "edges/s", "steps": steps,
           "ms_per_step": elapsed * 1e3 / steps, "num_nodes": g.num_nodes, "nnz": g.nnz, "dim": w.dim,
           "partSize": w.ps, "num_parts": w.P, "column_phases_used": w.phases,
           "aggregation": {"sag": "SAG (unweighted sum)", "gin": "GIN (eps = 0.5 scaled sum)"}.get(getattr(w, "kind", "sag")),
           "lifecycle": getattr(w, "lifecycle", None), "node_order": getattr(w, "order", None),
           "avg_edge_span": float(getattr(g, "avg_edgeSpan", float("nan"))),      # mean |src - dst| (dataset.py:99-100, the Decider's reorder rule)
           "verified": check["verified"], "verification": check,
           "roofline": roofline_record(w, prof["main_ms"], prof["prologue_ms"], traffic)}
    if getattr(w, "reorder_seconds", None) is not None:
        rec["reorder_seconds"] = w.reorder_seconds
    return rec


def run_single(args, result_fd):
    import gc
    import torch
    from gnnadvisor_osdi21_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.config.startswith("rank-of-"):
        # profiling aid (tools/profile_gpu.sh): the timed loop of one config-5 form on its own, e.g.
        #   bench.py --headline-only --config rank-of-8/allgather-one-call --dim 128 --steps 5 --warmup 2
        world5, form5 = args.config[len("rank-of-"):].split("/")
        w5 = RankOf8Workload(dev, args.dim, form=form5, world=int(world5), scale=args.scale, manual=args.manual)
        e5, p5 = w5.time(args.steps, args.warmup)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"aggregated": w5.out})
        rec = {"metric": "aggregated edges/sec, config 5 per-rank shape", "value": w5.g.nnz * args.steps / e5, "unit": "edges/s",
               "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": e5 * 1e3 / args.steps,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": args.config, "shape": w5.describe()},
               "roofline": roofline_record(w5, p5["main_ms"], p5["prologue_ms"], None)}
        emit(rec, result_fd, compact_single, args, "_rank_of")
        return
    extras = args.full and not args.headline_only     # a plain run: set-up, warm-up, the timed steps, the line
    detail = extras and args.detail

    def free():
        gc.collect()
        torch.cuda.empty_cache()

    # ---- the headline: BASELINE config 3 as a caller of the reference API runs it (lifecycle "dropin"; --prepared times
    # the build's own lifecycle extension instead, for profiling) --------------------------------------------------------
    w = Workload(args.config, args.dim, dev, scale=args.scale, locality=args.locality, manual=args.manual,
                 part_size=args.partSize, lifecycle="prepared" if args.prepared else "dropin", calibrate=not args.headline_only)
    elapsed, prof = w.time(args.steps, args.warmup, blocks=5 if extras else 1)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"aggregated": w.out})
    tmpdir = tempfile.mkdtemp(prefix="gnna_bench_", dir="/tmp") if detail else None
    g = w.g
    kern_ms, pro_ms = prof["main_ms"], prof["prologue_ms"]
    check = w.verify() if extras else {"verified": None}
    auto_prepared = int(w.GNNA.auto_prepared_graphs())
    floor = floor_probe(w, w.phases) if extras and args.scale == 1.0 else None
    ref_style = reference_style_ms(w) if extras else None
    modes = other_modes(w) if extras else None
    tuning_dropin = _lib.get_tuning()
    measured = [w]                     # workloads whose traffic the PMC children measure (the headline first)
    legs = {}                          # name -> (workload record kept alive only through what the line needs)

    def run_leg(name, what, steps, warm, **kw):
        wl = Workload(kw.pop("config"), kw.pop("dim"), dev, manual=args.manual, **kw)
        wl.perm_file = kw.get("perm_file")
        e, p = wl.time(steps, warm, blocks=1)
        chk = wl.verify(64)
        legs[name] = (wl, e, p, steps, chk, what)
        measured.append(wl)
        # (the record needs the graph's sizes and the schedule, not the tensors)
        class _G:
            pass
        gg = _G()
        gg.nnz, gg.num_nodes, gg.avg_edgeSpan = wl.g.nnz, wl.g.num_nodes, wl.g.avg_edgeSpan
        wl.g, wl.Xc, wl.X, wl.out, wl.ppd, wl.p2nd, wl.pp, wl.p2n = gg, None, None, None, None, None, None, None
        free()

    prepared = None
    if detail and not args.prepared and not args.manual:
        # the build's lifecycle extension on the same graph: hints + gnna_prepare_graph + measured phase count + the
        # producer-written gapped layout through gnna_agg_ld_f32 (flat keys prepared_*; never `value`)
        wp = Workload(args.config, args.dim, dev, scale=args.scale, locality=args.locality, part_size=args.partSize,
                      lifecycle="prepared")
        ep, pp_ = wp.time(args.steps, args.warmup, blocks=1)
        chkp = wp.verify(64)
        prepared = {"value": wp.g.nnz * args.steps / ep, "ms_per_step": ep * 1e3 / args.steps, "kernel_ms": pp_["main_ms"],
                    "column_phases_used": wp.phases, "calibrated_phases": wp.calibrated, "input_leading_dimension": wp.ld,
                    "verified": chkp["verified"], "tuning": _lib.get_tuning()}
        _lib.release_graph(wp.g.column_index)
        del wp
        _lib.reset_tuning()            # (apply_tuning set process-wide knobs: the legs below run on the defaults again)
        free()
    if detail and not args.no_secondary and args.scale == 1.0:
        sec = args.secondary_config
        # BASELINE config 4 in its own shape: GIN aggregation (eps x sum, GNNAdvisor_kernel.cu:620-689) of layer 1 at the
        # input width D = 100 and of layers 2-5 at D = 64; features 980 / 627 MB > Infinity Cache (HBM-resident)
        run_leg("config4_gin_D100", f"{sec} power-law graph, random node order, GIN layer-1 aggregation at D = 100 (aggregate-then-"
                "update at the input width)", 5, 3, config=sec, dim=100, kind="gin")
        run_leg("config4_gin_D64", f"{sec} power-law graph, random node order, GIN aggregation of layers 2-5 at D = 64", 8, 3,
                config=sec, dim=64, kind="gin")
        run_leg("hbm_resident", f"{sec} power-law graph, random node order, SAG at D = 64 (features 627 MB > 256 MiB Infinity Cache)",
                8, 3, config=sec, dim=64, kind="sag")
        # both node orders (the role of rabbit_module/src/reorder.cpp:235-295): graphs with hidden community
        # structure (90 % of the edges within +-4096 ids of the generator's order) whose ids were scrambled, before and after
        # the native community renumbering
        for cfg_name, tag in ((args.config, "config3"), (sec, "config4")):
            pf = os.path.join(tmpdir, f"renumbering_{tag}.pt")
            run_leg(f"{tag}_hidden_locality_scrambled", f"{cfg_name} graph with hidden locality, ids scrambled (random order), SAG D = 64",
                    8, 3, config=cfg_name, dim=64, locality=0.9, order="scrambled")
            run_leg(f"{tag}_hidden_locality_renumbered", f"the same graph after gnna_reorder_community_i32 (locality-friendly order), SAG D = 64",
                    8, 3, config=cfg_name, dim=64, locality=0.9, order="renumbered", perm_file=pf)
            # the order the generator planted the communities in: what a perfect renumbering of this graph would find (Rabbit Order
            # itself cannot be built here -- boost / numa / tcmalloc -- so this is the yardstick the native renumbering is held to)
            run_leg(f"{tag}_hidden_locality_planted", f"the same graph in the generator's own community order (yardstick for the renumbering), SAG D = 64",
                    8, 3, config=cfg_name, dim=64, locality=0.9, order="generator")
    # BASELINE config 5 in its true per-rank shape (rank 0 of 8; the 56.9 GB all-gather buffer, then the compact halo
    # buffer the automatic exchange takes): one after the other -- each keeps the global features resident
    fives = []
    if detail and not args.no_config5 and args.scale == 1.0:
        for form in ("allgather-one-call", "halo"):
            w5 = RankOf8Workload(dev, 128, form=form, manual=args.manual, scale=args.config5_scale)
            e5, p5 = w5.time(4, 2)
            chk5 = w5.verify(200)
            fives.append((w5, e5, p5, 4, chk5, w5.describe()))
            w5.source_bytes = int(desc_bytes(w5))
            w5.release()
            free()
    traffic = {}
    if extras and not args.no_pmc:
        ws = measured + [f[0] for f in fives]
        for wl, t in zip(ws, measure_traffic(ws, args)):
            traffic[id(wl)] = t

    ms_per_step = elapsed * 1e3 / args.steps
    order_name = "random node order" if not args.locality else f"generator's community order (locality={args.locality})"
    wl_name = (f"{args.config} power-law graph, {order_name}" + (f", scale={args.scale}" if args.scale != 1.0 else ""))
    x_mb = g.num_nodes * args.dim * 4 / 1e6
    rec = {
        "metric": "aggregated edges/sec, GCN sum-aggregation SpMM (SAG) hidden=64",
        "value": g.nnz * args.steps / elapsed, "unit": "edges/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "verified": check["verified"],
        "config": {"workload": wl_name, "num_nodes_per_gpu": g.num_nodes, "nnz_per_gpu": g.nnz, "dim": args.dim,
                   "partSize": w.ps, "num_parts_per_gpu": w.P, "source_nodes": g.num_nodes,
                   "feature_MB": x_mb, "parallelism": "single GPU", "world_size": 1, "device": str(dev),
                   "decider": "manual (partSize 32)" if args.manual else "auto (mi355x policy): inputProperty.decider() -> partSize",
                   "call": ("GNNA.SAG(X, row_pointers, column_index, degrees, partPtr, part2Node, partSize, 32, 4) through the pybind "
                            "module `GNNAdvisor` (GNNAdvisor.cpp:75-96): contiguous tensors, a fresh output tensor per call"
                            if w.lifecycle == "dropin" else "gnna_agg_ld_f32 through the C ABI (extension lifecycle, --prepared)"),
                   "column_phases_used": w.phases, "tuning": tuning_dropin,
                   "input_leading_dimension": w.ld,
                   "input_layout": "contiguous rows" if w.ld == args.dim else "rows written with leading dimension %d" % w.ld,
                   "graph_lifecycle": "none (six reference functions only)" if w.lifecycle == "dropin" else
                                      "gnna_prepare_graph before the timed region (extension)",
                   "module_prepared_graphs_by_itself": auto_prepared,
                   "packed_column_ids_in_use": bool(getattr(w, "packed", False)),
                   "build_id": _lib.build_id()},
        "roofline": roofline_record(w, kern_ms, pro_ms, traffic.get(id(w)), floor),
    }
    rec["config"]["verified"] = rec["verified"]
    rec["config"]["verification"] = check
    # flat keys (the driver's parser keeps scalars of `config`, not nested records): the spread of the headline over 5
    # blocks of K steps, the prepared-lifecycle figure and the other modes
    blocks = sorted(getattr(w, "block_ms", [ms_per_step]))
    rec["config"].update({"ms_per_step_min": blocks[0], "ms_per_step_median": blocks[len(blocks) // 2],
                          "ms_per_step_max": blocks[-1], "blocks_timed": len(blocks),
                          "value_min": g.nnz / (blocks[-1] * 1e-3), "value_median": g.nnz / (blocks[len(blocks) // 2] * 1e-3),
                          "value_max": g.nnz / (blocks[0] * 1e-3)})
    if prepared:
        rec["config"].update({"prepared_value": prepared["value"], "prepared_ms_per_step": prepared["ms_per_step"],
                              "prepared_kernel_ms": prepared["kernel_ms"], "prepared_verified": prepared["verified"],
                              "prepared_input_leading_dimension": prepared["input_leading_dimension"],
                              "dropin_over_prepared": rec["value"] / prepared["value"],
                              "prepared_lifecycle": prepared})
    if modes:
        rec["config"].update({"gcn_weighted_value": modes.get("gcn_weighted_edges_per_s"),
                              "gin_value": modes.get("gin_eps_edges_per_s"),
                              "sddmm_value": (modes.get("sddmm") or {}).get("edges_per_s"),
                              "other_modes": modes})
    if ref_style:
        rec["config"]["reference_style_ms"] = ref_style
        rec["config"]["reference_style_ms_hidden64"] = ref_style.get("64")
        rec["config"]["reference_style_ms_hidden16"] = ref_style.get("16")
    others = {}
    for name, (wl, e, p, k, chk, what) in legs.items():
        others[name] = leg_record(wl, e, p, k, chk, traffic.get(id(wl)), what)
    for tag in ("config3", "config4"):
        a_, b_ = others.get(f"{tag}_hidden_locality_scrambled"), others.get(f"{tag}_hidden_locality_renumbered")
        c_ = others.get(f"{tag}_hidden_locality_planted")
        if a_ and b_:
            ra, rb = a_["roofline"], b_["roofline"]
            rec["config"][f"{tag}_renumbering"] = {
                "ms_scrambled": a_["ms_per_step"], "ms_renumbered": b_["ms_per_step"], "speedup": a_["ms_per_step"] / b_["ms_per_step"],
                "reorder_seconds": b_.get("reorder_seconds"),
                "l2_hit_before": ra.get("l2_hit_rate"), "l2_hit_after": rb.get("l2_hit_rate"),
                "traffic_over_compulsory_before": ra.get("traffic_over_compulsory"),
                "traffic_over_compulsory_after": rb.get("traffic_over_compulsory"),
                "avg_edge_span_scrambled": a_.get("avg_edge_span"), "avg_edge_span_renumbered": b_.get("avg_edge_span")}
            if c_:
                rec["config"][f"{tag}_renumbering"].update({
                    "ms_planted_order": c_["ms_per_step"], "avg_edge_span_planted": c_.get("avg_edge_span"),
                    "planted_over_renumbered_ms": c_["ms_per_step"] / b_["ms_per_step"],
                    "l2_hit_planted": c_["roofline"].get("l2_hit_rate"),
                    "traffic_over_compulsory_planted": c_["roofline"].get("traffic_over_compulsory")})
    for w5, e5, p5, k5, chk5, desc5 in fives:
        key = "config5_rank_of_8" if w5.form == "allgather-one-call" else "config5_rank_of_8_" + w5.form.replace("-", "_")
        others[key] = {
            "workload": f"papers100M-like power-law graph, rank {w5.rank} of {w5.world} in its true shape: "
                        f"{w5.n_local} destination rows gathering D = 128 rows of {w5.n_global} source nodes; "
                        + ("ONE rectangular call over the resident all-gather buffer"
                           if w5.form == "allgather-one-call" else
                           "local-source part from the rank's own block + remote part piece by piece from the compact "
                           "halo buffer (what --exchange auto takes)")
                        + "; kernels only, receive buffer filled from the global features instead of by RCCL",
            "value": w5.g.nnz * k5 / e5, "unit": "edges/s", "steps": k5, "ms_per_step": e5 * 1e3 / k5,
            "num_nodes": w5.n_local, "nnz": w5.g.nnz, "dim": 128, "shape": desc5,
            "column_phases_used": w5.phases, "verified": chk5["verified"], "verification": chk5,
            "roofline": roofline_record(w5, p5["main_ms"], p5["prologue_ms"], traffic.get(id(w5))),
        }
    if others:
        # the legs repeat long constant strings of the headline's records: say them once (the line stays well under the
        # size of a pipe buffer)
        for leg in others.values():
            for key in ("frac_definition", "traffic_detail", "traffic_source"):
                leg["roofline"].pop(key, None)
            leg["verification"].pop("bound_form", None)
            if "hbm_read_rate_note" in leg["roofline"] and leg["roofline"].get("ceiling") != "hbm":
                leg["roofline"].pop("hbm_read_rate_note")
        rec["roofline"]["other_workloads"] = others
    if extras and not args.no_cpu_baseline:
        rec["cpu_baseline"] = cpu_baseline(g.to("cpu"), w.Xc.cpu(), w.pp, w.p2n, args.dim)
    if tmpdir:
        shutil.rmtree(tmpdir, ignore_errors=True)
    emit(rec, result_fd, compact_single, args)


def desc_bytes(w5):
    """Bytes of the source buffer a config-5 rank gathers from (decides which ceiling its roofline is quoted against)."""
    return int(w5.buf.shape[0]) * w5.dim * 4


# ---------------------------------------------------------------------------------------------- N ranks

def sharded_leg(args, dev, world, rank, name, rp, ci, bounds, D, feat, avg_span, steps, warmup, dist, exchange):
    """One workload of the N-rank line: this rank's destination shard (local CSR rows `rp`, GLOBAL column ids `ci`),
    `steps` timed aggregations (exchange + kernels) bracketed by barriers, then exchange-only / kernels-only timings
    and the known-answer check on every rank.  -> dict of this leg's numbers (max / sum over the ranks)."""
    import torch
    from gnnadvisor_osdi21_amd import _lib
    from gnnadvisor_osdi21_amd.decider import inputProperty
    from gnnadvisor_osdi21_amd.dist import ShardedAggregator
    n_local = bounds[rank + 1] - bounds[rank]
    n_global = bounds[-1]

    class _Profile:
        pass
    prof_obj = _Profile()
    prof_obj.num_nodes, prof_obj.avg_degree = n_local, float(ci.numel()) / max(1, n_local)
    prof_obj.avg_edgeSpan = avg_span
    prof_obj.num_features, prof_obj.reorder_flag = feat, False
    prof_obj.rabbit_reorder = lambda: None
    info = inputProperty(None, None, None, 32, 32, 4, 100, hiddenDim=D, dataset_obj=prof_obj,
                         enable_rabbit=False, manual_mode=args.manual)
    info.decider()
    if not args.manual:
        info.apply_tuning()
    ps = args.partSize if args.partSize > 0 else info.partSize
    if exchange == "auto" and world > 1:
        # a wire to time: both forms are built and run three steps each, the faster is kept (dist.timed_aggregator)
        from gnnadvisor_osdi21_amd.dist import timed_aggregator
        agg = timed_aggregator(rp, ci, bounds, ps, dim=D, reps=3, device=dev, force_overlap=args.force_dist,
                               pipeline_chunks=args.pipeline_chunks)
    else:
        agg = ShardedAggregator(rp, ci, bounds, ps, device=dev, force_overlap=args.force_dist,
                                pipeline_chunks=args.pipeline_chunks, exchange=exchange,
                                force_collectives=args.force_collectives)
    calibrated = agg.calibrate([D]) if not (args.manual or args.headline_only) else None
    nnz_local = agg.nnz_local
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    X = torch.randn(n_local, D, device=dev, generator=gen)
    out = torch.empty_like(X)
    P = int(agg.part2Node.numel())

    def step():
        agg.sag(X, out=out)

    def sync_all():
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    sync_all()
    _lib.profile_begin(steps * 64)                         # a sharded step is several library calls
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync_all()
    elapsed = time.perf_counter() - t0
    prof = _lib.profile_end()
    if args.dump_outputs and name == "weak":              # (the headline leg: every rank writes its own block of rows)
        dump_outputs(args.dump_outputs, {f"aggregated_rank{rank}": out}, limit=DUMP_LIMIT_BYTES // world)
    calls_per_step = prof["calls"] / max(1, steps)
    kern_ms = prof["main_ms"] * calls_per_step
    phases_last = _lib.last_num_phases()

    # the two halves of a step on their own (same buffers, after the timed loop): exchange only, kernels only
    def timed_ms(fn, n=5):
        fn()
        sync_all()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        sync_all()
        return (time.perf_counter() - t) * 1e3 / n
    exchange_ms = timed_ms(lambda: agg.exchange_only(X))
    aggregate_ms = timed_ms(lambda: agg.aggregate_only(X, out=out))

    per_rank = [None] * world
    dist.all_gather_object(per_rank, (rank, exchange_ms, aggregate_ms))
    per_rank.sort()

    # verification of the timed configuration: X = ones everywhere -> exact row nnz on every rank.  STRICT: a rank that is off
    # dumps what it computed (rows, values, expected) under gpurun_out/dist_dump/ before the run fails
    ones = torch.ones_like(X)
    y1 = agg.sag(ones)
    deg = (rp[1:] - rp[:-1]).to(torch.float32).to(dev)
    bad_rows = torch.nonzero((y1 != deg[:, None]).any(dim=1)).flatten()
    if bad_rows.numel():
        ddir = os.path.join(ROOT, "gpurun_out", "dist_dump")
        os.makedirs(ddir, exist_ok=True)
        torch.save({"leg": name, "rank": rank, "world": world, "rows": bad_rows.cpu(), "got": y1[bad_rows[:256]].cpu(),
                    "expected_row_nnz": deg[bad_rows[:256]].cpu(), "exchange": agg.exchange, "pieces": agg.chunks,
                    "bounds": bounds}, os.path.join(ddir, f"bench_{name}_rank{rank}_of_{world}.pt"))
    exact = torch.tensor([0.0 if bad_rows.numel() else 1.0], dtype=torch.float64, device=dev)
    del ones, y1

    stats = torch.tensor([elapsed, kern_ms, float(agg.bytes_received_per_step(D)),
                          float(agg.allgather_bytes_per_step(D)), exchange_ms, aggregate_ms, float(calls_per_step)],
                         dtype=torch.float64, device=dev)
    sums = torch.tensor([float(nnz_local)], dtype=torch.float64, device=dev)
    if args.backend != "nccl":
        stats, sums, exact = stats.cpu(), sums.cpu(), exact.cpu()
    dist.all_reduce(stats, op=dist.ReduceOp.MAX)
    dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    dist.all_reduce(exact, op=dist.ReduceOp.MIN)
    elapsed, kern_ms = float(stats[0]), float(stats[1])
    total_edges = float(sums[0])
    t = kern_ms * 1e-3
    comp = compulsory_bytes(nnz_local, n_local, n_global, D)
    alg = gather_model_bytes(nnz_local, n_local, P, D)
    leg = {
        "leg": name, "value": total_edges * steps / elapsed, "unit": "edges/s", "steps": steps, "warmup": warmup,
        "ms_per_step": elapsed * 1e3 / steps, "total_nnz": total_edges, "dim": D,
        "verified": bool(float(exact[0]) == 1.0),
        "num_nodes_per_gpu": n_local, "nnz_per_gpu": nnz_local, "partSize": ps, "num_parts_per_gpu": P,
        "source_nodes": n_global, "parallelism": f"dst-range shards x{world} + " + agg.describe_exchange(),
        "exchange": agg.exchange, "exchange_requested": exchange, "pieces": agg.chunks,
        "exchange_timed": getattr(agg, "exchange_timed", None),
        "bytes_received_per_rank_per_step": float(stats[2]), "allgather_bytes_per_rank_per_step": float(stats[3]),
        "exchange_volume_vs_allgather": float(stats[2]) / float(stats[3]) if float(stats[3]) else None,
        "exchange_only_ms": float(stats[4]), "aggregate_only_ms": float(stats[5]),
        "exchange_only_ms_per_rank": [round(v[1], 4) for v in per_rank],
        "aggregate_only_ms_per_rank": [round(v[2], 4) for v in per_rank],
        "exchange_GBs_per_rank": float(stats[2]) / (float(stats[4]) * 1e-3) / 1e9 if float(stats[4]) > 0 else None,
        "calibrated_phases": calibrated,
        "kernel": {"name": "stream_kernel (libgnna streaming kernel; one launch per library call)",
                   "library_calls_per_step": float(stats[6]), "kernel_ms_per_step_max_over_ranks": kern_ms,
                   "column_phases_last_call": phases_last,
                   "kernel_edges_per_s": nnz_local / t if t > 0 else 0.0,
                   "gather_model": {"bytes_per_step": alg, "GBs": alg / t / 1e9 if t > 0 else 0.0},
                   "compulsory_model": {"bytes_per_step": comp, "GBs": comp / t / 1e9 if t > 0 else 0.0}},
    }
    del agg, X, out
    torch.cuda.empty_cache()
    return leg


def run_sharded(args, result_fd, world, rank, local_rank):
    """N ranks (one per GPU): the weak-scaling leg is the headline (`value`; every rank a Reddit-sized block -- at N = 1
    exactly the single-GPU workload); `--scaling` adds the strong-scaling leg (the SAME Reddit-like graph split into N
    nnz-balanced destination blocks) and, at 8 ranks (or with --config5-leg), BASELINE config 5 (papers100M-like,
    D = 128, exchange chosen collectively)."""
    import datetime
    import torch
    import torch.distributed as dist
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    limit = datetime.timedelta(seconds=600)                # a rank that dies must not hang the others for long
    if args.backend == "nccl":
        dist.init_process_group("nccl", device_id=dev, timeout=limit)
    else:
        dist.init_process_group(args.backend, timeout=limit)

    from gnnadvisor_osdi21_amd import _lib, graph
    from gnnadvisor_osdi21_amd.dist import balanced_row_splits, shard_csr
    _lib.load()
    # the communicator itself says how many ranks it has: one all-reduce of ones through it (RCCL when --backend nccl), and
    # the launcher's count, torch.distributed's count and --gpus must all agree -- a run that silently fell back to fewer
    # ranks (or to N independent 1-rank jobs) fails here instead of reporting an N-GPU number
    one = torch.ones(1, device=dev if args.backend == "nccl" else "cpu")
    dist.all_reduce(one)
    counted = int(one.item())
    if not (counted == world == dist.get_world_size() == max(1, args.gpus)):
        raise RuntimeError(f"rank {rank}: communicator counts {counted} ranks, torch.distributed {dist.get_world_size()}, "
                           f"launcher WORLD_SIZE {world}, --gpus {args.gpus}")
    print(f"# rank {rank}/{world}: {dist.get_backend()} communicator of {counted} rank(s), device cuda:{local_rank} "
          f"({torch.cuda.get_device_name(dev)})", file=sys.stderr, flush=True)
    cfg = graph.CONFIGS[args.config]
    D = args.dim
    legs = {}

    # ---- weak scaling (headline): every rank owns a Reddit-sized block whose sources are drawn from all ranks' nodes
    n_local = max(2, int(cfg["num_nodes"] * args.scale))
    e_target = int(cfg["num_edges"] * args.scale * cfg.get("oversample", 1.0))
    n_global = n_local * world
    rp, ci = graph.powerlaw_shard(n_local, n_global, e_target, min(cfg["max_degree"], n_global - 1),
                                  seed=cfg["seed"] * 1000 + rank, device=dev, locality=args.locality,
                                  block_start=rank * n_local)
    bounds = [i * n_local for i in range(world + 1)]
    legs["weak"] = sharded_leg(args, dev, world, rank, "weak", rp, ci, bounds, D, cfg["feat"],
                               (1.0 - args.locality) * n_global / 3.0, args.steps, args.warmup, dist, args.exchange)
    del rp, ci
    single = None
    if world == 1 and args.full and not args.headline_only:
        # the sharded path with one rank must be the single-GPU workload: the reference caller's line (lifecycle "dropin") is
        # timed beside it, and a sharded value more than 3 % below it fails the run (VERDICT r4 task 6b)
        w1 = Workload(args.config, D, dev, scale=args.scale, locality=args.locality, manual=args.manual, part_size=args.partSize)
        e1, _ = w1.time(args.steps, args.warmup, blocks=1)
        single = {"value": w1.g.nnz * args.steps / e1, "ms_per_step": e1 * 1e3 / args.steps,
                  "sharded_over_single": legs["weak"]["value"] / (w1.g.nnz * args.steps / e1)}
        del w1
        torch.cuda.empty_cache()
        # (enforced on the real N = 1 path; with --force-collectives the rank ships half of its block to itself through
        # RCCL and runs local + remote parts -- another workload, reported only; shrunken debug graphs are launch-bound)
        if single["sharded_over_single"] < 0.97 and args.scale == 1.0 and not args.force_collectives:
            raise RuntimeError("the one-rank sharded path reaches %.3f of the single-GPU value (%.1f vs %.1f G edges/s): more than 3 %% "
                               "below it" % (single["sharded_over_single"], legs["weak"]["value"] / 1e9, single["value"] / 1e9))

    want = [v for v in args.scaling.split(",") if v] if args.full else []      # (the extra legs run with --full)
    failed = {}
    # ---- strong scaling: the SAME graph as the single-GPU line, split into `world` nnz-balanced destination blocks
    if "strong" in want and world > 1:
        try:
            g = graph.make_config_graph(args.config, device=dev, locality=args.locality, scale=args.scale)
            sb = balanced_row_splits(g.row_pointers, world)
            # every rank generated the graph itself (same seed): the row bounds are taken from rank 0 so that the ranks
            # agree on them even if a generator ever differed between devices
            holder = [sb]
            dist.broadcast_object_list(holder, src=0)
            sb = [int(v) for v in holder[0]]
            srp, sci = shard_csr(g.row_pointers, g.column_index, sb[rank], sb[rank + 1])
            span = g.avg_edgeSpan
            n_all, nnz_all = g.num_nodes, g.nnz
            del g
            legs["strong"] = sharded_leg(args, dev, world, rank, "strong", srp, sci, sb, D, cfg["feat"], span,
                                         args.steps, args.warmup, dist, args.exchange)
            legs["strong"].update({"graph_nodes": n_all, "graph_nnz": nnz_all, "row_bounds": sb,
                                   "what": "the single-GPU line's graph split by nnz-balanced destination ranges"})
            del srp, sci
        except Exception as exc:      # the headline leg must survive a failure of an extra leg (same failure on every rank)
            failed["strong"] = repr(exc)[:300]
    # ---- BASELINE config 5: papers100M-like, D = 128, one destination shard per rank
    if ("config5" in want and world == 8) or args.config5_leg:
        try:
            c5 = graph.CONFIGS["papers100M-like"]
            n5 = max(64, int(c5["num_nodes"] * args.config5_scale) // world)
            e5 = int(c5["num_edges"] * args.config5_scale * c5.get("oversample", 1.0)) // world
            rp5, ci5 = graph.powerlaw_shard(n5, n5 * world, e5, min(c5["max_degree"], n5 * world - 1),
                                            seed=c5["seed"] * 1000 + rank, device=dev, block_start=rank * n5)
            b5 = [i * n5 for i in range(world + 1)]
            legs["config5"] = sharded_leg(args, dev, world, rank, "config5", rp5, ci5, b5, 128, c5["feat"],
                                          n5 * world / 3.0, max(3, args.steps // 5), 2, dist, "auto")
            legs["config5"]["what"] = ("BASELINE config 5: papers100M-like graph" + (f" at scale {args.config5_scale}" if args.config5_scale != 1.0 else "")
                                       + f", D = 128, destination-partitioned over {world} ranks, exchange chosen collectively")
            del rp5, ci5
        except Exception as exc:
            failed["config5"] = repr(exc)[:300]

    # who ran: RCCL's view of the job and every rank's device
    names = [None] * world
    dist.all_gather_object(names, f"rank {rank}: {torch.cuda.get_device_name(dev)} (cuda:{local_rank})")
    if rank == 0:
        weak = legs["weak"]
        k = weak["kernel"]
        t = k["kernel_ms_per_step_max_over_ranks"] * 1e-3
        rec = {
            "metric": "aggregated edges/sec, GCN sum-aggregation SpMM (SAG) hidden=64",
            "value": weak["value"], "unit": "edges/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": weak["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "verified": all(l["verified"] for l in legs.values()),
            "config": {"workload": f"{args.config} power-law graph, "
                                   + (f"id-local partition (locality={args.locality})" if args.locality else "random node order")
                                   + (f", scale={args.scale}" if args.scale != 1.0 else ""),
                       "num_nodes_per_gpu": weak["num_nodes_per_gpu"], "nnz_per_gpu": weak["nnz_per_gpu"], "dim": D,
                       "partSize": weak["partSize"], "num_parts_per_gpu": weak["num_parts_per_gpu"],
                       "source_nodes": weak["source_nodes"],
                       "world_size": dist.get_world_size(), "backend": dist.get_backend(), "ranks": names,
                       "rccl_world_size": dist.get_world_size() if dist.get_backend() == "nccl" else None,
                       "communicator_ranks_counted": counted, "single_gpu_line": single,
                       "exchange_only_ms_per_rank": weak["exchange_only_ms_per_rank"],
                       "aggregate_only_ms_per_rank": weak["aggregate_only_ms_per_rank"],
                       "force_collectives": bool(args.force_collectives),
                       "device": str(dev) + (" (shared by all ranks)" if args.share_gpu else ""),
                       "parallelism": weak["parallelism"], "exchange": weak["exchange"],
                       "exchange_requested": args.exchange, "exchange_timed": weak.get("exchange_timed"),
                       "bytes_received_per_rank_per_step": weak["bytes_received_per_rank_per_step"],
                       "allgather_bytes_per_rank_per_step": weak["allgather_bytes_per_rank_per_step"],
                       "exchange_volume_vs_allgather": weak["exchange_volume_vs_allgather"],
                       "exchange_only_ms": weak["exchange_only_ms"], "aggregate_only_ms": weak["aggregate_only_ms"],
                       "exchange_GBs_per_rank": weak["exchange_GBs_per_rank"],
                       "decider": "manual (partSize 32)" if args.manual else "auto (mi355x policy)",
                       "calibrated_phases": weak["calibrated_phases"], "tuning": _lib.get_tuning(),
                       "verified": all(l["verified"] for l in legs.values()),
                       "verification": {n: {"ones_exact_on_every_rank": l["verified"]} for n, l in legs.items()},
                       "legs": {n: l for n, l in legs.items() if n != "weak"}, "failed_legs": failed,
                       "values": {n: {"value": l["value"], "unit": "edges/s", "ms_per_step": l["ms_per_step"],
                                      "verified": l["verified"], "exchange": l["exchange"],
                                      "scaling": "weak" if n == "weak" else ("strong" if n == "strong" else "config5 (fixed total graph)")}
                                  for n, l in legs.items()}},
            "roofline": {"bound": "hbm", "ceiling": roofline_ceiling(weak["source_nodes"] * D * 4)[0],
                         "peak": roofline_ceiling(weak["source_nodes"] * D * 4)[1], "unit": "GB/s",
                         "achieved": k["gather_model"]["GBs"], "algorithmic_bytes_per_step": k["gather_model"]["bytes_per_step"],
                         "frac": roofline_frac(k["gather_model"]["bytes_per_step"], t, weak["source_nodes"] * D * 4) if t > 0 else 0.0,
                         "frac_definition": "per rank: algorithmic (gather-model) bytes / kernel time (max over ranks) / ceiling, as on "
                                            "the single-GPU line (roofline_ceiling); no PMC passes in multi-rank runs",
                         "traffic": None, "kernel": k["name"], "kernel_ms": k["kernel_ms_per_step_max_over_ranks"],
                         "library_calls_per_step": k["library_calls_per_step"],
                         "compulsory_model": k["compulsory_model"], "kernel_edges_per_s": k["kernel_edges_per_s"],
                         "per_leg_kernels": {n: l["kernel"] for n, l in legs.items()}},
        }
        rec["config"]["build_id"] = _lib.build_id()
        emit(rec, result_fd, compact_sharded, args, "_n%d" % world)
    dist.barrier()
    dist.destroy_process_group()


def main():
    process_env()
    args = parse_args()
    args.full = args.full or args.detail
    if args.pmc_child:
        import torch  # noqa: F401
        return pmc_child(args)
    launched = "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not launched:
        self_launch(args.gpus)                                 # does not return

    # stdout carries exactly one JSON line: libraries that chat on fd 1 (RCCL prints a version banner
    # there at init) are pointed at stderr, the result is written to the saved descriptor
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (MI355X); there is no CPU path")
    if args.force_collectives:
        args.force_dist = True
    if world > 1 or args.force_dist:
        run_sharded(args, result_fd, world, rank, local_rank)
    else:
        run_single(args, result_fd)


if __name__ == "__main__":
    main()

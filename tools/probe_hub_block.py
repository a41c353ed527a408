"""Probe: the dense hub-to-hub block over forced hub counts on the drop-in headline (Reddit-like, D = 64, GNNA.SAG through
the module) -- the measurement behind kDenseEdgeSeconds / kDenseChunkSeconds / kDenseLaunchSeconds (csrc/gnna_agg.hip).

    python tools/probe_hub_block.py scan [H,H:T,...] [steps]
        one JSON line per hub count: the step by HIP events (min / median / max of `steps` calls, default 30).  H = 0: no
        block (GNNA_DENSE_BLOCK=0); H = -1: the rule's own choice; any other H: GNNA_DENSE_BLOCK=2 with the degree of
        the H-th highest-degree node as GNNA_DENSE_BLOCK_THETA (the library trims hub counts just beyond a whole round of
        workgroups and says what it took on stderr: GNNA_DENSE_BLOCK_LOG=1 is set).  H:T forces T = 32 or 64 destination
        ranks per workgroup as well (GNNA_DENSE_BLOCK_TILE); without it the library's own geometry is taken.  The default
        list runs past 1.25 rounds of workgroups on 256 compute units.
    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/probe_hub_block.py scan ...
    python tools/probe_hub_block.py kernels DIR/**/*kernel_trace.csv
        per-kernel times of that scan: hub_block_kernel by its padded hub count and tile height (read off the kernel's
        name), each with the hub_split_kernel and the sweep_kernel launch in front of it; the sweeps that no
        hub_block_kernel follows are the legs without a block."""
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_HUBS = "0,2048,4096,6144,8192,10240,12288,16384,-1,0"


def scan(hubs, steps):
    import torch
    import bench
    from gnnadvisor_osdi21_amd import _lib
    dev = torch.device("cuda", 0)
    os.environ["GNNA_DENSE_BLOCK_LOG"] = "1"
    os.environ["GNNA_DENSE_BLOCK"] = "0"
    w = bench.Workload("reddit-like", 64, dev, lifecycle="dropin", calibrate=False)
    g = w.g
    degs = torch.sort(g.row_pointers[1:] - g.row_pointers[:-1], descending=True).values.cpu()
    first = None
    for H, tile in hubs:
        theta = 0 if H <= 0 else int(degs[min(H, degs.numel()) - 1])
        os.environ["GNNA_DENSE_BLOCK"] = "0" if H == 0 else ("1" if H < 0 else "2")
        os.environ["GNNA_DENSE_BLOCK_THETA"] = str(theta) if H > 0 else ""
        os.environ["GNNA_DENSE_BLOCK_TILE"] = str(tile) if H > 0 and tile else ""
        w.GNNA.forget_graph(g.column_index)
        before = _lib.runtime_counters()
        for _ in range(6):                      # the module prepares a graph that has stood still for three calls
            w.step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record()
            w.step()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        after = _lib.runtime_counters()
        y = w.out
        if first is None:
            first = y.clone()
        print(json.dumps({"H_target": H, "tile_forced": tile, "theta": theta, "hubs_at_theta": int((degs >= theta).sum()) if H > 0 else 0,
                          "ms_min": ms[0], "ms_median": statistics.median(ms), "ms_max": ms[-1],
                          "dense_builds": after["dense_block_builds"] - before["dense_block_builds"],
                          "dense_launches": after["dense_block_launches"] - before["dense_block_launches"],
                          "sweep_launches": after["sweep_launches"] - before["sweep_launches"],
                          "max_abs_diff_vs_first": float((y - first).abs().max()), "max_abs_first": float(first.abs().max()),
                          "phases": _lib.last_num_phases(), "ps": w.ps}), flush=True)


def kernels(paths):
    rows = []
    for path in paths:
        with open(path) as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                kind = "hub" if "hub_block_kernel" in name else "split" if "hub_split_kernel" in name else "sweep" if "sweep_kernel" in name else None
                if kind is None:
                    continue
                wg = max(1, int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1))
                m = re.search(r"hub_block_kernel<\s*\d+\s*,\s*(\d+)", name)
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind,
                             int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) // wg, int(m.group(1)) if m else 32))
    rows.sort()
    legs = {}                                   # (padded hub count, tile) of hub_block_kernel ((0, 0): no block) -> ([sweep us], [hub us], [split us])
    pending = split = None
    for start, end, kind, groups, tile in rows:
        us = (end - start) / 1e3
        if kind == "split":
            split = us
        elif kind == "sweep":
            if pending is not None:
                legs.setdefault((0, 0), ([], [], []))[0].append(pending)
            pending = us
        else:
            leg = legs.setdefault((groups * tile, tile), ([], [], []))
            if pending is not None:
                leg[0].append(pending)
            leg[1].append(us)
            if split is not None:
                leg[2].append(split)
            pending = split = None
    if pending is not None:
        legs.setdefault((0, 0), ([], [], []))[0].append(pending)
    for key in sorted(legs):
        sweep, hub, splits = legs[key]
        line = {"H_pad": key[0], "tile": key[1], "hub_workgroups": key[0] // key[1] if key[1] else 0, "launches": len(sweep),
                "sweep_us_median": round(statistics.median(sweep), 2) if sweep else None,
                "sweep_us_min": round(min(sweep), 2) if sweep else None}
        if hub:
            line.update({"hub_us_median": round(statistics.median(hub), 2), "hub_us_min": round(min(hub), 2),
                         "hub_us_max": round(max(hub), 2)})
        if splits:
            line.update({"split_us_median": round(statistics.median(splits), 2), "split_us_min": round(min(splits), 2)})
        print(json.dumps(line))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "kernels":
        kernels(sys.argv[2:])
    elif len(sys.argv) >= 2 and sys.argv[1] == "scan":
        scan([(int(v.split(":")[0]), int(v.split(":")[1]) if ":" in v else 0)
              for v in (sys.argv[2] if len(sys.argv) > 2 else DEFAULT_HUBS).split(",")],
             int(sys.argv[3]) if len(sys.argv) > 3 else 30)
    else:
        sys.exit(__doc__)

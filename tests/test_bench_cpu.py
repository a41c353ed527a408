"""bench.py host logic that needs no GPU: the driver's contract (defaults, the self-launch command for
`--gpus N`), the byte models of SURVEY.md 8(d), and the bookkeeping that turns a rocprofv3 counter CSV into
per-step traffic (dispatch order, calibration copies)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_defaults_follow_the_driver_contract():
    a = bench.parse_args([])
    assert a.gpus == 1 and a.steps > 0 and a.warmup > 0 and a.dim == 64 and a.config == "reddit-like"
    a = bench.parse_args(["--gpus", "8", "--steps", "5", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (8, 5, 2) and a.backend == "nccl" and a.exchange == "auto"
    # N-rank line: the weak-scaling headline plus (with --full) the strong-scaling and (at 8 ranks) config-5 legs by default
    assert a.scaling == "strong,config5" and not a.config5_leg and a.config5_scale == 1.0
    # a plain run measures the headline only and writes no outputs; --full adds the rest
    assert not a.full and not a.detail and a.dump_outputs == ""
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_whole_or_a_seeded_sample_of_rows(tmp_path):
    import numpy as np
    import torch
    small = torch.arange(12 * 4, dtype=torch.float32).reshape(12, 4)
    bench.dump_outputs(str(tmp_path / "a"), {"aggregated": small})
    assert sorted(os.listdir(tmp_path / "a")) == ["aggregated.npy"]
    got = np.load(tmp_path / "a" / "aggregated.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())
    # larger than the limit: a fixed sample of rows (the same for the same shape) and the row ids beside it
    big = torch.randn(50000, 64, generator=torch.Generator().manual_seed(3))
    limit = 1 << 20
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"aggregated": big}, limit=limit)
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["aggregated.npy", "aggregated_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= limit
    rows, vals = np.load(tmp_path / "b" / "aggregated_rows.npy"), np.load(tmp_path / "b" / "aggregated.npy")
    assert rows.dtype == np.float64 and vals.dtype == np.float32 and len(rows) == len(vals) > 1000
    assert np.all(np.diff(rows) > 0) and rows[-1] < 50000
    assert np.array_equal(vals, big.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "c" / "aggregated_rows.npy"))


def test_kernel_labels_name_what_ran():
    class W:
        launches, phases = 1, 8
    assert "sliced schedule" in bench.kernel_label(W)
    W.phases = 1
    assert bench.kernel_label(W) == "stream_kernel"
    W.calls = 5
    assert "5 library calls" in bench.kernel_label(W)
    W.calls, W.launches = 1, 4
    assert "4 launches" in bench.kernel_label(W)


def test_gpus_n_launches_n_ranks_on_localhost(monkeypatch):
    seen = {}

    def fake_execv(path, argv):
        seen["path"], seen["argv"] = path, list(argv)
        raise SystemExit(0)
    monkeypatch.setattr(os, "execv", fake_execv)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "3"])
    with pytest.raises(SystemExit):
        bench.self_launch(4)
    argv = seen["argv"]
    assert seen["path"] == sys.executable and argv[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in argv and "--nproc-per-node=4" in argv
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(argv[argv.index("--master-port") + 1]) < 65536
    tail = argv[argv.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "4", "--steps", "7", "--warmup", "3"]      # the ranks get the caller's flags unchanged


def test_byte_models():
    nnz, n, parts, dim = 114623790, 232965, 1901647, 64
    assert bench.gather_model_bytes(nnz, n, parts, dim) == nnz * 260 + n * 260 + parts * 8 == 29877969476
    assert bench.compulsory_bytes(nnz, n, n, dim) == nnz * 4 + (n + 1) * 4 + 2 * n * dim * 4


def test_counter_rows_are_split_by_workload_and_calibrated_on_the_last_copies():
    manifest = {"workloads": [{"warmup": 2, "steps": 3, "launches_per_step": 1, "phases": 8},
                              {"warmup": 1, "steps": 3, "launches_per_step": 2, "phases": 2}],
                "calib_copies": 3, "calib_gathers": 2}
    rows = []

    def add(kernel, value):
        rows.append({"Dispatch_Id": str(len(rows) + 1), "Kernel_Name": kernel, "Counter_Name": "FETCH_SIZE",
                     "Counter_Value": str(value)})
    add("__amd_rocclr_copyBuffer", 7.0)                       # host-to-device transfers of the set-up: not calibration
    add("slice_count_kernel", 999.0)
    for v in (50.0, 70.0, 100.0, 100.0, 100.0):               # workload 0 (drop-in): two settling calls + 3 steady steps
        add("stream_kernel", v)
    add("__amd_rocclr_copyBuffer", 9.0)
    for v in (1.0, 1.0, 10.0, 20.0, 10.0, 20.0, 10.0, 20.0):  # workload 1: two launches per step
        add("sweep_kernel", v)
    for _ in range(3):
        add("__amd_rocclr_copyBuffer", 524288.0)              # the 1 GiB calibration copies (KiB, half-counted)
    for _ in range(2):
        add("stream_kernel", 600000.0)                        # the read-only row-gather calibration: the child's last aggregations
    per_step, copies, gathers = bench.split_counters(manifest, rows, "FETCH_SIZE")
    assert per_step == [100.0, 30.0]
    assert copies == [524288.0] * 3 and gathers == [600000.0] * 2
    assert bench.CALIB_BYTES / (1024.0 * sum(copies) / len(copies)) == 2.0
    # a child whose dispatch count does not match the schedule is not trusted
    short, _, _ = bench.split_counters(manifest, [r for r in rows if r["Kernel_Name"] != "sweep_kernel"][:-1], "FETCH_SIZE")
    assert None in short


def test_roofline_frac_definition_is_frozen():
    """`roofline.frac` = SURVEY 8(d) algorithmic bytes / kernel time / ceiling, ceiling = 34.5 TB/s (aggregate L2) when the
    gathered source matrix is < 256 MiB, 8 TB/s (HBM) otherwise.  ONE formula (VERDICT r4 task 4: the definition changed in
    every round 1-4); this test fails if it changes again.  Round 4's driver record (sweep kernel 1.3456 ms on the
    Reddit-like headline, 29.871 GB) re-derives to 0.643."""
    assert bench.roofline_ceiling(232965 * 64 * 4) == ("l2", 34500.0)                 # 59.6 MB: Infinity-Cache resident
    assert bench.roofline_ceiling(2449029 * 64 * 4) == ("hbm", 8000.0)                # 627 MB
    assert bench.roofline_ceiling((256 << 20) - 1)[0] == "l2" and bench.roofline_ceiling(256 << 20)[0] == "hbm"
    alg = bench.gather_model_bytes(114623790, 232965, 1008217, 64)
    assert alg == 114623790 * 260 + 232965 * 260 + 1008217 * 8
    f = bench.roofline_frac(alg, 1.3456e-3, 232965 * 64 * 4)
    assert abs(f - alg / 1.3456e-3 / 34.5e12) < 1e-12 and abs(f - 0.6435) < 1e-3
    assert abs(bench.roofline_frac(32.8e9, 3.41e-3, 2449029 * 64 * 4) - 32.8e9 / 3.41e-3 / 8e12) < 1e-12
    # faster kernel -> larger frac, nothing else enters
    assert bench.roofline_frac(alg, 1.0e-3, 232965 * 64 * 4) > f


def test_roofline_record_follows_the_definition_and_keeps_measured_terms_beside_it():
    class G:
        nnz, num_nodes = 114623790, 232965

    class W:
        g, P, dim, launches, phases, swept = G, 1008217, 64, 1, 16, True
    traffic = {"bytes_per_step": 3.66e9, "l2_requests_per_step": 228.3e6, "l2_hit_rate": 0.872}
    floor = {"ms": 1.18, "what": "bare stream"}
    rec = bench.roofline_record(W, 1.3456, 0.021, traffic, floor)
    alg = bench.gather_model_bytes(G.nnz, G.num_nodes, W.P, 64)
    assert rec["bound"] == "hbm" and rec["ceiling"] == "l2" and rec["peak"] == 34500.0 and rec["unit"] == "GB/s"
    assert rec["achieved"] == alg / 1.3456e-3 / 1e9 and rec["frac"] == rec["achieved"] / rec["peak"]
    assert rec["frac"] == bench.roofline_frac(alg, 1.3456e-3, G.num_nodes * 64 * 4)
    assert rec["traffic"] == 3.66e9 and abs(rec["frac_hbm_measured"] - 3.66e9 / 1.3456e-3 / 8e12) < 1e-9
    assert abs(rec["frac_l2"] - 228.3e6 * 128 / 1.3456e-3 / 34.5e12) < 1e-9 and abs(rec["l2_requests_per_edge"] - 1.99) < 0.01
    assert rec["floor_ms"] == 1.18 and abs(rec["frac_of_floor"] - 1.18 / 1.3456) < 1e-12
    assert abs(rec["traffic_over_compulsory"] - 3.66e9 / bench.compulsory_bytes(G.nnz, G.num_nodes, G.num_nodes, 64)) < 1e-9
    # an HBM-resident workload is quoted against the HBM peak
    class G2:
        nnz, num_nodes = 123718280, 2449029

    class W2:
        g, P, dim, launches, phases = G2, 3000000, 64, 1, 4
    r2 = bench.roofline_record(W2, 3.41, 0.1, None)
    assert r2["ceiling"] == "hbm" and r2["peak"] == 8000.0 and r2["frac"] == r2["achieved"] / 8000.0
    # without counters nothing is invented
    rec0 = bench.roofline_record(W, 1.3456, 0.021, {"error": "rocprofv3 not found"})
    assert rec0["traffic"] is None and rec0["frac_l2"] is None and rec0["frac_hbm_measured"] is None
    assert rec0["frac"] == rec["frac"] and rec0["traffic_error"] == "rocprofv3 not found"


def _canned():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "bench_full_record.json")) as f:
        return json.load(f)


def test_the_line_is_short_strict_json_and_carries_the_contract(tmp_path):
    """VERDICT r5 task 1: round 5's line was 34.7 KB and the driver (8 KB tail) could not parse it.  The line is built from
    the full record (here: round 5's own, 34.7 KB) by `compact_single`; everything else goes to the detail file."""
    import json
    rec = _canned()
    assert len(json.dumps(rec)) > 30000
    rec["config"]["verification"]["max_err_over_abs_ref"] = float("nan")          # a NaN must not reach the line as a token
    rec["roofline"]["floor_ms"] = float("inf")
    line = bench.compact_single(rec, "gpurun_out/bench_detail.json")
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(text) < bench.LINE_TARGET < bench.LINE_LIMIT == 8000
    back = json.loads(text, parse_constant=lambda tok: pytest.fail("non-strict token " + tok))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "verified"):
        assert key in back, key
    assert back["vs_baseline"] is None and back["dtype"] == "f32" and back["config"]["workload"].startswith("reddit-like")
    r = back["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5
    assert r["kernel"] == "sweep_kernel" and r["traffic"] > 0 and r["algorithmic_bytes"] == pytest.approx(29870822036, rel=1e-6)
    assert back["cpu_baseline"]["value"] > 0 and back["cpu_baseline"]["cores"] == 16 and back["cpu_baseline"]["kind"] == "port"
    assert abs(back["value"] - rec["value"]) / rec["value"] < 1e-6
    assert not any(isinstance(v, (dict, list)) for v in back["config"].values())       # flat scalars only
    assert all(not isinstance(v, (dict, list)) and (not isinstance(v, str) or len(v) <= 160) for v in r.values())
    assert "other_workloads" not in r and r.get("floor_ms") is None


def test_emit_writes_the_detail_file_and_one_line(tmp_path, capfd):
    import json

    class A:
        detail_file = str(tmp_path / "d" / "detail.json")
    rd, wr = os.pipe()
    bench.emit(_canned(), wr, bench.compact_single, A)
    os.close(wr)
    out = os.read(rd, 1 << 16).decode()
    os.close(rd)
    assert out.endswith("\n") and out.count("\n") == 1 and len(out) < bench.LINE_TARGET
    full = json.load(open(A.detail_file))
    assert "other_workloads" in full["roofline"] and len(full["roofline"]["other_workloads"]) >= 9
    assert "line" in capfd.readouterr().err


def test_a_plain_run_writes_no_detail_file(tmp_path, monkeypatch):
    import json
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))           # (where the default detail file would go)
    rd, wr = os.pipe()
    bench.emit(_canned(), wr, bench.compact_single, bench.parse_args(["--steps", "20", "--warmup", "5"]))
    os.close(wr)
    line = json.loads(os.read(rd, 1 << 16).decode())
    os.close(rd)
    assert os.listdir(tmp_path) == [] and "detail_file" not in line["config"]


def test_the_n_rank_line_is_short_too():
    import json
    legs = {n: {"value": 1e11, "unit": "edges/s", "ms_per_step": 9.5, "scaling": n, "verified": True, "exchange": "halo"}
            for n in ("weak", "strong", "config5")}
    rec = {"metric": "m", "value": 6.5e11, "unit": "edges/s", "n_gpus": 8, "steps": 20, "warmup": 5, "ms_per_step": 1.41,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "verified": True,
           "config": {"workload": "reddit-like", "world_size": 8, "backend": "nccl", "communicator_ranks_counted": 8,
                      "ranks": ["rank %d: AMD Instinct MI355X (cuda:%d)" % (i, i) for i in range(8)], "values": legs,
                      "legs": {n: {"kernel": {"x": list(range(400))}} for n in legs}, "failed_legs": {},
                      "exchange_only_ms_per_rank": [1.0] * 8, "parallelism": "dst-range shards x8 + halo " * 20,
                      "tuning": {"a": 1}, "exchange": "halo"},
           "roofline": {"bound": "hbm", "ceiling": "hbm", "peak": 8000.0, "unit": "GB/s", "achieved": 9000.0, "frac": 1.125,
                        "kernel": "stream_kernel (x)", "kernel_ms": 1.2, "traffic": None,
                        "per_leg_kernels": {n: {"x": list(range(300))} for n in legs}}}
    line = bench.compact_sharded(rec, "gpurun_out/bench_detail_n8.json")
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(text) < bench.LINE_TARGET
    assert line["config"]["values"]["config5"]["value"] == 1e11 and line["config"]["communicator_ranks_counted"] == 8
    assert "legs" not in line["config"] and "per_leg_kernels" not in line["roofline"] and line["roofline"]["traffic"] is None


def test_importing_bench_does_not_touch_the_process_environment():
    """Round 6: `import bench` used to put OMP_PROC_BIND=close into the environment; in the pytest process (this module imports
    bench) libgomp then bound the main thread to one core and every native host pass ran its threads there.  The environment of
    a bench PROCESS is set by bench.main() only."""
    import subprocess
    import sys
    code = ("import os, sys; sys.path.insert(0, %r); before = dict(os.environ); import bench; "
            "changed = {k for k in set(os.environ) | set(before) if os.environ.get(k) != before.get(k)}; "
            "assert not changed, changed; bench.process_env(); assert os.environ['OMP_PROC_BIND'] == 'close'; print('ok')" % ROOT)
    env = {k: v for k, v in os.environ.items() if not k.startswith("OMP_")}
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr[-1500:]

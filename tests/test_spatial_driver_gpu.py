"""graph_main.py --model schnet on the GPU, in fresh child processes: the driver builds the graph of every mini-batch from the batch's
positions, trains SchNetInteraction layers and prints what the other models print; the fused and the composed graph construction
give the same structure sizes and train alike from one seed; a --model gin run prints what it printed before.

Fused against composed: the two runs multiply and add the same numbers over the same edges -- the structures are identical bit for
bit -- so the loss after the first epoch agrees within 1e-4 relative and the loss after the last within 1e-3 * max(1, |loss|): the
bounds test_edgefeat_driver_gpu.py puts on its fused and composed runs."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = ["--num_graphs", "64", "--graph_nodes", "4,24", "--batch_graphs", "16", "--dim", "8", "--hidden", "16", "--classes", "3"]
SCHNET = SMALL + ["--model", "schnet", "--cutoff", "1.5", "--num_gaussians", "8", "--readout", "mean,max", "--seed", "3", "--lr", "0.01",
                  "--num_epoches", "2", "--verbose_mode", "True"]


def drive(argv):
    run = subprocess.run([sys.executable, "-m", "gnnadvisor_osdi21_amd.graph_main"] + argv, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout


def _number(out, label):
    return float(re.search(re.escape(label) + r" (-?[0-9.]+(?:e-?[0-9]+)?|nan|inf)", out).group(1))


@pytest.mark.parametrize("cap", [None, "4"])
def test_schnet_runs_and_fused_and_composed_graphs_train_alike(cap):
    seen = {}
    for fused in ("True", "False"):
        out = drive(SCHNET + ["--fused_graph", fused] + (["--max_neighbors", cap] if cap else []))
        print(out)
        assert out.count("Time (ms): ") == 1 and _number(out, "Time (ms):") > 0
        sizes = re.search(r"# radius graph: cutoff 1.5, (.*), built per step \((fused|composed)\): (\d+) nodes (\d+) edges per epoch", out)
        assert sizes and sizes.group(2) == ("fused" if fused == "True" else "composed")
        assert sizes.group(1) == ("at most 4 neighbours" if cap else "no cap")
        first, final = _number(out, "# loss after 1 epoch:"), _number(out, "# final loss:")
        assert first == first and final == final and abs(first) < float("inf") and abs(final) < float("inf")          # finite
        seen[fused] = (int(sizes.group(3)), int(sizes.group(4)), first, final)
    a, b = seen["True"], seen["False"]
    assert a[:2] == b[:2] and a[1] > a[0]                      # the same structure sizes
    assert abs(a[2] - b[2]) <= 1e-4 * abs(b[2])
    assert abs(a[3] - b[3]) <= 1e-3 * max(1.0, abs(b[3]))


def test_a_gin_run_prints_what_it_printed_before():
    out = drive(SMALL + ["--model", "gin", "--num_epoches", "2", "--verbose_mode", "True", "--seed", "3"])
    lines = [line for line in out.splitlines() if line]
    assert re.fullmatch(r"# 64 graphs, \d+ nodes, \d+ edges, 4 batches of up to 16 graphs, readout sum \(fused\)", lines[0])
    assert re.fullmatch(r"# loss after 1 epoch: \d+\.\d{6}", lines[1]) and re.fullmatch(r"# final loss: \d+\.\d{6}", lines[2])
    assert re.fullmatch(r"Time \(ms\): \d+\.\d{3}", lines[3]) and len(lines) == 4
    assert "radius graph" not in out

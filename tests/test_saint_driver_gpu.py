"""The driver on GraphSAINT random-walk subgraphs: main.py --saint_roots R --walk_length L [--saint_steps S] [--saint_coverage T]."""
import math

import pytest
import torch

from gnnadvisor_osdi21_amd import main as driver

pytestmark = pytest.mark.gpu

SMALL = ["--synthetic", "cora-like", "--scale", "0.5", "--dim", "16", "--hidden", "16", "--classes", "4"]
SAINT = ["--saint_roots", "64", "--walk_length", "2", "--saint_steps", "4"]


def _run(extra, seed=3):
    cap = {}
    torch.manual_seed(seed)
    assert driver.main(SMALL + SAINT + extra, capture=cap) == 0
    return cap


@pytest.mark.parametrize("model", ["gcn", "sage"])
def test_two_runs_start_alike_and_the_loss_falls(model, capsys):
    a = _run(["--model", model, "--num_epoches", "5"])
    assert "Time (ms):" in capsys.readouterr().out
    b = _run(["--model", model, "--num_epoches", "1"])
    print(f"{model}: first loss {a['first_loss']:.6f}, final loss {a['final_loss']:.6f}")
    assert math.isfinite(a["first_loss"]) and a["first_loss"] == b["first_loss"]
    assert a["final_loss"] < a["first_loss"]
    sub = a["sampler"].sample(0)
    assert sub.num_graphs == 1 and 1 <= sub.num_nodes <= 3 * 64 and sub.node_weight is None      # 64 walks of 3 nodes at most


def test_coverage_weighs_the_loss(capsys):
    cap = _run(["--model", "gcn", "--num_epoches", "1", "--saint_coverage", "4"])
    assert math.isfinite(cap["first_loss"]) and math.isfinite(cap["final_loss"])
    sampler = cap["sampler"]
    assert sampler.node_weight is not None and int(sampler.node_count.max()) <= 4
    sub = sampler.sample(0)
    assert sub.node_weight.numel() == sub.num_nodes and float(sub.node_weight.min()) > 0


@pytest.mark.parametrize("model, extra", [("gin", []), ("gat", ["--fused_attention", "True"]), ("gatv2", ["--fused_attention", "True"]),
                                          ("transformer", ["--fused_attention", "True"]), ("pna", []), ("gen", [])])
def test_every_model_that_takes_a_graph_batch_runs(model, extra):
    cap = _run(["--model", model, "--num_epoches", "1"] + extra)
    assert math.isfinite(cap["first_loss"]) and math.isfinite(cap["final_loss"])


def test_fanout_together_with_saint_roots_exits_with_the_stated_message():
    with pytest.raises(SystemExit, match="--saint_roots does not go with --fanout"):
        driver.main(SMALL + SAINT + ["--model", "sage", "--fanout", "5,5"])

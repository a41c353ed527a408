"""The driver on sampled mini-batches: main.py --model sage --fanout ... --batch_size ..."""
import math

import pytest
import torch

from gnnadvisor_osdi21_amd import main as driver

pytestmark = pytest.mark.gpu

SMALL = ["--model", "sage", "--synthetic", "cora-like", "--scale", "0.5", "--dim", "16", "--hidden", "16", "--classes", "4"]


def test_minibatch_training_runs(capsys):
    cap = {}
    rc = driver.main(SMALL + ["--fanout", "5,5", "--batch_size", "256", "--num_epoches", "2"], capture=cap)
    assert rc == 0 and "Time (ms):" in capsys.readouterr().out
    assert math.isfinite(cap["final_loss"]) and math.isfinite(cap["first_loss"])


def test_full_fanout_one_batch_starts_from_the_full_graph_loss():
    full, sampled = {}, {}
    torch.manual_seed(3)
    assert driver.main(SMALL + ["--num_epoches", "1"], capture=full) == 0
    n = full["dataset"].num_nodes
    torch.manual_seed(3)
    assert driver.main(SMALL + ["--num_epoches", "1", "--fanout", "-1,-1", "--batch_size", str(n)], capture=sampled) == 0
    assert abs(sampled["first_loss"] - full["first_loss"]) <= 1e-4 * abs(full["first_loss"])

"""main.py --model gen on an MI355X: two GENConv layers train in the driver's loop for 3 epochs -- on the full graph, with
--directed True, on sampled blocks and with a learnt temperature.  The loss stays finite and falls; a learnt temperature moves."""
import math

import pytest
import torch

from gnnadvisor_osdi21_amd import main as driver

pytestmark = pytest.mark.gpu
ARGV = ["--model", "gen", "--synthetic", "cora-like", "--scale", "0.5", "--dim", "64", "--hidden", "16", "--classes", "7",
        "--verbose_mode", "True", "--num_epoches", "3"]


def _run(extra, capsys):
    run = {}
    torch.manual_seed(3)
    assert driver.main(ARGV + extra, capture=run) == 0
    assert "Time (ms):" in capsys.readouterr().out
    first, final = run["first_loss"], run["final_loss"]
    print(f"{extra}: first loss {first:.6f}, final loss {final:.6f}")
    assert math.isfinite(first) and math.isfinite(final) and final < first, (first, final)
    return run


@pytest.mark.parametrize("extra", [[], ["--directed", "True"], ["--fanout", "5,5", "--batch_size", "64"]],
                         ids=["symmetric", "directed", "blocks"])
def test_driver_trains_gen(capsys, extra):
    run = _run(extra, capsys)
    model = run["model"]
    assert type(model.conv1).__name__ == "GENConv" and type(model.conv2).__name__ == "GENConv"
    # a fixed temperature is a buffer at the value asked for
    assert dict(model.conv1.aggr.named_parameters()) == {} and model.conv1.aggr.t.tolist() == [1.0]
    if "--directed" in extra:
        assert run["inputInfo"].directed and run["inputInfo"]._edge_arrays().get("transposed") is not None
    if "--fanout" in extra:
        assert run["sampler"].fanouts == [5, 5]


def test_a_learnt_temperature_moves(capsys):
    run = _run(["--learn_t", "True", "--softmax_t", "0.5"], capsys)
    for conv in (run["model"].conv1, run["model"].conv2):
        t = conv.aggr.t
        assert isinstance(t, torch.nn.Parameter) and t.shape == (1,)
        assert math.isfinite(float(t)) and float(t) != 0.5, "the temperature has not changed after training"

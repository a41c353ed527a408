"""graph_main.py on the GPU: both models run, the driver prints its time line, and training lowers the loss."""
import pytest

from gnnadvisor_osdi21_amd import graph_main

pytestmark = pytest.mark.gpu

SMALL = ["--num_graphs", "64", "--graph_nodes", "4,24", "--batch_graphs", "16", "--dim", "8", "--hidden", "16", "--classes", "3"]


@pytest.mark.parametrize("model, readout", [("gcn", "mean"), ("gin", "sum,max"), ("gin", "sum,mean,max,min")])
def test_both_models_run_and_print_the_time_line(model, readout, capsys):
    assert graph_main.main(SMALL + ["--model", model, "--readout", readout, "--num_epoches", "2"]) == 0
    out = capsys.readouterr().out
    assert out.count("Time (ms): ") == 1 and float(out.split("Time (ms): ")[1].split()[0]) > 0


@pytest.mark.parametrize("fused", ["True", "False"])
def test_the_loss_falls(fused):
    seen = {}
    args = SMALL + ["--model", "gin", "--readout", "mean,max", "--num_epoches", "30", "--seed", "3", "--lr", "0.01", "--fused_readout", fused]
    assert graph_main.main(args, capture=seen) == 0
    print(seen)
    assert seen["final_loss"] == seen["final_loss"] and seen["final_loss"] < seen["first_loss"]

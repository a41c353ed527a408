"""graph_main.py with --attention_readout on the GPU: both gate widths run next to the --readout statistics, the driver prints its
time line, and training lowers the loss with the fused and with the composed readout."""
import pytest

from gnnadvisor_osdi21_amd import graph_main
from test_pool_driver_gpu import SMALL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", ["True", "False"])
@pytest.mark.parametrize("gate", ["scalar", "channel"])
def test_it_runs_prints_one_time_line_and_the_loss_falls(gate, fused, capsys):
    seen = {}
    args = SMALL + ["--model", "gin", "--readout", "mean,max", "--attention_readout", gate, "--num_epoches", "30", "--seed", "3",
                    "--lr", "0.01", "--fused_readout", fused]
    assert graph_main.main(args, capture=seen) == 0
    out = capsys.readouterr().out
    assert out.count("Time (ms): ") == 1 and float(out.split("Time (ms): ")[1].split()[0]) > 0
    print(seen)
    assert seen["final_loss"] == seen["final_loss"] and seen["final_loss"] < seen["first_loss"]

"""graph_main.py with hierarchical pooling on the GPU: --pool topk and --pool sag train, and --pool none is the driver as it was."""
import pytest

from gnnadvisor_osdi21_amd import graph_main

pytestmark = pytest.mark.gpu

SMALL = ["--num_graphs", "64", "--graph_nodes", "4,24", "--batch_graphs", "16", "--dim", "8", "--hidden", "16", "--classes", "3"]


@pytest.mark.parametrize("model", ["gcn", "gin"])
@pytest.mark.parametrize("pool", ["topk", "sag"])
def test_pooling_trains(pool, model, capsys):
    seen = {}
    args = SMALL + ["--model", model, "--pool", pool, "--readout", "sum,max", "--num_layers", "3", "--num_epoches", "2", "--seed", "3",
                    "--verbose_mode", "True"]
    assert graph_main.main(args, capture=seen) == 0
    out = capsys.readouterr().out
    print(out, seen)
    assert out.count("Time (ms): ") == 1 and float(out.split("Time (ms): ")[1].split()[0]) > 0
    # three levels: the rows and edges fall from level to level
    line = [l for l in out.splitlines() if l.startswith("# pooling %s at ratio 0.5 (fused)" % pool)]
    assert len(line) == 1
    levels = [tuple(int(v) for v in part.split() if v.isdigit()) for part in line[0].split(": ")[1].split(", ")]
    assert len(levels) == 3 and levels[0][0] > levels[1][0] > levels[2][0] > 0 and levels[0][1] > levels[1][1] >= levels[2][1]
    assert seen["final_loss"] == seen["final_loss"] and seen["final_loss"] < seen["first_loss"]


def test_the_composed_pooling_sees_the_same_levels(capsys):
    lines = {}
    for fused in ("True", "False"):
        args = SMALL + ["--pool", "topk", "--num_epoches", "1", "--seed", "5", "--verbose_mode", "True", "--fused_pool", fused]
        assert graph_main.main(args) == 0
        out = capsys.readouterr().out
        lines[fused] = [l.split("level by level: ")[1] for l in out.splitlines() if "level by level" in l]
    assert len(lines["True"]) == 1 and lines["True"] == lines["False"]


def test_pool_none_is_the_driver_as_it_was(capsys):
    """Without --pool, and with --pool none, the driver builds the same model from the same random numbers -- no parameter is added
    and none is drawn in another order -- and prints the same lines: no line about pooling, and the same losses up to the order of
    the float atomics of the aggregation (a model drawn from other random numbers starts from another loss in the first
    decimals)."""
    args = graph_main.build_parser().parse_args(SMALL + ["--model", "gin", "--seed", "3"])
    assert sorted(graph_main.build_model(args, ("mean", "max")).state_dict()) == ["convs.0.weights", "convs.1.weights", "lin.bias", "lin.weight"]
    losses = []
    for extra in ([], ["--pool", "none"], ["--pool", "none", "--pool_ratio", "0.25"]):
        assert graph_main.main(SMALL + ["--model", "gin", "--readout", "mean,max", "--num_epoches", "2", "--seed", "3", "--verbose_mode",
                                        "True"] + extra) == 0
        out = capsys.readouterr().out
        assert "pooling" not in out and "level" not in out
        lines = [l for l in out.splitlines() if "loss" in l]
        assert [l.split(":")[0] for l in lines] == ["# loss after 1 epoch", "# final loss"]
        losses.append([float(l.split(":")[1]) for l in lines])
    print(losses)
    for other in losses[1:]:
        assert all(abs(a - b) <= 1e-4 * max(1.0, abs(a)) for a, b in zip(losses[0], other))

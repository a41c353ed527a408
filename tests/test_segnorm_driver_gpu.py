"""graph_main.py with per-graph normalisation on the GPU: --norm graph trains, fused and composed start from the same loss, and
--norm none is the driver as it was."""
import pytest

from gnnadvisor_osdi21_amd import _lib, graph_main

pytestmark = pytest.mark.gpu

SMALL = ["--num_graphs", "64", "--graph_nodes", "4,24", "--batch_graphs", "16", "--dim", "8", "--hidden", "16", "--classes", "3"]


@pytest.mark.parametrize("model", ["gcn", "gin"])
def test_graph_norm_trains(model, capsys):
    seen = {}
    args = SMALL + ["--model", model, "--norm", "graph", "--readout", "sum,max", "--num_epoches", "3", "--seed", "3", "--verbose_mode", "True"]
    assert graph_main.main(args, capture=seen) == 0
    out = capsys.readouterr().out
    print(out, seen)
    assert out.count("Time (ms): ") == 1 and float(out.split("Time (ms): ")[1].split()[0]) > 0
    assert out.count("# normalisation: GraphNorm after every conv layer (fused)") == 1
    assert seen["final_loss"] == seen["final_loss"] and seen["final_loss"] < seen["first_loss"]


def test_graph_norm_with_pooling_trains(capsys):
    seen = {}
    args = SMALL + ["--norm", "graph", "--pool", "topk", "--num_layers", "3", "--num_epoches", "2", "--seed", "4"]
    assert graph_main.main(args, capture=seen) == 0
    capsys.readouterr()
    assert seen["final_loss"] == seen["final_loss"] and seen["final_loss"] < seen["first_loss"]


def test_fused_and_composed_start_from_the_same_loss(capsys):
    """One epoch of the same model from the same random numbers: the two paths compute the same function, so the mean loss of the
    first epoch agrees to 1e-4 relative (the steps in between amplify the last bits of fp32, not more)."""
    first = {}
    for fused in ("True", "False"):
        seen = {}
        assert graph_main.main(SMALL + ["--norm", "graph", "--fused_norm", fused, "--num_epoches", "1", "--seed", "5", "--verbose_mode", "True"],
                               capture=seen) == 0
        out = capsys.readouterr().out
        assert ("(fused)" if fused == "True" else "(composed)") in out
        first[fused] = seen["first_loss"]
    print(first)
    assert abs(first["True"] - first["False"]) <= 1e-4 * abs(first["False"])


def test_norm_none_is_the_driver_as_it_was(capsys):
    """Without --norm, and with --norm none, the driver builds the same model from the same random numbers -- no module is created and
    no random number drawn -- and prints the same lines."""
    args = graph_main.build_parser().parse_args(SMALL + ["--model", "gin", "--seed", "3"])
    assert sorted(graph_main.build_model(args, ("mean", "max")).state_dict()) == ["convs.0.weights", "convs.1.weights", "lin.bias", "lin.weight"]
    args = graph_main.build_parser().parse_args(SMALL + ["--model", "gin", "--seed", "3", "--norm", "graph"])
    assert sorted(k for k in graph_main.build_model(args, ("mean",)).state_dict() if k.startswith("norms.")) == [
        "norms.%d.%s" % (k, name) for k in (0, 1) for name in ("bias", "mean_scale", "weight")]
    runs = []
    try:
        # (the deterministic schedule: the float atomics of the aggregation would let two runs of one model differ in the last bits)
        _lib.set_tuning(deterministic=1)
        for extra in ([], ["--norm", "none"], ["--norm", "none", "--fused_norm", "False"]):
            seen = {}
            assert graph_main.main(SMALL + ["--model", "gin", "--readout", "mean,max", "--num_epoches", "1", "--seed", "3", "--verbose_mode",
                                            "True"] + extra, capture=seen) == 0
            out = capsys.readouterr().out
            assert "normalisation" not in out
            runs.append((seen["first_loss"], [l.split(":")[0] for l in out.splitlines() if l.startswith("#")]))
    finally:
        _lib.reset_tuning()
    print(runs)
    assert runs[0][1] == runs[1][1] == runs[2][1]
    assert runs[0][0] == runs[1][0] == runs[2][0]              # to the bit


def test_the_refusals():
    with pytest.raises(SystemExit, match=r"--norm takes none or graph \(got 'layer'\)"):
        graph_main.main(SMALL + ["--norm", "layer"])
    with pytest.raises(SystemExit, match="is float32 only"):
        graph_main.main(SMALL + ["--norm", "graph", "--dtype", "bfloat16"])

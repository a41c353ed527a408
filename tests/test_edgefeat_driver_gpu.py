"""graph_main.py --model gine on the GPU: the driver runs, training lowers the loss, the fused and the composed edge-feature
aggregation train alike from one seed, and the edge features follow a pooling layer.

Fused against composed: the loss after the first epoch within 1e-4 relative (the bound test_segnorm_driver_gpu.py puts on its
fused and composed first epochs) and the loss after 30 more within 1e-3 * max(1, |loss|) (the bound test_driver_gpu.py puts on
the final losses of two runs that differ in summation order only)."""
import pytest

from gnnadvisor_osdi21_amd import graph_main

pytestmark = pytest.mark.gpu

SMALL = ["--num_graphs", "64", "--graph_nodes", "4,24", "--batch_graphs", "16", "--dim", "8", "--hidden", "16", "--classes", "3"]
GINE = SMALL + ["--model", "gine", "--edge_dim", "4", "--readout", "mean,max", "--seed", "3", "--lr", "0.01"]


def test_gine_trains_and_fused_and_composed_end_alike(capsys):
    seen = {}
    for fused in ("True", "False"):
        seen[fused] = {}
        assert graph_main.main(GINE + ["--num_epoches", "30", "--fused_edge", fused, "--verbose_mode", "True"], capture=seen[fused]) == 0
        out = capsys.readouterr().out
        assert out.count("Time (ms): ") == 1 and float(out.split("Time (ms): ")[1].split()[0]) > 0
        assert "# edge features: 4 per edge, GINEConv (%s)" % ("fused" if fused == "True" else "composed") in out
        run = seen[fused]
        print(fused, run)
        assert run["final_loss"] == run["final_loss"] and run["final_loss"] < run["first_loss"]          # finite, and lower
    a, b = seen["True"], seen["False"]
    assert abs(a["first_loss"] - b["first_loss"]) <= 1e-4 * abs(b["first_loss"])
    assert abs(a["final_loss"] - b["final_loss"]) <= 1e-3 * max(1.0, abs(b["final_loss"]))


def test_the_label_depends_on_the_edge_features():
    import torch
    args = graph_main.build_parser().parse_args(GINE)
    with_edges = graph_main.make_dataset(args, 4, 24, torch.device("cuda"))
    args.model, args.edge_dim = "gin", 0
    without = graph_main.make_dataset(args, 4, 24, torch.device("cuda"))
    assert with_edges.edge_attr.shape == (with_edges.column_index.numel(), 4) and without.edge_attr is None
    assert torch.equal(with_edges.x, without.x) and not torch.equal(with_edges.y, without.y)
    b = with_edges.batch(torch.arange(16, device="cuda"), directed=True)
    rev = None
    try:
        rev = b.reverse_edges()
    except Exception:                                                # (a batch whose structure is not symmetric has no such map)
        pass
    if rev is not None:
        assert not torch.equal(b.edge_attr[rev.long()], b.edge_attr), "e_ij must differ from e_ji"


@pytest.mark.parametrize("pool", ["topk", "sag"])
def test_the_edge_features_follow_the_pooling(pool, capsys):
    seen = {}
    assert graph_main.main(GINE + ["--pool", pool, "--num_layers", "3", "--num_epoches", "2", "--verbose_mode", "True"], capture=seen) == 0
    out = capsys.readouterr().out
    assert "level by level" in out and seen["final_loss"] == seen["final_loss"]

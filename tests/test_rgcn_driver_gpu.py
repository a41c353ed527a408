"""main.py --model rgcn on an MI355X: the two-layer R-GCN trains in the driver's loop, with and without renumbering."""
import re

import pytest
import torch

from gnnadvisor_osdi21_amd import main as driver
from gnnadvisor_osdi21_amd.relational import synthetic_edge_types

pytestmark = pytest.mark.gpu
ARGV = ["--model", "rgcn", "--synthetic", "cora-like", "--scale", "0.5", "--num_relations", "4", "--num_bases", "2",
        "--num_epoches", "2", "--verbose_mode", "True"]


def _run(extra, capsys):
    run = {}
    torch.manual_seed(3)
    assert driver.main(ARGV + extra, capture=run) == 0
    out = capsys.readouterr().out
    assert re.search(r"^Time \(ms\): \d+\.\d{3}$", out, flags=re.M), out[-2000:]
    first = float(re.search(r"# first loss: ([-\d.e+]+)", out).group(1))
    final = float(re.search(r"# final loss: ([-\d.e+]+)", out).group(1))
    assert final < first, (first, final)
    info, rel = run["inputInfo"], run["rel"]
    # the types belong to the CSR the kernels ran on
    assert rel.info is info and rel.edge_type.numel() == info.column_index.numel()
    assert torch.equal(rel.edge_type, synthetic_edge_types(info.row_pointers, info.column_index, 4, seed=0x52474E))
    assert rel._transposed is not None                      # built before the first epoch, for the second layer's dX
    assert isinstance(run["model"].conv1.coef, torch.nn.Parameter) and tuple(run["model"].conv1.coef.shape) == (4, 2)
    return run


def test_driver_trains_rgcn(capsys):
    run = _run([], capsys)
    assert not run["inputInfo"].reorder_status


def test_driver_trains_rgcn_on_the_renumbered_graph(capsys):
    run = _run(["--enable_rabbit", "True", "--force_rabbit", "True"], capsys)
    assert run["inputInfo"].reorder_status                  # the CSR was renumbered; the types were made after it


def test_driver_trains_rgcn_without_bases(capsys):
    run = {}
    argv = [a for a in ARGV]
    argv[argv.index("--num_bases") + 1] = "0"
    assert driver.main(argv, capture=run) == 0
    assert "Time (ms):" in capsys.readouterr().out
    assert not isinstance(run["model"].conv1.coef, torch.nn.Parameter) and tuple(run["model"].conv1.V.shape)[0] == 4

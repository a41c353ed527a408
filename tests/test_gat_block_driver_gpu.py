"""The driver on sampled mini-batches with the fused attention: main.py --model gat --fused_attention True --fanout ..."""
import math
import re

import pytest

from gnnadvisor_osdi21_amd import main as driver

pytestmark = pytest.mark.gpu

SMALL = ["--model", "gat", "--fused_attention", "True", "--synthetic", "cora-like", "--scale", "0.5", "--dim", "16", "--hidden", "16",
         "--classes", "4"]


def test_minibatch_gat_trains(capsys):
    cap = {}
    rc = driver.main(SMALL + ["--heads", "2", "--fanout", "5,5", "--batch_size", "256", "--num_epoches", "5", "--verbose_mode", "True"],
                     capture=cap)
    out = capsys.readouterr().out
    assert rc == 0 and "Time (ms):" in out
    first = float(re.search(r"# first loss: ([-\d.e+naif]+)", out).group(1))
    final = float(re.search(r"# final loss: ([-\d.e+naif]+)", out).group(1))
    assert math.isfinite(first) and math.isfinite(final) and math.isfinite(cap["first_loss"]) and math.isfinite(cap["final_loss"])
    assert final < first, (first, final)
    assert cap["sampler"].fanouts == [5, 5]

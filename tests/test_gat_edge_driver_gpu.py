"""main.py --model gat --fused_attention True --edge_dim 8: three epochs on the smallest synthetic graph, full-batch (fused,
directed, composed) and on sampled mini-batches, whose blocks take the edge features of their own edges; the loss must be finite
and falling.  Every run is a child process with a timeout."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--model", "gat", "--synthetic", "cora-like", "--scale", "0.5", "--dim", "16", "--hidden", "16", "--classes", "4",
         "--num_epoches", "3", "--verbose_mode", "True", "--edge_dim", "8", "--heads", "2"]


def _run(extra, falling=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-m", "gnnadvisor_osdi21_amd.main"] + SMALL + extra, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    out = done.stdout
    assert "Time (ms):" in out and "model='gat'" in out and "edge_dim=8" in out
    first = float(re.search(r"# first loss: ([-\d.e+naif]+)", out).group(1))
    final = float(re.search(r"# final loss: ([-\d.e+naif]+)", out).group(1))
    assert math.isfinite(first) and math.isfinite(final), (first, final)
    if falling:
        assert final < first, (first, final)
    return out


@pytest.mark.parametrize("extra", [
    ["--fused_attention", "True"],
    ["--fused_attention", "True", "--directed", "True"],
    ["--fused_attention", "False"],
], ids=["fused", "fused-directed", "composed"])
def test_full_batch_training(extra):
    out = _run(extra)
    assert "GATConv" in out


def test_minibatch_training():
    _run(["--fused_attention", "True", "--fanout", "5,5", "--batch_size", "64"])


def test_minibatch_training_with_attention_dropout():
    """A new mask every step: the loss is only required to stay finite."""
    _run(["--fused_attention", "True", "--fanout", "5,5", "--batch_size", "64", "--attn_drop", "0.3"], falling=False)

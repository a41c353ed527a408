"""main.py --model pna on an MI355X: two PNAConv layers train in the driver's loop -- on the full graph, on sampled blocks and
with --directed True.  The first loss is restated in fp64 (centred statistics, test_pna_ops_gpu._stats64) from the weights the
model started with and the structure the step ran on.

Bound of the loss: the layers' bound 1e-4 * max(1, sum of |terms|) on the logits Z, carried through the loss.  log_softmax
moves by at most twice the largest error of a row's logits, and the loss is the mean over the rows, so
|loss - loss64| <= 1e-4 * max(1, mean over the rows of 2 * max_k Za[i, k]), Za the logits of the |.|-network (the same two
layers on |X|, |W| with every statistic replaced by a bound of its magnitude)."""
import math
import re

import pytest
import torch

from gnnadvisor_osdi21_amd import main as driver
from test_pna_ops_gpu import NAMES, _stats64
from test_reduce_ops_gpu import _rows_of

pytestmark = pytest.mark.gpu
ARGV = ["--model", "pna", "--synthetic", "cora-like", "--scale", "0.5", "--dim", "64", "--hidden", "16", "--classes", "7",
        "--verbose_mode", "True"]


class _Capture(dict):
    """The driver's capture dict, which also keeps the weights the model had when the driver handed it over (before any step)."""

    def update(self, **kw):
        super().update(**kw)
        if "model" in kw:
            self["initial"] = {k: v.detach().double().cpu().clone() for k, v in kw["model"].state_dict().items()}


def _layer64(state, prefix, conv, X, Xa, rows, src, n_out):
    """(Y, Ya): the layer in fp64 and the same layer on magnitudes."""
    c = torch.bincount(rows, minlength=n_out).clamp(min=1).double().unsqueeze(1)
    logd, delta = torch.log(c + 1), float(state[prefix + "delta"])
    scale_of = {"identity": torch.ones_like(logd), "amplification": logd / delta, "attenuation": delta / logd}
    stats = dict(zip(NAMES, _stats64(X, rows, src, n_out, conv.eps)))
    Ga = Xa[src]
    z = lambda: torch.zeros(n_out, X.shape[1], dtype=torch.float64)
    amax = z().scatter_reduce(0, rows[:, None].expand_as(Ga), Ga, reduce="amax", include_self=False)
    bound = {"mean": z().index_add(0, rows, Ga) / c, "std": torch.sqrt(z().index_add(0, rows, Ga ** 2) / c + conv.eps),
             "max": amax, "min": amax}
    out = []
    for x, st, f in ((X, stats, lambda t: t), (Xa, bound, torch.abs)):
        A = torch.cat([st[a] for a in conv.aggregators], 1)
        Y = x[:n_out] @ f(state[prefix + "weights_self"])
        for k, s in enumerate(conv.scalers):
            Y = Y + scale_of[s] * (A @ f(state[prefix + f"weights_scaler.{k}"]))
        out.append(Y)
    return out


def _loss64(run, structures, x, y):
    """structures: [(rows, src, n_out)] of the two layers."""
    model, state = run["model"], run["initial"]
    X = x.double().cpu()
    H, Ha = _layer64(state, "conv1.", model.conv1, X, X.abs(), *structures[0])
    H, Ha = torch.relu(H), Ha
    Z, Za = _layer64(state, "conv2.", model.conv2, H, Ha, *structures[1])
    loss = -torch.log_softmax(Z, 1).gather(1, y.cpu().long().view(-1, 1)).mean()
    tol = 1e-4 * max(1.0, float((2 * Za.max(1).values).mean()))
    return float(loss), tol


def _run(extra, capsys):
    run = _Capture()
    torch.manual_seed(3)
    assert driver.main(ARGV + extra, capture=run) == 0
    assert "Time (ms):" in capsys.readouterr().out
    first, final = run["first_loss"], run["final_loss"]
    assert math.isfinite(first) and math.isfinite(final) and final < first, (first, final)
    return run


@pytest.mark.parametrize("extra", [[], ["--directed", "True"]], ids=["symmetric", "directed"])
def test_driver_trains_pna_on_the_full_graph(capsys, extra):
    run = _run(["--num_epoches", "20"] + extra, capsys)
    info, ds = run["inputInfo"], run["dataset"]
    rows, src = _rows_of(info.row_pointers.cpu()), info.column_index.cpu().long()
    full = (rows, src, ds.num_nodes)
    loss64, tol = _loss64(run, [full, full], ds.x, ds.y)
    print(f"first loss {run['first_loss']:.6f}, fp64 {loss64:.6f}, bound {tol:.2e}; final loss {run['final_loss']:.6f}")
    assert abs(run["first_loss"] - loss64) <= tol
    from gnnadvisor_osdi21_amd.ops import PNAConv
    assert float(run["model"].conv1.delta) == pytest.approx(PNAConv.delta_of(info)) == pytest.approx(float(run["model"].conv2.delta))
    if extra:
        assert info.directed and info._edge_arrays().get("transposed") is not None


def test_driver_trains_pna_on_sampled_blocks(capsys):
    run = _run(["--num_epoches", "3", "--fanout", "5,5", "--batch_size", "256"], capsys)
    info, ds, sampler = run["inputInfo"], run["dataset"], run["sampler"]
    assert sampler.fanouts == [5, 5]
    # the first step's blocks again (the sampler is a function of the seeds and the rng_seed)
    seeds = torch.arange(256, dtype=torch.int32, device="cuda")
    blocks, input_nodes = sampler.sample(seeds, 0x5A17)
    structures = [(_rows_of(b.row_pointers.cpu()), b.column_index.cpu().long(), b.num_dst) for b in blocks]
    loss64, tol = _loss64(run, structures, ds.x.index_select(0, input_nodes), ds.y.index_select(0, seeds))
    print(f"first loss {run['first_loss']:.6f}, fp64 {loss64:.6f}, bound {tol:.2e}; final loss {run['final_loss']:.6f}")
    assert abs(run["first_loss"] - loss64) <= tol
    # delta is the full graph's, not a block's
    from gnnadvisor_osdi21_amd.ops import PNAConv
    assert float(run["model"].conv1.delta) == pytest.approx(PNAConv.delta_of(info))
    assert PNAConv.delta_of(blocks[0]) != pytest.approx(PNAConv.delta_of(info))


def test_driver_trains_pna_under_a_captured_epoch(capsys):
    """--hip_graph True: 10 eager steps on the capture stream, then 20 replays of one captured step (statistics call, backward
    sum, scatters).  The sums meet in another order on every run, so the run is held to what training must do, not to the eager
    run's bits: a finite loss below the loss the same seed starts from."""
    eager = _run(["--num_epoches", "20"], capsys)
    torch.manual_seed(3)
    assert driver.main(ARGV + ["--num_epoches", "20", "--hip_graph", "True"]) == 0
    out = capsys.readouterr().out
    assert "Time (ms):" in out
    final = float(re.search(r"# final loss: (\S+)", out).group(1))
    print(f"eager first loss {eager['first_loss']:.6f}, final {eager['final_loss']:.6f}; captured final {final:.6f}")
    assert math.isfinite(final) and final < eager["first_loss"]

"""gnna_agg_softmax_ld_f32 and gnna_agg_softmax_backward_ld_f32 through _lib, on the GPU.

Every output (out, lse, sq, dX) is held to the fp64 reference of softagg_ref.py within the project's bound
|got - ref| <= 1e-4 * max(1, scale) (assert_close_f64), scale the result's sum of |terms| as softagg_ref states it.  A CPU
emulation of the fp32 arithmetic stayed below 1e-6 * max(1, scale) on these inputs, so the bound is not expected to bind; every
test prints its largest ratio to the bound.

Graphs: make_case(3000, 40000, kind="uniform") and make_case(3000, 60000, kind="powerlaw"), seed 3; the second has rows without
edges and a row of more than 1000 edges, which the whole workgroup takes."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, load_extension
from util import assert_close_f64, make_case

import softagg_ref as S

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 16, 33, 64, 100, 257, 300)    # every lane layout, a partial last vector, column blocks past 256
SCALARS = (1.0, 0.0, -2.0, 50.0)                     # one per width in turn; every one is met at least twice


def _randn(n, d, seed, scale=1.0):
    return scale * torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


def _per_channel(d, seed):
    """3 * randn, with 0, a negative value and 50 among the first channels"""
    t = 3.0 * torch.randn(d, generator=torch.Generator().manual_seed(seed))
    for k, v in enumerate((0.0, -2.0, 50.0)[:d]):
        t[k] = v
    return t


@pytest.fixture(scope="module")
def cases():
    made = {}
    for kind, (n, e) in (("uniform", (3000, 40000)), ("powerlaw", (3000, 60000))):
        g, _, _, _ = make_case(n, e, 1, 32, seed=3, kind=kind)
        t_rp, t_ci = S.transpose_csr(g.row_pointers, g.column_index, n)
        made[kind] = (g, g.row_pointers.cuda(), g.column_index.cuda(), t_rp.cuda(), t_ci.cuda())
    deg = np.diff(made["powerlaw"][0].row_pointers.numpy())
    assert (deg == 0).any() and deg.max() > 1000           # rows without edges, and the long-row path
    return made


def _run(X, t, rp, ci, t_rp, t_ci, dY, n_out=None):
    """(out, lse, sq, dX) on the device"""
    out, lse, sq = _lib.agg_softmax(X, t, rp, ci, n_out, want_sq=True)
    dX = _lib.agg_softmax_backward(X, t, lse, out, dY, t_rp, t_ci)
    return out, lse, sq, dX


def _check(got, ref, what):
    """every output within the bound; -> the largest ratio to it"""
    worst = 0.0
    for name, g in zip(("out", "lse", "sq", "dX"), got):
        if g is None:
            continue
        worst = max(worst, S.worst_ratio(g, ref[name], ref[name + "_scale"]))
        assert_close_f64(g.cpu().numpy(), ref[name].numpy(), scale=ref[name + "_scale"].numpy(), what=f"{what} {name}")
    print(f"{what}: worst error / bound {worst:.5f}")
    return worst


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_outputs_and_gradient_against_fp64(cases, kind, d):
    g, rp, ci, t_rp, t_ci = cases[kind]
    n = g.num_nodes
    X, dY = _randn(n, d, 100 + d), _randn(n, d, 200 + d)
    for k, t in enumerate((torch.tensor([SCALARS[WIDTHS.index(d) % 4]]), _per_channel(d, 300 + d))):
        ref = S.reference(X, t, g.row_pointers, g.column_index, dY)
        got = _run(X.cuda(), t.cuda(), rp, ci, t_rp, t_ci, dY.cuda())
        _check(got, ref, f"{kind} D={d} t={'per-channel' if k else float(t[0])}")


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_temperature_zero_is_the_mean(cases, kind):
    g, rp, ci, t_rp, t_ci = cases[kind]
    n = g.num_nodes
    for d in (5, 64):
        X = _randn(n, d, 400 + d)
        out, lse, sq = _lib.agg_softmax(X.cuda(), torch.zeros(1).cuda(), rp, ci, n, want_sq=True)
        rows, src = S.edges_of(g.row_pointers, g.column_index, n)
        cnt = torch.bincount(rows, minlength=n).double().unsqueeze(1)
        G = X.double()[src]
        z = lambda: torch.zeros(n, d, dtype=torch.float64)
        mean = z().index_add_(0, rows, G) / cnt.clamp(min=1)
        mabs = z().index_add_(0, rows, G.abs()) / cnt.clamp(min=1)
        assert_close_f64(out.cpu().numpy(), mean.numpy(), scale=mabs.numpy(), what=f"{kind} D={d} t=0 out against the mean")
        log_count = torch.where(cnt > 0, torch.log(cnt.clamp(min=1)), torch.zeros_like(cnt)).expand(n, d)
        assert_close_f64(lse.cpu().numpy(), log_count.numpy(), what=f"{kind} D={d} t=0 lse against log(count)")


@pytest.mark.parametrize("t", [1.0, -2.0])
@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_large_scores_stay_finite(cases, kind, t):
    """X = 100 * randn: |lse| passes 100, where exp(-lse) is no fp32 number -- a backward factored into exp(t x_j) times node-sized
    sums of exp(-lse_i) overflows here; alpha = exp(t x_j - lse_i) per edge does not."""
    g, rp, ci, t_rp, t_ci = cases[kind]
    n = g.num_nodes
    for d in (5, 64):
        X, dY = _randn(n, d, 500 + d, scale=100.0), _randn(n, d, 600 + d)
        tt = torch.tensor([t])
        ref = S.reference(X, tt, g.row_pointers, g.column_index, dY)
        assert float(ref["lse"].abs().max()) > 100.0
        for name in ("out", "lse", "sq", "dX", "dt"):
            assert bool(torch.isfinite(ref[name]).all()), name
        got = _run(X.cuda(), tt.cuda(), rp, ci, t_rp, t_ci, dY.cuda())
        for name, v in zip(("out", "lse", "sq", "dX"), got):
            assert bool(torch.isfinite(v).all()), f"{kind} D={d} t={t}: {name} is not finite"
        _check(got, ref, f"{kind} 100 * randn D={d} t={t}")


@pytest.mark.parametrize("d", [7, 64, 300])
def test_the_same_bits_on_every_run_and_under_deterministic_tuning(cases, d):
    g, rp, ci, t_rp, t_ci = cases["powerlaw"]
    n = g.num_nodes
    X, dY, t = _randn(n, d, 700 + d).cuda(), _randn(n, d, 800 + d).cuda(), _per_channel(d, 900 + d).cuda()
    first = _run(X, t, rp, ci, t_rp, t_ci, dY)
    again = _run(X, t, rp, ci, t_rp, t_ci, dY)
    try:
        _lib.set_tuning(deterministic=1)
        det = _run(X, t, rp, ci, t_rp, t_ci, dY)
    finally:
        _lib.reset_tuning()
    for name, a, b, c in zip(("out", "lse", "sq", "dX"), first, again, det):
        assert torch.equal(a, b), f"D={d}: {name} differs between two calls"
        assert torch.equal(a, c), f"D={d}: {name} differs under deterministic = 1"


@pytest.mark.parametrize("want_sq", [True, False], ids=["sq", "no_sq"])
@pytest.mark.parametrize("d", [64, 7])
def test_padded_outputs_are_fully_written_and_the_padding_is_left_alone(cases, d, want_sq):
    g, rp, ci, t_rp, t_ci = cases["powerlaw"]
    n, ld = g.num_nodes, d + 9
    X, dY, t = _randn(n, d, 1000 + d), _randn(n, d, 1100 + d), torch.tensor([1.5])
    ref = S.reference(X, t, g.row_pointers, g.column_index, dY)
    nan = lambda: torch.full((n, ld), float("nan"), device="cuda")
    bufs = {k: nan() for k in ("out", "lse", "sq", "dX")}
    out, lse, sq = _lib.agg_softmax(X.cuda(), t.cuda(), rp, ci, n, out=bufs["out"][:, :d], lse=bufs["lse"][:, :d],
                                    sq=bufs["sq"][:, :d] if want_sq else None)
    assert (sq is None) == (not want_sq)
    dX = _lib.agg_softmax_backward(X.cuda(), t.cuda(), lse, out, dY.cuda(), t_rp, t_ci, out=bufs["dX"][:, :d])
    _check((out, lse, sq, dX), ref, f"padded D={d} sq={want_sq}")
    for name, buf in bufs.items():
        written = name != "sq" or want_sq
        assert bool(torch.isnan(buf[:, d:]).all()), f"{name}: the padding was written"
        assert bool(torch.isnan(buf[:, :d]).any()) != written, f"{name}: {'not every element was written' if written else 'written without being asked for'}"
    empty = torch.from_numpy(np.diff(g.row_pointers.numpy()) == 0).cuda()
    assert bool(empty.any()) and float(out[empty].abs().max()) == 0.0 and float(lse[empty].abs().max()) == 0.0
    assert sq is None or float(sq[empty].abs().max()) == 0.0


def test_rectangular_structure_duplicate_edges_and_ids_outside_the_rows():
    """5 destination rows over 9 source rows, by hand: duplicates, a row without edges, ids below 0 and at or beyond the row count
    on both sides -- they match the reference with those edges removed."""
    n_out, n_in = 5, 9
    lists = [[0, 3, 3, 8], [], [2, 2, 2, 7, 1], [4], [8, 0, 5, 5, 6, 3]]
    dirty = [[0, -1, 3, 3, 9, 8], [100, -7], [2, 2, 9, 2, 7, 1], [4, 2 ** 31 - 1], [8, 0, 5, -2 ** 31, 5, 6, 3]]
    to_csr = lambda ls: (torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in ls])]), dtype=torch.int32),
                         torch.tensor([j for l in ls for j in l], dtype=torch.int32))
    rp_clean, ci_clean = to_csr(lists)
    rp, ci = to_csr(dirty)
    t_rp_clean, t_ci_clean = S.transpose_csr(rp_clean, ci_clean, n_in)
    # the transposed structure with ids outside [0, n_out) put into three of its rows
    t_lists = [t_ci_clean[int(t_rp_clean[j]):int(t_rp_clean[j + 1])].tolist() for j in range(n_in)]
    t_lists[0] = [-1] + t_lists[0] + [5]
    t_lists[1] = [77] + t_lists[1]          # (source row 1 has one edge)
    t_lists[8] = t_lists[8] + [-3, 2 ** 31 - 1]
    t_rp, t_ci = to_csr(t_lists)
    for d in (3, 64, 257):
        X, dY, t = _randn(n_in, d, 1200 + d), _randn(n_out, d, 1300 + d), _per_channel(d, 1400 + d)
        ref = S.reference(X, t, rp_clean, ci_clean, dY)
        got = _run(X.cuda(), t.cuda(), rp.cuda(), ci.cuda(), t_rp.cuda(), t_ci.cuda(), dY.cuda())
        assert got[0].shape == (n_out, d) and got[3].shape == (n_in, d)
        _check(got, ref, f"5 x 9 D={d}")
        assert float(got[0][1].abs().max()) == 0.0 and float(got[1][1].abs().max()) == 0.0        # the row without edges


def test_column_slices_through_both_bindings(cases):
    GNNA = load_extension()
    g, rp, ci, t_rp, t_ci = cases["uniform"]
    n, d = g.num_nodes, 33
    wide = lambda seed: _randn(n, d + 11, seed).cuda()
    Xw, Gw = wide(1500), wide(1501)
    X, dY, t = Xw[:, 3:3 + d], Gw[:, 5:5 + d], _per_channel(d, 1502).cuda()
    assert not X.is_contiguous() and not dY.is_contiguous()
    plain = _run(X.contiguous(), t, rp, ci, t_rp, t_ci, dY.contiguous())
    # lse and Y as column slices too
    Lw, Yw = torch.empty(n, d + 4, device="cuda"), torch.empty(n, d + 6, device="cuda")
    out, lse, sq = _lib.agg_softmax(X, t, rp, ci, n, want_sq=True, out=Yw[:, 2:2 + d], lse=Lw[:, 1:1 + d])
    dX = _lib.agg_softmax_backward(X, t, lse, out, dY, t_rp, t_ci)
    eo, el, es = GNNA.aggregate_softmax(X, t, rp, ci, True)
    edx = GNNA.aggregate_softmax_backward(X, t, lse, out, dY, t_rp, t_ci)
    for name, a, b, c in zip(("out", "lse", "sq", "dX"), plain, (out, lse, sq, dX), (eo, el, es, edx)):
        assert torch.equal(a, b), f"{name}: the sliced call differs from the contiguous one"
        assert torch.equal(b, c), f"{name}: GNNA.aggregate_softmax differs from _lib.agg_softmax"
    assert GNNA.aggregate_softmax(X, t, rp, ci)[2] is None


def test_a_captured_forward_and_backward_pair_replays_the_eager_bits(cases):
    g, rp, ci, t_rp, t_ci = cases["powerlaw"]
    n, d = g.num_nodes, 64
    X, dY, t = _randn(n, d, 1600).cuda(), _randn(n, d, 1601).cuda(), _per_channel(d, 1602).cuda()
    eager = _run(X, t, rp, ci, t_rp, t_ci, dY)
    bufs = [torch.empty(n, d, device="cuda") for _ in range(4)]

    def pair():
        out, lse, sq = _lib.agg_softmax(X, t, rp, ci, n, out=bufs[0], lse=bufs[1], sq=bufs[2])
        _lib.agg_softmax_backward(X, t, lse, out, dY, t_rp, t_ci, out=bufs[3])

    torch.cuda.synchronize()
    before = _lib.runtime_counters()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pair()
    after = _lib.runtime_counters()
    assert after["capture_scratch"] > before["capture_scratch"], "the captured backward got no scratch of its capture"
    for rep in range(3):
        for b in bufs:
            b.fill_(float("nan"))
        gr.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "lse", "sq", "dX"), eager, bufs):
            assert torch.equal(a, b), f"replay {rep}: {name} differs from the eager call"

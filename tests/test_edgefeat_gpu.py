"""Edge-feature message passing on the GPU through the C ABI (include/gnna_edgefeat.h, ``_lib.agg_edge_feat`` /
``_lib.agg_edge_feat_backward``): every case runs both combines and both activations against the fp64 restatement
(edgefeat_ref.py) within the project's bound 1e-4 * max(1, sum |terms|) and prints the worst ratio to the bound."""
import numpy as np
import pytest
import torch

import edgefeat_ref as ref
from gnnadvisor_osdi21_amd import _lib
from util import make_case

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 5, 16, 33, 64, 100, 257, 300]
# the kernel's constants (gnna_edgefeat.hip): edges per slot and step, steps before a row goes to the whole block, edges a slot takes alone
K_EDGES, K_LONG_STEPS, K_SLOT_EDGES = 2, 32, 8


def lanes_per_row(dim):
    lpr = 1
    while lpr < 64 and 4 * lpr < dim:
        lpr *= 2
    return lpr


def long_threshold(dim):
    return (64 // lanes_per_row(dim)) * K_EDGES * K_LONG_STEPS


class Case(object):
    """A structure on the device with its transpose and position map, built once."""

    def __init__(self, rp, ci, num_in_rows, t=None):
        self.rp_h, self.ci_h, self.m = np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32), int(num_in_rows)
        self.n = len(self.rp_h) - 1
        self.rp, self.ci = torch.from_numpy(self.rp_h).cuda(), torch.from_numpy(self.ci_h).cuda()
        self.t = t if t is not None else _lib.transpose_csr(self.rp, self.ci, num_in_rows=self.m)
        self.nnz = len(self.ci_h)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for kind, edges in (("uniform", 40000), ("powerlaw", 60000)):
        g = make_case(3000, edges, 1, 32, 3, kind=kind)[0]
        out[kind] = Case(g.row_pointers.numpy(), g.column_index.numpy(), 3000)
    rp, ci = ref.small_rows_graph(5000, 5000, seed=11)
    out["small"] = Case(rp, ci, 5000)
    return out


def _ratio(got, want, scale):
    got = got.double().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want) / (1e-4 * np.maximum(1.0, scale))
    return float(np.nan_to_num(err, nan=np.inf).max()) if err.size else 0.0


def run_modes(case, x, e, dy, label, num_edges=None, exact=False):
    """Forward, d_input and d_edge of the four (combine, act) on `case` against the restatement; -> the worst ratio to the bound."""
    X, E, dY = (torch.from_numpy(a).cuda() for a in (x, e, dy))
    worst = 0.0
    for combine, act in ref.MODES:
        c, a = ref.COMBINES[combine], ref.ACTS[act]
        out = _lib.agg_edge_feat(X, E, case.rp, case.ci, combine=c, act=a)
        dX, dE = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, *case.t, combine=c, act=a)
        torch.cuda.synchronize()
        w_out, s_out = ref.forward(case.rp_h, case.ci_h, x, e, combine, act, num_edges)
        w_din, s_din, w_de, s_de = ref.backward(case.rp_h, case.ci_h, x, e, dy, combine, act, num_edges)
        ratios = {"out": _ratio(out, w_out, s_out), "d_input": _ratio(dX, w_din, s_din), "d_edge": _ratio(dE, w_de, s_de)}
        print("%s %s/%s: ratio to the bound out %.3g d_input %.3g d_edge %.3g" % (label, combine, act, *ratios.values()))
        for name, r in ratios.items():
            assert r <= 1.0, f"{label} {combine}/{act}: {name} is {r:.3g} x the bound"
        # d_edge is one product or a copy: exact against the same fp32 arithmetic, always
        assert np.array_equal(dE.cpu().numpy(), w_de.astype(np.float32)), f"{label} {combine}/{act}: d_edge is not exact"
        if exact:
            assert np.array_equal(out.cpu().numpy(), w_out.astype(np.float32)), f"{label} {combine}/{act}: out is not exact"
            assert np.array_equal(dX.cpu().numpy(), w_din.astype(np.float32)), f"{label} {combine}/{act}: d_input is not exact"
        worst = max(worst, *ratios.values())
    return worst


def test_the_graphs_reach_every_path(cases):
    deg = np.diff(cases["powerlaw"].rp_h)
    assert (deg == 0).any(), "the powerlaw graph has no row without edges"
    # a row beyond the whole-block threshold at every width from 16 (narrower layouts have a threshold of 2048 edges and more:
    # test_one_very_long_row_at_narrow_widths covers them)
    assert deg.max() > max(long_threshold(d) for d in WIDTHS if d >= 16) and deg.max() <= long_threshold(5)
    between = (deg > K_SLOT_EDGES) & (deg <= long_threshold(300))
    assert between.any() and (deg <= K_SLOT_EDGES).any()
    t_deg = np.diff(cases["powerlaw"].t[0].cpu().numpy())
    assert t_deg.max() > K_SLOT_EDGES and (t_deg == 0).any()
    sdeg = np.diff(cases["small"].rp_h)
    assert sdeg.min() == 2 and sdeg.max() == 4, "the batch of small rows must have 2 .. 4 edges per row"


@pytest.mark.parametrize("dim", WIDTHS)
@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_every_width_on_both_graphs(cases, kind, dim):
    case = cases[kind]
    x, e, dy = ref.operands(case.m, case.n, case.nnz, dim, seed=100 + dim)
    run_modes(case, x, e, dy, f"{kind} D={dim}")


@pytest.mark.parametrize("dim", [1, 5, 16, 64, 100, 128, 300])
def test_rows_of_two_to_four_edges_take_the_slot_per_row_path(cases, dim):
    case = cases["small"]
    x, e, dy = ref.operands(case.m, case.n, case.nnz, dim, seed=200 + dim)
    run_modes(case, x, e, dy, f"small rows D={dim}")


@pytest.mark.parametrize("dim", [1, 3, 4, 5, 16])
def test_one_very_long_row_at_narrow_widths(dim):
    # row 0 gathers 9000 edges (beyond the whole-block threshold of every layout: at most 4096), rows 1 .. 9000 one edge from
    # source 0 each, so that row 0 of the transposed structure is as long
    long_edges = 9000
    assert long_edges > long_threshold(1)
    rng = np.random.default_rng(dim)
    rp = np.concatenate([[0], long_edges + np.arange(long_edges + 1)]).astype(np.int32)
    ci = np.concatenate([rng.integers(0, 50, size=long_edges), np.zeros(long_edges)]).astype(np.int32)
    case = Case(rp, ci, 50)
    assert np.diff(case.t[0].cpu().numpy()).max() > long_threshold(1)
    x, e, dy = ref.operands(50, case.n, case.nnz, dim, seed=300 + dim)
    run_modes(case, x, e, dy, f"long row D={dim}")


@pytest.mark.parametrize("kind, dim", [("powerlaw", 33), ("powerlaw", 300), ("small", 64), ("uniform", 5)])
def test_integer_inputs_are_exact_to_the_bit(cases, kind, dim):
    case = cases[kind]
    x, e, dy = ref.operands(case.m, case.n, case.nnz, dim, seed=400 + dim, integer=True)
    assert run_modes(case, x, e, dy, f"integers {kind} D={dim}", exact=True) == 0.0


@pytest.mark.parametrize("dim", [5, 64])
def test_planted_zeros_give_no_message_and_no_gradient(cases, dim):
    case = cases["small"]
    x, e, dy = ref.operands(case.m, case.n, case.nnz, dim, seed=500 + dim)
    planted = np.arange(0, case.nnz, 3)
    e_add = e.copy()
    e_add[planted] = -x[case.ci_h[planted]]                          # x + e == 0 exactly
    e_mul = e.copy()
    e_mul[planted] = 0.0                                             # x * e == 0 exactly
    X, dY = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    for combine, ee in (("add", e_add), ("mul", e_mul)):
        E = torch.from_numpy(ee).cuda()
        _, dE = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, combine=ref.COMBINES[combine], act=ref.ACTS["relu"],
                                            want_dx=False)
        assert not dE[torch.from_numpy(planted).cuda()].any(), f"{combine}: a gradient flows at pre == 0"
        run_modes(case, x, ee, dy, f"planted zeros {combine} D={dim}")
    # the other magnitudes are well inside the normal range: the fp32 and fp64 masks agree
    src = case.ci_h
    rest = np.setdiff1d(np.arange(case.nnz), planted)
    pre = x[src[rest]].astype(np.float64) + e_add[rest].astype(np.float64)
    assert ((x[src[rest]] + e_add[rest] > 0) == (pre > 0)).all()


def test_rectangular_structures_and_duplicate_edges():
    rp, ci = ref.small_rows_graph(700, 1300, seed=21, lo=0, hi=12)
    ci[1::2] = ci[0::2][:len(ci[1::2])]                              # every second edge repeats the one before it
    dup = sum(len(set(ci[a:b])) < b - a for a, b in zip(rp[:-1], rp[1:]))
    assert dup > 100
    for n_in, seed in ((1300, 1), (2000, 2)):                        # more sources than destinations, and sources no edge names
        case = Case(rp, ci, n_in)
        assert case.n != case.m
        x, e, dy = ref.operands(n_in, case.n, case.nnz, 33, seed=600 + seed)
        run_modes(case, x, e, dy, f"rectangular {case.n} x {n_in}")
    few = Case(*ref.small_rows_graph(1300, 90, seed=22), 90)         # more destinations than sources: long rows of A^T
    x, e, dy = ref.operands(90, few.n, few.nnz, 64, seed=603)
    run_modes(few, x, e, dy, "rectangular 1300 x 90")


def _raw(case, X, E, dY, num_edges, combine, act):
    """Both entries called with a num_edges of the caller's choosing (the wrappers take it from column_index)."""
    dim, dev = X.shape[1], X.device
    out, dX = _lib._fresh_output((case.n, dim), dev), _lib._fresh_output((case.m, dim), dev)
    dE = _lib._fresh_output((num_edges, dim), dev)
    _lib._call(dev, "gnna_agg_edge_feat_ld_f32", X.data_ptr(), dim, case.m, E.data_ptr(), dim, num_edges, case.rp.data_ptr(),
               case.ci.data_ptr(), out.data_ptr(), dim, case.n, dim, combine, act, 0)
    _lib._call(dev, "gnna_agg_edge_feat_backward_ld_f32", X.data_ptr(), dim, case.m, E.data_ptr(), dim, num_edges, dY.data_ptr(), dim,
               case.rp.data_ptr(), case.ci.data_ptr(), *(t.data_ptr() for t in case.t), dX.data_ptr(), dim, dE.data_ptr(), dim, case.n,
               dim, combine, act, 0)
    torch.cuda.synchronize()
    return out, dX, dE


@pytest.mark.parametrize("dim", [4, 100])
def test_ids_and_positions_out_of_range_are_skipped_in_all_three_passes(dim):
    rp, ci = ref.small_rows_graph(900, 400, seed=31, lo=0, hi=20)
    ci[::7], ci[3::11], ci[5::13] = -1, 400, 2 ** 31 - 1             # below, just beyond, far beyond the source rows
    case = Case(rp, ci, 400)
    x, e, dy = ref.operands(400, case.n, case.nnz, dim, seed=700 + dim)
    run_modes(case, x, e, dy, f"bad ids D={dim}")                    # (skipped edges: d_edge rows of 0, checked exactly)
    skipped = (ci < 0) | (ci >= 400)
    X, E, dY = (torch.from_numpy(a).cuda() for a in (x, e, dy))
    # positions: only the positions below num_edges exist; the row the cut falls into loses its tail, the rows behind it are empty
    r = 500 + int(np.argmax(np.diff(rp)[500:] >= 2))
    num_edges = int(rp[r]) + 1
    assert rp[r] < num_edges < rp[r + 1] < case.nnz                  # the cut falls inside a row
    Ecut = E[:num_edges].contiguous()
    for combine, act in ref.MODES:
        out, dX, dE = _raw(case, X, Ecut, dY, num_edges, ref.COMBINES[combine], ref.ACTS[act])
        w_out, s_out = ref.forward(rp, ci, x, e[:num_edges], combine, act, num_edges)
        w_din, s_din, w_de, s_de = ref.backward(rp, ci, x, e[:num_edges], dy, combine, act, num_edges)
        for name, got, want, scale in (("out", out, w_out, s_out), ("d_input", dX, w_din, s_din), ("d_edge", dE, w_de, s_de)):
            r = _ratio(got, want, scale)
            assert r <= 1.0, f"positions D={dim} {combine}/{act}: {name} is {r:.3g} x the bound"
        assert not dE[torch.from_numpy(skipped[:num_edges]).cuda()].any()
    # a structure that ends before num_edges: the d_edge rows no row reaches are 0, not what the buffer held
    short = Case(rp[:501], ci[:rp[500]], 400)
    short.ci = case.ci
    out, dX, dE = _raw(short, X, E, dY[:500].contiguous(), case.nnz, 0, 1)
    assert not dE[int(rp[500]):].any() and bool(torch.isfinite(dE).all())


@pytest.mark.parametrize("dim", [3, 64])
def test_no_edges_gives_zero_outputs(dim):
    rp = np.zeros(41, dtype=np.int32)
    case = Case(rp, np.zeros(0, dtype=np.int32), 17)
    x, e, dy = ref.operands(17, 40, 0, dim, seed=800)
    X, E, dY = (torch.from_numpy(a).cuda() for a in (x, e, dy))
    for combine, act in ref.MODES:
        c, a = ref.COMBINES[combine], ref.ACTS[act]
        out = _lib.agg_edge_feat(X, E, case.rp, case.ci, combine=c, act=a)
        dX, dE = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, *case.t, combine=c, act=a)
        assert out.shape == (40, dim) and not out.any() and dX.shape == (17, dim) and not dX.any() and dE.shape == (0, dim)


@pytest.mark.parametrize("dim", [5, 64, 257])
def test_padded_outputs_are_fully_written_and_the_padding_is_left_alone(cases, dim):
    case = cases["powerlaw"]
    x, e, dy = ref.operands(case.m, case.n, case.nnz, dim, seed=900 + dim)
    pad = 3

    def padded(a):                                                   # the rows of `a` inside a wider buffer of NaN
        big = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device="cuda")
        big[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        return big, big[:, :a.shape[1]]

    (_, X), (_, E), (_, dY) = padded(x), padded(e), padded(dy)
    Xc, Ec, dYc = X.contiguous(), E.contiguous(), dY.contiguous()
    for combine, act in ref.MODES:
        c, a = ref.COMBINES[combine], ref.ACTS[act]
        bufs = [torch.full((rows, dim + pad), float("nan"), device="cuda") for rows in (case.n, case.m, case.nnz)]
        out = _lib.agg_edge_feat(X, E, case.rp, case.ci, combine=c, act=a, out=bufs[0][:, :dim])
        dX, dE = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, *case.t, combine=c, act=a, dX=bufs[1][:, :dim],
                                             dE=bufs[2][:, :dim])
        want = (_lib.agg_edge_feat(Xc, Ec, case.rp, case.ci, combine=c, act=a),
                *_lib.agg_edge_feat_backward(Xc, Ec, dYc, case.rp, case.ci, *case.t, combine=c, act=a))
        for name, buf, got, ref_t in zip(("out", "d_input", "d_edge"), bufs, (out, dX, dE), want):
            assert bool(torch.isfinite(got).all()), f"{combine}/{act}: {name} has elements that were not written"
            assert bool(torch.isnan(buf[:, dim:]).all()), f"{combine}/{act}: the padding of {name} was touched"
            assert torch.equal(got, ref_t), f"{combine}/{act}: {name} differs between strided and contiguous operands"


def test_one_output_at_a_time_gives_the_bits_of_both(cases):
    case = cases["uniform"]
    x, e, dy = ref.operands(case.m, case.n, case.nnz, 33, seed=1000)
    X, E, dY = (torch.from_numpy(a).cuda() for a in (x, e, dy))
    for combine, act in ref.MODES:
        c, a = ref.COMBINES[combine], ref.ACTS[act]
        dX, dE = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, *case.t, combine=c, act=a)
        only_x, none_e = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, *case.t, combine=c, act=a, want_de=False)
        none_x, only_e = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, combine=c, act=a, want_dx=False)     # no transpose given
        assert none_e is None and none_x is None and torch.equal(only_x, dX) and torch.equal(only_e, dE)


@pytest.mark.parametrize("dim", [16, 100])
def test_asymmetric_edge_rows_on_a_symmetric_structure_through_the_reverse_edge_map(dim):
    rp, ci = ref.symmetric_graph(1500, 6000, seed=41)
    RP, CI = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    rev = _lib.reverse_edges(RP, CI).to("cuda")
    case = Case(rp, ci, 1500, t=(RP, CI, rev))                       # the structure is its own transpose; rev finds the edge's E row
    x, e, dy = ref.operands(1500, 1500, case.nnz, dim, seed=1100 + dim)
    assert not np.array_equal(e[rev.cpu().numpy()], e), "E must differ between the two directions of an edge"
    run_modes(case, x, e, dy, f"reverse-edge map D={dim}")
    # the wrong map (every transposed position its own edge row) gives another d_input wherever E matters
    X, E, dY = (torch.from_numpy(a).cuda() for a in (x, e, dy))
    own = torch.arange(case.nnz, dtype=torch.int32, device="cuda")
    good = _lib.agg_edge_feat_backward(X, E, dY, RP, CI, RP, CI, rev, combine=_lib.EDGE_MUL, want_de=False)[0]
    bad = _lib.agg_edge_feat_backward(X, E, dY, RP, CI, RP, CI, own, combine=_lib.EDGE_MUL, want_de=False)[0]
    assert not torch.equal(good, bad)


def _all_three(case, X, E, dY, c, a, bufs=(None, None, None)):
    out = _lib.agg_edge_feat(X, E, case.rp, case.ci, combine=c, act=a, out=bufs[0])
    dX, dE = _lib.agg_edge_feat_backward(X, E, dY, case.rp, case.ci, *case.t, combine=c, act=a, dX=bufs[1], dE=bufs[2])
    return out, dX, dE


@pytest.mark.parametrize("kind, dim", [("powerlaw", 64), ("powerlaw", 300), ("small", 7)])
def test_the_same_bits_on_every_run_and_under_deterministic_tuning(cases, kind, dim):
    case = cases[kind]
    X, E, dY = (torch.from_numpy(a).cuda() for a in ref.operands(case.m, case.n, case.nnz, dim, seed=1200 + dim))
    for combine, act in ref.MODES:
        c, a = ref.COMBINES[combine], ref.ACTS[act]
        first, again = _all_three(case, X, E, dY, c, a), _all_three(case, X, E, dY, c, a)
        try:
            _lib.set_tuning(deterministic=1)
            det = _all_three(case, X, E, dY, c, a)                   # accepted: no GnnaError
        finally:
            _lib.reset_tuning()
        for name, p, q, r in zip(("out", "d_input", "d_edge"), first, again, det):
            assert torch.equal(p, q), f"{combine}/{act}: {name} differs between two calls"
            assert torch.equal(p, r), f"{combine}/{act}: {name} differs under deterministic = 1"


def test_a_captured_call_replays_to_the_same_bits(cases):
    case = cases["powerlaw"]
    dim, c, a = 64, _lib.EDGE_ADD, _lib.EDGE_ACT_RELU
    X, E, dY = (torch.from_numpy(v).cuda() for v in ref.operands(case.m, case.n, case.nnz, dim, seed=1300))
    eager = _all_three(case, X, E, dY, c, a)
    bufs = [torch.empty(rows, dim, device="cuda") for rows in (case.n, case.m, case.nnz)]
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        _all_three(case, X, E, dY, c, a, bufs)
    for rep in range(2):
        for b in bufs:
            b.fill_(float("nan"))
        gr.replay()
        torch.cuda.synchronize()
        for name, p, q in zip(("out", "d_input", "d_edge"), eager, bufs):
            assert torch.equal(p, q), f"replay {rep}: {name} differs from the eager call"

"""gnna_segment_attn_pool_ld_f32 / gnna_segment_attn_pool_backward_ld_f32 on the GPU, through the C ABI (_lib) and through GNNA,
against tests/attnpool_ref.py (fp64).  The layouts are those of test_pool_gpu.py, derived from the tile (_lib.POOL_TILE_ROWS) and
from the number of tiles at which a segment's join moves from a wavefront to the workgroup (_lib.POOL_LONG_STEPS per slot).

Every output is held within the project's bound 1e-4 * max(1, scale) of fp64 (util.assert_close_f64), with the scales of
attnpool_ref.  Why the bound holds: the weights alpha sum to 1, so a sum of n weighted terms errs by about n * 2^-24 * scale in any
order -- below 1e-4 * scale for n <= 1600 -- plus one v_exp_f32 per term (1 ulp) and the rounding of its argument, |d| * 2^-24
relative for a weight exp(d), d <= 0, which is largest, 2^-24 / e of the segment's largest weight, at d = -1.  Gates near +-100
add half an ulp of 100, 4e-6, to lse (bound: 1e-2) and the same, relative, to the backward's alpha = exp(s - lse).  long_join has a
segment of up to 262,656 rows (dim 1): its rows are added slot by slot, tile by tile and then piece by piece, so no single
accumulator sees more than a few hundred terms.
An fp32 numpy emulation of the kernels' arithmetic (tools/emulate_attnpool_fp32.py: the slots, the steps of four rows, the
butterfly, the pieces and their join in tile order, exp2 of the product with log2 e) on the inputs of these tests -- every layout,
dims 1, 3, 33, 64 and 257, both gate widths, the three score families -- stayed below 0.04 of the bound for every output: the
worst |error| / bound was 8.1e-3 for out, 1.8e-3 for lse, 4.0e-2 for dX and 3.3e-2 for dGate (both from the scores near +-100, the
4e-6 of lse above).  Each test prints its worst ratio on the GPU."""
import numpy as np
import pytest
import torch

import attnpool_ref
import pool_ref
from gnnadvisor_osdi21_amd import _lib, load_extension
from util import assert_close_f64

pytestmark = pytest.mark.gpu

T = _lib.POOL_TILE_ROWS
DIMS = (1, 3, 4, 33, 64, 100, 257)
NAN = float("nan")
FWD, BWD = "gnna_segment_attn_pool_ld_f32", "gnna_segment_attn_pool_backward_ld_f32"


def _slots(dim):
    """Partial rows of a wavefront at this width: 64 / lanes per row."""
    lanes = 1
    while lanes < 64 and 4 * lanes < dim:
        lanes *= 2
    return 64 // lanes


def _cum(first, lengths):
    return [first] + list(first + np.cumsum(lengths))


def layouts(dim):
    """name -> (num_rows, graph_pointers): those of test_pool_gpu.py that the issue names"""
    long_tiles = _lib.POOL_LONG_STEPS * _slots(dim) + 2        # joined by the whole workgroup
    return {
        "single_rows": (T + 3, list(range(T + 4))),
        "empties": (T + 9, [0, 0, 5, 5, T, T, T + 9, T + 9]),     # first, middle, on the tile boundary, last
        "len_63_64_65": (192, _cum(0, [63, 64, 65])),
        "len_T-1_T_T+1": (3 * T, _cum(0, [T - 1, T, T + 1])),
        "two_tiles": (T + 20, [0, T - 10, T + 10, T + 20]),
        "three_tiles_and_5": (3 * T + 20, [0, 7, 3 * T + 12, 3 * T + 20]),
        "begins_on_a_tile": (2 * T + 5, [0, T, 2 * T + 5]),
        "rows_of_no_graph": (T + 30, [3, 40, T + 2]),
        "long_join": (long_tiles * T + 5, [2, 9, long_tiles * T - 3, long_tiles * T + 5]),
    }


LAYOUT_NAMES = tuple(layouts(1))


def inputs(n, dim, gate_dim, gp, seed, family="normal"):
    """(X, gate [n, gate_dim], dY [G, dim]) in float32.  normal: scores of standard deviation 2.  shifted: +100 on the scores of
    every even segment, -100 on those of every odd one (exp(s) overflows, resp. underflows to denormals and 0 in fp32).  dominant: one row per
    segment scores 30 above the others."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    gate = (2.0 * rng.standard_normal((n, gate_dim))).astype(np.float32)
    dY = rng.standard_normal((len(gp) - 1, dim)).astype(np.float32)
    for g, (a, b) in enumerate(pool_ref.segments(gp, n)):
        if b <= a:
            continue
        if family == "shifted":
            gate[a:b] += np.float32(100.0 if g % 2 == 0 else -100.0)
        elif family == "dominant":
            gate[a + (b - a) // 2] += np.float32(30.0)
    return X, gate, dY


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _padded(rows, width, pad):
    """A NaN-filled buffer [rows, width + pad] and its view [rows, width]."""
    buf = torch.full((rows, width + pad), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[:, :width]


def _filled(a, pad):
    buf, view = _padded(a.shape[0], a.shape[1], pad)
    view.copy_(_dev(a))
    return buf, view


def _run(X, gate, gp, dY, pad=3, want_lse=True, need_input=True, need_gate=True, gate_is_x=False):
    """Forward and backward through the C ABI with leading dimensions > the width on every input and output; checks that the
    padding of the outputs is untouched.  -> dict of numpy arrays."""
    n, dim = X.shape
    gd = gate.shape[1]
    G = len(gp) - 1
    gpd = _dev(gp, torch.int32)
    _, xv = _filled(X, pad)
    gv = xv if gate_is_x else _filled(gate, pad + 1)[1]
    bufs, out = {}, {}
    bufs["out"], out["out"] = _padded(G, dim, pad)
    if want_lse:
        bufs["lse"], out["lse"] = _padded(G, gd, pad + 2)
    res = _lib.segment_attn_pool(xv, gv, gpd, out=out)
    assert set(res) == set(out) and all(res[k] is out[k] for k in out)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    if dY is not None:
        lse = res["lse"] if want_lse else _lib.segment_attn_pool(xv, gv, gpd)["lse"]
        _, dyv = _filled(dY, pad)
        given = {}
        if need_input:
            bufs["d_input"], given["d_input"] = _padded(n, dim, pad + 1)
        if need_gate:
            bufs["d_gate"], given["d_gate"] = _padded(n, gd, pad)
        d_input, d_gate = _lib.segment_attn_pool_backward(xv, gv, lse, res["out"], dyv, gpd, need_input=need_input, need_gate=need_gate,
                                                          out=given)
        assert (d_input is given.get("d_input")) and (d_gate is given.get("d_gate"))
        got.update({k: v.cpu().numpy() for k, v in given.items()})
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        width = got[name].shape[1]
        assert bool(torch.isnan(buf[:, width:]).all()), name
    return got


def _worst(got, ref, names):
    """The largest |got - ref| / (1e-4 * max(1, scale)) over the outputs named, after asserting the bound."""
    worst = 0.0
    for name in names:
        key = {"d_input": "dX", "d_gate": "dGate"}.get(name, name)
        scale = ref[key + "_scale"]
        assert_close_f64(got[name], ref[key], what=name, scale=scale)
        if got[name].size:
            worst = max(worst, float((np.abs(got[name] - ref[key]) / (1e-4 * np.maximum(1.0, scale))).max()))
    return worst


ALL = ("out", "lse", "d_input", "d_gate")


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("per", ["row", "element"])
@pytest.mark.parametrize("dim", DIMS)
def test_forward_and_backward_are_within_the_bound_of_fp64(dim, per, layout):
    n, gp = layouts(dim)[layout]
    if layout != "long_join":
        assert max(b - a for a, b in pool_ref.segments(gp, n)) <= 1600
    X, gate, dY = inputs(n, dim, 1 if per == "row" else dim, gp, 1000 + dim)
    ref = attnpool_ref.reference(X, gate, gp, dY)
    got = _run(X, gate, gp, dY)
    print("worst ratio to the bound:", _worst(got, ref, ALL))
    # a row of no graph and an empty segment get exact zeros
    inside = np.zeros(n, dtype=bool)
    for g, (a, b) in enumerate(pool_ref.segments(gp, n)):
        inside[a:b] = True
        if b <= a:
            assert not got["out"][g].any() and not got["lse"][g].any()
    assert not got["d_input"][~inside].any() and not got["d_gate"][~inside].any()


@pytest.mark.parametrize("family", ["shifted", "dominant"])
@pytest.mark.parametrize("per", ["row", "element"])
@pytest.mark.parametrize("dim, layout", [(3, "two_tiles"), (33, "three_tiles_and_5"), (64, "len_63_64_65"), (257, "len_T-1_T_T+1"),
                                         (100, "long_join")])
def test_scores_near_plus_and_minus_100_and_one_dominant_score(dim, layout, per, family):
    n, gp = layouts(dim)[layout]
    X, gate, dY = inputs(n, dim, 1 if per == "row" else dim, gp, 7 + dim, family)
    if family == "shifted":
        with np.errstate(over="ignore"):
            naive = np.exp(gate)                            # the form that is not used: inf for +100, denormals and 0 for -100
        assert np.isinf(naive).any() and (naive < np.finfo(np.float32).tiny).any()
    ref = attnpool_ref.reference(X, gate, gp, dY)
    got = _run(X, gate, gp, dY)
    assert all(np.isfinite(v).all() for v in got.values())
    print("worst ratio to the bound:", _worst(got, ref, ALL))


@pytest.mark.parametrize("dim, layout", [(4, "two_tiles"), (64, "three_tiles_and_5"), (257, "begins_on_a_tile")])
def test_the_gate_is_the_feature_matrix(dim, layout):
    """Softmax aggregation as a readout: input and gate are one pointer."""
    n, gp = layouts(dim)[layout]
    X, _, dY = inputs(n, dim, dim, gp, 5)
    ref = attnpool_ref.reference(X, X, gp, dY)
    got = _run(X, X, gp, dY, gate_is_x=True)
    print("worst ratio to the bound:", _worst(got, ref, ALL))


def test_pointers_are_clamped_and_a_descending_pair_is_an_empty_segment():
    n, dim, gp = 50, 5, [-5, 20, 10, 10, 70]                      # -> [0, 20), empty, empty, [10, 50)
    assert pool_ref.segments(gp, n) == [(0, 20), (20, 20), (10, 10), (10, 50)]
    for gd in (1, dim):
        X, gate, _ = inputs(n, dim, gd, gp, 3)
        _worst(_run(X, gate, gp, None), attnpool_ref.reference(X, gate, gp), ("out", "lse"))
    # the backward of clamped pointers that do not descend
    gp = [-5, 20, 20, 70]
    for gd in (1, dim):
        X, gate, dY = inputs(n, dim, gd, gp, 4)
        _worst(_run(X, gate, gp, dY), attnpool_ref.reference(X, gate, gp, dY), ALL)


@pytest.mark.parametrize("per", ["row", "element"])
@pytest.mark.parametrize("dim, layout", [(33, "two_tiles"), (257, "three_tiles_and_5")])
def test_null_lse_and_either_gradient_alone(dim, layout, per):
    n, gp = layouts(dim)[layout]
    X, gate, dY = inputs(n, dim, 1 if per == "row" else dim, gp, 11)
    ref = attnpool_ref.reference(X, gate, gp, dY)
    both = _run(X, gate, gp, dY)
    no_lse = _run(X, gate, gp, dY, want_lse=False)
    assert set(no_lse) == {"out", "d_input", "d_gate"}
    only_x = _run(X, gate, gp, dY, need_gate=False)
    only_g = _run(X, gate, gp, dY, need_input=False)
    assert set(only_x) == {"out", "lse", "d_input"} and set(only_g) == {"out", "lse", "d_gate"}
    _worst(both, ref, ALL)
    for other in (no_lse, only_x, only_g):
        for name, value in other.items():
            assert np.array_equal(value.view(np.uint32), both[name].view(np.uint32)), name
    with pytest.raises(ValueError, match="needs need_input or need_gate"):
        _lib.segment_attn_pool_backward(_dev(X), _dev(gate), _dev(both["lse"]), _dev(both["out"]), _dev(dY), _dev(gp, torch.int32),
                                        need_input=False, need_gate=False)


def test_a_batch_without_graphs():
    gp = _dev([0], torch.int32)
    X, gate = torch.randn(40, 5, device="cuda"), torch.randn(40, device="cuda")
    res = _lib.segment_attn_pool(X, gate, gp)
    assert tuple(res["out"].shape) == (0, 5) and tuple(res["lse"].shape) == (0, 1)
    # the C entry itself: nothing is written
    keep = torch.full((2, 5), 7.0, device="cuda")
    _lib._call(X.device, FWD, X.data_ptr(), 5, 40, gate.data_ptr(), 1, 1, gp.data_ptr(), 0, keep.data_ptr(), 5, None, 1, 5, 0)
    assert bool((keep == 7.0).all())
    # backward: every row is a row of no graph
    for gated in (gate, torch.randn(40, 5, device="cuda")):
        gd = 1 if gated.dim() == 1 else 5
        d_input, d_gate = _lib.segment_attn_pool_backward(X, gated, torch.zeros(0, gd, device="cuda"), res["out"],
                                                          torch.zeros(0, 5, device="cuda"), gp)
        assert tuple(d_input.shape) == (40, 5) and tuple(d_gate.shape) == (40, gd)
        assert bool((d_input == 0).all()) and bool((d_gate == 0).all())


@pytest.mark.parametrize("per", ["row", "element"])
@pytest.mark.parametrize("dim, layout", [(33, "three_tiles_and_5"), (64, "long_join"), (257, "len_T-1_T_T+1")])
def test_the_same_bits_on_two_runs_and_deterministic_tuning_accepts_the_calls(dim, layout, per):
    n, gp = layouts(dim)[layout]
    X, gate, dY = inputs(n, dim, 1 if per == "row" else dim, gp, 4)
    first = _run(X, gate, gp, dY)
    try:
        _lib.set_tuning(deterministic=1)
        second = _run(X, gate, gp, dY)
    finally:
        _lib.reset_tuning()
    for name in first:
        assert np.array_equal(first[name].view(np.uint32), second[name].view(np.uint32)), name


@pytest.mark.parametrize("per", ["row", "element"])
@pytest.mark.parametrize("dim, layout", [(64, "three_tiles_and_5"), (3, "empties"), (100, "rows_of_no_graph")])
def test_through_the_extension_module(dim, layout, per):
    GNNA = load_extension()
    n, gp = layouts(dim)[layout]
    X, gate, dY = inputs(n, dim, 1 if per == "row" else dim, gp, 21)
    via_lib = _run(X, gate, gp, dY, pad=0)
    gpd, Xd, gd_, dYd = _dev(gp, torch.int32), _dev(X), _dev(gate), _dev(dY)
    out, lse = GNNA.segment_attn_pool(Xd, gd_, gpd)
    d_input, d_gate = GNNA.segment_attn_pool_backward(Xd, gd_, lse, out, dYd, gpd)
    got = dict(out=out, lse=lse, d_input=d_input, d_gate=d_gate)
    for name, value in got.items():
        assert np.array_equal(value.cpu().numpy().view(np.uint32), via_lib[name].view(np.uint32)), name
    only_x, none = GNNA.segment_attn_pool_backward(Xd, gd_, lse, out, dYd, gpd, True, False)
    assert none is None and torch.equal(only_x, d_input)
    none, only_g = GNNA.segment_attn_pool_backward(Xd, gd_, lse, out, dYd, gpd, need_input=False, need_gate=True)
    assert none is None and torch.equal(only_g, d_gate)
    _worst(via_lib, attnpool_ref.reference(X, gate, gp, dY), ALL)


@pytest.mark.parametrize("per", ["row", "element"])
def test_one_captured_call_replayed_on_new_inputs(per):
    """torch.cuda.graph without stream=, as in test_pool_gpu.py: forward and backward in one graph, replayed twice on new input
    values; every output is NaN-filled before a replay and compared after it."""
    dim = 64
    n, gp = layouts(dim)["three_tiles_and_5"]
    G = len(gp) - 1
    gd = 1 if per == "row" else dim
    gpd = _dev(gp, torch.int32)
    X, gate, dY = torch.empty(n, dim, device="cuda"), torch.empty(n, gd, device="cuda"), torch.empty(G, dim, device="cuda")
    out = dict(out=torch.empty(G, dim, device="cuda"), lse=torch.empty(G, gd, device="cuda"))
    grads = dict(d_input=torch.empty(n, dim, device="cuda"), d_gate=torch.empty(n, gd, device="cuda"))

    def step():
        _lib.segment_attn_pool(X, gate, gpd, out=out)
        _lib.segment_attn_pool_backward(X, gate, out["lse"], out["out"], dY, gpd, out=grads)

    for t, h in zip((X, gate, dY), inputs(n, dim, gd, gp, 0)):
        t.copy_(_dev(h))
    if torch.cuda.graph.default_capture_stream is None:
        torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.graph.default_capture_stream):
        step()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    torch.cuda.synchronize()
    for seed in (1, 2):
        host = inputs(n, dim, gd, gp, seed)
        for t, h in zip((X, gate, dY), host):
            t.copy_(_dev(h))
        for t in list(out.values()) + list(grads.values()):
            t.fill_(NAN)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in {**out, **grads}.items()}
        _worst(got, attnpool_ref.reference(*host[:2], gp, host[2]), ALL)

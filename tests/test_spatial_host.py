"""Graph construction from coordinates (include/gnna_spatial.h), the part that needs no GPU: the numpy restatement of the rule
(tests/spatial_ref.py) on hand-worked cases, its symmetry without a cap, the torch composition of spatial.radius_graph on CPU tensors
against it, the argument checks that return before any device work, and the SchNet modules against fp64 autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spatial_ref as ref
from gnnadvisor_osdi21_amd import _lib, spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")
HEADER = "gnna_spatial.h"


# ---- the restatement on hand-worked cases ----

def _int_d2(pos, i, j):
    return int(((pos[j].astype(np.int64) - pos[i].astype(np.int64)) ** 2).sum())


@pytest.mark.parametrize("radius", list(ref.LATTICE_RADII))
@pytest.mark.parametrize("loop", [False, True])
def test_the_lattice_boundary_and_the_coincident_points(radius, loop):
    pos, gp = ref.lattice()
    largest = ref.LATTICE_RADII[radius]
    got = ref.radius_graph(pos, gp, radius, loop=loop)
    want = set()
    for g in range(len(gp) - 1):
        for i in range(gp[g], gp[g + 1]):
            for j in range(gp[g], gp[g + 1]):
                if _int_d2(pos, i, j) <= largest and (loop or i != j):          # integer arithmetic: nothing rounds
                    want.add((i, j))
    assert ref.edge_set(got) == want
    rows = np.repeat(np.arange(len(pos)), np.diff(got["row_pointers"]))
    assert [_int_d2(pos, i, j) for i, j in zip(rows, got["column_index"])] == got["dist2"].tolist()
    assert all((np.diff(got["column_index"][got["row_pointers"][i]:got["row_pointers"][i + 1]]) > 0).all() for i in range(len(pos)))
    # the four coincident points of the second set are each other's neighbours at d2 = 0
    first = int(gp[1])
    for i in range(first, first + 4):
        assert {(i, j) for j in range(first, first + 4) if loop or j != i} <= ref.edge_set(got)


def test_the_cap_breaks_ties_by_row_id_on_the_lattice():
    pos, gp = ref.lattice()
    first = int(gp[1])                    # set 1: rows first .. first + 3 are one point, +4, +6, +8 at d2 = 1, +5 at d2 = 2
    got = ref.radius_graph(pos, gp, 2.0, max_neighbors=4)
    row = lambda i: got["column_index"][got["row_pointers"][i]:got["row_pointers"][i + 1]].tolist()          # noqa: E731
    assert row(first) == [first + 1, first + 2, first + 3, first + 4]         # three at d2 = 0, then the smallest id at d2 = 1
    assert row(first + 3) == [first, first + 1, first + 2, first + 4]
    got2 = ref.radius_graph(pos, gp, 2.0, max_neighbors=2)
    assert got2["column_index"][got2["row_pointers"][first]:got2["row_pointers"][first + 1]].tolist() == [first + 1, first + 2]
    assert (np.diff(got["row_pointers"]) <= 4).all()
    # a capped structure is in general not symmetric
    edges = ref.edge_set(got)
    assert any((j, i) not in edges for i, j in edges)


def test_the_key_orders_by_distance_then_id():
    pos = np.array([[0.0], [3.0], [1.0], [-1.0], [1.0]], dtype=np.float32)
    got = ref.radius_graph(pos, [0, 5], np.inf, max_neighbors=2)
    assert got["column_index"][:2].tolist() == [2, 3] and got["dist2"][:2].tolist() == [1.0, 1.0]        # 2, 3, 4 tie: ids 2, 3


@pytest.mark.parametrize("dim", [1, 3, 7])
def test_without_a_cap_the_restatement_is_symmetric(dim):
    pos, gp = ref.random_batch([5, 0, 33, 1, 20], dim, seed=dim)
    for radius in (0.0, 1.0, np.inf):
        got = ref.radius_graph(pos, gp, radius)
        edges = ref.edge_set(got)
        assert all((j, i) in edges for i, j in edges)
        d2 = {e: v for e, v in zip(sorted(edges), got["dist2"].view(np.uint32).tolist())}
        assert all(d2[(i, j)] == d2[(j, i)] for i, j in edges)


def test_special_values_and_pointers_of_the_restatement():
    pos, gp = ref.random_batch([12, 8], 2, seed=3)
    got = ref.radius_graph(pos, gp, np.inf, loop=True)
    edges = ref.edge_set(got)
    assert (3, 3) not in edges and not any(3 in e for e in edges)      # a NaN row: every d2 with it is NaN
    assert (5, 5) not in edges and (5, 0) in edges and (0, 5) in edges   # an inf row: d2 = inf to the others, inf - inf = NaN to itself
    assert (7, 7) in edges and (7, 0) in edges        # 1e30: d2 overflows to inf, and inf <= inf
    assert np.isinf(got["dist2"][got["row_pointers"][7]])
    assert (8, 9) in edges and (9, 8) in edges
    finite = ref.edge_set(ref.radius_graph(pos, gp, 1e30, loop=True))    # r2 = inf as well: 1e30 * 1e30 overflows
    assert finite == edges
    # pointers outside [0, N] are clamped; rows outside every segment are empty
    got = ref.radius_graph(pos, [-5, 4, 4, 10, 99], 1.0)
    same = ref.radius_graph(pos, [0, 4, 4, 10, 20], 1.0)
    assert (got["row_pointers"] == same["row_pointers"]).all() and (got["column_index"] == same["column_index"]).all()
    outside = ref.radius_graph(pos, [2, 6], np.inf)
    assert set(np.repeat(np.arange(20), np.diff(outside["row_pointers"])).tolist()) == {2, 4, 5}
    assert ref.edge_set(outside) == {(2, 4), (2, 5), (4, 2), (4, 5), (5, 2), (5, 4)}
    with pytest.raises(ValueError, match="segment 1"):
        ref.radius_graph(pos, [0, 9, 4, 20], 1.0)


# ---- the torch composition on CPU tensors ----

@pytest.mark.parametrize("cap", [None, 1, 3, 64])
@pytest.mark.parametrize("loop", [False, True])
def test_the_composition_selects_the_restated_edges(cap, loop):
    cases = [ref.lattice() + (2.0,), ref.lattice() + (ref.SQRT2_ABOVE,), ref.random_batch([5, 0, 33, 1, 20], 3, seed=1) + (1.0,),
             ref.random_batch([7, 13], 4, seed=2) + (np.inf,)]
    for pos, gp, radius in cases:
        want = ref.radius_graph(pos, gp, radius, max_neighbors=cap, loop=loop)
        batch = spatial.radius_graph(torch.from_numpy(pos), radius, torch.from_numpy(gp), loop=loop, max_num_neighbors=cap, fused=False)
        assert (batch.row_pointers.numpy() == want["row_pointers"]).all()
        assert (batch.column_index.numpy() == want["column_index"]).all()
        assert (batch.edge_dist2.numpy().view(np.uint32) == want["dist2"].view(np.uint32)).all()
        assert batch.directed == (cap is not None)
    knn = spatial.knn_graph(torch.from_numpy(pos), 3, torch.from_numpy(gp), fused=False)
    want = ref.radius_graph(pos, gp, np.inf, max_neighbors=3)
    assert (knn.column_index.numpy() == want["column_index"]).all() and knn.directed


# ---- the argument checks: every call returns before it touches the device ----

_F = (ctypes.c_float * 64)()
F = ctypes.cast(_F, ctypes.c_void_p).value
_I = (ctypes.c_int32 * 64)()
I = ctypes.cast(_I, ctypes.c_void_p).value
_J = (ctypes.c_int32 * 64)()
J = ctypes.cast(_J, ctypes.c_void_p).value
_COUNTS = (ctypes.c_int64 * 3)()
INVALID, UNSUPPORTED = -1, -3


def _radius(**kw):
    a = dict(pos=F, ld=3, n=4, dim=3, gp=I, G=1, radius=1.0, cap=0, loop=0, partSize=0, rp=J, ci=ctypes.cast(_J, ctypes.c_void_p).value + 64,
             d2=None, pp=None, p2n=None, ecap=8, counts=_COUNTS)
    a.update(kw)
    return _lib.load().gnna_radius_graph_f32(a["pos"], a["ld"], a["n"], a["dim"], a["gp"], a["G"], a["radius"], a["cap"], a["loop"],
                                             a["partSize"], a["rp"], a["ci"], a["d2"], a["pp"], a["p2n"], a["ecap"], a["counts"], None)


@pytest.mark.parametrize("change, code, message", [
    (dict(counts=None), INVALID, "null counts"),
    (dict(dim=0), INVALID, r"dim must be in \[1, 64\]"),
    (dict(dim=65, ld=65), INVALID, r"dim must be in \[1, 64\]"),
    (dict(n=-1), INVALID, "negative size"),
    (dict(G=-1), INVALID, "negative size"),
    (dict(ecap=-1), INVALID, "negative size"),
    (dict(n=(1 << 31) - 1), UNSUPPORTED, "rows"),
    (dict(ld=2), INVALID, "ld_pos must be in"),
    (dict(radius=-1.0), INVALID, "radius must be >= 0"),
    (dict(radius=float("nan")), INVALID, "radius must be >= 0"),
    (dict(cap=-1), INVALID, r"max_neighbors must be in \[0, 64\]"),
    (dict(cap=65), INVALID, r"max_neighbors must be in \[0, 64\]"),
    (dict(pos=None), INVALID, "null pointer"),
    (dict(gp=None), INVALID, "null pointer"),
    (dict(rp=None), INVALID, "null pointer"),
    (dict(ci=None), INVALID, "null pointer"),
    (dict(p2n=I), INVALID, "partPtr and part2Node come together"),
    (dict(pp=J + 128, p2n=J + 192, partSize=0), INVALID, "partSize must be positive"),
    (dict(rp=I), INVALID, "an output must not alias an input"),
    (dict(d2=F), INVALID, "an output must not alias an input"),
    (dict(ci=J), INVALID, "the outputs must not alias each other"),
])
def test_what_the_entry_refuses_before_any_device_work(change, code, message):
    assert _radius(**change) == code
    text = _lib.load().gnna_last_error().decode()
    assert re.search(message, text) and text.startswith("gnna_radius_graph_f32"), text


def test_the_bindings_refuse_bad_arguments_and_host_tensors():
    pos, gp = torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32)
    for kw, message in ((dict(radius=-1.0), "radius must be >= 0"), (dict(radius=float("nan")), "radius must be >= 0"),
                        (dict(radius=1.0, max_neighbors=0), r"max_neighbors must be in \[1, 64\]"),
                        (dict(radius=1.0, max_neighbors=65), r"max_neighbors must be in \[1, 64\]"),
                        (dict(radius=1.0, partSize=0), "partSize must be positive"),
                        (dict(radius=1.0, edge_capacity=-1), "capacities must not be negative"),
                        (dict(radius=1.0), "radius_graph needs device tensors")):
        with pytest.raises(_lib.GnnaError, match=message):
            _lib.radius_graph(pos, gp, **kw)
    with pytest.raises(_lib.GnnaError, match="pos must be a float32 tensor"):
        _lib.radius_graph(pos.double(), gp, 1.0)
    with pytest.raises(_lib.GnnaError, match="1 .. 64 columns"):
        _lib.radius_graph(torch.zeros(4, 65), gp, 1.0)
    with pytest.raises(_lib.GnnaError, match="max_neighbors"):
        spatial.radius_graph(pos, 1.0, gp, max_num_neighbors=65, fused=False)
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    with pytest.raises(RuntimeError, match="pos must be a CUDA tensor"):
        GNNA.radius_graph(pos, gp, 1.0)


def test_the_header_the_module_and_the_exported_constants():
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert 'extern "C"' in header
    assert '#include "gnna_spatial.h"' in open(os.path.join(CSRC, "gnna_torch.cpp")).read()
    for name in ("LONG_ROWS", "SOURCE_TILE", "REGISTER_DIM", "MAX_DIM", "MAX_NEIGHBORS"):
        assert "#define GNNA_SPATIAL_%s %d\n" % (name, getattr(_lib, "SPATIAL_" + name)) in header
    text = " ".join(header.replace("\n *", " ").split())
    for sentence in ("Every pointer is clamped to [0, num_rows].", "No fused multiply-add is used.", "d2(i,j) == d2(j,i) to the bit.",
                     "A point exactly at the cutoff is a neighbour.", "Ties in distance go to the smaller row id.",
                     "The key is (uint64(bits(d2)) << 32) | uint32(j).", "Nothing is ever written beyond a capacity.",
                     "With max_neighbors = 0 the structure is symmetric"):
        assert sentence in text, sentence


# ---- the SchNet modules against fp64 autograd (CPU, composed) ----

def test_smearing_and_cutoff_values():
    d = torch.tensor([0.0, 0.5, 2.0, 2.5])
    smear = spatial.GaussianSmearing(0.0, 2.0, 5)
    want = torch.exp(-0.5 / 0.25 * (d[:, None] - torch.linspace(0, 2, 5)[None, :]) ** 2)
    assert torch.allclose(smear(d), want, atol=1e-6) and smear(d).shape == (4, 5)
    cut = spatial.CosineCutoff(2.0)(d)
    assert torch.allclose(cut, torch.tensor([1.0, 0.5 * (np.cos(np.pi / 4) + 1), 0.0, 0.0], dtype=torch.float32), atol=1e-6)


def test_the_interaction_gradients_match_fp64_autograd_on_cpu():
    torch.manual_seed(0)
    pos, gp = ref.random_batch([6, 9, 1, 12], 3, seed=4, specials=False)
    batch = spatial.radius_graph(torch.from_numpy(pos), 1.5, torch.from_numpy(gp), fused=False)
    assert batch.column_index.numel() > 20
    layer = spatial.SchNetInteraction(8, 8, 6, 1.5, fused=False)
    x = torch.randn(len(pos), 8, requires_grad=True)
    out = layer(x, batch)
    out.square().sum().backward()
    # the composed formula in fp64
    P = {k: v.detach().double().requires_grad_() for k, v in layer.named_parameters()}
    x64 = x.detach().double().requires_grad_()
    d = torch.from_numpy(batch.edge_dist2.numpy()).double().sqrt()
    mu = torch.linspace(0.0, 1.5, 6, dtype=torch.float32).double()
    ssp = lambda t: torch.nn.functional.softplus(t) - np.log(2.0)                                           # noqa: E731
    g = torch.exp(-0.5 / float(mu[1] - mu[0]) ** 2 * (d[:, None] - mu[None, :]) ** 2)
    W = ssp(g @ P["conv.filter_nn.lin1.weight"].T + P["conv.filter_nn.lin1.bias"]) @ P["conv.filter_nn.lin2.weight"].T \
        + P["conv.filter_nn.lin2.bias"]
    W = W * (0.5 * (torch.cos(d * np.pi / 1.5) + 1.0) * (d < 1.5))[:, None]
    rows = torch.repeat_interleave(torch.arange(len(pos)), batch.row_pointers.long().diff())
    msg = (x64 @ P["conv.lin1.weight"].T)[batch.column_index.long()] * W
    agg = torch.zeros(len(pos), 8, dtype=torch.float64).index_add_(0, rows, msg)
    want = x64 + ssp(agg @ P["conv.lin2.weight"].T + P["conv.lin2.bias"]) @ P["lin.weight"].T + P["lin.bias"]
    want.square().sum().backward()
    assert torch.allclose(out.detach().double(), want.detach(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(x.grad.double(), x64.grad, rtol=1e-3, atol=1e-4)
    for name, p in layer.named_parameters():
        assert torch.allclose(p.grad.double(), P[name].grad, rtol=1e-3, atol=1e-4), name


# ---- the driver and the synthetic point sets ----

def test_the_driver_checks_the_schnet_flags():
    from gnnadvisor_osdi21_amd import graph_main
    parser = graph_main.build_parser()
    args = parser.parse_args([])
    assert args.cutoff is None and args.max_neighbors is None and args.num_gaussians == 32 and args.fused_graph is True
    assert graph_main._parse(parser.parse_args(["--model", "schnet", "--cutoff", "1.5", "--max_neighbors", "8"]))[:2] == (8, 72)
    for argv, message in ((["--model", "gin", "--cutoff", "1.0"], "only --model schnet builds its graph from positions"),
                          (["--model", "schnet"], "--model schnet needs --cutoff R"),
                          (["--model", "schnet", "--cutoff", "1.0", "--max_neighbors", "65"], r"--max_neighbors must be in \[1, 64\]"),
                          (["--model", "schnet", "--cutoff", "1.0", "--pool", "topk"], "runs without --pool and --norm")):
        with pytest.raises(SystemExit, match=message):
            graph_main._parse(parser.parse_args(argv))


def test_small_point_clouds_are_seeded_and_labelled_by_geometry():
    from gnnadvisor_osdi21_amd import graph
    pos, gp, y = graph.small_point_clouds(48, 3, 20, seed=2, classes=4)
    again = graph.small_point_clouds(48, 3, 20, seed=2, classes=4)
    assert torch.equal(pos, again[0]) and torch.equal(gp, again[1]) and torch.equal(y, again[2])
    assert pos.dtype == torch.float32 and pos.shape == (int(gp[-1]), 3) and gp.dtype == torch.int32 and y.bincount().tolist() == [12] * 4
    mean = []
    for g in range(48):
        P = pos[int(gp[g]):int(gp[g + 1])].double()
        n = len(P)
        mean.append(float(torch.cdist(P, P).sum()) / max(n * (n - 1), 1))
    order = np.argsort(mean, kind="stable")
    assert (y[torch.from_numpy(order)].diff() >= 0).all()             # the class grows with the mean pairwise distance
    assert graph.small_point_clouds(0, 1, 2)[0].shape == (0, 3)

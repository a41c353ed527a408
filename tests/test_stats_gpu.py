"""gnna_agg_stats_ld_f32 through _lib, on the GPU: sum, sum of squares, max and min of the neighbours from one gather.

The moments are held to an fp64 reference within the project's bound 1e-4 * max(1, sum of |terms|) (assert_close_f64 with
scale = sum |x| for the sum, sum x^2 for the sum of squares).  The extrema and their positions are compared with torch.equal
against what gnna_agg_reduce_ld_f32 writes for the same arguments, and the values against an fp64 scatter_reduce.

The fp64 reference walks the partition AS GIVEN (every group [pp[p], pp[p + 1]) adds to row p2n[p]; a pair that runs backwards
is empty; ids outside the source rows are skipped), which for a partition built from a CSR is the CSR's rows."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, load_extension
from util import assert_close_f64, make_case

import test_reduce_gpu as R          # _features, _hub_graph: the inputs of the reduce tests

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 16, 33, 64, 100, 257, 300)    # every lane layout, a partial last vector, column blocks past 256
PART_SIZES = (2, 32)
ALL = ("sum", "sumsq", "max", "min")


def _edges(ci, pp, p2n, n_in, n_out):
    """(destination row, source row, position) of every edge the partition names, in int64 tensors; skipped ids left out."""
    ci, pp, p2n = (torch.as_tensor(t).cpu().long() for t in (ci, pp, p2n))
    lens = (pp[1:] - pp[:-1]).clamp(min=0)
    lens = torch.where((pp[:-1] < 0) | (p2n < 0) | (p2n >= n_out), torch.zeros_like(lens), lens)
    first = torch.cumsum(lens, 0) - lens
    pos = torch.repeat_interleave(pp[:-1] - first, lens) + torch.arange(int(lens.sum()))
    rows = torch.repeat_interleave(p2n, lens)
    src = ci[pos]
    ok = (src >= 0) & (src < n_in)
    return rows[ok], src[ok], pos[ok]


def _reference(X, ci, pp, p2n, n_out):
    """fp64: {"sum", "sumsq", "max", "min"} and the scales {"abs", "sq"} (sum |x|, sum x^2)."""
    X64 = X.cpu().double()
    rows, src, _ = _edges(ci, pp, p2n, X64.shape[0], n_out)
    G = X64[src]
    z = lambda: torch.zeros(n_out, X64.shape[1], dtype=torch.float64)
    idx = rows.unsqueeze(1).expand_as(G)
    ref = {"sum": z().index_add_(0, rows, G), "sumsq": z().index_add_(0, rows, G * G), "abs": z().index_add_(0, rows, G.abs())}
    ref["sq"] = ref["sumsq"]
    has = torch.zeros(n_out, dtype=torch.bool).index_fill_(0, rows, True).unsqueeze(1)
    for name, how in (("max", "amax"), ("min", "amin")):
        ref[name] = torch.where(has, z().scatter_reduce_(0, idx, G, how, include_self=False), z())
    return ref


def _check_moments(res, ref, what):
    for name, scale in (("sum", "abs"), ("sumsq", "sq")):
        if name in res:
            assert_close_f64(res[name].cpu().numpy(), ref[name].numpy(), scale=ref[scale].numpy(), what=f"{what} {name}")


def _check_extrema(res, X, ci, pp, p2n, ps, n_out, what, ref=None):
    """bit for bit what the reduce entry writes (values and positions); the values equal the fp64 extreme."""
    for name, op in (("max", _lib.REDUCE_MAX), ("min", _lib.REDUCE_MIN)):
        if name not in res:
            continue
        out, arg = _lib.agg_reduce_ld(op, X, ci, pp, p2n, ps, num_out_rows=n_out)
        # (NaN != NaN: the bits are compared as integers)
        assert torch.equal(res[name].view(torch.int32), out.view(torch.int32)), f"{what}: {name} differs from the reduce entry"
        assert torch.equal(res["arg" + name], arg), f"{what}: arg{name} differs from the reduce entry"
        if ref is not None:
            assert torch.equal(res[name].cpu().double(), ref[name]), f"{what}: {name} differs from fp64"


@pytest.fixture(scope="module")
def cases():
    made = {}
    for kind, (n, e) in (("uniform", (3000, 40000)), ("powerlaw", (3000, 60000))):
        g, _, _, _ = make_case(n, e, 1, 32, seed=3, kind=kind)
        parts = {ps: [t.cuda() for t in _lib.build_part(ps, g.row_pointers)] for ps in (1, 2, 8, 32)}
        made[kind] = (g, g.column_index.cuda(), parts)
    return made


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_all_four_against_fp64_and_the_reduce_entry(cases, kind):
    g, ci, parts = cases[kind]
    n = g.num_nodes
    if kind == "powerlaw":          # rows without edges and one very long row (many wavefronts at partSize 2)
        deg = np.diff(g.row_pointers.numpy())
        assert (deg == 0).any() and deg.max() > 1000
    for d in WIDTHS:
        X = R._features(n, d, "randn", seed=100 + d).cuda()
        ref = _reference(X, ci, *parts[32], n)
        for ps in PART_SIZES:
            pp, p2n = parts[ps]
            res = _lib.agg_stats_ld(X, ci, pp, p2n, n, ps)
            assert set(res) == {"sum", "sumsq", "max", "argmax", "min", "argmin"}
            what = f"{kind} D={d} partSize={ps}"
            _check_moments(res, ref, what)
            _check_extrema(res, X, ci, pp, p2n, ps, n, what, ref)


def _randint_features(n, d, seed):
    """five values with both zeros, and a few NaNs of both signs"""
    X = R._features(n, d, "randint", seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    X[torch.rand(n, d, generator=gen) < 0.2] *= -1.0             # 0 -> -0
    nan = torch.rand(n, d, generator=gen) < 0.002
    X[nan] = float("nan")
    X[nan & (torch.rand(n, d, generator=gen) < 0.5)] = -float("nan")
    bits = X.view(torch.int32)
    assert (bits == -2 ** 31).any() and (bits == 0).any() and (torch.isnan(X) & (bits < 0)).any() and (torch.isnan(X) & (bits > 0)).any()
    return X


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
def test_ties_signed_zeros_and_nans_follow_the_reduce_entry(cases, kind):
    g, ci, parts = cases[kind]
    n = g.num_nodes
    for d in (5, 64, 257):
        X = _randint_features(n, d, seed=200 + d).cuda()
        ref = _reference(torch.nan_to_num(X, nan=0.0), ci, *parts[32], n)
        for ps in PART_SIZES:
            pp, p2n = parts[ps]
            res = _lib.agg_stats_ld(X, ci, pp, p2n, n, ps)
            _check_extrema(res, X, ci, pp, p2n, ps, n, f"{kind} randint D={d} partSize={ps}")
            # the moments of the rows that no NaN reaches (a NaN in a row makes its sums NaN)
            clean = _lib.agg_stats_ld(torch.nan_to_num(X, nan=0.0), ci, pp, p2n, n, ps, want=("sum", "sumsq"))
            _check_moments(clean, ref, f"{kind} randint D={d} partSize={ps}")
            reached = torch.isnan(_lib.agg_ld(_lib.MODE_SAG, X, ci, pp, p2n, n, ps))
            assert torch.equal(torch.isnan(res["sum"]), reached) and torch.equal(torch.isnan(res["sumsq"]), reached)
            assert torch.equal(res["sum"][~reached], clean["sum"][~reached])


def _subsets():
    return [tuple(w for k, w in enumerate(ALL) if m >> k & 1) for m in range(1, 16)]


@pytest.mark.parametrize("d", [64, 7])
def test_every_subset_of_the_outputs_into_padded_buffers(cases, d):
    g, ci, parts = cases["powerlaw"]
    n, ld = g.num_nodes, d + 9
    pp, p2n = parts[32]
    X = R._features(n, d, "randn", seed=300 + d).cuda()
    ref = _reference(X, ci, pp, p2n, n)
    full = _lib.agg_stats_ld(X, ci, pp, p2n, n, 32)
    for want in _subsets():
        bufs = {w: torch.full((n, ld), float("nan"), device="cuda") for w in want}
        bufs.update({"arg" + w: torch.full((n, ld), -7, dtype=torch.int32, device="cuda") for w in want if w in ("max", "min")})
        res = _lib.agg_stats_ld(X, ci, pp, p2n, n, 32, want=want, out={k: b[:, :d] for k, b in bufs.items()})
        assert set(res) == set(bufs), want
        _check_moments(res, ref, f"subset {want}")
        for k in res:
            if k not in ("sum", "sumsq"):
                assert torch.equal(res[k], full[k]), f"subset {want}: {k} differs from the full call"
            assert res[k].data_ptr() == bufs[k].data_ptr()
            pad = bufs[k][:, d:]
            assert (torch.isnan(pad) if pad.is_floating_point() else pad == -7).all(), f"subset {want}: {k} wrote its padding"
            assert not torch.isnan(res[k]).any() and (k[:3] != "arg" or int(res[k].min()) >= -1), f"subset {want}: {k} not written"
    # positions not asked for: the value alone
    alone = _lib.agg_stats_ld(X, ci, pp, p2n, n, 32, want=("max",), out={"max": torch.empty(n, d, device="cuda")})
    assert set(alone) == {"max"} and torch.equal(alone["max"], full["max"])


@pytest.mark.parametrize("d", [64, 7])
@pytest.mark.parametrize("ps", [1, 8])
def test_shuffled_partition_and_reversed_pairs(d, ps):
    """The construction of the reduce tests: groups in shuffled order (rows split over distant groups), an empty group and a
    pair of part_pointers that runs backwards.  The answer is the statistic over the partition as given."""
    g, _, pp0, p2n0 = make_case(3000, 60000, 1, ps, seed=3, kind="powerlaw")
    P = p2n0.numel()
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(1))
    lens = (pp0[1:] - pp0[:-1]).long()[perm]
    pp = torch.zeros(P + 1, dtype=torch.int64)
    pp[1:] = torch.cumsum(lens, 0)
    starts = pp0[:-1].long()[perm]
    src = torch.repeat_interleave(starts - pp[:-1], lens) + torch.arange(int(pp[-1]))
    ci_new = g.column_index[src].contiguous()
    p2n = p2n0[perm].clone()
    pp = pp.int()
    mid = P // 2
    cut = int(pp[mid])
    pp = torch.cat([pp[:mid + 1], torch.tensor([cut, cut - 5], dtype=torch.int32), pp[mid + 1:]])
    p2n = torch.cat([p2n[:mid], torch.tensor([5, 6], dtype=torch.int32), p2n[mid:]])
    assert (pp[1:] < pp[:-1]).any() and (pp[1:] == pp[:-1]).any() and not torch.equal(p2n, p2n.sort().values)
    ci_d, pp_d, p2n_d = ci_new.cuda(), pp.cuda(), p2n.cuda()
    for xkind in ("randint", "randn"):
        X = R._features(3000, d, xkind, seed=7).cuda()
        ref = _reference(X, ci_new, pp, p2n, 3000)
        res = _lib.agg_stats_ld(X, ci_d, pp_d, p2n_d, 3000, ps)
        what = f"shuffled {xkind} D={d} partSize={ps}"
        _check_moments(res, ref, what)
        _check_extrema(res, X, ci_d, pp_d, p2n_d, ps, 3000, what, ref)


@pytest.mark.parametrize("d", [64, 7])
def test_hub_row_spanning_many_wavefronts(d):
    rp, ci, hub = R._hub_graph()
    n = rp.numel() - 1
    assert int(rp[hub + 1] - rp[hub]) > 64 * 1 * 4 and ci.numel() // 64 >= _lib.device_cus() * 16
    pp, p2n = [t.cuda() for t in _lib.build_part(1, rp)]
    ci = ci.cuda()
    X = R._features(n, d, "randn", seed=21).cuda()
    ref = _reference(X, ci, pp, p2n, n)
    res = _lib.agg_stats_ld(X, ci, pp, p2n, n, 1)
    _check_moments(res, ref, f"hub D={d}")
    _check_extrema(res, X, ci, pp, p2n, 1, n, f"hub D={d}", ref)


def test_rectangular_with_ids_outside_the_source_rows():
    n_in, n_out, d = 5000, 700, 33
    gen = torch.Generator().manual_seed(5)
    deg = torch.randint(0, 60, (n_out,), generator=gen)
    deg[::9] = 0
    rp = torch.zeros(n_out + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    ci = torch.randint(0, n_in, (int(rp[-1]),), generator=gen, dtype=torch.int32)
    pick = torch.rand(ci.numel(), generator=gen)
    ci[pick < 0.03] = -1
    ci[pick > 0.97] = n_in + 5
    ci[rp[3]:rp[4]] = -1                                     # a row whose every id is skipped: as a row without edges
    pp, p2n = [t.cuda() for t in _lib.build_part(32, rp)]
    ci_d = ci.cuda()
    X = R._features(n_in, d, "randn", seed=6).cuda()
    ref = _reference(X, ci, pp, p2n, n_out)
    res = _lib.agg_stats_ld(X, ci_d, pp, p2n, n_out, 32)
    assert all(t.shape == (n_out, d) for t in res.values())
    _check_moments(res, ref, "rectangular")
    _check_extrema(res, X, ci_d, pp, p2n, 32, n_out, "rectangular", ref)
    for i in (0, 3, 9):
        assert all(float(res[k][i].abs().max()) == 0 for k in ALL) and (res["argmax"][i] == -1).all() and (res["argmin"][i] == -1).all()
    # no group at all: every output is written, 0 and -1
    none = _lib.agg_stats_ld(X, ci_d, torch.zeros(1, dtype=torch.int32, device="cuda"),
                             torch.zeros(0, dtype=torch.int32, device="cuda"), n_out, 32)
    assert all(int(torch.count_nonzero(none[k])) == 0 for k in ALL) and (none["argmax"] == -1).all() and (none["argmin"] == -1).all()


def test_deterministic_tuning(cases):
    g, ci, parts = cases["powerlaw"]
    pp, p2n = parts[32]
    X = R._features(g.num_nodes, 64, "randn", seed=8).cuda()
    full = _lib.agg_stats_ld(X, ci, pp, p2n, g.num_nodes, 32)
    try:
        _lib.set_tuning(deterministic=1)
        for want in (ALL, ("sum",), ("sumsq", "min")):
            with pytest.raises(_lib.GnnaError, match="deterministic"):
                _lib.agg_stats_ld(X, ci, pp, p2n, g.num_nodes, 32, want=want)
        a = _lib.agg_stats_ld(X, ci, pp, p2n, g.num_nodes, 32, want=("max", "min"))
        b = _lib.agg_stats_ld(X, ci, pp, p2n, g.num_nodes, 32, want=("max", "min"))
    finally:
        _lib.reset_tuning()
    for k in ("max", "argmax", "min", "argmin"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], full[k])


def test_the_torch_binding_agrees(cases):
    GNNA = load_extension()
    g, ci, parts = cases["powerlaw"]
    pp, p2n = parts[32]
    n = g.num_nodes
    X = R._features(n, 64, "randn", seed=9).cuda()
    ref = _reference(X, ci, pp, p2n, n)
    res = _lib.agg_stats_ld(X, ci, pp, p2n, n, 32)
    got = dict(zip(("sum", "sumsq", "max", "argmax", "min", "argmin"), GNNA.aggregate_stats(X, ci, pp, p2n, 32)))
    _check_moments(got, ref, "torch binding")
    for k in ("max", "argmax", "min", "argmin"):
        assert torch.equal(got[k], res[k]), k
    s, q, mx, amx, mn, amn = GNNA.aggregate_stats(X[:, 8:24], ci, pp, p2n, 32, num_out_rows=n, want_sumsq=False, want_min=False)
    assert q is None and mn is None and amn is None and torch.equal(mx, res["max"][:, 8:24]) and torch.equal(amx, res["argmax"][:, 8:24])
    assert_close_f64(s.cpu().numpy(), ref["sum"][:, 8:24].numpy(), scale=ref["abs"][:, 8:24].numpy(), what="torch binding, strided X")


def test_captured_call_replayed_with_new_inputs(cases):
    g, ci, parts = cases["powerlaw"]
    pp, p2n = parts[32]
    n, d = g.num_nodes, 64
    X = R._features(n, d, "randn", seed=30).cuda()
    bufs = {k: torch.empty(n, d, device="cuda") for k in ALL}
    bufs.update({k: torch.empty(n, d, dtype=torch.int32, device="cuda") for k in ("argmax", "argmin")})
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=torch.cuda.Stream()):    # a stream that never ran the library: no eager scratch on it
        _lib.agg_stats_ld(X, ci, pp, p2n, n, 32, out=bufs)
    for rep in range(2):
        X.copy_(R._features(n, d, "randn", seed=40 + rep))
        for k, b in bufs.items():
            b.fill_(-9 if k[:3] == "arg" else float("nan"))
        gr.replay()
        torch.cuda.synchronize()
        eager = _lib.agg_stats_ld(X, ci, pp, p2n, n, 32)
        ref = _reference(X, ci, pp, p2n, n)
        _check_moments(bufs, ref, f"replay {rep}")
        _check_moments(eager, ref, f"eager {rep}")
        for k in ("max", "argmax", "min", "argmin"):
            assert torch.equal(bufs[k], eager[k]), f"replay {rep}: {k}"

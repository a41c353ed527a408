"""The dense hub-to-hub block of a prepared graph (csrc/gnna_dense.hip): the sweep kernel walks the residual graph and
hub_block_kernel adds the bitmap block with f32 MFMA.

Shapes.  The block is only taken by a call whose sweep is not forced to a phase count, so the graph has to be one the
library slices by itself: more than 8 MiB of gathered source rows, i.e. a little over 32,768 rows of 64 floats.  36,000
nodes, 1.66 M edges, degrees up to 2,300 (powerlaw_graph, seed 11).  hub_block_kernel gives a workgroup 32 destination ranks
and pads the ranks to 128 (its chunk of source ranks).  Counted on the CPU for that graph: degree >= 400 gives 524 hubs (17
workgroups, the last with 12 ranks; padded to 640) and 119,718 block entries; >= 1,500 gives 104 hubs (less than one chunk)
and 10,472 entries; the 20 highest degrees give fewer than 32 hubs (less than one workgroup's tile); >= 100 gives 2,603 hubs
and 451,024 entries; >= 32 gives 9,497 hubs, which a 256-CU chip trims to 8,192 (one workgroup per compute unit).
`Case.hubs` re-counts them in the cases that rely on them.

Bound: |got - ref| <= 1e-4 * max(1, |ref|) against the fp64 CSR formula (no row has more than 4,096 edges); the
degree-weighted form uses the sum of |terms| as everywhere in the suite (tests/util.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from gnnadvisor_osdi21_amd import _lib, graph
from util import assert_close_f64

pytestmark = pytest.mark.gpu

N, E, MAXDEG, PS = 36000, 1800000, 3000, 32


@functools.lru_cache(maxsize=None)
def _base():
    g = graph.powerlaw_graph(N, E, MAXDEG, seed=11)
    rp, ci = g.row_pointers.numpy().astype(np.int64), g.column_index.numpy().astype(np.int64)
    rows = np.repeat(np.arange(N), np.diff(rp))
    rows.setflags(write=False)
    ci.setflags(write=False)
    return rows, ci


@functools.lru_cache(maxsize=None)
def _features(dim, kind="randn"):
    if kind == "ones":
        return torch.ones(N, dim)
    return torch.randn(N, dim, generator=torch.Generator().manual_seed(1000 + dim))


class Case:
    """A CSR built from (row, column) pairs AS THEY ARE (repeats stay), its partition, and everything on the device."""

    def __init__(self, rows, cols, shuffle_groups=False):
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
        self.rp = np.zeros(N + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows, minlength=N), out=self.rp[1:])
        self.ci = cols.astype(np.int32)
        self.deg_count = np.diff(self.rp)
        pp, p2n = _lib.build_part(PS, torch.from_numpy(self.rp))
        ci_t = torch.from_numpy(self.ci)
        if shuffle_groups:
            # the same groups in another order: neither part2Node nor part_pointers is non-decreasing any more
            P = p2n.numel()
            perm = torch.randperm(P, generator=torch.Generator().manual_seed(5))
            lens = (pp[1:] - pp[:-1])[perm].long()
            starts = pp[:-1][perm].long()
            new_pp = torch.zeros(P + 1, dtype=pp.dtype)
            new_pp[1:] = torch.cumsum(lens, 0)
            take = torch.repeat_interleave(starts - new_pp[:-1].long(), lens) + torch.arange(int(lens.sum()))
            new_ci = ci_t[take]
            # column_index keeps its CSR meaning for the reference (self.rp / self.ci); the library sees the shuffled arrays
            ci_t, pp, p2n = new_ci.contiguous(), new_pp, p2n[perm].contiguous()
        self.deg = torch.from_numpy(1.0 / np.sqrt(np.maximum(self.deg_count, 1)).astype(np.float32))
        self.ci_d, self.pp_d, self.p2n_d, self.deg_d = ci_t.cuda(), pp.int().cuda(), p2n.int().cuda(), self.deg.cuda()

    def hubs(self, theta):
        hub = self.deg_count >= theta
        rows = np.repeat(np.arange(N), self.deg_count)
        pairs = np.unique(rows[hub[rows] & hub[self.ci]].astype(np.int64) * N + self.ci[hub[rows] & hub[self.ci]])
        return int(hub.sum()), int(pairs.size), hub

    def ref(self, mode, X, eps=1.0):
        return oracle.csr_f64(mode, X.numpy(), self.rp, self.ci, self.deg.numpy() if mode == 1 else None, eps)

    def gcn_scale(self, X):
        return oracle.csr_f64(1, np.abs(X.numpy()), self.rp, self.ci, self.deg.numpy())

    def run(self, mode, Xd, eps=1.0, **kw):
        deg = self.deg_d if mode == 1 else None
        return _lib.agg_ld(mode, Xd, self.ci_d, self.pp_d, self.p2n_d, N, PS, degrees_out=deg, degrees_in=deg, epsilon=eps, **kw)

    def prepare(self, dims=(64,)):
        return _lib.prepare_graph(self.ci_d, self.pp_d, self.p2n_d, N, N, PS, list(dims))


@functools.lru_cache(maxsize=None)
def _plain():
    rows, ci = _base()
    return Case(rows, ci)


class dense:
    """GNNA_DENSE_BLOCK (and the tests' theta) for the prepares inside, sweep = 1, no forced phase count."""

    def __init__(self, mode=2, theta=400, **tuning):
        self.env = {"GNNA_DENSE_BLOCK": str(mode), "GNNA_DENSE_BLOCK_THETA": "" if theta is None else str(theta)}
        self.tuning = dict(sweep=1, deterministic=0, gcn_prescale=1)
        self.tuning.update(tuning)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        _lib.release_graph(None)
        _lib.reset_tuning()
        _lib.set_tuning(**self.tuning)
        self.before = _lib.runtime_counters()
        return self

    def delta(self, name):
        return _lib.runtime_counters()[name] - self.before[name]

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.reset_tuning()
        _lib.release_graph(None)


def _check_block(case, theta, min_hubs, max_hubs):
    H, entries, _ = case.hubs(theta)
    assert min_hubs <= H <= max_hubs and entries > 0, (theta, H, entries)
    return H, entries


@pytest.mark.parametrize("dim", [64, 41])
def test_ones_are_exact(dim):
    c = _plain()
    _check_block(c, 400, 500, 550)
    with dense() as d:
        c.prepare([dim])
        assert d.delta("dense_block_builds") == 1
        y = c.run(0, _features(dim, "ones").cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    want = np.repeat(c.deg_count.astype(np.float32)[:, None], dim, 1)
    assert np.array_equal(y, want), int((y != want).any(1).sum())


@pytest.mark.parametrize("theta,lo,hi,what", [("top20", 8, 31, "less than one workgroup's 32 ranks"), (1500, 64, 127, "less than one chunk"),
                                              (400, 513, 639, "ragged last tile and chunk"), (None, 1, 16384, "the rule's own theta")])
def test_hub_counts(theta, lo, hi, what):
    c = _plain()
    if theta == "top20":
        theta = int(np.sort(c.deg_count)[-20])
    if theta is not None:
        H, _ = _check_block(c, theta, lo, hi)
        assert H % 128 != 0 and H % 32 != 0
    X = _features(64)
    with dense(theta=theta) as d:
        c.prepare()
        y = c.run(0, X.cuda())
        assert d.delta("dense_block_launches") == 1, what
    assert_close_f64(y.cpu().numpy(), c.ref(0, X), what=what)


@functools.lru_cache(maxsize=None)
def _planted():
    """Self-loops on hubs, hub-to-hub edges stored two and three times, and a hub whose row is exactly the hubs (its residual
    row is empty)."""
    rows, ci = _base()
    plain = _plain()
    _, _, hub = plain.hubs(400)
    hub_ids = np.flatnonzero(hub)
    hh = np.flatnonzero(hub[rows] & hub[ci])
    rng = np.random.default_rng(3)
    twice = rng.choice(hh, 300, replace=False)
    thrice = twice[:100]
    full = hub_ids[np.argmax(plain.deg_count[hub_ids])]         # this row becomes: every hub once (itself included)
    keep = rows != full
    new_rows = np.concatenate([rows[keep], rows[twice], rows[thrice], hub_ids[:50], np.full(hub_ids.size, full)])
    new_cols = np.concatenate([ci[keep], ci[twice], ci[thrice], hub_ids[:50], hub_ids])
    c = Case(new_rows, new_cols)
    H, entries, hub2 = c.hubs(400)
    assert hub2[full] and H >= 500, (H, int(c.deg_count[full]))
    assert np.all(hub2[c.ci[c.rp[full]: c.rp[full + 1]]]), "the full row holds hubs only"
    assert c.ci.size > entries + 400, "the repeats are extra edges"
    return c, int(full)


def test_self_loops_repeated_ids_and_an_empty_residual_row():
    c, full = _planted()
    X = _features(64)
    out = torch.full((N, 64), float("nan"), device="cuda")
    with dense() as d:
        c.prepare()
        c.run(0, X.cuda(), out=out)
        assert d.delta("dense_block_launches") == 1
        ones = c.run(0, _features(64, "ones").cuda()).cpu().numpy()
    assert_close_f64(out.cpu().numpy(), c.ref(0, X), what="planted")
    # multiplicity: an id stored three times counts three times
    assert np.array_equal(ones, np.repeat(c.deg_count.astype(np.float32)[:, None], 64, 1))
    assert ones[full, 0] == c.deg_count[full]


def test_gin_gcn_accumulate_and_padded_output():
    c = _plain()
    X = _features(50)
    Xd = X.cuda()
    with dense() as d:
        c.prepare([50])
        yi = c.run(2, Xd, eps=0.5)
        yg = c.run(1, Xd)
        acc = torch.full((N, 50), 3.0, device="cuda")
        c.run(0, Xd, out=acc, accumulate=True)
        wide = torch.full((N, 72), float("nan"), device="cuda")
        c.run(0, Xd, out=wide[:, 8:58])
        assert d.delta("dense_block_launches") == 4
    assert_close_f64(yi.cpu().numpy(), c.ref(2, X, 0.5), what="gin")
    assert_close_f64(yg.cpu().numpy(), c.ref(1, X), what="gcn (pre-scaled)", scale=c.gcn_scale(X))
    sag = c.ref(0, X)
    assert_close_f64(acc.cpu().numpy(), sag + 3.0, what="accumulate", scale=np.abs(sag) + 3.0)
    w = wide.cpu().numpy()
    assert_close_f64(w[:, 8:58], sag, what="padded output")
    assert np.isnan(w[:, :8]).all() and np.isnan(w[:, 58:]).all(), "the padding of the output was written"


def test_shuffled_partition():
    rows, ci = _base()
    c = Case(rows, ci, shuffle_groups=True)
    X = _features(64)
    with dense() as d:
        c.prepare()
        y = c.run(0, X.cuda())
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y.cpu().numpy(), _plain().ref(0, X), what="shuffled partition")


def test_first_call_in_a_capture():
    c = _plain()
    X = _features(64)
    Xd = X.cuda()
    out = torch.empty_like(Xd)
    with dense() as d:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c.prepare()
            side.synchronize()
            before = _lib.runtime_counters()
            graph_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_, stream=side):
                c.run(0, Xd, out=out)
        after = _lib.runtime_counters()
        assert after["dense_block_launches"] == before["dense_block_launches"] + 1
        for k in ("plan_builds", "launch_syncs", "launch_mallocs", "launch_frees"):
            assert after[k] == before[k], k
        for _ in range(2):
            out.fill_(float("nan"))
            graph_.replay()
            torch.cuda.synchronize()
            assert_close_f64(out.cpu().numpy(), c.ref(0, X), what="replay")
        del graph_


def test_stale_ids_follow_the_new_ids():
    rows, ci = _base()
    c = Case(rows, ci)                       # (its own tensors: they are overwritten)
    _, _, hub = c.hubs(400)
    X = _features(64)
    Xd = X.cuda()
    with dense(ids_check_every=1) as d:
        c.prepare()
        y0 = c.run(0, Xd)
        assert_close_f64(y0.cpu().numpy(), c.ref(0, X), what="before the change")
        all_rows = np.repeat(np.arange(N), c.deg_count)
        e = int(np.flatnonzero(hub[all_rows] & hub[c.ci])[7])
        new_src = int(np.flatnonzero(c.deg_count == c.deg_count[c.deg_count > 0].min())[0])
        assert not hub[new_src] and new_src != c.ci[e]
        c.ci_d[e] = new_src                  # in place: the promise of gnna_prepare_graph is broken
        c.ci[e] = new_src
        y1 = c.run(0, Xd)
        assert d.delta("full_hashes") >= 2
    assert_close_f64(y1.cpu().numpy(), c.ref(0, X), what="after the change")
    assert not np.array_equal(y0.cpu().numpy(), y1.cpu().numpy())


@pytest.mark.parametrize("how", ["relu", "deterministic", "forced phases", "env 0"])
def test_the_path_stays_off(how):
    c = _plain()
    X = _features(64)
    Xd = X.cuda()
    relu = how == "relu"
    with dense(mode=0 if how == "env 0" else 2) as d:
        c.prepare()
        assert d.delta("dense_block_builds") == (0 if how == "env 0" else 1)
        if how == "deterministic":
            _lib.set_tuning(deterministic=1)
        if how == "forced phases":
            _lib.set_tuning(column_phases=8)
        y = c.run(0, Xd, relu=relu)
        assert d.delta("dense_block_launches") == 0, how
        # today's path: the same call on a graph that has no block
        os.environ["GNNA_DENSE_BLOCK"] = "0"
        _lib.release_graph(None)
        c.prepare()
        y_off = c.run(0, Xd, relu=relu)
        assert d.delta("dense_block_launches") == 0
    ref = c.ref(0, X)
    ref = np.maximum(ref, 0.0) if relu else ref
    assert_close_f64(y.cpu().numpy(), ref, what=how)
    assert_close_f64(y_off.cpu().numpy(), ref, what=how + ", no block")
    if how == "deterministic":
        assert torch.equal(y, y_off)         # (the other schedules add shared rows with float atomics: no fixed order)


def test_release_stops_the_launches():
    c = _plain()
    X = _features(64)
    with dense() as d:
        c.prepare()
        c.run(0, X.cuda())
        assert d.delta("dense_block_launches") == 1
        _lib.release_graph(c.ci_d)
        y = c.run(0, X.cuda())
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y.cpu().numpy(), c.ref(0, X), what="after release")


def test_hubs_beyond_a_whole_round_of_workgroups_are_trimmed(capfd):
    """A few hubs more than 32 x compute units would give some compute units a second workgroup and double the kernel's time:
    the lowest-degree hubs beyond the round stay in the gather (sorted by degree, cut, ranked by id again)."""
    c = _plain()
    round_ = 32 * _lib.device_cus()
    thetas = [t for t in range(8, 200) if round_ < int((c.deg_count >= t).sum()) < round_ + round_ // 4]
    assert thetas, "no threshold of this graph puts the hub count just beyond one round on this chip"
    theta = thetas[-1]
    H_all = int((c.deg_count >= theta).sum())
    X = _features(64)
    with dense(theta=theta) as d:
        os.environ["GNNA_DENSE_BLOCK_LOG"] = "1"
        try:
            c.prepare()
        finally:
            os.environ.pop("GNNA_DENSE_BLOCK_LOG", None)
        log = capfd.readouterr().err
        y = c.run(0, X.cuda())
        ones = c.run(0, _features(64, "ones").cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 2
    assert f"theta {theta}, H {round_} " in log, (H_all, log)
    assert_close_f64(y.cpu().numpy(), c.ref(0, X), what="trimmed hubs")
    assert np.array_equal(ones, np.repeat(c.deg_count.astype(np.float32)[:, None], 64, 1))


@pytest.mark.parametrize("dim", [16, 32])
def test_rows_of_one_line_get_no_block(dim):
    """The rule's constants hold for rows of two 128-byte lines (33 .. 64 floats).  A narrower row is one request per edge: the
    sweep would save half as much per edge taken out.  No block is built or used there, under any GNNA_DENSE_BLOCK."""
    c = _plain()
    X = _features(dim)
    with dense(column_phases=0) as d:
        c.prepare([dim])
        y = c.run(0, X.cuda())
        assert d.delta("dense_block_builds") == 0 and d.delta("dense_block_launches") == 0
    assert_close_f64(y.cpu().numpy(), c.ref(0, X), what=f"dim {dim}")


def test_a_graph_that_gets_no_block_is_counted_once():
    """No node reaches the threshold, so the build ends after its degree and histogram passes with no block.  That is
    remembered on the plan: the next width of the same prepare and a second prepare of the same graph allocate nothing."""
    c = _plain()
    X = _features(64)
    with dense(theta=100000) as d:
        c.prepare([64])
        assert d.delta("dense_block_builds") == 0
        before = _lib.runtime_counters()
        c.prepare([64, 48])
        c.prepare([64])
        after = _lib.runtime_counters()
        assert after["launch_frees"] == before["launch_frees"]       # (the build's scratch is freed when it returns)
        y = c.run(0, X.cuda())
        assert d.delta("dense_block_launches") == 0
    assert_close_f64(y.cpu().numpy(), c.ref(0, X), what="no block")

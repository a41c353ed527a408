"""The pre-pass launch (csrc/gnna_agg.hip: prepass_kernel): the staging copy, the dense prologue (zero-fill, partition
validation, the sweep's sync words), the packed-id sample check and the hub-row split of the dense block as block ranges of ONE
launch in front of the aggregation kernel.  GNNA_PREPASS=0 keeps every pass a launch of its own; GNNA_PREPASS_LOG=1 prints the
roles of a pre-pass launch and their block counts, which is how these tests see which path a call took.

Shapes.  The case of tests/test_hub_block_rate_gpu.py: powerlaw_graph(36000, 1800000, 3000, seed=11), partSize 32 -- the smallest
graph the library sweeps by itself; its contiguous rows of 17 .. 64 floats are staged to a stride of 128 floats, so every role
runs.  Widths 33 / 36 / 48 / 64: the split's partial-piece form (33) and its whole-piece form, and both column-tile counts of
the block kernel (3 up to 48 floats, 4 beyond).  Dense blocks of two and of three 128-rank chunks.

Bounds.  Against the fp64 CSR formula: the suite's |got - ref| <= 1e-4 * max(1, |ref|) (util.assert_close_f64; the degree-weighted
form against the sum of |coef * x|, as everywhere in the suite).  Integer-valued features -- values in -3 .. 3, degree factors
that are powers of two from 1/4 to 2 -- make every partial sum a multiple of 1/4 below 2 * 3 * 3000 = 18,000, i.e. an integer
below 2^17 in units of 1/4: exact in fp32 in any order, so both paths must equal the reference bit for bit."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import oracle
from gnnadvisor_osdi21_amd import _lib
from test_hub_block_rate_gpu import CHUNK, N, PS, Case, _case, _features, _ones_want, _sag_ref, dense
from util import assert_close_f64

pytestmark = pytest.mark.gpu

DIMS = [33, 36, 48, 64]
LINE = re.compile(r"gnna prepass: stage (\d+), fill (\d+) \(zero-fill (\d), validate (\d)\), check (\d+), split (\d+) blocks")


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def logged(capfd, fn, prepass=None):
    """fn() under GNNA_PREPASS_LOG=1 (and GNNA_PREPASS=prepass, None: unset) -> (its result, one dict per pre-pass launch)."""
    capfd.readouterr()
    with env(GNNA_PREPASS_LOG=1, GNNA_PREPASS=prepass):
        got = fn()
        torch.cuda.synchronize()
    found = [LINE.search(line) for line in capfd.readouterr().err.splitlines()]
    names = ("stage", "fill", "zero_fill", "validate", "check", "split")
    return got, [dict(zip(names, (int(x) for x in m.groups()))) for m in found if m]


def theta_of(chunks):
    theta, H = _case().theta_for((chunks - 1) * CHUNK, chunks * CHUNK)
    assert (H + CHUNK - 1) // CHUNK == chunks
    return theta, (H + CHUNK - 1) // CHUNK * CHUNK


@functools.lru_cache(maxsize=None)
def _int_features(dim):
    return torch.randint(-3, 4, (N, dim), generator=torch.Generator().manual_seed(3000 + dim)).float()


@functools.lru_cache(maxsize=None)
def _pow2_degrees():
    return torch.from_numpy(np.exp2((np.arange(N) % 4) - 2.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _int_refs(dim):
    """SAG, GIN (eps 0.5) and GCN (power-of-two factors) of the integer features by the fp64 formula; each is checked to be
    exactly representable in fp32 with room to spare, partial sums included (the header)."""
    c, X, deg = _case(), _int_features(dim), _pow2_degrees()
    assert int(c.deg_count.max()) <= 3000 and float(X.abs().max()) <= 3.0 and 4 * 2 * 3 * 3000 < 2 ** 24
    refs = {0: c.ref(0, X), 2: c.ref(2, X, 0.5), 1: oracle.csr_f64(1, X.numpy(), c.rp, c.ci, deg.numpy())}
    for ref in refs.values():
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(ref).max() < 2 ** 22
        ref.setflags(write=False)
    return refs


def _run_mode(c, mode, Xd, degd, **kw):
    if mode == 1:
        return c.run(1, Xd, degrees_out=degd, degrees_in=degd, **kw)
    return c.run(mode, Xd, eps=0.5 if mode == 2 else 1.0, **kw)


@pytest.mark.parametrize("chunks", [2, 3])
@pytest.mark.parametrize("dim", DIMS)
def test_same_bits_as_the_separate_launches(capfd, dim, chunks):
    c = _case()
    theta, H_pad = theta_of(chunks)
    Xd, degd = _int_features(dim).cuda(), _pow2_degrees().cuda()
    refs = _int_refs(dim)
    with dense(theta) as d:
        c.prepare([dim])
        for mode in (0, 2, 1):
            apart, log0 = logged(capfd, lambda: _run_mode(c, mode, Xd, degd).cpu().numpy(), prepass=0)
            fused, log1 = logged(capfd, lambda: _run_mode(c, mode, Xd, degd).cpu().numpy(), prepass=1)
            assert log0 == [], log0
            assert len(log1) == 1 and log1[0]["stage"] > 0 and log1[0]["fill"] > 0 and log1[0]["check"] == 1, log1
            assert log1[0]["split"] == H_pad // 32 and log1[0]["zero_fill"] == 1 and log1[0]["validate"] == 1, log1
            want = refs[mode].astype(np.float32)
            assert np.array_equal(apart, fused), (mode, int((apart != fused).any(1).sum()))
            assert np.array_equal(fused, want), (mode, int((fused != want).any(1).sum()))
        assert d.delta("dense_block_launches") == 6


@functools.lru_cache(maxsize=None)
def _gcn_ref(dim):
    c, X = _case(), _features(dim)
    ref = oracle.csr_f64(1, X.numpy(), c.rp, c.ci, c.deg.numpy())
    scale = oracle.csr_f64(1, X.abs().numpy(), c.rp, c.ci, c.deg.numpy())
    ref.setflags(write=False)
    scale.setflags(write=False)
    return ref, scale


@pytest.mark.parametrize("dim", DIMS)
def test_random_features_and_ones(capfd, dim):
    c = _case()
    theta, H_pad = theta_of(3)
    Xd, degd = _features(dim).cuda(), c.deg.cuda()
    with dense(theta):
        c.prepare([dim])
        (sag, gin, gcn, ones), log = logged(capfd, lambda: [y.cpu().numpy() for y in (
            c.run(0, Xd), c.run(2, Xd, eps=0.5), c.run(1, Xd, degrees_out=degd, degrees_in=degd),
            c.run(0, torch.ones(N, dim, device="cuda")))])
    assert len(log) == 4 and all(r["stage"] > 0 and r["split"] == H_pad // 32 and r["check"] == 1 for r in log), log
    assert_close_f64(sag, _sag_ref(dim), what=f"sag, D {dim}")
    assert_close_f64(gin, 0.5 * _sag_ref(dim), what=f"gin, D {dim}")
    ref, scale = _gcn_ref(dim)
    assert_close_f64(gcn, ref, what=f"gcn, D {dim}", scale=scale)
    want = _ones_want(dim)
    assert np.array_equal(ones, want), int((ones != want).any(1).sum())


@pytest.mark.parametrize("dim,ld,first", [(64, 67, 1), (48, 68, 4)])
def test_strided_input_and_output(capfd, dim, ld, first):
    """The split reads the caller's rows: ld_in 67 at column 1 is the partial-piece form (no 16-byte piece is aligned), ld_in 68 at
    column 4 the whole-piece form.  NaN around the input's columns, sevens around the output's."""
    c = _case()
    theta, H_pad = theta_of(3)
    buf = torch.full((N, ld), float("nan"))
    buf[:, first:first + dim] = _features(dim)
    view = buf.cuda()[:, first:first + dim]
    assert view.stride(0) == ld and view.data_ptr() % 16 == (4 * first) % 16
    out = torch.full((N, 68), 7.0, device="cuda")
    with dense(theta):
        c.prepare([dim])
        _, log = logged(capfd, lambda: c.run(0, view, out=out[:, 2:2 + dim]))
    assert len(log) == 1 and log[0]["stage"] > 0 and log[0]["split"] == H_pad // 32, log
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    assert (got[:, :2] == 7.0).all() and (got[:, 2 + dim:] == 7.0).all(), "the padding of the output was written"
    assert_close_f64(got[:, 2:2 + dim], _sag_ref(dim), what=f"ld_in {ld}, ld_out 68")


def test_accumulate(capfd):
    c = _case()
    theta, H_pad = theta_of(2)
    dim = 48
    base = torch.randn(N, dim, generator=torch.Generator().manual_seed(77))
    acc = base.cuda()
    with dense(theta):
        c.prepare([dim])
        _, log = logged(capfd, lambda: c.run(0, _features(dim).cuda(), out=acc, accumulate=True))
    assert len(log) == 1 and log[0]["zero_fill"] == 0 and log[0]["stage"] > 0 and log[0]["split"] == H_pad // 32, log
    assert_close_f64(acc.cpu().numpy(), base.numpy().astype(np.float64) + _sag_ref(dim), what="accumulate")


def test_a_gapped_layout_from_the_caller_has_no_stage_role(capfd):
    c = _case()
    theta, H_pad = theta_of(3)
    dim = 64
    buf = torch.zeros(N, 128, device="cuda")
    assert buf.data_ptr() % 512 == 0
    view = buf[:, :dim]
    view.copy_(_features(dim))
    ones = torch.zeros(N, 128, device="cuda")
    ones[:, :dim] = 1.0
    with dense(theta):
        c.prepare([dim])
        (y, y1), log = logged(capfd, lambda: [t.cpu().numpy() for t in (c.run(0, view), c.run(0, ones[:, :dim]))])
    assert len(log) == 2, log
    for r in log:
        assert r["stage"] == 0 and r["fill"] > 0 and r["check"] == 1 and r["split"] == H_pad // 32, log
    assert_close_f64(y, _sag_ref(dim), what="gapped layout")
    assert np.array_equal(y1, _ones_want(dim))


def test_a_partition_that_is_not_canonical(capfd):
    """The groups of the same partition in reversed order: part2Node decreases, the validation inside the pre-pass raises the
    call's flag and every row is added atomically."""
    c = _case()
    theta, H_pad = theta_of(2)
    dim = 64
    pp, p2n = c.pp_d.cpu().numpy().astype(np.int64), c.p2n_d.cpu().numpy()
    P = p2n.size
    order = np.arange(P)[::-1]
    lens = np.diff(pp)[order]
    pp_new = np.zeros(P + 1, dtype=np.int64)
    pp_new[1:] = np.cumsum(lens)
    take = np.repeat(pp[:-1][order] - pp_new[:-1], lens) + np.arange(int(pp_new[-1]))
    ci_d = torch.from_numpy(c.ci[take].copy()).cuda()
    pp_d = torch.from_numpy(pp_new.astype(np.int32)).cuda()
    p2n_d = torch.from_numpy(p2n[order].copy()).cuda()
    assert (np.diff(p2n[order]) < 0).any()
    with dense(theta) as d:
        _lib.prepare_graph(ci_d, pp_d, p2n_d, N, N, PS, [dim])
        y, log = logged(capfd, lambda: _lib.agg_ld(0, _features(dim).cuda(), ci_d, pp_d, p2n_d, N, PS).cpu().numpy())
        assert d.delta("dense_block_launches") == 1
    assert len(log) == 1 and log[0]["validate"] == 1 and log[0]["split"] == H_pad // 32, log
    assert_close_f64(y, _sag_ref(dim), what="reversed groups")


def test_stale_ids_follow_the_new_ids(capfd):
    """column_index rewritten in place behind a prepared graph: the check role raises the stale flag, the split of the same
    launch runs for nothing, the sweep reads the caller's arrays and the block kernel returns."""
    c = Case()                                # (its own tensors: they are overwritten)
    theta, H_pad = theta_of(3)
    dim = 64
    X = _features(dim)
    Xd = X.cuda()
    relabel = torch.randperm(N, generator=torch.Generator().manual_seed(123)).numpy().astype(np.int32)
    ci2 = relabel[c.ci]                       # another graph with the same row lengths
    assert (ci2 != c.ci).mean() > 0.99
    with dense(theta):
        c.prepare([dim])
        y0 = c.run(0, Xd).cpu().numpy()
        c.ci_d.copy_(torch.from_numpy(ci2))
        y1, log = logged(capfd, lambda: c.run(0, Xd).cpu().numpy())
    assert len(log) == 1 and log[0]["check"] == 1 and log[0]["split"] == H_pad // 32, log
    assert_close_f64(y0, _sag_ref(dim), what="before the change")
    assert_close_f64(y1, oracle.csr_f64(0, X.numpy(), c.rp, ci2), what="after the change")


def test_no_dense_block_prepared(capfd):
    c = _case()
    theta, _ = theta_of(2)
    dim = 64
    ctx = dense(theta)
    ctx.env["GNNA_DENSE_BLOCK"] = "0"
    with ctx as d:
        c.prepare([dim])
        y, log = logged(capfd, lambda: c.run(0, _features(dim).cuda()).cpu().numpy())
        assert d.delta("dense_block_builds") == 0 and d.delta("dense_block_launches") == 0 and d.delta("sweep_launches") == 1
    assert len(log) == 1 and log[0]["stage"] > 0 and log[0]["fill"] > 0 and log[0]["check"] == 1 and log[0]["split"] == 0, log
    assert_close_f64(y, _sag_ref(dim), what="no block")


@pytest.mark.parametrize("dim", [41, 3])
def test_unprepared_call_on_the_streaming_kernel(capfd, dim):
    """No prepared graph, the sweep off: the streaming kernel behind the dense prologue (the output is far below the 32 MB from
    which the sparse one runs).  Rule (b) of the row stride: 41-float rows are staged to a stride of 48; 3-float rows are always
    gathered as 4-float rows.  Stage + fill, nothing else."""
    c = _case()
    X = torch.randn(N, dim, generator=torch.Generator().manual_seed(4000 + dim))
    _lib.release_graph(None)
    _lib.reset_tuning()
    _lib.set_tuning(sweep=2, pad_rows=1)
    try:
        before = _lib.runtime_counters()["sweep_launches"]
        y, log = logged(capfd, lambda: c.run(0, X.cuda()).cpu().numpy())
        assert _lib.runtime_counters()["sweep_launches"] == before
    finally:
        _lib.reset_tuning()
        _lib.release_graph(None)
    assert len(log) == 1 and log[0]["stage"] > 0 and log[0]["fill"] > 0 and log[0]["check"] == 0 and log[0]["split"] == 0, log
    assert_close_f64(y, c.ref(0, X), what=f"streaming kernel, D {dim}")


def test_capture_and_replay_on_new_features():
    c = _case()
    theta, _ = theta_of(3)
    dim = 64
    Xd = torch.zeros(N, dim, device="cuda")
    out = torch.empty_like(Xd)
    with dense(theta) as d:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c.prepare([dim])
            c.run(0, Xd, out=out)             # warm-up (scratch)
            side.synchronize()
            before = _lib.runtime_counters()
            graph_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_, stream=side):
                c.run(0, Xd, out=out)
        assert d.delta("dense_block_launches") == 2
        Xd.copy_(_features(dim))              # in place: the replay reads the new rows
        out.fill_(float("nan"))
        graph_.replay()
        torch.cuda.synchronize()
        after = _lib.runtime_counters()
        for k in ("plan_builds", "launch_syncs", "launch_mallocs", "launch_frees"):
            assert after[k] == before[k], k
        assert_close_f64(out.cpu().numpy(), _sag_ref(dim), what="replay")
        del graph_


def test_two_streams_one_prepared_graph():
    c = _case()
    theta, _ = theta_of(3)
    dims = (64, 64)
    Xs = [_features(64).cuda(), (2.0 * _features(64) + 1.0).cuda()]
    refs = [_sag_ref(64), c.ref(0, 2.0 * _features(64) + 1.0)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    with dense(theta):
        c.prepare([dims[0]])
        for k, s in enumerate(streams):       # warm-up: each stream's scratch
            with torch.cuda.stream(s):
                c.run(0, Xs[k])
        torch.cuda.synchronize()
        for k, s in enumerate(streams):       # back to back: nothing waits in between
            with torch.cuda.stream(s):
                outs[k] = c.run(0, Xs[k])
        torch.cuda.synchronize()
    for k in range(2):
        assert_close_f64(outs[k].cpu().numpy(), refs[k], what=f"stream {k}")

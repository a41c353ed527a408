"""hub_block_kernel's schedule (csrc/gnna_dense.hip): two LDS images that take the 128-rank chunks in turn, loads two
chunks ahead, one instantiation per count of 16-column tiles (3 for D <= 48, 4 beyond) and per staging form (whole
16-byte pieces when D and the leading dimension are multiples of 4, the partial-piece form otherwise).

Shapes.  The graph of tests/test_dense_block_gpu.py: powerlaw_graph(36000, 1800000, 3000, seed=11), partSize 32 -- the
smallest graph the library sweeps by itself.  The hub counts are chosen by the number of chunks a workgroup walks:
(0, 128] is the prologue alone (the first image, nothing to swap), (128, 256] one swap, (256, 384] the wrap-around back
to the first image, with an odd and an even count (the loop takes two chunks per trip).  The thresholds are read off the
degree counts here and every case asserts the hub count it relies on.  Widths 33 / 48 and 49 / 64 are the edges of the
two column-tile instantiations.

Bound: |got - ref| <= 1e-4 * max(1, |ref|) against the fp64 CSR formula, as in test_dense_block_gpu.py.  X = ones and the
single-source-row case are exact: sums of small integers, and sums of one value with zeros."""
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
CHUNK = 128


class Case:
    """The plain graph (no repeated pairs), its partition, and everything on the device."""

    def __init__(self):
        g = graph.powerlaw_graph(N, E, MAXDEG, seed=11)
        self.rp = g.row_pointers.numpy().astype(np.int32)
        self.ci = g.column_index.numpy().astype(np.int32)
        self.deg_count = np.diff(self.rp)
        self.rows = np.repeat(np.arange(N), self.deg_count)
        pp, p2n = _lib.build_part(PS, torch.from_numpy(self.rp))
        self.deg = torch.from_numpy(1.0 / np.sqrt(np.maximum(self.deg_count, 1)).astype(np.float32))
        self.ci_d, self.pp_d, self.p2n_d = torch.from_numpy(self.ci).cuda(), pp.int().cuda(), p2n.int().cuda()

    def hubs(self, theta):
        hub = self.deg_count >= theta
        both = hub[self.rows] & hub[self.ci]
        return int(hub.sum()), int(both.sum()), hub

    def theta_for(self, lo, hi):
        """A degree threshold with lo < hub count <= hi: the degree of the node in the middle of that range of ranks."""
        theta = int(np.sort(self.deg_count)[::-1][(lo + hi) // 2 - 1])
        H, entries, _ = self.hubs(theta)
        assert lo < H <= hi and entries > 0, (theta, H, entries)
        return theta, H

    def ref(self, mode, X, eps=1.0):
        return oracle.csr_f64(mode, X.numpy(), self.rp, self.ci, None, eps)

    def run(self, mode, Xd, eps=1.0, **kw):
        return _lib.agg_ld(mode, Xd, self.ci_d, self.pp_d, self.p2n_d, N, PS, epsilon=eps, **kw)

    def prepare(self, dims):
        return _lib.prepare_graph(self.ci_d, self.pp_d, self.p2n_d, N, N, PS, list(dims))


@functools.lru_cache(maxsize=None)
def _case():
    return Case()


@functools.lru_cache(maxsize=None)
def _features(dim):
    return torch.randn(N, dim, generator=torch.Generator().manual_seed(2000 + dim))


@functools.lru_cache(maxsize=None)
def _sag_ref(dim):
    ref = _case().ref(0, _features(dim))
    ref.setflags(write=False)
    return ref


def _ones_want(dim):
    return np.repeat(_case().deg_count.astype(np.float32)[:, None], dim, 1)


class dense:
    """GNNA_DENSE_BLOCK = 2 and the tests' theta for the prepares inside, sweep = 1, no forced phase count."""

    def __init__(self, theta):
        self.env = {"GNNA_DENSE_BLOCK": "2", "GNNA_DENSE_BLOCK_THETA": str(theta)}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        _lib.release_graph(None)
        _lib.reset_tuning()
        _lib.set_tuning(sweep=1, deterministic=0, gcn_prescale=1)
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


@pytest.mark.parametrize("dim", [33, 48, 49, 64])
@pytest.mark.parametrize("chunks", [1, 2, 3])
def test_chunk_counts_and_column_tiles(chunks, dim):
    c = _case()
    theta, H = c.theta_for((chunks - 1) * CHUNK, chunks * CHUNK)
    assert (H + CHUNK - 1) // CHUNK == chunks
    X = _features(dim)
    with dense(theta) as d:
        c.prepare([dim])
        assert d.delta("dense_block_builds") == 1
        y = c.run(0, X.cuda()).cpu().numpy()
        ones = c.run(0, torch.ones(N, dim, device="cuda")).cpu().numpy()
        assert d.delta("dense_block_launches") == 2
    assert_close_f64(y, _sag_ref(dim), what=f"{chunks} chunk(s), D {dim}")
    want = _ones_want(dim)
    assert np.array_equal(ones, want), int((ones != want).any(1).sum())


@pytest.mark.parametrize("dim,ld,first", [(41, 47, 3), (64, 67, 1), (44, 48, 1)])
def test_leading_dimension_beyond_the_width(dim, ld, first):
    """X is a column block of a wider buffer: ldx != D.  (41, 47) and (64, 67): ldx is no multiple of 4, the partial-piece
    form (with a partial last piece at 41); (44, 48): whole pieces that start 4 bytes off a 16-byte boundary."""
    c = _case()
    theta, H = c.theta_for(2 * CHUNK, 3 * CHUNK)
    X = _features(dim)
    buf = torch.full((N, ld), float("nan"))
    buf[:, first:first + dim] = X
    view = buf.cuda()[:, first:first + dim]
    assert view.stride(0) == ld and not view.is_contiguous()
    with dense(theta) as d:
        c.prepare([dim])
        y = c.run(0, view).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y, _sag_ref(dim), what=f"D {dim}, ldx {ld}")


def test_two_rounds_of_workgroups():
    c = _case()
    round_ = 32 * _lib.device_cus()
    fits = [t for t in range(2, 200) if round_ + round_ // 4 <= int((c.deg_count >= t).sum()) <= 16384]
    if not fits:
        pytest.skip(f"no threshold of this graph gives 1.25 x {round_} .. 16,384 hubs on this chip")
    theta = fits[-1]
    H, entries, _ = c.hubs(theta)
    assert round_ + round_ // 4 <= H <= 16384 and entries > 0, (theta, H, entries)
    X = _features(64)
    with dense(theta) as d:
        c.prepare([64])
        y = c.run(0, X.cuda()).cpu().numpy()
        ones = c.run(0, torch.ones(N, 64, device="cuda")).cpu().numpy()
        assert d.delta("dense_block_launches") == 2
    assert_close_f64(y, _sag_ref(64), what=f"two rounds, H {H}")
    assert np.array_equal(ones, _ones_want(64))


@pytest.mark.parametrize("dim", [48, 64])
def test_one_source_row_with_full_mantissas_is_exact(dim):
    """X is zero except one hub's row, so every output element is one value plus zeros: exact in any order, and equal to
    float32(ref) bit for bit.  The row holds values with all 24 mantissa bits in use from 1e-30 to 3e38, both signs: a
    wrong operand lane order moves a value to another column or row, and a form that splits the operands inexactly loses
    low bits.  (Floats that compare equal and are not zero have equal bits; a zero's sign is not looked at.)"""
    c = _case()
    theta, H = c.theta_for(2 * CHUNK, 3 * CHUNK)
    _, _, hub = c.hubs(theta)
    hub_ids = np.flatnonzero(hub)
    src = int(hub_ids[CHUNK + 37])          # a rank inside the second chunk, off every tile and step boundary
    users = c.rows[c.ci == src]
    assert hub[users].sum() >= 16 and (~hub[users]).sum() >= 16, "the row is read through the block and through the gather"
    rng = np.random.default_rng(dim)
    mant = (rng.integers(1 << 22, 1 << 23, dim).astype(np.float64) * 2 + 1) / float(1 << 24)      # odd 24-bit mantissas in [0.5, 1)
    expo = np.linspace(np.log2(1e-30), np.log2(3e38), dim)       # (2^-99 .. 2^128 times a mantissa below 1: finite)
    vals = (mant * np.exp2(np.ceil(expo)) * np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    assert np.isfinite(vals).all() and (np.abs(vals) >= 1e-31).all() and np.abs(vals).max() > 1e38
    assert ((vals.view(np.uint32) & 1) == 1).all(), "the lowest mantissa bit is in use"
    X = torch.zeros(N, dim)
    X[src] = torch.from_numpy(vals)
    with dense(theta) as d:
        c.prepare([dim])
        y = c.run(0, X.cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    ref = c.ref(0, X).astype(np.float32)
    assert np.array_equal(ref[users], np.repeat(vals[None, :], users.size, 0)) and np.count_nonzero(ref.any(1)) == users.size
    assert np.array_equal(y, ref), int((y != ref).any(1).sum())


@pytest.mark.parametrize("dim", [50, 64])
def test_gin_scale_and_accumulate(dim):
    c = _case()
    theta, H = c.theta_for(2 * CHUNK, 3 * CHUNK)
    X = _features(dim)
    Xd = X.cuda()
    with dense(theta) as d:
        c.prepare([dim])
        yi = c.run(2, Xd, eps=0.5).cpu().numpy()
        acc = torch.full((N, dim), 3.0, device="cuda")
        c.run(0, Xd, out=acc, accumulate=True)
        assert d.delta("dense_block_launches") == 2
    sag = _sag_ref(dim)
    assert_close_f64(yi, c.ref(2, X, 0.5), what="gin")
    assert_close_f64(acc.cpu().numpy(), sag + 3.0, what="accumulate", scale=np.abs(sag) + 3.0)

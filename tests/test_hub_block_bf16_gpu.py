"""hub_block_kernel on the bf16 MFMA (csrc/gnna_dense.hip): every value of X is split at staging into three bf16 pieces
(hi = x truncated to 16 bits, mid = the truncated remainder, lo = the rest) which are multiplied with the 0 / 1 bitmap by
v_mfma_f32_16x16x32_bf16; the hi products have one fp32 accumulator, the mid and lo products another.

Shapes.  The graph and the way of forcing a block of tests/test_hub_block_rate_gpu.py (powerlaw_graph(36000, 1800000, 3000,
seed=11), partSize 32, GNNA_DENSE_BLOCK = 2 with a threshold, sweep = 1), its features and its fp64 references, shared.
Unless said otherwise the block has 129 .. 256 hubs: two chunks, one swap of the LDS images.

Exact cases compare with float32(fp64 reference) bit for bit (floats that compare equal and are not zero have equal bits; a
zero's sign is not looked at): their sums are sums of integers times one power of two that stay below 2^24 of it, so every
order of adding them is exact.  The others use the suite's bound, |got - ref| <= 1e-4 * max(1, |ref|)."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib
from test_hub_block_rate_gpu import CHUNK, N, _case, _features, _ones_want, _sag_ref, dense
from util import assert_close_f64

pytestmark = pytest.mark.gpu


def _two_chunks():
    c = _case()
    theta, H = c.theta_for(CHUNK, 2 * CHUNK)
    _, _, hub = c.hubs(theta)
    return c, theta, hub, np.flatnonzero(hub)


def _common_hub_users(c, hub, a, b):
    """Hub rows that have both a and b as neighbours."""
    both = np.intersect1d(c.rows[c.ci == a], c.rows[c.ci == b])
    return both[hub[both]]


@pytest.mark.parametrize("dim", [33, 48, 49, 64])
def test_each_piece_alone_and_together_is_exact(dim):
    """X is zero except three hub rows of odd integers k * 2^s: k < 2^8 (hi alone), 2^8 <= k < 2^16 (hi and mid), 2^21 <= k <
    2^22 (all three pieces); mixed signs, one exponent s per column from -90 to +100.  A sum of at most three of them is below
    2^24 * 2^s."""
    c, theta, hub, hub_ids = _two_chunks()
    srcs = [int(hub_ids[5]), int(hub_ids[CHUNK + 37]), int(hub_ids[-1])]
    rng = np.random.default_rng(100 + dim)
    s = np.round(np.linspace(-90, 100, dim)).astype(np.int64)
    k = np.stack([rng.integers(0, 1 << 7, dim) * 2 + 1,
                  rng.integers(1 << 7, 1 << 15, dim) * 2 + 1,
                  rng.integers(1 << 20, 1 << 21, dim) * 2 + 1]).astype(np.float64)
    assert (k[0] < 1 << 8).all() and (k[1] >= 1 << 8).all() and (k[1] < 1 << 16).all() and (k[2] >= 1 << 21).all() and (k[2] < 1 << 22).all()
    sign = np.where(rng.integers(0, 2, (3, dim)) == 0, 1.0, -1.0)
    vals = (sign * k * np.exp2(s)[None, :]).astype(np.float32)
    assert np.array_equal(vals.astype(np.float64), sign * k * np.exp2(s)[None, :]), "the values are float32 values"
    X = torch.zeros(N, dim)
    for i, src in enumerate(srcs):
        X[src] = torch.from_numpy(vals[i])
    users = [c.rows[c.ci == src] for src in srcs]
    assert all(hub[u].sum() >= 8 for u in users), "each row is read through the block"
    assert _common_hub_users(c, hub, srcs[0], srcs[2]).size > 0 and _common_hub_users(c, hub, srcs[1], srcs[2]).size > 0
    with dense(theta) as d:
        c.prepare([dim])
        y = c.run(0, X.cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    ref64 = c.ref(0, X)
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64), "the reference is exact in float32"
    assert np.array_equal(y, ref), int((y != ref).any(1).sum())


def test_cancellation_leaves_the_difference():
    """Two hub rows hold x and -x + delta with full 24-bit mantissas, delta = 2^-20 |x| rounded to a multiple of the last bit
    of x (8 .. 16 of them).  A row that has both as neighbours, and no other row that is not zero, gets delta exactly."""
    dim = 64
    c, theta, hub, hub_ids = _two_chunks()
    a, b = int(hub_ids[CHUNK - 3]), int(hub_ids[CHUNK + 50])
    both = _common_hub_users(c, hub, a, b)
    assert both.size > 0, "a hub row reads both rows through the block"
    rng = np.random.default_rng(7)
    m = rng.integers(1 << 22, 1 << 23, dim) * 2 + 1                 # odd, 24 bits
    steps = np.round(m / float(1 << 20)).astype(np.int64)
    assert (steps >= 8).all() and (steps <= 16).all()
    e = np.exp2(np.round(np.linspace(-60, 60, dim)))
    sign = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)
    x = (sign * m * e).astype(np.float32)
    other = (-sign * (m - steps) * e).astype(np.float32)
    delta = (sign * steps * e).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) + other.astype(np.float64), delta.astype(np.float64))
    X = torch.zeros(N, dim)
    X[a] = torch.from_numpy(x)
    X[b] = torch.from_numpy(other)
    with dense(theta) as d:
        c.prepare([dim])
        y = c.run(0, X.cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert np.array_equal(y[both], np.repeat(delta[None, :], both.size, 0)), int((y[both] != delta[None, :]).any(1).sum())
    ref = c.ref(0, X).astype(np.float32)
    assert np.array_equal(y, ref), int((y != ref).any(1).sum())


def test_integer_sums_are_exact():
    """Random integers of |x| <= 4,095 on all rows (hi and mid on every term): every row's sum of |x| stays below 2^24."""
    dim = 64
    c, theta, hub, hub_ids = _two_chunks()
    X = torch.randint(-4095, 4096, (N, dim), generator=torch.Generator().manual_seed(31)).float()
    assert int(c.deg_count.max()) * 4095 < 1 << 24
    with dense(theta) as d:
        c.prepare([dim])
        y = c.run(0, X.cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    ref64 = c.ref(0, X)                  # (integers below 2^24 in fp64: the int64 sum)
    want = ref64.astype(np.int64)
    assert np.array_equal(want.astype(np.float64), ref64) and int(np.abs(want).max()) < 1 << 24
    assert np.array_equal(y, want.astype(np.float32)), int((y != want).any(1).sum())


def test_an_infinity_reaches_its_neighbours_and_nan_the_other_hubs():
    """One hub's row holds +Inf in column 0 and -Inf in column 1 (the contract in the header of gnna_dense.hip)."""
    dim = 64
    c, theta, hub, hub_ids = _two_chunks()
    src = int(hub_ids[CHUNK + 37])
    X = _features(dim).clone()
    X[src, 0], X[src, 1] = float("inf"), float("-inf")
    users = np.zeros(N, dtype=bool)
    users[c.rows[c.ci == src]] = True
    assert (users & hub).sum() >= 16 and (~users & hub).sum() >= 8 and (users & ~hub).sum() >= 16
    with dense(theta) as d:
        c.prepare([dim])
        y = c.run(0, X.cuda()).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    ref = _sag_ref(dim)                  # (X differs from the shared features in two elements of one row)
    near = users & hub
    assert (y[near, 0] == np.inf).all() and (y[near, 1] == -np.inf).all(), "hub rows with that neighbour"
    assert np.isnan(y[~users & hub][:, :2]).all(), "the other hub rows"
    assert (y[users & ~hub, 0] == np.inf).all() and (y[users & ~hub, 1] == -np.inf).all(), "rows that gather it"
    assert_close_f64(y[:, 2:], ref[:, 2:], what="the other columns")
    assert_close_f64(y[~users & ~hub][:, :2], ref[~users & ~hub][:, :2], what="rows without that neighbour outside the block")


def test_more_than_a_round_of_workgroups():
    """A block beyond a whole round of workgroups (one per compute unit) and outside the window that trimmed_hubs cuts back
    to the round: 1.25 rounds .. 16,384 hubs."""
    c = _case()
    round_ = 32 * _lib.device_cus()
    fits = [t for t in range(2, 200) if round_ + round_ // 4 <= int((c.deg_count >= t).sum()) <= 16384]
    assert fits, f"no threshold of this graph gives 1.25 x {round_} .. 16,384 hubs on this chip"
    theta = fits[-1]
    H, entries, _ = c.hubs(theta)
    assert round_ + round_ // 4 <= H <= 16384 and entries > 0, (theta, H, entries)
    with dense(theta) as d:
        c.prepare([64])
        y = c.run(0, _features(64).cuda()).cpu().numpy()
        ones = c.run(0, torch.ones(N, 64, device="cuda")).cpu().numpy()
        assert d.delta("dense_block_launches") == 2
    assert_close_f64(y, _sag_ref(64), what=f"H {H}")
    assert np.array_equal(ones, _ones_want(64))


def test_gin_scale():
    c, theta, hub, hub_ids = _two_chunks()
    X = _features(64)
    with dense(theta) as d:
        c.prepare([64])
        y = c.run(2, X.cuda(), eps=0.5).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y, c.ref(2, X, 0.5), what="gin")


def test_row_scale():
    """GCN with pre-scaled rows: the block's rows are multiplied by row_scale."""
    import oracle
    c, theta, hub, hub_ids = _two_chunks()
    X = _features(64)
    deg = c.deg.cuda()
    with dense(theta) as d:
        c.prepare([64])
        y = _lib.agg_ld(1, X.cuda(), c.ci_d, c.pp_d, c.p2n_d, N, 32, degrees_out=deg, degrees_in=deg).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    ref = oracle.csr_f64(1, X.numpy(), c.rp, c.ci, c.deg.numpy(), 1.0)
    scale = oracle.csr_f64(1, np.abs(X.numpy()), c.rp, c.ci, c.deg.numpy())
    assert_close_f64(y, ref, what="gcn (pre-scaled)", scale=scale)


def test_accumulate_into_the_output():
    c, theta, hub, hub_ids = _two_chunks()
    sag = _sag_ref(64)
    with dense(theta) as d:
        c.prepare([64])
        acc = torch.full((N, 64), 3.0, device="cuda")
        c.run(0, _features(64).cuda(), out=acc, accumulate=True)
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(acc.cpu().numpy(), sag + 3.0, what="accumulate", scale=np.abs(sag) + 3.0)


def test_leading_dimension_beyond_the_width():
    c, theta, hub, hub_ids = _two_chunks()
    buf = torch.full((N, 68), float("nan"))
    buf[:, 4:68] = _features(64)
    view = buf.cuda()[:, 4:68]
    assert view.stride(0) == 68 and not view.is_contiguous()
    with dense(theta) as d:
        c.prepare([64])
        y = c.run(0, view).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y, _sag_ref(64), what="ldx 68")

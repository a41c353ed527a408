"""The split pass and the image-reading hub_block_kernel (csrc/gnna_dense.hip): hub_split_kernel writes the three bf16 pieces
of the call's hub rows once, into the scratch of the call's stream, and hub_block_kernel loads them as MFMA operands, with 32
or 64 destination ranks per workgroup (GNNA_DENSE_BLOCK_TILE under GNNA_DENSE_BLOCK = 2 forces the height).

Shapes.  The graph and the way of forcing a block of tests/test_hub_block_rate_gpu.py (powerlaw_graph(36000, 1800000, 3000,
seed=11), partSize 32, GNNA_DENSE_BLOCK = 2 with a threshold, sweep = 1), its features and its fp64 references, shared.  The hub
counts are chosen by the number of 128-rank chunks a workgroup walks: 1 .. 5 cover the first fetches alone, every tail of the
loop (three chunks per trip) and one full trip with each tail behind it.  Every case asserts the hub count it relies on.

Bound: |got - ref| <= 1e-4 * max(1, |ref|) against the fp64 CSR formula, as in test_dense_block_gpu.py.  Exact cases compare
bit for bit.  The two tile heights are never compared with each other on random features: the sweep's shared rows have no
fixed order."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib
from test_hub_block_rate_gpu import CHUNK, N, _case, _features, _ones_want, _sag_ref, dense
from util import assert_close_f64

pytestmark = pytest.mark.gpu

TILES = [32, 64]
WIDTHS = [33, 36, 48, 49, 63, 64]        # both column-tile counts at their edges; 33, 49, 63: the partial form of the split pass


class tiled(dense):
    """`dense` with the tile height forced."""

    def __init__(self, theta, tile):
        super().__init__(theta)
        self.env["GNNA_DENSE_BLOCK_TILE"] = str(tile)


def _two_chunks():
    c = _case()
    theta, H = c.theta_for(CHUNK, 2 * CHUNK)
    _, _, hub = c.hubs(theta)
    return c, theta, hub, np.flatnonzero(hub)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("chunks", [1, 2, 3, 4, 5])
def test_chunk_counts_and_widths(chunks, tile):
    """Every width into the first columns of a wider buffer of sevens: the columns from D on are never written."""
    c = _case()
    theta, H = c.theta_for((chunks - 1) * CHUNK, chunks * CHUNK)
    assert (H + CHUNK - 1) // CHUNK == chunks
    with tiled(theta, tile) as d:
        c.prepare(WIDTHS)
        assert d.delta("dense_block_builds") == 1
        for i, dim in enumerate(WIDTHS):
            wide = torch.full((N, 68), 7.0, device="cuda")
            c.run(0, _features(dim).cuda(), out=wide[:, :dim])
            ones = c.run(0, torch.ones(N, dim, device="cuda")).cpu().numpy()
            assert d.delta("dense_block_launches") == 2 * (i + 1)
            wide = wide.cpu().numpy()
            assert (wide[:, dim:] == 7.0).all(), f"D {dim}: columns beyond D were written"
            assert_close_f64(wide[:, :dim], _sag_ref(dim), what=f"{chunks} chunk(s), tile {tile}, D {dim}")
            want = _ones_want(dim)
            assert np.array_equal(ones, want), (dim, int((ones != want).any(1).sum()))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ld,first", [(68, 4), (67, 1)])
def test_leading_dimensions(ld, first, tile):
    """ldx = 68 on a view at column offset 4 (whole, aligned 16-byte pieces) and ldx = 67 (the partial form)."""
    c, theta, hub, hub_ids = _two_chunks()
    buf = torch.full((N, ld), float("nan"))
    buf[:, first:first + 64] = _features(64)
    view = buf.cuda()[:, first:first + 64]
    assert view.stride(0) == ld and not view.is_contiguous()
    with tiled(theta, tile) as d:
        c.prepare([64])
        y = c.run(0, view).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y, _sag_ref(64), what=f"ldx {ld}, tile {tile}")


@pytest.mark.parametrize("tile", TILES)
def test_the_image_is_rebuilt_on_every_call(tile):
    c, theta, hub, hub_ids = _two_chunks()
    X2 = torch.randn(N, 64, generator=torch.Generator().manual_seed(977))
    with tiled(theta, tile) as d:
        c.prepare([64, 36])
        y1 = c.run(0, _features(64).cuda()).cpu().numpy()
        y2 = c.run(0, X2.cuda()).cpu().numpy()
        y3 = c.run(0, _features(36).cuda()).cpu().numpy()      # (a narrower call behind a wider one: no stale columns)
        ones = c.run(0, torch.ones(N, 36, device="cuda")).cpu().numpy()
        assert d.delta("dense_block_launches") == 4
    assert_close_f64(y1, _sag_ref(64), what="first X")
    assert_close_f64(y2, c.ref(0, X2), what="second X")
    assert_close_f64(y3, _sag_ref(36), what="width 36 behind width 64")
    assert np.array_equal(ones, _ones_want(36))


@pytest.mark.parametrize("tile", TILES)
def test_two_streams_one_graph_different_features(tile):
    """Both calls are enqueued back to back on two streams: the scratch of the split image is per stream."""
    c, theta, hub, hub_ids = _two_chunks()
    Xa, Xb = _features(64), torch.randn(N, 64, generator=torch.Generator().manual_seed(978))
    Xa_d, Xb_d = Xa.cuda(), Xb.cuda()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with tiled(theta, tile) as d:
        for s in (sa, sb):
            with torch.cuda.stream(s):
                c.prepare([64])
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            ya = c.run(0, Xa_d)
        with torch.cuda.stream(sb):
            yb = c.run(0, Xb_d)
        torch.cuda.synchronize()
        assert d.delta("dense_block_launches") == 2
    assert_close_f64(ya.cpu().numpy(), _sag_ref(64), what="stream a")
    assert_close_f64(yb.cpu().numpy(), c.ref(0, Xb), what="stream b")


@pytest.mark.parametrize("tile", TILES)
def test_capture_follows_new_features_and_nothing_allocates(tile):
    """The split pass is inside the captured graph: X is overwritten in place before the replay."""
    c, theta, hub, hub_ids = _two_chunks()
    X1 = _features(64)
    X2 = torch.randn(N, 64, generator=torch.Generator().manual_seed(979))
    quiet = ("plan_builds", "launch_syncs", "launch_mallocs", "launch_frees")
    with tiled(theta, tile) as d:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c.prepare([64])
            side.synchronize()
            Xd = X1.cuda()
            out = torch.empty_like(Xd)
            side.synchronize()
            before = _lib.runtime_counters()
            for _ in range(10):
                y = c.run(0, Xd)
            side.synchronize()
            eager = _lib.runtime_counters()
            assert eager["dense_block_launches"] == before["dense_block_launches"] + 10
            for k in quiet:
                assert eager[k] == before[k], ("eager", k)
            assert_close_f64(y.cpu().numpy(), _sag_ref(64), what="eager")
            graph_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_, stream=side):
                c.run(0, Xd, out=out)
        after = _lib.runtime_counters()
        assert after["dense_block_launches"] == eager["dense_block_launches"] + 1
        for k in quiet:
            assert after[k] == eager[k], ("capture", k)
        Xd.copy_(X2.cuda())
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        graph_.replay()
        torch.cuda.synchronize()
        assert_close_f64(out.cpu().numpy(), c.ref(0, X2), what="replay on the new X")
        del graph_


def test_integer_sums_are_exact_at_both_tile_heights():
    """Random integers of |x| <= 4,095 on all rows: every row's sum of |x| stays below 2^24, so both heights give the int64 sums
    bit for bit (and so each other's)."""
    dim = 64
    c, theta, hub, hub_ids = _two_chunks()
    X = torch.randint(-4095, 4096, (N, dim), generator=torch.Generator().manual_seed(31)).float()
    assert int(c.deg_count.max()) * 4095 < 1 << 24
    ref64 = c.ref(0, X)
    want = ref64.astype(np.int64)
    assert np.array_equal(want.astype(np.float64), ref64) and int(np.abs(want).max()) < 1 << 24
    got = {}
    for tile in TILES:
        with tiled(theta, tile) as d:
            c.prepare([dim])
            got[tile] = c.run(0, X.cuda()).cpu().numpy()
            assert d.delta("dense_block_launches") == 1
        assert np.array_equal(got[tile], want.astype(np.float32)), (tile, int((got[tile] != want).any(1).sum()))
    assert np.array_equal(got[32], got[64])


def test_an_infinity_at_the_tall_tile():
    """One hub's row holds +Inf in column 0 and -Inf in column 1 (the contract in the header of gnna_dense.hip)."""
    dim = 64
    c, theta, hub, hub_ids = _two_chunks()
    src = int(hub_ids[CHUNK + 37])
    X = _features(dim).clone()
    X[src, 0], X[src, 1] = float("inf"), float("-inf")
    users = np.zeros(N, dtype=bool)
    users[c.rows[c.ci == src]] = True
    assert (users & hub).sum() >= 16 and (~users & hub).sum() >= 8 and (users & ~hub).sum() >= 16
    with tiled(theta, 64) as d:
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


def test_gin_scale_at_the_tall_tile():
    c, theta, hub, hub_ids = _two_chunks()
    X = _features(64)
    with tiled(theta, 64) as d:
        c.prepare([64])
        y = c.run(2, X.cuda(), eps=0.5).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(y, c.ref(2, X, 0.5), what="gin")


def test_row_scale_at_the_tall_tile():
    """GCN with pre-scaled rows: the block's rows are multiplied by row_scale."""
    import oracle
    c, theta, hub, hub_ids = _two_chunks()
    X = _features(64)
    deg = c.deg.cuda()
    with tiled(theta, 64) as d:
        c.prepare([64])
        y = _lib.agg_ld(1, X.cuda(), c.ci_d, c.pp_d, c.p2n_d, N, 32, degrees_out=deg, degrees_in=deg).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    ref = oracle.csr_f64(1, X.numpy(), c.rp, c.ci, c.deg.numpy(), 1.0)
    scale = oracle.csr_f64(1, np.abs(X.numpy()), c.rp, c.ci, c.deg.numpy())
    assert_close_f64(y, ref, what="gcn (pre-scaled)", scale=scale)


def test_accumulate_at_the_tall_tile():
    c, theta, hub, hub_ids = _two_chunks()
    sag = _sag_ref(64)
    with tiled(theta, 64) as d:
        c.prepare([64])
        acc = torch.full((N, 64), 3.0, device="cuda")
        c.run(0, _features(64).cuda(), out=acc, accumulate=True)
        assert d.delta("dense_block_launches") == 1
    assert_close_f64(acc.cpu().numpy(), sag + 3.0, what="accumulate", scale=np.abs(sag) + 3.0)


def test_the_natural_choice_of_tile_beyond_a_round():
    """No tile forced: a block of at least 1.25 rounds of 32-rank workgroups (the threshold search of
    test_more_than_a_round_of_workgroups) takes the tall tile by itself; X = ones gives the exact row counts."""
    c = _case()
    round_ = 32 * _lib.device_cus()
    fits = [t for t in range(2, 200) if round_ + round_ // 4 <= int((c.deg_count >= t).sum()) <= 16384]
    assert fits, f"no threshold of this graph gives 1.25 x {round_} .. 16,384 hubs on this chip"
    theta = fits[-1]
    H, entries, _ = c.hubs(theta)
    assert round_ + round_ // 4 <= H <= 16384 and entries > 0, (theta, H, entries)
    with dense(theta) as d:
        c.prepare([64])
        ones = c.run(0, torch.ones(N, 64, device="cuda")).cpu().numpy()
        assert d.delta("dense_block_launches") == 1
    assert np.array_equal(ones, _ones_want(64))

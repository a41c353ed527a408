"""gnna_agg_typed_expand_ld_f32 / gnna_agg_typed_contract_ld_f32 / gnna_typed_coef_grad_ld_f32 against fp64 numpy, on an MI355X.

Every case runs the three entries on one graph: a ~300-row power-law graph with a hub row of 230 more edges, ten rows without
edges, duplicate edges, self loops, one relation without any edge, five column ids and five type ids outside their ranges
(the reference drops those edges), leading dimensions larger than the width on every matrix.  The reference walks the partition as
it is given, so a shuffled partition with empty and negative groups has the same reference code.  Tolerance: 1e-4 of the same
formula evaluated on the absolute values of every factor (util.assert_close_f64)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnnadvisor_osdi21_amd import _lib
from util import assert_close_f64, make_case

pytestmark = pytest.mark.gpu
UNSUPPORTED = -3


class Case(object):
    pass


def _edges_of_partition(pp, p2n, n_out):
    """(positions, rows) of every edge the partition as given covers: a group with e <= s, s < 0 or a row outside counts for nothing."""
    pp, p2n = np.asarray(pp, np.int64), np.asarray(p2n, np.int64)
    s, e = pp[:-1], pp[1:]
    ok = (e > s) & (s >= 0) & (p2n >= 0) & (p2n < n_out)
    s, lens, r = s[ok], (e - s)[ok], p2n[ok]
    if not len(s):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.cumsum(lens) - lens                                   # where every group starts in the list of edges
    pos = np.repeat(s - first, lens) + np.arange(int(lens.sum()))
    return pos, np.repeat(r, lens)


def make(dim, B, R, ps, n_out=300, n_in=300, seed=0, norm=True, shuffle=False, pad=3, nnz=3000, shuffle_block=1):
    rng = np.random.default_rng(1000 + seed)
    g = make_case(n_out, nnz, 4, ps, seed, kind="powerlaw")[0]
    rp = g.row_pointers.numpy().astype(np.int64)
    rows = np.repeat(np.arange(n_out), np.diff(rp))
    cols = g.column_index.numpy().astype(np.int64) * n_in // n_out
    keep = ~((rows >= 10) & (rows < 20))                                     # ten rows without edges
    rows, cols = rows[keep], cols[keep]
    hub_cols = rng.integers(0, n_in, size=220)
    hub_cols[:3] = min(5, n_in - 1)                                            # self loops of the hub row, three times over
    dup = rng.integers(0, len(rows), size=20)                                  # duplicate edges
    rows = np.concatenate([rows, np.full(230, 5), rows[dup], np.arange(30, 40)])
    cols = np.concatenate([cols, hub_cols, hub_cols[:10], cols[dup], np.minimum(np.arange(30, 40), n_in - 1)])
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    nnz = len(rows)
    ety = rng.integers(0, R, size=nnz)
    if R >= 3:
        ety[ety == 1] = 0                                                      # relation 1 has no edge at all
    bad = rng.choice(nnz, size=10, replace=False)
    cols[bad[:5]] = [n_in, -1, n_in + 7, 2 ** 30, -(2 ** 31)]
    ety[bad[5:]] = [R, -1, R + 3, 2 ** 30, -7]
    nrm = rng.uniform(0.5, 1.5, size=nnz).astype(np.float32) if norm else None
    rp = np.zeros(n_out + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp)
    pp, p2n = _lib.build_part(ps, torch.from_numpy(rp.astype(np.int32)))
    pp, p2n = pp.numpy().astype(np.int64), p2n.numpy().astype(np.int64)
    if shuffle:
        # groups in random order: every group keeps its edges through per-edge arrays rewritten in the new order; then an empty
        # group, a group with decreasing pointers (the group behind it re-reads five positions) and a group with a row outside
        # (shuffle_block > 1: blocks of that many consecutive groups move together, so groups of one row still follow each
        # other inside a block and a wavefront that takes several groups merges them, while the row goes on in a distant block)
        P = len(p2n)
        nblk = -(-P // shuffle_block)
        perm = (rng.permutation(nblk)[:, None] * shuffle_block + np.arange(shuffle_block)[None, :]).ravel()
        perm = perm[perm < P]
        lens = (pp[1:] - pp[:-1])[perm]
        first = np.cumsum(lens) - lens
        idx = np.repeat(pp[:-1][perm] - first, lens) + np.arange(int(lens.sum()))
        cols, ety = cols[idx], ety[idx]
        nrm = None if nrm is None else nrm[idx]
        pp = np.concatenate([[0], np.cumsum(lens)])
        p2n = p2n[perm]
        for mid in sorted({P // 2, P // 3 + 1, (2 * P) // 3 + 2}, reverse=True):
            cut = int(pp[mid])
            pp = np.concatenate([pp[:mid + 1], [cut, cut - 5], pp[mid + 1:]])
            p2n = np.concatenate([p2n[:mid], [5, 6], p2n[mid:]])
        p2n[[3, P // 4, P // 4 + 1, P - 2]] = [n_out + 2, -1, n_out, 2 ** 30]
    c = Case()
    c.dim, c.B, c.R, c.ps, c.n_out, c.n_in = dim, B, R, ps, n_out, n_in
    c.cols, c.ety, c.nrm, c.pp, c.p2n = cols, ety, nrm, pp, p2n
    c.X = rng.standard_normal((n_in, dim)).astype(np.float32)
    c.C = rng.standard_normal((R, B)).astype(np.float32)
    c.Gt = rng.standard_normal((n_in, B * dim)).astype(np.float32)             # what contract gathers
    c.Go = rng.standard_normal((n_out, B * dim)).astype(np.float32)            # the coef grad's destination side
    c.pad = pad
    return c


def reference(c, absolute=False):
    """fp64 (T, contracted, dC); absolute=True: the same sums over |X|, |C|, |n|, |G| (the scale of the tolerance)."""
    f = np.abs if absolute else (lambda a: a)
    X, C, Gt, Go = (f(a.astype(np.float64)) for a in (c.X, c.C, c.Gt, c.Go))
    pos, rows = _edges_of_partition(c.pp, c.p2n, c.n_out)
    col, t = c.cols[pos], c.ety[pos]
    n = np.ones(len(pos)) if c.nrm is None else f(c.nrm[pos].astype(np.float64))
    ok = (col >= 0) & (col < c.n_in) & (t >= 0) & (t < c.R)
    rows, col, t, n = rows[ok], col[ok], t[ok], n[ok]
    T = np.zeros((c.n_out, c.B * c.dim))
    out = np.zeros((c.n_out, c.dim))
    dC = np.zeros((c.R, c.B))
    for b in range(c.B):
        A = sp.csr_matrix((n * C[t, b], (rows, col)), shape=(c.n_out, c.n_in))
        blk = slice(b * c.dim, (b + 1) * c.dim)
        T[:, blk] = A @ X
        out += A @ Gt[:, blk]
        d = (X[col] * Go[rows][:, blk]).sum(1) * n
        dC[:, b] = np.bincount(t, weights=d, minlength=c.R)
    return T, out, dC


def _padded(a, pad):
    """A device view [rows, width] of a wider matrix (leading dimension = width + pad), NaN outside."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=a.dtype).cuda()
    view = buf[:, :a.shape[1]]
    view.copy_(a)
    return view


def device(c):
    d = Case()
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64).astype(np.int32)).cuda()    # (wraps like the C side would)
    d.ci, d.ety, d.pp, d.p2n = i32(c.cols), i32(c.ety), i32(c.pp), i32(c.p2n)
    d.nrm = None if c.nrm is None else torch.from_numpy(c.nrm).cuda()
    d.X, d.Gt, d.Go = _padded(c.X, c.pad), _padded(c.Gt, c.pad), _padded(c.Go, c.pad)
    d.C = torch.from_numpy(c.C).cuda()
    return d


def run_and_check(c, what):
    d = device(c)
    (T, out, dC), (Ts, outs, dCs) = reference(c), reference(c, absolute=True)
    W = c.B * c.dim
    gT = torch.full((c.n_out, W + c.pad), float("nan"), device="cuda")
    _lib.agg_typed_expand(d.X, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps, out=gT[:, :W])
    g_out = torch.full((c.n_out, c.dim + c.pad), float("nan"), device="cuda")
    _lib.agg_typed_contract(d.Gt, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps, out=g_out[:, :c.dim])
    g_dC = _lib.typed_coef_grad(d.X, d.Go, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.R, c.ps)
    torch.cuda.synchronize()
    assert_close_f64(gT[:, :W].cpu().numpy(), T, what=f"expand {what}", scale=Ts)
    assert_close_f64(g_out[:, :c.dim].cpu().numpy(), out, what=f"contract {what}", scale=outs)
    assert_close_f64(g_dC.cpu().numpy(), dC, what=f"coef grad {what}", scale=dCs)
    if c.pad:
        assert torch.isnan(gT[:, W:]).all() and torch.isnan(g_out[:, c.dim:]).all(), f"{what}: wrote beyond the row width"
    return d, (T, Ts, dC, dCs)


DIMS = [1, 3, 4, 7, 16, 41, 64, 100, 260]          # 260: a second column block; the odd ones: tail loads
BASES = [1, 2, 3, 8, 16]
TYPES = [1, 3, 40]
PARTS = [1, 3, 32]


@pytest.mark.parametrize("k,dim", list(enumerate(DIMS)))
def test_every_width(k, dim):
    """Every width, with the bases, types and partSize going round their lists."""
    B, R, ps = BASES[k % 5], TYPES[k % 3], PARTS[(k + 1) % 3]
    run_and_check(make(dim, B, R, ps, seed=k), f"dim={dim} B={B} R={R} partSize={ps}")


@pytest.mark.parametrize("R", TYPES)
@pytest.mark.parametrize("B", BASES)
def test_every_bases_types_pair(B, R):
    """All (bases, types) pairs -- (16, 40) makes a table of 640 cells -- at widths and partSizes going round their lists."""
    k = BASES.index(B) * 3 + TYPES.index(R)
    dim, ps = [7, 16, 41, 64][k % 4], PARTS[k % 3]
    run_and_check(make(dim, B, R, ps, seed=20 + k, norm=k % 2 == 0), f"dim={dim} B={B} R={R} partSize={ps}")


@pytest.mark.parametrize("B", [3, 16])
def test_table_beyond_the_lds_path(B):
    """num_types * num_bases above _lib.TYPED_LDS_CELLS: C is read from global memory and dC is added to dcoef edge by edge."""
    R = _lib.TYPED_LDS_CELLS // B + 7
    assert R * B > _lib.TYPED_LDS_CELLS
    run_and_check(make(41, B, R, 3, seed=50 + B), f"table of {R * B} cells")
    Rin = _lib.TYPED_LDS_CELLS // 16                  # and the largest table that still fits, at the widest stride
    run_and_check(make(16, 16, Rin, 32, seed=52), f"table of {Rin * 16} cells")


@pytest.mark.parametrize("n_out,n_in", [(300, 170), (170, 300)])
@pytest.mark.parametrize("ps", PARTS)
def test_rectangular(n_out, n_in, ps):
    run_and_check(make(41, 3, 3, ps, n_out=n_out, n_in=n_in, seed=60 + ps), f"{n_out} x {n_in} partSize={ps}")


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "no_norm"])
@pytest.mark.parametrize("dim,B,ps", [(64, 8, 32), (7, 2, 3), (260, 3, 1)])
def test_shuffled_partition(dim, B, ps, norm):
    """Groups and part2Node in random order, an empty group, a group with decreasing pointers, a group with a row outside."""
    run_and_check(make(dim, B, 3, ps, seed=70 + dim, norm=norm, shuffle=True, pad=0 if dim == 7 else 3),
                  f"shuffled dim={dim} B={B} partSize={ps}")


def test_hub_row_is_long_and_the_graph_has_what_the_cases_claim():
    c = make(16, 2, 3, 32, seed=0)
    pos, rows = _edges_of_partition(c.pp, c.p2n, c.n_out)
    counts = np.bincount(rows, minlength=c.n_out)
    assert counts[5] >= 200 and (counts[10:20] == 0).all()
    assert not (c.ety == 1).any() and ((c.ety < 0) | (c.ety >= c.R)).sum() == 5 and ((c.cols < 0) | (c.cols >= c.n_in)).sum() == 5
    assert (c.cols[rows == 5] == 5).sum() >= 3                                  # self loops, duplicated


@pytest.mark.parametrize("dim,B,ps", [(16, 3, 256), (64, 4, 256), (100, 8, 512), (3, 16, 100), (260, 2, 256)])
def test_a_group_longer_than_one_step(dim, B, ps):
    """partSize above 64: the hub row's 230+ edges are ONE neighbor-group, so one run walks three full 64-edge steps and a
    tail whatever the launch makes of the groups (partSize 100: two steps of 64 and 36, then a second group of the row)."""
    c = make(dim, B, 3, ps, seed=100 + dim)
    lens = np.diff(c.pp)
    assert lens.max() >= min(ps, 230) and lens.max() > 64
    run_and_check(c, f"long groups dim={dim} B={B} partSize={ps}")


def _groups_per_wavefront(P, ps):
    """What launch_typed makes of P groups (gnna_typed.hip): 64, at most 2048 / partSize, halved while chunks < 16 per CU."""
    G = max(1, min(64, 2048 // ps))
    while G > 1 and -(-P // G) < _lib.device_cus() * 16:
        G >>= 1
    return G


# Enough neighbor-groups that a wavefront takes several (the launch gives every compute unit 16 chunks before it lets a chunk
# grow): only then are the groups of a row merged into runs, does a run end at a bad group inside a chunk, and does a run
# reach past 64 edges from several groups.  3,000 rows; 240,000 edges, 350,000 where 64 groups of one edge must fill a chunk.
@pytest.mark.parametrize("shuffle", [False, True], ids=["canonical", "shuffled"])
@pytest.mark.parametrize("ps,dim,B,R,nnz,want_G", [(1, 16, 3, 3, 480000, 64), (3, 41, 2, 40, 330000, 16), (32, 64, 4, 3, 330000, 2),
                                                   (8, 7, 8, 3, 330000, 4)])
def test_many_groups_per_wavefront(ps, dim, B, R, nnz, want_G, shuffle):
    """The paths every real graph takes.  shuffled: blocks of five consecutive groups in random order (rows split over distant
    chunks, partial runs inside a chunk), three empty groups, three groups with decreasing pointers, four rows outside."""
    c = make(dim, B, R, ps, seed=200 + ps, shuffle=shuffle, shuffle_block=5, norm=ps != 3, n_out=3000, n_in=3000, nnz=nnz)
    G = _groups_per_wavefront(len(c.p2n), ps)
    if _lib.device_cus() == 256:
        assert G == want_G, (G, len(c.p2n))
    assert G >= 2, f"the case must give a wavefront several groups (P = {len(c.p2n)})"
    if not shuffle:
        # the hub row's groups follow each other and fill more than one chunk: runs of G groups, each longer than a step where
        # G * partSize > 64
        assert (c.p2n == 5).sum() > G
    run_and_check(c, f"G={G} dim={dim} B={B} R={R} partSize={ps} shuffled={shuffle}")


def test_a_skipped_edge_reads_no_coefficients():
    """A non-finite row of C reaches only the edges of its type: here type 0 has no edge, and the skipped edges and the idle slots
    of every step must not bring row 0 in."""
    c = make(41, 3, 3, 3, seed=85)
    c.ety[c.ety == 0] = 2
    c.C[0, :] = [np.nan, np.inf, -np.inf]
    run_and_check(c, "coef[0, :] not finite, no edge of type 0")


def test_coef_grad_accumulates_and_tuning_deterministic_is_refused():
    c = make(16, 3, 3, 32, seed=80)
    d, (T, Ts, dC, dCs) = run_and_check(c, "accumulate base")
    start = torch.arange(c.R * c.B, dtype=torch.float32, device="cuda").view(c.R, c.B) - 4.0
    got = _lib.typed_coef_grad(d.X, d.Go, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.R, c.ps, out=start.clone(), accumulate=True)
    assert_close_f64(got.cpu().numpy(), dC + start.cpu().numpy().astype(np.float64), what="coef grad accumulate",
                     scale=dCs + np.abs(start.cpu().numpy()))
    before = _lib.get_tuning()
    lib = _lib.load()
    try:
        _lib.set_tuning(deterministic=1)
        for call in (lambda: _lib.agg_typed_expand(d.X, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps),
                     lambda: _lib.agg_typed_contract(d.Gt, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps),
                     lambda: _lib.typed_coef_grad(d.X, d.Go, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.R, c.ps)):
            with pytest.raises(_lib.GnnaError, match=f"libgnna error {UNSUPPORTED}.*deterministic"):
                call()
    finally:
        _lib.reset_tuning()
    assert _lib.get_tuning() == before
    assert lib.gnna_version() == 601


def test_expand_inside_a_captured_graph():
    c = make(64, 4, 8, 32, seed=90)
    d = device(c)
    (T, _, _), (Ts, _, _) = reference(c), reference(c, absolute=True)
    eager = _lib.agg_typed_expand(d.X, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps)
    out = torch.full_like(eager, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.agg_typed_expand(d.X, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps, out=out)      # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _lib.agg_typed_expand(d.X, d.C, d.ci, d.ety, d.nrm, d.pp, d.p2n, c.n_out, c.ps, out=out)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert_close_f64(eager.cpu().numpy(), T, what="eager expand", scale=Ts)
    assert_close_f64(out.cpu().numpy(), T, what="replayed expand", scale=Ts)
    d.X.mul_(2.0)                                                                # a replay reads the inputs as they are now
    graph.replay()
    torch.cuda.synchronize()
    assert_close_f64(out.cpu().numpy(), 2.0 * T, what="replayed expand, new inputs", scale=2.0 * Ts)

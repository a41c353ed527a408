"""What test_far_offsets_gpu.py is built from (checker side only): the geometry of the arena, the column windows with their
borders, and the 272-node graph with its variants.  The graph part needs no GPU (test_far_offsets_host.py)."""
import types

import numpy as np
import torch

ROWS, LD = 272, 1 << 24                 # node-sized operands: row r starts r * 64 MiB past the base
SEG_ROWS, SEG_LD = 18, 1 << 28          # segment-sized operands: row s starts s * 1 GiB past the base
ARENA_FLOATS = (1 << 32) + (1 << 29)    # 18 GiB: 272 * 2^24 + 2^28 = 18 * 2^28
WINDOW = 4096                           # floats between the column windows of two operands
PAD = 4                                 # floats on each side of a window: NaN beside an input, the sentinel beside an output
SENTINEL = 12288.0                      # (exact in bfloat16 and float16)
INT_SENTINEL = 0x5A5A5A5A
INT_POISON = -(2 ** 31)
REGIONS = ((0, 32), (32, 64), (64, 128), (128, 256), (256, 272))     # between the marks of the node-sized rows
MARKS = {"2^31 bytes": 32, "2^32 bytes": 64, "2^31 floats": 128, "2^32 floats": 256}
SEG_MARKS = {"2^31 bytes": 2, "2^32 bytes": 4, "2^31 floats": 8, "2^32 floats": 16}


def distinct_rows(data, moduli, what):
    """Rows r and r mod m of `data` differ for every m: a kernel that drops the high bits of an offset meets other values."""
    a = np.asarray(data.cpu() if isinstance(data, torch.Tensor) else data)
    for m in moduli:
        for r in range(m, a.shape[0]):
            assert not np.array_equal(a[r], a[r % m]), f"{what}: rows {r} and {r % m} hold the same values (modulus {m})"


class Windows:
    """The column windows of one call: every operand gets the next one, at (k * WINDOW + shift) floats into every arena row."""

    def __init__(self, arena, shift):
        self.arena, self.shift, self.k, self.outs = arena, int(shift), 0, []

    def _views(self, kind, width, dtype, rows):
        n, ld = (ROWS, LD) if kind == "node" else (SEG_ROWS, SEG_LD)
        n = n if rows is None else rows
        self.k += 1
        per = 4 // torch.empty(0, dtype=dtype).element_size()          # elements per float: the 16-bit views cover the same bytes
        base = self.arena if dtype == torch.float32 else self.arena.view(dtype)
        off = (self.k * WINDOW + self.shift) * per
        assert (width + 2 * PAD * per) <= WINDOW * per and (n - 1) * ld + (self.k + 1) * WINDOW + 1 < ARENA_FLOATS
        padded = torch.as_strided(base, (n, width + 2 * PAD * per), (ld * per, 1), off - PAD * per)
        view = padded[:, PAD * per: PAD * per + width]
        assert view.stride(0) == ld * per and view.data_ptr() == base.data_ptr() + off * base.element_size()
        return padded, view

    def inp(self, data, kind="node", moduli=None, what="input"):
        """`data` (a CPU tensor [rows, width]) as a window of the arena, NaN (INT_MIN) on the 4 floats each side of it."""
        data = data.contiguous()
        if moduli is None:
            moduli = ((64, 128, 256) if data.shape[0] > 256 else (32,)) if kind == "node" else (4, 8, 16)
        distinct_rows(data.view(torch.int16) if data.element_size() == 2 else data, moduli, what)
        padded, view = self._views(kind, data.shape[1], data.dtype, data.shape[0])
        padded.fill_(float("nan") if data.dtype.is_floating_point else INT_POISON)
        view.copy_(data.cuda())
        return view

    def out(self, kind, width, dtype=torch.float32, rows=None, fill=None, what="output"):
        """An output window: the sentinel on the 4 floats each side, inside it the poison value, or `fill` (accumulate)."""
        padded, view = self._views(kind, width, dtype, rows)
        padded.fill_(SENTINEL if dtype.is_floating_point else INT_SENTINEL)
        if fill is None:
            view.fill_(float("nan") if dtype.is_floating_point else INT_POISON)
        else:
            view.copy_(fill.cuda())
        self.outs.append((padded, view, what))
        return view

    def check(self):
        """Every output window is fully written and nothing beside it was touched."""
        for padded, view, what in self.outs:
            p = padded.cpu()
            lo = (p.shape[1] - view.shape[1]) // 2
            inner, border = p[:, lo: lo + view.shape[1]], torch.cat([p[:, :lo], p[:, lo + view.shape[1]:]], 1)
            if p.dtype.is_floating_point:
                assert not torch.isnan(inner).any(), f"{what}: elements the call did not write"
                assert (border == SENTINEL).all(), f"{what}: written outside the window"
            else:
                assert (inner != INT_POISON).all(), f"{what}: elements the call did not write"
                assert (border == INT_SENTINEL).all(), f"{what}: written outside the window"


def _csr(adj):
    rp = np.r_[0, np.cumsum([len(a) for a in adj])].astype(np.int32)
    ci = np.array([j for a in adj for j in sorted(a)], dtype=np.int32)
    return rp, ci


def _covers_regions(rp, ci, what):
    for i in range(len(rp) - 1):
        ids = ci[rp[i]:rp[i + 1]]
        if len(ids) >= 5:
            for lo, hi in REGIONS:
                assert ((ids >= lo) & (ids < hi)).any(), f"{what}: row {i} has no source in [{lo}, {hi})"


def graphs():
    """-> namespace(sym, directed, rect, small), each (row_pointers, column_index, num_in_rows) as numpy int32, ids sorted.

    sym: 272 nodes, the edge multiset is symmetric.  Row 0 has no edge; row 1 one (the hub); rows 2, 3, 4 have 63, 64 and 65,
    spread evenly over the rows 6 .. 271; row 5 is the hub: row 1, every row 6 .. 271, and the rows 6 .. 21 a second time (283
    edges).  Every row i >= 6 is tied to 6 + i % 26, 32 + i % 32, 64 + i % 64, 128 + i % 128 and 256 + i % 16 (one source on
    each side of every mark), to the hub, and to whoever picked it.
    directed: sym plus, for every third row i >= 6, the source (5 i + 7) % 266 + 6 without its reverse, and the source 0 for the
    rows with i % 40 == 7.  rect: the first 270 rows of directed over all 272 sources.
    small: 63 rows over 63 sources (63 * 2^26 bytes < 2^32): row i gathers (i + 1, 2 i + 5, 3 i + 11, 5 i, 7 i + 40) % 63 and
    32 + i % 31; row 62 gathers every row."""
    n = ROWS
    adj = [[] for _ in range(n)]

    def link(a, b):
        adj[a].append(b)
        if a != b:
            adj[b].append(a)

    pairs = set()
    for i in range(6, n):
        for p in (6 + i % 26, 32 + i % 32, 64 + i % 64, 128 + i % 128, 256 + i % 16):
            pairs.add((min(i, p), max(i, p)))
    for a, b in sorted(pairs):
        link(a, b)
    for row, deg in ((2, 63), (3, 64), (4, 65)):
        for t in range(deg):
            link(row, 6 + (t * 266) // deg)
    link(5, 1)
    for j in list(range(6, n)) + list(range(6, 22)):
        link(5, j)
    sym = _csr(adj)
    dadj = [list(a) for a in adj]
    for i in range(6, n):
        if i % 3 == 0:
            dadj[i].append((5 * i + 7) % 266 + 6)
        if i % 40 == 7:
            dadj[i].append(0)
    directed = _csr(dadj)
    rect = _csr(dadj[:270])
    sadj = [sorted({(i + 1) % 63, (2 * i + 5) % 63, (3 * i + 11) % 63, (5 * i) % 63, (7 * i + 40) % 63, 32 + i % 31}) for i in range(63)]
    sadj[62] = list(range(63))
    small = _csr(sadj)

    deg = np.diff(sym[0])
    assert [int(d) for d in deg[:5]] == [0, 1, 63, 64, 65] and deg[5] == 283, deg[:6]
    assert len(set(sym[1][sym[0][5]:sym[0][6]])) < deg[5], "the hub holds repeated ids"
    assert [int(d) for d in np.diff(directed[0])[:6]] == [0, 1, 63, 64, 65, 283]
    rows = np.repeat(np.arange(n), deg)
    fwd = sorted(zip(rows.tolist(), sym[1].tolist()))
    assert fwd == sorted(zip(sym[1].tolist(), rows.tolist())), "sym: the edge multiset is not symmetric"
    drows = np.repeat(np.arange(n), np.diff(directed[0]))
    assert sorted(zip(drows.tolist(), directed[1].tolist())) != sorted(zip(directed[1].tolist(), drows.tolist()))
    assert set(directed[1].tolist()) == set(range(n)), "directed: every row is a source"
    for name, (rp, ci) in (("sym", sym), ("directed", directed), ("rect", rect)):
        _covers_regions(rp, ci, name)
    assert all(((small[1][small[0][i]:small[0][i + 1]]) >= 32).any() for i in range(63)), "small: every row gathers past 2^31 bytes"
    return types.SimpleNamespace(sym=(*sym, n), directed=(*directed, n), rect=(*rect, n), small=(*small, 63))


# 18 segments over the 272 rows with an empty one; the second leaves rows 0 .. 2, 270 and 271 to no graph
SEGMENTS = {
    "all_rows": np.r_[0, np.cumsum([1, 0, 63, 64, 65, 2, 3, 5, 7, 1, 11, 4, 6, 8, 9, 10, 12, 1])].astype(np.int32),
    "rows_of_no_graph": (3 + np.r_[0, np.cumsum([5, 40, 0, 17, 33, 64, 1, 1, 2, 30, 20, 10, 8, 7, 6, 5, 9, 9])]).astype(np.int32),
}
assert all(len(p) == SEG_ROWS + 1 for p in SEGMENTS.values()) and SEGMENTS["all_rows"][-1] == ROWS and SEGMENTS["rows_of_no_graph"][-1] == 270

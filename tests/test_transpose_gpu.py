"""Device builders of a directed graph's backward structure: gnna_transpose_csr_i32 (the transposed CSR + edge permutation) and
gnna_build_part_device_i32 (the partition of device row pointers).  Every result is compared EXACTLY, as integers, with
numpy's stable argsort / the host partitioner."""
import numpy as np
import pytest
import torch

from gnnadvisor_osdi21_amd import _lib, graph, load_extension

pytestmark = pytest.mark.gpu
GNNA = load_extension()


def _csr(rp, ci):
    return torch.as_tensor(np.asarray(rp), dtype=torch.int32), torch.as_tensor(np.asarray(ci), dtype=torch.int32)


def _directed():
    g = graph.uniform_graph(300, 3000, symmetric=False)
    return g.row_pointers.clone(), g.column_index.clone(), 300


def _shuffled_with_duplicates():
    """The directed graph with 5 % of its edges duplicated and every row's ids in random order."""
    rp, ci, n = _directed()
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(n), np.diff(rp.numpy()))
    cols = ci.numpy()
    dup = rng.choice(len(cols), size=len(cols) // 20, replace=False)
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    order = np.lexsort((rng.random(len(rows)), rows))          # by row, random inside a row
    rows, cols = rows[order], cols[order]
    new_rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (*_csr(new_rp, cols), n)


def _self_loops():
    rp, ci, n = _directed()
    rows = np.repeat(np.arange(n), np.diff(rp.numpy()))
    rows, cols = np.concatenate([rows, np.arange(n)]), np.concatenate([ci.numpy(), np.arange(n)])
    order = np.argsort(rows, kind="stable")                    # the loop comes last in its row
    new_rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return (*_csr(new_rp, cols[order]), n)


def _one_node():
    return (*_csr([0, 2], [0, 0]), 1)


def _no_edges():
    return (*_csr(np.zeros(8, dtype=np.int32), []), 7)


def _rectangular():
    """200 destination rows over 350 source rows."""
    rng = np.random.default_rng(5)
    deg = rng.integers(0, 12, size=200)
    return (*_csr(np.concatenate([[0], np.cumsum(deg)]), rng.integers(0, 350, size=int(deg.sum()))), 350)


def _out_of_range():
    """1 % of the ids set to -1 or num_in_rows."""
    rp, ci, n = _directed()
    rng = np.random.default_rng(7)
    bad = rng.choice(ci.numel(), size=max(2, ci.numel() // 100), replace=False)
    ci = ci.clone()
    ci[torch.as_tensor(bad[::2])] = -1
    ci[torch.as_tensor(bad[1::2])] = n
    return rp, ci, n


def _hub():
    """N = 6000: destination row 17 has 5,000 edges, source id 4242 is named by 5,000 rows, plus two random edges per row.
    More edges than one tile of the sort holds, so the digit counts are scanned across blocks."""
    n = 6000
    rng = np.random.default_rng(3)
    rows = [np.full(5000, 17), rng.choice(n, size=5000, replace=False), np.repeat(np.arange(n), 2)]
    cols = [rng.choice(n, size=5000, replace=False), np.full(5000, 4242), rng.integers(0, n, size=2 * n)]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((rng.random(len(rows)), rows))
    rows, cols = rows[order], cols[order]
    return (*_csr(np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]), cols), n)


CASES = {"directed": _directed, "shuffled_duplicates": _shuffled_with_duplicates, "self_loops": _self_loops, "one_node": _one_node,
         "no_edges": _no_edges, "rectangular": _rectangular, "out_of_range": _out_of_range, "hub": _hub}
_made = {}


def _case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def _expected(rp, ci, n_in):
    """(t_row_pointers, t_column_index, t_perm) by numpy: a stable argsort of the ids, invalid ids dropped, -1 tails."""
    rp, ci = rp.numpy().astype(np.int64), ci.numpy().astype(np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    valid = (ci >= 0) & (ci < n_in)
    key = np.where(valid, ci, n_in)
    perm = np.argsort(key, kind="stable")
    kept = int(valid.sum())
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(ci[valid], minlength=n_in))])
    t_ci, t_perm = rows[perm], perm.copy()
    t_ci[kept:] = -1
    t_perm[kept:] = -1
    return t_rp.astype(np.int32), t_ci.astype(np.int32), t_perm.astype(np.int32)


@pytest.mark.parametrize("name", list(CASES))
def test_transpose_equals_numpy_stable_argsort(name):
    rp, ci, n_in = _case(name)
    want = _expected(rp, ci, n_in)
    got = _lib.transpose_csr(rp.cuda(), ci.cuda(), num_in_rows=n_in)
    for g, w, what in zip(got, want, ("t_row_pointers", "t_column_index", "t_perm")):
        assert g.dtype == torch.int32 and g.is_cuda
        assert np.array_equal(g.cpu().numpy(), w), f"{name}: {what} differs"
    assert int(got[0][-1]) == int((want[2] >= 0).sum())
    # without t_perm: the same ids
    t_rp, t_ci, none = _lib.transpose_csr(rp.cuda(), ci.cuda(), num_in_rows=n_in, want_perm=False)
    assert none is None and torch.equal(t_rp, got[0]) and torch.equal(t_ci, got[1])
    # the module's entry is the same call
    m = GNNA.transpose_csr(rp.cuda(), ci.cuda(), n_in)
    assert len(m) == 3 and all(torch.equal(a, b) for a, b in zip(m, got))


@pytest.mark.parametrize("name", ["shuffled_duplicates", "hub"])
def test_two_calls_give_identical_bits(name):
    rp, ci, n_in = _case(name)
    a = _lib.transpose_csr(rp.cuda(), ci.cuda(), num_in_rows=n_in)
    b = _lib.transpose_csr(rp.cuda(), ci.cuda(), num_in_rows=n_in)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_symmetric_sorted_graph_is_its_own_transpose_and_perm_is_the_reverse_edge_map():
    """Cross-check against the host code: on a symmetric CSR with sorted, duplicate-free rows A^T = A and t_perm pairs every
    edge with its reverse exactly as gnna_reverse_edges_i32 does."""
    g = graph.uniform_graph(300, 3000, seed=2)
    t_rp, t_ci, t_perm = _lib.transpose_csr(g.row_pointers.cuda(), g.column_index.cuda())
    assert torch.equal(t_rp.cpu(), g.row_pointers) and torch.equal(t_ci.cpu(), g.column_index)
    assert torch.equal(t_perm.cpu(), _lib.reverse_edges(g.row_pointers, g.column_index))


@pytest.mark.parametrize("partSize", [1, 3, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_build_part_device_equals_the_host_partitioner(name, partSize):
    rp, _ci, _n = _case(name)
    pp, p2n = _lib.build_part(partSize, rp)
    assert _lib.count_parts_device(partSize, rp.cuda()) == p2n.numel()
    d_pp, d_p2n = _lib.build_part_device(partSize, rp.cuda())
    assert d_pp.is_cuda and d_pp.dtype == torch.int32 and d_p2n.dtype == torch.int32
    assert torch.equal(d_pp.cpu(), pp) and torch.equal(d_p2n.cpu(), p2n)
    m_pp, m_p2n = GNNA.build_part_device(partSize, rp.cuda())
    assert torch.equal(m_pp, d_pp) and torch.equal(m_p2n, d_p2n)


def test_transposed_partition_equals_the_host_partition_of_the_transposed_rows():
    """Empty rows and the hub column: the partition of the transposed hub graph, built from the device-made row pointers."""
    rp, ci, n_in = _case("hub")
    t_rp, _t_ci, _ = _lib.transpose_csr(rp.cuda(), ci.cuda(), num_in_rows=n_in, want_perm=False)
    for partSize in (3, 32):
        pp, p2n = _lib.build_part(partSize, t_rp.cpu())
        d_pp, d_p2n = _lib.build_part_device(partSize, t_rp)
        assert torch.equal(d_pp.cpu(), pp) and torch.equal(d_p2n.cpu(), p2n)


def test_builders_refuse_host_tensors_and_stream_captures():
    rp, ci, _n = _case("directed")
    with pytest.raises(_lib.GnnaError, match="device"):
        _lib.transpose_csr(rp, ci)
    with pytest.raises(_lib.GnnaError, match="device"):
        _lib.build_part_device(32, rp)
    d_rp, d_ci = rp.cuda(), ci.cuda()
    t_rp = torch.empty_like(d_rp)
    t_ci, t_perm = torch.empty_like(d_ci), torch.empty_like(d_ci)
    _lib.transpose_csr(d_rp, d_ci)                      # (scratch exists: the capture below has nothing to allocate)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc_t = rc_p = None
    with torch.cuda.stream(side):
        graph_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph_, stream=side):
            lib = _lib.load()
            rc_t = lib.gnna_transpose_csr_i32(d_rp.data_ptr(), d_ci.data_ptr(), d_rp.numel() - 1, d_rp.numel() - 1, t_rp.data_ptr(),
                                              t_ci.data_ptr(), t_perm.data_ptr(), side.cuda_stream)
            rc_p = lib.gnna_count_parts_device_i32(32, d_rp.data_ptr(), d_rp.numel() - 1, side.cuda_stream)
            d_ci.add_(0)                                # (a capture must record something)
    assert rc_t == -3 and rc_p == -3                    # GNNA_ERR_UNSUPPORTED

"""gnna_sample_neighbors_i32 on the GPU, exact against the numpy restatement of the rule (tests/sampling_ref.py)."""
import functools

import numpy as np
import pytest
import torch

import sampling_ref as ref
from gnnadvisor_osdi21_amd import _lib

pytestmark = pytest.mark.gpu

RNG_SEEDS = (2024, (1 << 63) + 0x1234_5678_9ABC)
FANOUTS = (1, 2, 5, 25, 64, 100, -1)


@functools.lru_cache(maxsize=None)
def device_graph():
    rp, ci = ref.shared_graph()
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


@functools.lru_cache(maxsize=None)
def expected(size, fanout, rng_seed):
    rp, ci = ref.shared_graph()
    return ref.sample_block(rp, ci, ref.seed_sets()[size], fanout, rng_seed)


def run(size, fanout, rng_seed, partSize=None, **kw):
    rp, ci = device_graph()
    seeds = torch.from_numpy(ref.seed_sets()[size]).cuda()
    return _lib.sample_neighbors(rp, ci, seeds, fanout, rng_seed, partSize=partSize, **kw)


def same(got, want):
    got = got.cpu().numpy().astype(np.int64)
    return got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize("fanout", FANOUTS)
@pytest.mark.parametrize("size", [1, 64, 65, 1000])
def test_block_equals_the_restatement(size, fanout):
    for k, rng_seed in enumerate(RNG_SEEDS):
        partSize = (1, 3, 32)[(size + fanout + k) % 3]
        want = expected(size, fanout, rng_seed)
        got = run(size, fanout, rng_seed, partSize)
        assert got["num_dst"] == size and got["num_src"] == len(want["src_nodes"])
        assert same(got["row_pointers"], want["row_pointers"])
        assert same(got["edge_ids"], want["edge_ids"])
        assert same(got["column_index"], want["column_index"])
        assert same(got["src_nodes"], want["src_nodes"])
        pp, p2n = ref.host_build_part(partSize, want["row_pointers"])
        assert same(got["partPtr"], pp) and same(got["part2Node"], p2n)
        src = got["src_nodes"].cpu().numpy()
        assert (src[:size] == ref.seed_sets()[size]).all() and (np.diff(src[size:]) > 0).all()


@pytest.mark.parametrize("partSize", [1, 3, 32])
def test_partition_equals_host_build_part(partSize):
    got = run(1000, 25, RNG_SEEDS[0], partSize)
    pp, p2n = _lib.build_part(partSize, got["row_pointers"].cpu())
    assert torch.equal(got["partPtr"].cpu(), pp.int()) and torch.equal(got["part2Node"].cpu(), p2n.int())


def test_second_call_gives_the_same_bits_and_edge_ids_are_optional():
    a, b = run(1000, 5, RNG_SEEDS[1], 32), run(1000, 5, RNG_SEEDS[1], 32, want_edge_ids=False)
    assert b["edge_ids"] is None
    for name in ("row_pointers", "column_index", "src_nodes", "partPtr", "part2Node"):
        assert torch.equal(a[name], b[name]), name


def test_another_rng_seed_changes_the_picks():
    a, b = run(65, 5, RNG_SEEDS[0]), run(65, 5, RNG_SEEDS[1])
    assert torch.equal(a["row_pointers"], b["row_pointers"])
    assert not torch.equal(a["edge_ids"], b["edge_ids"])


def test_no_seeds():
    rp, ci = device_graph()
    got = _lib.sample_neighbors(rp, ci, torch.zeros(0, dtype=torch.int32, device="cuda"), 5, 1, partSize=32)
    assert got["num_src"] == 0 and got["row_pointers"].tolist() == [0] and got["partPtr"].tolist() == [0]
    assert got["column_index"].numel() == 0 and got["part2Node"].numel() == 0


def test_errors_name_their_cause_and_the_next_call_succeeds():
    rp, ci = device_graph()
    seeds = ref.seed_sets()[65].copy()
    dup = torch.from_numpy(np.concatenate([seeds, seeds[3:4]])).cuda()
    with pytest.raises(_lib.GnnaError, match="duplicate seed"):
        _lib.sample_neighbors(rp, ci, dup, 5, 1, partSize=32)
    assert same(run(65, 5, RNG_SEEDS[0], 32)["edge_ids"], expected(65, 5, RNG_SEEDS[0])["edge_ids"])
    outside = torch.tensor([5, rp.numel() - 1, 7], dtype=torch.int32, device="cuda")         # a seed equal to num_nodes
    with pytest.raises(_lib.GnnaError, match=r"seeds\[1\] is outside"):
        _lib.sample_neighbors(rp, ci, outside, 5, 1, partSize=32)
    assert same(run(65, 5, RNG_SEEDS[0], 32)["edge_ids"], expected(65, 5, RNG_SEEDS[0])["edge_ids"])
    want = expected(65, 5, RNG_SEEDS[0])
    nnz = len(want["edge_ids"])
    with pytest.raises(_lib.GnnaError, match="capacity too small") as info:
        run(65, 5, RNG_SEEDS[0], 32, edge_capacity=nnz - 1)
    parts = len(ref.host_build_part(32, want["row_pointers"])[1])
    assert info.value.counts == (nnz, len(want["src_nodes"]), parts)
    assert same(run(65, 5, RNG_SEEDS[0], 32)["edge_ids"], want["edge_ids"])
    with pytest.raises(_lib.GnnaError, match="partSize must be positive"):
        run(65, 5, RNG_SEEDS[0], 0)


def test_refused_inside_a_stream_capture():
    import ctypes
    rp, ci = device_graph()
    seeds = torch.from_numpy(ref.seed_sets()[64]).cuda()
    _lib.sample_neighbors(rp, ci, seeds, 5, 1)               # (scratch exists: the capture below has nothing to allocate)
    blk_rp = torch.empty(65, dtype=torch.int32, device="cuda")
    counts = (ctypes.c_int64 * 3)()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = None
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lib = _lib.load()
            rc = lib.gnna_sample_neighbors_i32(rp.data_ptr(), ci.data_ptr(), rp.numel() - 1, seeds.data_ptr(), 64, 5, 1, 0,
                                               blk_rp.data_ptr(), None, None, None, None, None, 0, 0, counts, side.cuda_stream)
            blk_rp.add_(0)                                   # (a capture must record something)
    assert rc == -3 and "stream capture" in lib.gnna_last_error().decode()      # GNNA_ERR_UNSUPPORTED


def test_uniformity_of_the_rule_as_run():
    rows, d, fanout = 2000, 40, 10
    rp = (torch.arange(rows + 1, dtype=torch.int32) * d).cuda()
    ci = (torch.arange(rows * d, dtype=torch.int32) % rows).cuda()
    got = _lib.sample_neighbors(rp, ci, torch.arange(rows, dtype=torch.int32).cuda(), fanout, 2024)
    eid = got["edge_ids"].cpu().numpy()
    assert len(eid) == rows * fanout
    counts = np.bincount(eid % d, minlength=d)
    sd = np.sqrt(rows * 0.25 * 0.75)
    print("largest deviation: %.2f standard deviations" % (np.abs(counts - 500).max() / sd))
    assert np.abs(counts - 500).max() <= 5 * sd

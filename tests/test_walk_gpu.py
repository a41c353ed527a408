"""gnna_random_walk_i32 on the GPU, exact against the numpy restatement of the walk rule (tests/walk_ref.py)."""
import functools

import numpy as np
import pytest
import torch

import walk_ref as ref
from gnnadvisor_osdi21_amd import _lib

pytestmark = pytest.mark.gpu

RNG_SEEDS = (0, 2024, (1 << 64) - 3)
LENGTHS = (0, 1, 4, 10)


@functools.lru_cache(maxsize=None)
def device_graph(dead_ends=False):
    rp, ci = ref.dead_end_graph() if dead_ends else ref.shared_graph()
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


@functools.lru_cache(maxsize=None)
def expected(size, length, rng_seed, dead_ends=False):
    rp, ci = ref.dead_end_graph() if dead_ends else ref.shared_graph()
    return ref.random_walks(rp, ci, ref.root_sets()[size], length, rng_seed)


def run(size, length, rng_seed, dead_ends=False, want_edge_ids=True):
    rp, ci = device_graph(dead_ends)
    return _lib.random_walk(rp, ci, torch.from_numpy(ref.root_sets()[size]).cuda(), length, rng_seed, want_edge_ids=want_edge_ids)


def same(got, want):
    got = got.cpu().numpy().astype(np.int64)
    return got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("size", [1, 64, 65, 1000])
def test_walks_equal_the_restatement(size, length):
    for rng_seed in RNG_SEEDS:
        walks, eids = run(size, length, rng_seed)
        want_walks, want_eids = expected(size, length, rng_seed)
        assert walks.dtype == eids.dtype == torch.int32
        assert same(walks, want_walks), rng_seed
        assert same(eids, want_eids), rng_seed


def test_the_roots_cover_the_special_rows_and_the_bad_roots():
    roots = ref.root_sets()[1000]
    assert set(range(11)) | set(range(20, 30)) | {-1, ref.N} <= set(roots.tolist())
    walks, eids = run(1000, 4, 2024)
    bad = torch.from_numpy((roots < 0) | (roots >= ref.N)).cuda()
    assert bool((walks[bad] == -1).all()) and bool((eids[bad] == -1).all())
    edgeless = torch.from_numpy((roots >= 20) & (roots < 30)).cuda()
    assert bool((walks[edgeless] == walks[edgeless][:, :1]).all()) and bool((eids[edgeless] == -1).all())


@pytest.mark.parametrize("length", [1, 10])
def test_dead_ends_are_never_followed(length):
    walks, eids = run(1000, length, 2024, dead_ends=True)
    want_walks, want_eids = expected(1000, length, 2024, dead_ends=True)
    assert same(walks, want_walks) and same(eids, want_eids)
    assert not (want_walks == expected(1000, length, 2024)[0]).all()             # (some draw did hit one)
    assert int(walks.max()) < ref.N and int(walks.min()) >= -1


def test_two_calls_give_equal_bits_and_edge_ids_are_optional():
    a, b = run(1000, 10, RNG_SEEDS[2]), run(1000, 10, RNG_SEEDS[2], want_edge_ids=False)
    assert b[1] is None and torch.equal(a[0], b[0])
    c = run(1000, 10, RNG_SEEDS[2])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert not torch.equal(a[0], run(1000, 10, RNG_SEEDS[1])[0])


def test_accepted_under_the_deterministic_switch():
    _lib.set_tuning(deterministic=1)
    try:
        walks, eids = run(65, 4, 2024)
    finally:
        _lib.reset_tuning()
    want_walks, want_eids = expected(65, 4, 2024)
    assert same(walks, want_walks) and same(eids, want_eids)


def test_no_roots_and_no_steps():
    rp, ci = device_graph()
    walks, eids = _lib.random_walk(rp, ci, torch.zeros(0, dtype=torch.int32, device="cuda"), 3, 1, want_edge_ids=True)
    assert tuple(walks.shape) == (0, 4) and tuple(eids.shape) == (0, 3)
    walks, eids = run(64, 0, 5)
    assert tuple(eids.shape) == (64, 0) and same(walks, expected(64, 0, 5)[0])


def test_a_captured_call_replays_to_the_same_arrays():
    rp, ci = device_graph()
    roots = torch.from_numpy(ref.root_sets()[1000]).cuda()
    length, rng_seed = 4, 2024
    walks = torch.full((1000, length + 1), -7, dtype=torch.int32, device="cuda")
    eids = torch.full((1000, length), -7, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = lib.gnna_random_walk_i32(rp.data_ptr(), ci.data_ptr(), rp.numel() - 1, ci.numel(), roots.data_ptr(), 1000, length,
                                          rng_seed, walks.data_ptr(), eids.data_ptr(), side.cuda_stream)
    assert rc == 0, lib.gnna_last_error().decode()
    torch.cuda.synchronize()
    want_walks, want_eids = expected(1000, length, rng_seed)
    for _ in range(2):
        walks.fill_(-7)
        eids.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert same(walks, want_walks) and same(eids, want_eids)


def test_uniformity_on_the_device():
    # node 0 has 40 distinct neighbours 1 .. 40, each of which has node 0 as its only edge
    d, walks_n = 40, 2000
    rp = torch.tensor([0] + [d + k for k in range(d + 1)], dtype=torch.int32).cuda()
    ci = torch.tensor(list(range(1, d + 1)) + [0] * d, dtype=torch.int32).cuda()
    walks, _ = _lib.random_walk(rp, ci, torch.zeros(walks_n, dtype=torch.int32, device="cuda"), 1, 2024)
    counts = np.bincount(walks[:, 1].cpu().numpy(), minlength=d + 1)
    assert counts[0] == 0 and counts.sum() == walks_n
    sd = np.sqrt(walks_n * (1 / d) * (1 - 1 / d))
    worst = np.abs(counts[1:] - walks_n / d).max() / sd
    print("largest deviation: %.2f standard deviations" % worst)
    assert worst <= 5

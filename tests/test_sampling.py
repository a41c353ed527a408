"""Neighbor sampling, the parts that need no GPU: the numpy restatement of the rule is self-consistent, the symbol is declared,
exported and bound, the driver parses --fanout / --batch_size and refuses the combinations it cannot run."""
import os
import re

import numpy as np
import pytest

import sampling_ref as ref
from gnnadvisor_osdi21_amd import _lib, main as driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fanout", [1, 5, 64, -1])
def test_restatement_picks_min_d_k_distinct_positions_in_order(fanout):
    rp, ci = ref.shared_graph()
    seeds = ref.seed_sets()[65]
    blk = ref.sample_block(rp, ci, seeds, fanout, 0xDEADBEEFCAFEF00D)
    for i, r in enumerate(seeds):
        picks = blk["edge_ids"][blk["row_pointers"][i]: blk["row_pointers"][i + 1]]
        d = int(rp[r + 1]) - int(rp[r])
        assert len(picks) == (d if fanout <= 0 else min(d, fanout))
        assert (np.diff(picks) > 0).all()
        assert len(picks) == 0 or (picks[0] >= rp[r] and picks[-1] < rp[r + 1])
    S = len(seeds)
    assert (blk["src_nodes"][:S] == seeds).all() and (np.diff(blk["src_nodes"][S:]) > 0).all()
    assert (blk["src_nodes"][blk["column_index"]] == ci[blk["edge_ids"]]).all()


def test_restatement_keys_wrap_mod_2_64():
    # one key by hand, in Python integers
    seed, e = (1 << 63) + 12345, 7
    z = (seed + 0x9E3779B97F4A7C15 * (e + 1)) & ref.M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ref.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ref.M64
    assert int(ref.keys_of(seed, [e])[0]) == z ^ (z >> 31)


def test_restatement_is_uniform_on_the_uniformity_input():
    # 2,000 rows of 40 positions, fanout 10, rng_seed 2024: every slot within 5 standard deviations of 500
    counts = np.zeros(40)
    for row in range(2000):
        counts[ref.pick_row(40 * row, 40 * row + 40, 10, 2024) - 40 * row] += 1
    assert np.abs(counts - 500).max() <= 5 * np.sqrt(2000 * 0.25 * 0.75)


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gnna.h")).read()
    assert re.search(r"GNNA_API\s+int\s+gnna_sample_neighbors_i32\s*\(", header)
    assert "gnna_sample_neighbors_i32" in _lib.EXPORTS and hasattr(_lib.load(), "gnna_sample_neighbors_i32")
    assert callable(_lib.sample_neighbors)
    # the rule is part of the contract
    for text in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "a tie goes to the smaller e"):
        assert text in header


def test_binding_refuses_host_tensors():
    import torch
    rp = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.GnnaError, match="device tensor"):
        _lib.sample_neighbors(rp, rp, rp[:1], 2, 0)


def test_driver_parses_fanout_and_batch_size():
    args = driver.build_parser().parse_args(["--model", "sage", "--fanout", "5,5", "--batch_size", "64"])
    assert args.fanout == "5,5" and args.batch_size == 64
    assert driver.build_parser().parse_args([]).fanout is None
    assert driver.build_parser().parse_args(["--fanout", "-1,-1", "--batch_size", "8"]).fanout == "-1,-1"


@pytest.mark.parametrize("extra, message", [
    (["--model", "gcn"], "--model sage"),
    (["--model", "sage", "--hip_graph", "True"], "--hip_graph"),
    (["--model", "sage", "--single_spmm", "True"], "--single_spmm"),
    (["--model", "sage", "--verify_spmm", "True"], "--verify_spmm"),
    (["--model", "sage", "--dtype", "bfloat16"], "float32"),
    (["--model", "gcn", "--dtype", "bfloat16"], "--model sage"),
])
def test_driver_refuses_what_fanout_cannot_run(extra, message):
    with pytest.raises(SystemExit, match=message):
        driver.main(["--fanout", "5,5", "--synthetic", "no-such-config"] + extra)

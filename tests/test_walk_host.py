"""Subgraph sampling (include/gnna_walk.h), the part that needs no GPU: the numpy restatements of the walk rule and the subgraph rule
(walk_ref.py) are self-consistent, one key and step are checked by hand in Python integers, the step rule is uniform; the header
carries the constants and the rule sentences (its entries, table and signatures are checked with every other header's in
test_binding_table_host.py); the bindings refuse host tensors; the driver parses the new flags and refuses what they cannot run with."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import walk_ref as ref
from gnnadvisor_osdi21_amd import _lib
from gnnadvisor_osdi21_amd import main as driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")
HEADER = "gnna_walk.h"
M64 = (1 << 64) - 1


# ---- the restatements ----

def test_one_key_and_one_step_by_hand():
    rng_seed, w, L, t, d = (1 << 63) + 0x1234_5678_9ABC, 3, 4, 2, 40
    u = w * L + t
    z = (rng_seed + 0x9E3779B97F4A7C15 * (u + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    key = z ^ (z >> 31)
    assert int(ref.keys_of(rng_seed, [u])[0]) == key
    j = (key * d) >> 64
    assert 0 <= j < d and ref.step_index(key, d) == j
    # a graph whose every row has the positions [40 v, 40 v + 40) and position 40 v + k leads to node k: step t = 2 of walk 3 must
    # take position 40 v + j of the node v it stands at
    n = 64
    rp, ci = np.arange(n + 1) * d, np.tile(np.arange(d), n)
    walks, eids = ref.random_walks(rp, ci, np.arange(8), L, rng_seed)
    v = walks[w, t]
    assert eids[w, t] == d * v + j and walks[w, t + 1] == j


def test_walk_restatement_is_self_consistent():
    rp, ci = ref.shared_graph()
    roots = ref.root_sets()[1000]
    walks, eids = ref.random_walks(rp, ci, roots, 10, 2024)
    bad = (roots < 0) | (roots >= ref.N)
    assert bad.sum() >= 2 and (walks[bad] == -1).all() and (eids[bad] == -1).all()
    good = ~bad
    assert (walks[good, 0] == roots[good]).all()
    here, there, e = walks[good, :-1], walks[good, 1:], eids[good]
    moved = e >= 0
    assert (there[~moved] == here[~moved]).all()                                    # the walk stays
    assert (ci[e[moved]] == there[moved]).all()
    assert (e[moved] >= rp[here[moved]]).all() and (e[moved] < rp[here[moved] + 1]).all()
    assert (np.diff(rp)[here[~moved]] == 0).all()                                   # (no dead ends in this graph: only edgeless rows)
    again, _ = ref.random_walks(rp, ci, roots, 10, 2024)
    assert (again == walks).all() and not (ref.random_walks(rp, ci, roots, 10, 2025)[0] == walks).all()
    # a prefix of the roots walks the same way only where u = w * L + t agrees: L is part of the key's position
    assert (ref.random_walks(rp, ci, roots[:5], 10, 2024)[0] == walks[:5]).all()


def test_walk_restatement_never_follows_a_dead_end():
    rp, ci = ref.dead_end_graph()
    walks, eids = ref.random_walks(rp, ci, ref.root_sets()[1000], 4, 7)
    taken = eids[eids >= 0]
    assert ((ci[taken] >= 0) & (ci[taken] < ref.N)).all()
    assert ((walks >= -1) & (walks < ref.N)).all()
    full, _ = ref.random_walks(*ref.shared_graph(), ref.root_sets()[1000], 4, 7)
    assert not (full == walks).all()                                                # some draw did hit a dead end


def test_the_step_rule_is_uniform():
    rows, d, L = 2000, 40, 10
    rp, ci = np.arange(rows + 1) * d, np.arange(rows * d) % rows
    _, eids = ref.random_walks(rp, ci, np.arange(rows), L, 2024)
    counts = np.bincount((eids % d).ravel(), minlength=d)
    sd = np.sqrt(rows * L * (1 / d) * (1 - 1 / d))
    worst = np.abs(counts - 500).max() / sd
    print("largest deviation: %.2f standard deviations" % worst)
    assert counts.sum() == rows * L and worst <= 5


def test_subgraph_restatement_is_self_consistent():
    rp, ci = ref.shared_graph()
    everything = ref.induced_subgraph(rp, ci, ref.id_lists()["all"], partSize=32)
    assert (everything["nodes"] == np.arange(ref.N)).all() and (everything["new_id"] == np.arange(ref.N)).all()
    assert (everything["row_pointers"] == rp).all() and (everything["column_index"] == ci).all()
    assert (everything["edge_ids"] == np.arange(len(ci))).all()
    pp, p2n = _lib.build_part(32, torch.from_numpy(rp))
    assert (everything["partPtr"] == pp.numpy()).all() and (everything["part2Node"] == p2n.numpy()).all()
    sub = ref.induced_subgraph(rp, ci, ref.id_lists()["1000"])
    S, e = sub["nodes"], sub["edge_ids"]
    assert (np.diff(S) > 0).all() and set(S) == set(ref.id_lists()["1000"]) - {-1}
    rows = np.repeat(np.arange(len(S)), np.diff(sub["row_pointers"]))
    assert (S[sub["column_index"]] == ci[e]).all() and (e >= rp[S[rows]]).all() and (e < rp[S[rows] + 1]).all()
    assert (np.diff(e)[np.diff(rows) == 0] > 0).all()                               # increasing position inside a row
    kept = np.isin(ci, S) & np.isin(np.repeat(np.arange(ref.N), np.diff(rp)), S)
    assert (np.flatnonzero(kept) == e).all()                                        # the edge-parallel statement of the same cut
    hub = ref.induced_subgraph(rp, ci, ref.id_lists()["hub"])
    assert hub["row_pointers"].tolist() == [0, int((ci[rp[10]:rp[11]] == 10).sum())] and hub["row_pointers"][1] >= 1
    empty = ref.induced_subgraph(rp, ci, ref.id_lists()["empty"], partSize=1)
    assert empty["row_pointers"].tolist() == [0] and empty["partPtr"].tolist() == [0] and (empty["new_id"] == -1).all()


def test_subgraph_restatement_names_the_first_bad_id_and_drops_bad_columns():
    rp, ci = ref.shared_graph()
    with pytest.raises(ValueError, match=r"nodes\[2\]"):
        ref.induced_subgraph(rp, ci, [5, -1, ref.N, -2])
    with pytest.raises(ValueError, match=r"nodes\[1\]"):
        ref.induced_subgraph(rp, ci, [5, -2])
    rp2, ci2 = ref.dead_end_graph()
    sub = ref.induced_subgraph(rp2, ci2, np.arange(ref.N))
    good = (ci2 >= 0) & (ci2 < ref.N)
    assert (sub["edge_ids"] == np.flatnonzero(good)).all()
    rp3 = rp.copy()
    rp3[8] = rp3[9] + 5                                       # row 7's pointers leave order: rows 7 (ends past 8's start) and 8 (decreases)
    sub = ref.induced_subgraph(rp3, ci, np.arange(ref.N))
    assert np.diff(sub["row_pointers"])[8] == 0


# ---- the header ----

def test_the_header_is_extern_c_and_the_module_includes_it():
    assert 'extern "C"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "gnna_walk.h"' in open(os.path.join(CSRC, "gnna_torch.cpp")).read()


RULE_SENTENCES = [
    "walks[w, 0] = roots[w].",
    "Step t of walk w stands at v = walks[w, t] with candidate positions [lo, hi) = [rp[v], rp[v+1]) and d = hi - lo.",
    "A row whose pointers decrease, or leave [0, nnz], has d = 0.",
    "If d = 0, the walk stays: walks[w, t+1] = v and edge_ids[w, t] = -1.",
    "u = w * walk_length + t",
    "z = rng_seed + 0x9E3779B97F4A7C15 * (u + 1)",
    "z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9",
    "z = (z ^ (z >> 27)) * 0x94D049BB133111EB",
    "key = z ^ (z >> 31)",
    "j = floor(key * d / 2^64)",
    "__umul64hi(key, d)",
    "e = lo + j and c = column_index[e]",
    "If c is outside [0, num_nodes), the edge is a dead end and is never followed: the walk stays and the edge id is -1.",
    "Else walks[w, t+1] = c and edge_ids[w, t] = e.",
    "A root outside [0, num_nodes) gives a row of -1 in both outputs.",
    "The result is a function of (rng_seed, w, t) and the graph only.",
    "There are no atomics.",
    "walk_length = 0 and num_roots = 0 are fine.",
    "num_roots * (walk_length + 1) < 2^31",
    "A nodes entry of -1 is skipped silently.",
    "sub_nodes = S.",
    "new_id[v] = rank of v in S, or -1.",
    "Column ids outside [0, num_nodes) are dropped.",
    "Duplicate edges and self loops are kept.",
    "A row whose pointers decrease or leave [0, nnz] is empty.",
    "counts = (|S|, nnz', num_parts).",
    "Nothing is written beyond a capacity.",
    "returns GNNA_ERR_UNSUPPORTED inside a capture.",
    "No atomic hands out a position, so the result is the same bits on every run.",
]


def test_the_header_states_the_constants_and_the_rules():
    text = " ".join(open(os.path.join(ROOT, "include", HEADER)).read().replace("\n *", " ").split())
    missing = [s for s in RULE_SENTENCES if s not in text]
    assert not missing, missing
    assert "INCREASING GLOBAL ID" in text and "IN INCREASING e" in text
    # the constants are those of gnna.h's sampling rule
    public = open(os.path.join(ROOT, "include", "gnna.h")).read()
    for constant in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert constant in public and constant in text


# ---- the argument checks: every call returns before it touches the device ----

_I = (ctypes.c_int32 * 64)()
I = ctypes.cast(_I, ctypes.c_void_p).value
_COUNTS = (ctypes.c_int64 * 3)()
INVALID, UNSUPPORTED = -1, -3


def _walk(**kw):
    a = dict(rp=I, ci=I, n=4, nnz=8, roots=I, R=2, L=3, seed=1, walks=I, eid=None)
    a.update(kw)
    return _lib.load().gnna_random_walk_i32(a["rp"], a["ci"], a["n"], a["nnz"], a["roots"], a["R"], a["L"], a["seed"], a["walks"],
                                            a["eid"], None)


def _cut(**kw):
    a = dict(rp=I, ci=I, n=4, nnz=8, nodes=I, K=2, partSize=0, sub=I, new_id=None, sub_rp=I, sub_ci=I, eid=None, pp=None, p2n=None,
             ncap=2, ecap=8, counts=_COUNTS)
    a.update(kw)
    return _lib.load().gnna_induced_subgraph_i32(a["rp"], a["ci"], a["n"], a["nnz"], a["nodes"], a["K"], a["partSize"], a["sub"],
                                                 a["new_id"], a["sub_rp"], a["sub_ci"], a["eid"], a["pp"], a["p2n"], a["ncap"],
                                                 a["ecap"], a["counts"], None)


@pytest.mark.parametrize("call, change, code, message", [
    (_walk, dict(R=-1), INVALID, "negative size"),
    (_walk, dict(L=-1), INVALID, "negative size"),
    (_walk, dict(nnz=-1), INVALID, "negative size"),
    (_walk, dict(roots=None), INVALID, "null pointer"),
    (_walk, dict(walks=None), INVALID, "null pointer"),
    (_walk, dict(ci=None), INVALID, "null pointer"),
    (_walk, dict(R=1 << 29, L=3), UNSUPPORTED, r"num_roots \* \(walk_length \+ 1\) must stay below 2\^31"),
    (_cut, dict(K=-1), INVALID, "negative size"),
    (_cut, dict(ecap=-1), INVALID, "negative size"),
    (_cut, dict(nodes=None), INVALID, "null pointer"),
    (_cut, dict(sub_rp=None), INVALID, "null pointer"),
    (_cut, dict(sub_ci=None), INVALID, "null pointer"),
    (_cut, dict(counts=None), INVALID, "null pointer"),
    (_cut, dict(p2n=I), INVALID, "partPtr and part2Node come together"),
    (_cut, dict(pp=I, p2n=I, partSize=0), INVALID, "partSize must be positive"),
])
def test_what_the_entries_refuse_before_any_device_work(call, change, code, message):
    assert call(**change) == code
    text = _lib.load().gnna_last_error().decode()
    assert re.search(message, text) and text.startswith("gnna_random_walk_i32" if call is _walk else "gnna_induced_subgraph_i32")


def test_a_walk_call_without_roots_returns_at_once():
    assert _walk(R=0, roots=None, walks=None) == 0


def test_the_bindings_refuse_host_tensors():
    rp, ci = (torch.from_numpy(a) for a in ref.shared_graph())
    ids = torch.tensor([1, 2], dtype=torch.int32)
    with pytest.raises(_lib.GnnaError, match="row_pointers must be a device tensor"):
        _lib.random_walk(rp, ci, ids, 2, 1)
    with pytest.raises(_lib.GnnaError, match="row_pointers must be a device tensor"):
        _lib.induced_subgraph(rp, ci, ids)
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    with pytest.raises(RuntimeError, match="row_pointers must be a CUDA tensor"):
        GNNA.random_walk(rp, ci, ids, 2, 1)
    with pytest.raises(RuntimeError, match="row_pointers must be a CUDA tensor"):
        GNNA.induced_subgraph(rp, ci, ids)


# ---- the driver ----

def test_driver_parses_the_saint_flags():
    args = driver.build_parser().parse_args([])
    assert args.saint_roots is None and args.walk_length is None and args.saint_steps == 8 and args.saint_coverage == 0
    args = driver.build_parser().parse_args(["--saint_roots", "2000", "--walk_length", "2", "--saint_steps", "3", "--saint_coverage", "4"])
    assert (args.saint_roots, args.walk_length, args.saint_steps, args.saint_coverage) == (2000, 2, 3, 4)


SAINT = ["--saint_roots", "64", "--walk_length", "2", "--synthetic", "no-such-config"]


@pytest.mark.parametrize("extra, message", [
    (["--model", "sage", "--fanout", "5,5"], "--saint_roots does not go with --fanout"),
    (["--hip_graph", "True"], "--saint_roots does not support --hip_graph True"),
    (["--single_spmm", "True"], "--saint_roots does not go with --single_spmm / --verify_spmm"),
    (["--verify_spmm", "True"], "--saint_roots does not go with --single_spmm / --verify_spmm"),
    (["--dtype", "bfloat16"], "--saint_roots: the subgraph steps are float32 only"),
    (["--model", "rgcn"], "--saint_roots trains on induced subgraphs, which --model rgcn"),
])
def test_driver_refuses_what_saint_cannot_run(extra, message):
    with pytest.raises(SystemExit, match=message):
        driver.main(SAINT + extra)


@pytest.mark.parametrize("argv, message", [
    (["--saint_roots", "64"], "--saint_roots and --walk_length come together"),
    (["--walk_length", "2"], "--saint_roots and --walk_length come together"),
    (["--saint_roots", "0", "--walk_length", "2"], "--saint_roots must be >= 1"),
    (["--saint_roots", "4", "--walk_length", "-1"], "--walk_length must be >= 0"),
    (["--saint_roots", "4", "--walk_length", "2", "--saint_steps", "0"], "--saint_steps must be >= 1"),
    (["--saint_roots", "4", "--walk_length", "2", "--saint_coverage", "-1"], "--saint_coverage must be >= 0"),
    (["--saint_steps", "3"], "--saint_steps and --saint_coverage belong to --saint_roots"),
])
def test_driver_checks_the_saint_values(argv, message):
    with pytest.raises(SystemExit, match=message):
        driver.main(argv + ["--synthetic", "no-such-config"])

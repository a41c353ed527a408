"""Fused GAT attention with a per-edge score term, the parts that need no GPU (the binding surface of include/gnna_gat_edge.h and
the build lists are pinned by test_binding_table_host.py): what the header states, the refusals the three entries make before any
device work, the wrappers, the layer's arguments and errors and the driver's flag."""
import ctypes
import inspect
import os
import re

import pytest

from gnnadvisor_osdi21_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gnna_gat_edge.h")).read()


def test_the_header_states_the_function_and_the_rules():
    flat = re.sub(r"[\s*]+", " ", _header())
    for piece in ("z[e,h] = el[i,h] + er[j,h] + ee[e,h]", "lse[i,h] = logsumexp over the edges of row i of leaky_relu(z)",
                  "(0 for a row without edges)", "alpha[e,h] = exp(leaky_relu(z) - lse[i,h])", "out[i,h,:] = sum_e alpha k H[j,h,:]",
                  "c[i,h] = <dY[i,h,:], Y[i,h,:]>", "dalpha = <dY[i,h,:], H[j,h,:]>",
                  "dz[e,h] = alpha (k dalpha - c) (z > 0 ? 1 : negative_slope)", "d_ee[e,h] = dz[e,h]",
                  "dH[j,h,:] = sum over the edges from source j of alpha k dY[i,h,:]", "[num_edges, heads] fp32, contiguous, edge-major",
                  "t_edge_pos [num_edges]", "the `perm` of gnna_transpose_csr_i32", "the reverse-edge map of gnna_reverse_edges_i32",
                  "outside [0, num_edges): it is never read through", "A skipped edge's d_ee row and alpha row are 0",
                  "Every element of every output is written", "one writer per element", "num_edges >= 0", "ee may be NULL",
                  "GNNA_ACCUMULATE refused for every gradient, d_ee included"):
        assert piece in flat, piece


_B = [(ctypes.c_float * 64)() for _ in range(12)]
_I = (ctypes.c_int32 * 64)()
_J = (ctypes.c_int32 * 64)()
F = [ctypes.cast(b, ctypes.c_void_p).value for b in _B]
I = ctypes.cast(_I, ctypes.c_void_p).value
J = ctypes.cast(_J, ctypes.c_void_p).value


def _forward(attn_drop=0.5, **kw):
    """Host buffers stand in for device memory: every call made here returns before it touches the device."""
    a = dict(h=F[0], el=F[1], er=F[2], ee=F[9], out=F[3], lse=F[4], ld_h=8, ld_out=8, n_out=2, n_in=2, E=3, heads=2, dim=4, P=1, ps=32,
             flags=0, rp=I)
    a.update(kw)
    return _lib.load().gnna_gat_edge_forward_f32(a["h"], a["ld_h"], a["el"], a["er"], a["ee"], a["rp"], I, I, I, 0.2, attn_drop, 7, a["out"],
                                                 a["ld_out"], a["lse"], a["n_out"], a["n_in"], a["E"], a["heads"], a["dim"], a["P"],
                                                 a["ps"], a["flags"], None)


def _backward(attn_drop=0.5, **kw):
    a = dict(h=F[0], el=F[1], er=F[2], ee=F[9], lse=F[4], y=F[3], dy=F[5], dh=F[6], d_el=F[7], d_er=F[8], d_ee=F[10], tpos=J, ld_h=8,
             ld_y=8, ld_dy=8, ld_dh=8, n_out=2, n_in=2, E=3, heads=2, dim=4, P=1, tP=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_gat_edge_backward_f32(a["h"], a["ld_h"], a["el"], a["er"], a["ee"], a["lse"], a["y"], a["ld_y"], a["dy"],
                                                  a["ld_dy"], I, I, I, I, a["P"], I, I, I, I, a["tP"], a["tpos"], 0.2, attn_drop, 7,
                                                  a["dh"], a["ld_dh"], a["d_el"], a["d_er"], a["d_ee"], a["n_out"], a["n_in"], a["E"],
                                                  a["heads"], a["dim"], a["ps"], a["flags"], None)


def _alpha(**kw):
    a = dict(el=F[1], er=F[2], ee=F[9], lse=F[4], rp=I, ci=I, alpha=F[11], n_out=2, n_in=2, E=3, heads=2)
    a.update(kw)
    return _lib.load().gnna_gat_alpha_f32(a["el"], a["er"], a["ee"], a["lse"], a["rp"], a["ci"], 0.2, a["alpha"], a["n_out"], a["n_in"],
                                          a["E"], a["heads"], None)


def _last():
    return _lib.load().gnna_last_error().decode()


@pytest.mark.parametrize("call, name", [(_forward, "gnna_gat_edge_forward_f32"), (_backward, "gnna_gat_edge_backward_f32")])
def test_refusals_both_entries_make_before_any_device_work(call, name):
    for bad, shown in ((-0.1, "-0.1"), (1.0, "1"), (float("nan"), "nan"), (1.5, "1.5")):
        assert call(bad) == -1
        assert _last().startswith(f"{name}: attn_drop must be in [0, 1) (got ") and shown in _last().lower()
    # the drop entries' refusals under the entry's own name
    assert call(heads=65) == -3 and _last() == f"{name}: at most 64 heads (got 65)"
    assert call(heads=0) == -1 and _last() == f"{name}: bad size (num_out_rows=2 num_in_rows=2 heads=0 dim=4 num_parts=1)"
    assert call(n_in=-1) == -1 and _last().startswith(f"{name}: bad size (num_out_rows=2 num_in_rows=-1 ")
    assert call(dim=257) == -3 and _last() == f"{name}: at most 256 floats per head (got 257)"
    assert call(ps=0) == -1 and _last() == f"{name}: partSize must be positive (got 0)"
    assert call(n_out=1 << 29) == -3 and _last() == f"{name}: 536870912 rows in one call (at most 536870911): shard the rows"
    assert call(flags=1) == -3 and _last() == f"{name}: GNNA_ACCUMULATE is not supported"
    assert call(flags=8) == -1 and _last() == f"{name}: unknown flag bits 0x8"
    assert call(ld_h=7) == -1 and "ld_h=7" in _last()
    for kw in (dict(h=None), dict(el=None), dict(er=None)):
        assert call(**kw) == -1 and _last() == f"{name}: null pointer", kw
    # new with these entries: the edge count and what it sizes
    assert call(E=-1) == -1 and _last() == f"{name}: bad size (num_edges=-1)"
    assert call(E=1 << 31) == -3 and _last() == f"{name}: 2147483648 edges in one call (at most 2147483647)"
    assert call(ee=None) == -1 and _last().startswith(f"{name}: null edge pointer (")
    assert call(2.0, E=-1) == -1 and "attn_drop" in _last()                   # (attn_drop is looked at first, as in the drop entries)
    try:
        _lib.set_tuning(deterministic=1)
        assert call() == -3
        assert _last() == f"{name} has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"
    finally:
        _lib.reset_tuning()


def test_refusals_of_the_forward():
    name = "gnna_gat_edge_forward_f32"
    assert _forward(flags=4) == -1 and _last() == f"{name}: unknown flag bits 0x4"
    assert _forward(ld_out=7) == -1 and "ld_out=7" in _last()
    for kw in (dict(out=None), dict(lse=None), dict(rp=None)):
        assert _forward(**kw) == -1 and _last() == f"{name}: null pointer", kw
    alias = f"{name}: an output must not alias an input or the other output"
    for kw in (dict(out=F[0]), dict(out=F[1]), dict(out=F[2]), dict(out=F[4]), dict(lse=F[0]), dict(lse=F[1]), dict(lse=F[2]),
               dict(out=F[9]), dict(lse=F[9])):                                  # (F[9]: ee)
        assert _forward(**kw) == -1 and _last() == alias, kw
    assert _forward(n_out=0, out=None, lse=None) == 0                          # no destination row: nothing to write
    assert _forward(n_out=0, out=None, lse=None, E=-1) == -1
    assert _forward(E=0, ee=None, out=None) == -1 and _last() == f"{name}: null pointer"    # ee may be null without edges; out not


def test_refusals_of_the_backward():
    name = "gnna_gat_edge_backward_f32"
    assert _backward(flags=2) == -1 and _last() == f"{name}: unknown flag bits 0x2"
    assert _backward(tP=-1) == -1 and _last() == f"{name}: bad size (t_num_parts=-1)"
    for kw in (dict(ld_y=7), dict(ld_dy=7), dict(ld_dh=7)):
        assert _backward(**kw) == -1 and f"{list(kw)[0]}=7" in _last(), kw
    for kw in (dict(lse=None), dict(y=None), dict(dy=None), dict(dh=None), dict(d_el=None), dict(d_er=None)):
        assert _backward(**kw) == -1 and _last() == f"{name}: null pointer", kw
    for kw in (dict(d_ee=None), dict(tpos=None), dict(ee=None)):
        assert _backward(**kw) == -1 and _last() == f"{name}: null edge pointer (ee, d_ee, t_edge_pos with num_edges > 0)", kw
    for out in ("dh", "d_el", "d_er", "d_ee"):
        for inp in (0, 1, 2, 3, 4, 5, 9):                                       # H, el, er, Y, lse, dY, ee
            assert _backward(**{out: F[inp]}) == -1 and _last() == f"{name}: an output must not alias an input", (out, inp)
    assert _backward(d_ee=J) == -1 and _last() == f"{name}: an output must not alias an input"          # t_edge_pos
    for kw in (dict(dh=F[7]), dict(dh=F[8]), dict(d_el=F[8]), dict(d_ee=F[6]), dict(d_ee=F[7]), dict(d_ee=F[8])):
        assert _backward(**kw) == -1 and _last() == f"{name}: the outputs must not alias each other", kw


def test_refusals_of_alpha():
    name = "gnna_gat_alpha_f32"
    assert _alpha(E=-1) == -1 and _last() == f"{name}: bad size (num_out_rows=2 num_in_rows=2 num_edges=-1 heads=2)"
    assert _alpha(heads=0) == -1 and _last().startswith(f"{name}: bad size (")
    assert _alpha(n_out=-1) == -1 and _last().startswith(f"{name}: bad size (")
    assert _alpha(heads=65) == -3 and _last() == f"{name}: at most 64 heads (got 65)"
    assert _alpha(n_in=1 << 29) == -3 and "shard the rows" in _last()
    assert _alpha(E=1 << 31) == -3 and "edges in one call" in _last()
    for kw in (dict(alpha=None), dict(el=None), dict(er=None), dict(lse=None), dict(rp=None), dict(ci=None)):
        assert _alpha(**kw) == -1 and _last() == f"{name}: null pointer", kw
    for inp in (1, 2, 4, 9):
        assert _alpha(alpha=F[inp]) == -1 and _last() == f"{name}: an output must not alias an input", inp
    assert _alpha(E=0, alpha=None) == 0                                         # nothing to write


def test_the_wrappers():
    fwd = list(inspect.signature(_lib.gat_edge_forward).parameters)
    bwd = inspect.signature(_lib.gat_edge_backward).parameters
    alpha = inspect.signature(_lib.gat_alpha).parameters
    assert fwd[:12] == ["H", "el", "er", "ee", "row_pointers", "column_index", "part_pointers", "part2Node", "partSize",
                        "negative_slope", "attn_drop", "rng_seed"]
    assert list(bwd)[:16] == ["H", "el", "er", "ee", "lse", "Y", "dY", "row_pointers", "column_index", "part_pointers", "part2Node",
                              "t_edge_pos", "partSize", "negative_slope", "attn_drop", "rng_seed"] and bwd["transposed"].default is None
    assert list(alpha)[:7] == ["el", "er", "ee", "lse", "row_pointers", "column_index", "negative_slope"]
    from gnnadvisor_osdi21_amd import load_extension
    GNNA = load_extension()
    assert "gnna_gat_edge.h" in GNNA.gat_edge_forward.__doc__ and "(dH, d_el, d_er, d_ee)" in GNNA.gat_edge_backward.__doc__
    assert "gnna_gat_edge.h" in GNNA.gat_alpha.__doc__


def test_driver_flag():
    from gnnadvisor_osdi21_amd import main as driver
    p = driver.build_parser()
    assert p.parse_args(["--model", "gat"]).edge_dim == 0
    args = p.parse_args(["--model", "gat", "--fused_attention", "True", "--edge_dim", "8", "--fanout", "5,5"])
    assert (args.model, args.edge_dim, args.fanout) == ("gat", 8, "5,5")
    assert "GATConv(edge_dim=D)" in p.format_help()


@pytest.mark.parametrize("extra, message", [
    (["--model", "gcn", "--edge_dim", "8"], "--edge_dim puts edge features into the GAT score: run it with --model gat \\(got --model gcn\\)"),
    (["--model", "gatv2", "--edge_dim", "8"], "run it with --model gat \\(got --model gatv2\\)"),
    (["--model", "transformer", "--edge_dim", "8"], "run it with --model gat \\(got --model transformer\\)"),
    (["--model", "gat", "--edge_dim", "-1"], "--edge_dim must be >= 0"),
    (["--model", "gat", "--edge_dim", "8", "--dtype", "bfloat16"], "run --model gat with --dtype float32"),
    (["--model", "gat", "--edge_dim", "8", "--hip_graph", "True"], "--model gat does not support --hip_graph True"),
    (["--model", "gat", "--edge_dim", "8", "--fanout", "5,5"], "--model gat --fanout runs on the fused attention kernels only"),
])
def test_driver_refusals(extra, message):
    from gnnadvisor_osdi21_amd import main as driver
    with pytest.raises(SystemExit, match=message):
        driver.main(["--synthetic", "no-such-config"] + extra)


def test_the_layer_and_its_argument_errors():
    import types

    import torch
    from gnnadvisor_osdi21_amd import ops
    sig = inspect.signature(ops.GATConv.__init__)
    assert list(sig.parameters) == ["self", "input_dim", "output_dim", "heads", "concat", "negative_slope", "fused", "attn_drop", "edge_dim"]
    assert sig.parameters["edge_dim"].default is None
    fwd = inspect.signature(ops.GATConv.forward).parameters
    assert list(fwd) == ["self", "X", "inputInfo", "rng_seed", "edge_attr", "return_attention_weights"]
    assert fwd["edge_attr"].default is None and fwd["return_attention_weights"].default is False
    conv = ops.GATConv(6, 5, heads=3, fused=True, edge_dim=4)
    assert {n: tuple(q.shape) for n, q in conv.named_parameters()} == {"weights": (6, 15), "att_l": (3, 5), "att_r": (3, 5),
                                                                      "weights_edge": (4, 15), "att_e": (3, 5)}
    assert all(float(q.detach().abs().max()) <= 1 / 5 ** 0.5 for q in conv.parameters())
    plain = ops.GATConv(6, 5, heads=3)
    assert [n for n, _ in plain.named_parameters()] == ["weights", "att_l", "att_r"] and plain.edge_dim is None
    with pytest.raises(ValueError, match="edge_dim must be positive"):
        ops.GATConv(6, 5, edge_dim=0)
    info = types.SimpleNamespace(column_index=torch.zeros(7, dtype=torch.int32))
    X = torch.zeros(3, 6)
    with pytest.raises(ValueError, match="forward needs edge_attr \\[nnz, 4\\]"):
        conv(X, info)
    with pytest.raises(ValueError, match="edge_attr given to a layer built without edge_dim"):
        plain(X, info, edge_attr=torch.zeros(7, 4))
    for bad in (torch.zeros(6, 4), torch.zeros(7, 3), torch.zeros(7)):
        with pytest.raises(ValueError, match="edge_attr must be \\[nnz = 7, edge_dim = 4\\]"):
            conv(X, info, edge_attr=bad)
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 only: 16-bit features and torch.autocast are not supported"):
            conv(X, info, edge_attr=torch.zeros(7, 4, dtype=dtype))
        with pytest.raises(TypeError, match="float32 only: 16-bit features and torch.autocast are not supported"):
            conv(X.to(dtype), info, edge_attr=torch.zeros(7, 4))
    # the Function: its arguments, and the errors it raises before it calls the library
    fn = list(inspect.signature(ops.GATEdgeAttention.forward).parameters)
    assert fn == ["ctx", "H", "el", "er", "ee", "inputInfo", "negative_slope", "attn_drop", "rng_seed"]
    d = inspect.signature(ops.GATEdgeAttention.forward).parameters
    assert d["attn_drop"].default == 0.0 and d["rng_seed"].default == 0
    assert list(inspect.signature(ops.GATAttention.forward).parameters) == ["ctx", "H", "el", "er", "inputInfo", "negative_slope",
                                                                            "attn_drop", "rng_seed"]
    H, s = torch.zeros(3, 8), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="attn_drop must be in \\[0, 1\\)"):
        ops.GATEdgeAttention.apply(H, s, s, torch.zeros(7, 2), info, 0.2, 1.0, 0)
    with pytest.raises(ValueError, match="ee must be \\[nnz = 7, heads = 2\\]"):
        ops.GATEdgeAttention.apply(H, s, s, torch.zeros(6, 2), info, 0.2)
    with pytest.raises(TypeError, match="float32 only"):
        ops.GATEdgeAttention.apply(H, s, s, torch.zeros(7, 2, dtype=torch.float64), info, 0.2)


def test_a_block_transpose_has_a_lazy_perm():
    from gnnadvisor_osdi21_amd import sampling
    assert isinstance(sampling._BlockTranspose.perm, property)
    src = inspect.getsource(sampling._BlockTranspose.__init__)
    assert "want_perm=False" in src                       # the transpose itself is still built without it

"""The argument errors of the 16-bit, reduce, GAT and typed entries, pinned (no GPU): the return code and the whole text of
gnna_last_error() for every refusal these entries make before they touch the device.  The pairs were recorded from the library
before its launchers were rewritten on shared helpers; the text is part of what a caller sees, so it is compared as a whole."""
import ctypes

import pytest

from gnnadvisor_osdi21_amd import _lib

ACCUMULATE, UNKNOWN_BIT = 1, 0x80
ROWS_2_29 = 1 << 29

# Host buffers stand in for device memory: every call below must return before it touches the device or its arguments' contents.
_B = [(ctypes.c_float * 64)() for _ in range(9)]
_I = (ctypes.c_int32 * 64)()


def _p(buf):
    return ctypes.cast(buf, ctypes.c_void_p).value


F = [_p(b) for b in _B]
I = _p(_I)


def _expand(**kw):
    a = dict(X=F[0], ld_x=4, n_in=2, col=I, ety=I, enorm=None, coef=F[1], R=3, B=2, pp=I, p2n=I, out=F[2], ld_out=8, n_out=2,
             dim=4, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_typed_expand_ld_f32(a["X"], a["ld_x"], a["n_in"], a["col"], a["ety"], a["enorm"], a["coef"], a["R"],
                                                    a["B"], a["pp"], a["p2n"], a["out"], a["ld_out"], a["n_out"], a["dim"], a["P"],
                                                    a["ps"], a["flags"], None)


def _contract(**kw):
    a = dict(G=F[0], ld_g=8, n_in=2, col=I, ety=I, enorm=None, coef=F[1], R=3, B=2, pp=I, p2n=I, out=F[2], ld_out=4, n_out=2,
             dim=4, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_typed_contract_ld_f32(a["G"], a["ld_g"], a["n_in"], a["col"], a["ety"], a["enorm"], a["coef"], a["R"],
                                                      a["B"], a["pp"], a["p2n"], a["out"], a["ld_out"], a["n_out"], a["dim"], a["P"],
                                                      a["ps"], a["flags"], None)


def _coef_grad(**kw):
    a = dict(X=F[0], ld_x=4, n_in=2, G=F[1], ld_g=8, n_out=2, col=I, ety=I, enorm=None, pp=I, p2n=I, dcoef=F[2], R=3, B=2, dim=4,
             P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_typed_coef_grad_ld_f32(a["X"], a["ld_x"], a["n_in"], a["G"], a["ld_g"], a["n_out"], a["col"], a["ety"],
                                                   a["enorm"], a["pp"], a["p2n"], a["dcoef"], a["R"], a["B"], a["dim"], a["P"],
                                                   a["ps"], a["flags"], None)


def _gat_fwd(rect):
    def call(**kw):
        a = dict(H=F[0], ld_h=8, el=F[1], er=F[2], rp=I, col=I, pp=I, p2n=I, slope=0.2, out=F[3], ld_out=8, lse=F[4], n_out=2,
                 n_in=2, heads=2, dim=4, P=1, ps=32, flags=0)
        a.update(kw)
        head = (a["H"], a["ld_h"], a["el"], a["er"], a["rp"], a["col"], a["pp"], a["p2n"], a["slope"], a["out"], a["ld_out"], a["lse"])
        tail = (a["heads"], a["dim"], a["P"], a["ps"], a["flags"], None)
        if rect:
            return _lib.load().gnna_gat_forward_rect_f32(*head, a["n_out"], a["n_in"], *tail)
        return _lib.load().gnna_gat_forward_f32(*head, a["n_out"], *tail)
    return call


def _gat_bwd(kind):
    def call(**kw):
        a = dict(H=F[0], ld_h=8, el=F[1], er=F[2], lse=F[3], Y=F[4], ld_y=8, dY=F[5], ld_dy=8, rp=I, col=I, pp=I, p2n=I, P=1,
                 slope=0.2, dH=F[6], ld_dh=8, d_el=F[7], d_er=F[8], n_out=2, n_in=2, heads=2, dim=4, ps=32, flags=0)
        a.update(kw)
        head = (a["H"], a["ld_h"], a["el"], a["er"], a["lse"], a["Y"], a["ld_y"], a["dY"], a["ld_dy"])
        struct = (a["rp"], a["col"], a["pp"], a["p2n"])
        outs = (a["slope"], a["dH"], a["ld_dh"], a["d_el"], a["d_er"])
        if kind == "sym":
            return _lib.load().gnna_gat_backward_f32(*head, *struct, *outs, a["n_out"], a["heads"], a["dim"], a["P"], a["ps"],
                                                     a["flags"], None)
        both = (*head, *struct, a["P"], *struct, a["P"], *outs)
        if kind == "dir":
            return _lib.load().gnna_gat_backward_dir_f32(*both, a["n_out"], a["heads"], a["dim"], a["ps"], a["flags"], None)
        return _lib.load().gnna_gat_backward_rect_f32(*both, a["n_out"], a["n_in"], a["heads"], a["dim"], a["ps"], a["flags"], None)
    return call


def _reduce(**kw):
    a = dict(op=0, X=F[0], ld_in=4, n_in=2, col=I, pp=I, p2n=I, out=F[1], ld_out=4, arg=I, ld_arg=4, n_out=2, dim=4, P=1, ps=32,
             flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_reduce_ld_f32(a["op"], a["X"], a["ld_in"], a["n_in"], a["col"], a["pp"], a["p2n"], a["out"],
                                              a["ld_out"], a["arg"], a["ld_arg"], a["n_out"], a["dim"], a["P"], a["ps"], a["flags"],
                                              None)


def _scatter(**kw):
    a = dict(go=F[0], ld_go=4, arg=I, ld_arg=4, col=I, n_out=2, gi=F[1], ld_gi=4, n_in=2, dim=4, flags=0)
    a.update(kw)
    return _lib.load().gnna_scatter_arg_ld_f32(a["go"], a["ld_go"], a["arg"], a["ld_arg"], a["col"], a["n_out"], a["gi"], a["ld_gi"],
                                               a["n_in"], a["dim"], a["flags"], None)


def _x16(**kw):
    # mode 0 = SAG, type 1 = bf16 in and out (an fp32 output, type 0, may be accumulated into)
    a = dict(mode=0, in_type=1, X=F[0], ld_in=8, n_in=2, col=I, deg_out=None, deg_in=None, eps=0.0, pp=I, p2n=I, out=F[1],
             out_type=1, ld_out=8, n_out=2, dim=8, P=1, ps=32, flags=0)
    a.update(kw)
    return _lib.load().gnna_agg_ld_x16(a["mode"], a["in_type"], a["X"], a["ld_in"], a["n_in"], a["col"], a["deg_out"], a["deg_in"],
                                       a["eps"], a["pp"], a["p2n"], a["out"], a["out_type"], a["ld_out"], a["n_out"], a["dim"],
                                       a["P"], a["ps"], a["flags"], None)


ENTRIES = {
    "expand": _expand, "contract": _contract, "coef_grad": _coef_grad,
    "gat_fwd": _gat_fwd(False), "gat_fwd_rect": _gat_fwd(True),
    "gat_bwd": _gat_bwd("sym"), "gat_bwd_dir": _gat_bwd("dir"), "gat_bwd_rect": _gat_bwd("rect"),
    "reduce": _reduce, "scatter": _scatter, "x16": _x16,
}
DET = "deterministic"     # a case that runs the entry's valid arguments under set_tuning(deterministic=1)

# (entry, what is wrong, arguments that differ from the entry's valid ones, return code, message).  GNNA_ACCUMULATE is a valid flag
# of coef_grad and scatter and of x16 with an fp32 output, so it is refused only where listed; reduce has a deterministic schedule
# of its own kind (one writer per key) and scatter has no partSize.
CASES = [
    ("expand", "stride", dict(ld_x=3), -1,
     "gnna_agg_typed_expand_ld_f32: row strides must be >= dim (X) and >= num_bases * dim (out) and < 2^29 floats (ld_x=3 ld_out=8)"),
    ("expand", "stride_2_29", dict(ld_x=ROWS_2_29), -1,
     "gnna_agg_typed_expand_ld_f32: row strides must be >= dim (X) and >= num_bases * dim (out) and < 2^29 floats (ld_x=536870912 ld_out=8)"),
    ("expand", "size", dict(n_in=-1), -1,
     "gnna_agg_typed_expand_ld_f32: bad size (num_in_rows=-1 num_out_rows=2 num_types=3 num_bases=2 dim=4 num_parts=1)"),
    ("expand", "size_bases", dict(B=17), -3, "gnna_agg_typed_expand_ld_f32: at most 16 bases (got 17)"),
    ("expand", "partsize", dict(ps=0), -1, "gnna_agg_typed_expand_ld_f32: partSize must be positive (got 0)"),
    ("expand", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_agg_typed_expand_ld_f32: GNNA_ACCUMULATE is not supported"),
    ("expand", "unknown_flag", dict(flags=UNKNOWN_BIT), -1,
     "gnna_agg_typed_expand_ld_f32: flag bits 0x80 are not accepted (GNNA_EPILOGUE_RELU among them)"),
    ("expand", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_agg_typed_expand_ld_f32: 536870912 x 2 rows in one call (at most 536870911 each): shard the rows"),
    ("expand", "null", dict(X=None), -1, "gnna_agg_typed_expand_ld_f32: null pointer"),
    ("expand", "null_index", dict(col=None), -1, "gnna_agg_typed_expand_ld_f32: null index pointer"),
    ("expand", "alias", dict(out=F[0]), -1, "gnna_agg_typed_expand_ld_f32: the output must not alias an input"),
    ("expand", "deterministic", DET, -3,
     "gnna_agg_typed_expand_ld_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its sums are added with float atomics"),
    ("contract", "stride", dict(ld_g=7), -1,
     "gnna_agg_typed_contract_ld_f32: row strides must be >= num_bases * dim (G) and >= dim (out) and < 2^29 floats (ld_g=7 ld_out=4)"),
    ("contract", "stride_2_29", dict(ld_g=ROWS_2_29), -1,
     "gnna_agg_typed_contract_ld_f32: row strides must be >= num_bases * dim (G) and >= dim (out) and < 2^29 floats (ld_g=536870912 ld_out=4)"),
    ("contract", "size", dict(n_in=-1), -1,
     "gnna_agg_typed_contract_ld_f32: bad size (num_in_rows=-1 num_out_rows=2 num_types=3 num_bases=2 dim=4 num_parts=1)"),
    ("contract", "size_bases", dict(B=17), -3, "gnna_agg_typed_contract_ld_f32: at most 16 bases (got 17)"),
    ("contract", "partsize", dict(ps=0), -1, "gnna_agg_typed_contract_ld_f32: partSize must be positive (got 0)"),
    ("contract", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_agg_typed_contract_ld_f32: GNNA_ACCUMULATE is not supported"),
    ("contract", "unknown_flag", dict(flags=UNKNOWN_BIT), -1,
     "gnna_agg_typed_contract_ld_f32: flag bits 0x80 are not accepted (GNNA_EPILOGUE_RELU among them)"),
    ("contract", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_agg_typed_contract_ld_f32: 536870912 x 2 rows in one call (at most 536870911 each): shard the rows"),
    ("contract", "null", dict(coef=None), -1, "gnna_agg_typed_contract_ld_f32: null pointer"),
    ("contract", "null_index", dict(col=None), -1, "gnna_agg_typed_contract_ld_f32: null index pointer"),
    ("contract", "alias", dict(out=F[1]), -1, "gnna_agg_typed_contract_ld_f32: the output must not alias an input"),
    ("contract", "deterministic", DET, -3,
     "gnna_agg_typed_contract_ld_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its sums are added with float atomics"),
    ("coef_grad", "stride", dict(ld_g=7), -1,
     "gnna_typed_coef_grad_ld_f32: row strides must be >= dim (X) and >= num_bases * dim (G) and < 2^29 floats (ld_x=4 ld_g=7)"),
    ("coef_grad", "stride_2_29", dict(ld_g=ROWS_2_29), -1,
     "gnna_typed_coef_grad_ld_f32: row strides must be >= dim (X) and >= num_bases * dim (G) and < 2^29 floats (ld_x=4 ld_g=536870912)"),
    ("coef_grad", "size", dict(n_in=-1), -1,
     "gnna_typed_coef_grad_ld_f32: bad size (num_in_rows=-1 num_out_rows=2 num_types=3 num_bases=2 dim=4 num_parts=1)"),
    ("coef_grad", "size_bases", dict(B=17), -3, "gnna_typed_coef_grad_ld_f32: at most 16 bases (got 17)"),
    ("coef_grad", "partsize", dict(ps=0), -1, "gnna_typed_coef_grad_ld_f32: partSize must be positive (got 0)"),
    ("coef_grad", "unknown_flag", dict(flags=UNKNOWN_BIT), -1,
     "gnna_typed_coef_grad_ld_f32: flag bits 0x80 are not accepted (GNNA_EPILOGUE_RELU among them)"),
    ("coef_grad", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_typed_coef_grad_ld_f32: 536870912 x 2 rows in one call (at most 536870911 each): shard the rows"),
    ("coef_grad", "null", dict(dcoef=None), -1, "gnna_typed_coef_grad_ld_f32: null pointer"),
    ("coef_grad", "null_index", dict(col=None), -1, "gnna_typed_coef_grad_ld_f32: null index pointer"),
    ("coef_grad", "alias", dict(dcoef=F[1]), -1, "gnna_typed_coef_grad_ld_f32: the output must not alias an input"),
    ("coef_grad", "deterministic", DET, -3,
     "gnna_typed_coef_grad_ld_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its sums are added with float atomics"),
    ("gat_fwd", "stride", dict(ld_h=7), -1,
     "gnna_gat_forward_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=7 ld_out=8)"),
    ("gat_fwd", "stride_2_29", dict(ld_out=ROWS_2_29), -1,
     "gnna_gat_forward_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_out=536870912)"),
    ("gat_fwd", "size", dict(heads=0), -1, "gnna_gat_forward_f32: bad size (num_nodes=2 heads=0 dim=4 num_parts=1)"),
    ("gat_fwd", "size_dim", dict(dim=257), -3, "gnna_gat_forward_f32: at most 256 floats per head (got 257)"),
    ("gat_fwd", "size_heads", dict(heads=65), -3, "gnna_gat_forward_f32: at most 64 heads (got 65)"),
    ("gat_fwd", "partsize", dict(ps=0), -1, "gnna_gat_forward_f32: partSize must be positive (got 0)"),
    ("gat_fwd", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_gat_forward_f32: GNNA_ACCUMULATE is not supported"),
    ("gat_fwd", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "gnna_gat_forward_f32: unknown flag bits 0x80"),
    ("gat_fwd", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_gat_forward_f32: 536870912 rows in one call (at most 536870911): shard the rows"),
    ("gat_fwd", "null", dict(lse=None), -1, "gnna_gat_forward_f32: null pointer"),
    ("gat_fwd", "null_index", dict(pp=None), -1, "gnna_gat_forward_f32: null index pointer"),
    ("gat_fwd", "alias", dict(out=F[0]), -1, "gnna_gat_forward_f32: an output must not alias an input or the other output"),
    ("gat_fwd", "deterministic", DET, -3,
     "gnna_gat_forward_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"),
    ("gat_fwd_rect", "stride", dict(ld_h=7), -1,
     "gnna_gat_forward_rect_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=7 ld_out=8)"),
    ("gat_fwd_rect", "stride_2_29", dict(ld_out=ROWS_2_29), -1,
     "gnna_gat_forward_rect_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_out=536870912)"),
    ("gat_fwd_rect", "size", dict(heads=0), -1,
     "gnna_gat_forward_rect_f32: bad size (num_out_rows=2 num_in_rows=2 heads=0 dim=4 num_parts=1)"),
    ("gat_fwd_rect", "size_dim", dict(dim=257), -3, "gnna_gat_forward_rect_f32: at most 256 floats per head (got 257)"),
    ("gat_fwd_rect", "size_heads", dict(heads=65), -3, "gnna_gat_forward_rect_f32: at most 64 heads (got 65)"),
    ("gat_fwd_rect", "partsize", dict(ps=0), -1, "gnna_gat_forward_rect_f32: partSize must be positive (got 0)"),
    ("gat_fwd_rect", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_gat_forward_rect_f32: GNNA_ACCUMULATE is not supported"),
    ("gat_fwd_rect", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "gnna_gat_forward_rect_f32: unknown flag bits 0x80"),
    ("gat_fwd_rect", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_gat_forward_rect_f32: 536870912 rows in one call (at most 536870911): shard the rows"),
    ("gat_fwd_rect", "null", dict(lse=None), -1, "gnna_gat_forward_rect_f32: null pointer"),
    ("gat_fwd_rect", "null_index", dict(pp=None), -1, "gnna_gat_forward_rect_f32: null index pointer"),
    ("gat_fwd_rect", "alias", dict(out=F[0]), -1,
     "gnna_gat_forward_rect_f32: an output must not alias an input or the other output"),
    ("gat_fwd_rect", "deterministic", DET, -3,
     "gnna_gat_forward_rect_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"),
    ("gat_bwd", "stride", dict(ld_dy=7), -1,
     "gnna_gat_backward_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_y=8 ld_dy=7 ld_dh=8)"),
    ("gat_bwd", "stride_2_29", dict(ld_dh=ROWS_2_29), -1,
     "gnna_gat_backward_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_y=8 ld_dy=8 ld_dh=536870912)"),
    ("gat_bwd", "size", dict(dim=0), -1, "gnna_gat_backward_f32: bad size (num_nodes=2 heads=2 dim=0 num_parts=1)"),
    ("gat_bwd", "partsize", dict(ps=0), -1, "gnna_gat_backward_f32: partSize must be positive (got 0)"),
    ("gat_bwd", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_gat_backward_f32: GNNA_ACCUMULATE is not supported"),
    ("gat_bwd", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "gnna_gat_backward_f32: unknown flag bits 0x80"),
    ("gat_bwd", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_gat_backward_f32: 536870912 rows in one call (at most 536870911): shard the rows"),
    ("gat_bwd", "null", dict(d_er=None), -1, "gnna_gat_backward_f32: null pointer"),
    ("gat_bwd", "null_index", dict(p2n=None), -1, "gnna_gat_backward_f32: null index pointer"),
    ("gat_bwd", "alias", dict(dH=F[5]), -1, "gnna_gat_backward_f32: an output must not alias an input"),
    ("gat_bwd", "alias_outputs", dict(d_el=F[8]), -1, "gnna_gat_backward_f32: the outputs must not alias each other"),
    ("gat_bwd", "deterministic", DET, -3,
     "gnna_gat_backward_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"),
    ("gat_bwd_dir", "stride", dict(ld_dy=7), -1,
     "gnna_gat_backward_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_y=8 ld_dy=7 ld_dh=8)"),
    ("gat_bwd_dir", "stride_2_29", dict(ld_dh=ROWS_2_29), -1,
     "gnna_gat_backward_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_y=8 ld_dy=8 ld_dh=536870912)"),
    ("gat_bwd_dir", "size", dict(dim=0), -1, "gnna_gat_backward_f32: bad size (num_nodes=2 heads=2 dim=0 num_parts=1)"),
    ("gat_bwd_dir", "partsize", dict(ps=0), -1, "gnna_gat_backward_f32: partSize must be positive (got 0)"),
    ("gat_bwd_dir", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_gat_backward_f32: GNNA_ACCUMULATE is not supported"),
    ("gat_bwd_dir", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "gnna_gat_backward_f32: unknown flag bits 0x80"),
    ("gat_bwd_dir", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_gat_backward_f32: 536870912 rows in one call (at most 536870911): shard the rows"),
    ("gat_bwd_dir", "null", dict(d_er=None), -1, "gnna_gat_backward_f32: null pointer"),
    ("gat_bwd_dir", "null_index", dict(p2n=None), -1, "gnna_gat_backward_f32: null index pointer"),
    ("gat_bwd_dir", "alias", dict(dH=F[5]), -1, "gnna_gat_backward_f32: an output must not alias an input"),
    ("gat_bwd_dir", "alias_outputs", dict(d_el=F[8]), -1, "gnna_gat_backward_f32: the outputs must not alias each other"),
    ("gat_bwd_dir", "deterministic", DET, -3,
     "gnna_gat_backward_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"),
    ("gat_bwd_rect", "stride", dict(ld_dy=7), -1,
     "gnna_gat_backward_rect_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_y=8 ld_dy=7 ld_dh=8)"),
    ("gat_bwd_rect", "stride_2_29", dict(ld_dh=ROWS_2_29), -1,
     "gnna_gat_backward_rect_f32: row strides must be >= heads * dim and < 2^29 floats (ld_h=8 ld_y=8 ld_dy=8 ld_dh=536870912)"),
    ("gat_bwd_rect", "size", dict(dim=0), -1,
     "gnna_gat_backward_rect_f32: bad size (num_out_rows=2 num_in_rows=2 heads=2 dim=0 num_parts=1)"),
    ("gat_bwd_rect", "partsize", dict(ps=0), -1, "gnna_gat_backward_rect_f32: partSize must be positive (got 0)"),
    ("gat_bwd_rect", "accumulate", dict(flags=ACCUMULATE), -3, "gnna_gat_backward_rect_f32: GNNA_ACCUMULATE is not supported"),
    ("gat_bwd_rect", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "gnna_gat_backward_rect_f32: unknown flag bits 0x80"),
    ("gat_bwd_rect", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "gnna_gat_backward_rect_f32: 536870912 rows in one call (at most 536870911): shard the rows"),
    ("gat_bwd_rect", "null", dict(d_er=None), -1, "gnna_gat_backward_rect_f32: null pointer"),
    ("gat_bwd_rect", "null_index", dict(p2n=None), -1, "gnna_gat_backward_rect_f32: null index pointer"),
    ("gat_bwd_rect", "alias", dict(dH=F[5]), -1, "gnna_gat_backward_rect_f32: an output must not alias an input"),
    ("gat_bwd_rect", "alias_outputs", dict(d_el=F[8]), -1, "gnna_gat_backward_rect_f32: the outputs must not alias each other"),
    ("gat_bwd_rect", "deterministic", DET, -3,
     "gnna_gat_backward_rect_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its rows are added with float atomics"),
    ("gat_bwd_rect", "one_side", dict(n_out=0, dH=None), -1,
     "gnna_gat_backward_rect_f32: dH / d_er: null pointer or a row stride outside [heads * dim, 2^29)"),
    ("gat_bwd_rect", "size_t_parts", dict(P=-1), -1,
     "gnna_gat_backward_rect_f32: bad size (num_out_rows=2 num_in_rows=2 heads=2 dim=4 num_parts=-1)"),
    ("reduce", "stride", dict(ld_arg=3), -1,
     "row strides must be >= dim and < 2^29 elements (ld_in=4 ld_out=4 ld_arg=3 dim=4)"),
    ("reduce", "stride_2_29", dict(ld_in=ROWS_2_29), -1,
     "row strides must be >= dim and < 2^29 elements (ld_in=536870912 ld_out=4 ld_arg=4 dim=4)"),
    ("reduce", "size", dict(n_in=-1), -1, "negative size (num_out_rows=2 num_in_rows=-1 num_parts=1)"),
    ("reduce", "size_dim", dict(dim=0), -1, "dim must be >= 1 (got 0)"),
    ("reduce", "op", dict(op=2), -1, "op must be GNNA_REDUCE_MAX or GNNA_REDUCE_MIN (got 2)"),
    ("reduce", "partsize", dict(ps=0), -1, "partSize must be positive (got 0)"),
    ("reduce", "accumulate", dict(flags=ACCUMULATE), -3,
     "gnna_agg_reduce_ld_f32: GNNA_ACCUMULATE has no meaning for a max / min"),
    ("reduce", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "unknown flag bits 0x80"),
    ("reduce", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "536870912 destination rows in one call (at most 536870911): shard the rows"),
    ("reduce", "null", dict(out=None), -1, "null output pointer"),
    ("reduce", "null_input", dict(X=None), -1, "null feature pointer"),
    ("reduce", "null_index", dict(col=None), -1, "null index pointer"),
    ("reduce", "alias", dict(out=F[0]), -1, "out must not alias input"),
    ("reduce", "misaligned", dict(arg=I + 2), -1, "feature and arg pointers must be 4-byte aligned"),
    ("scatter", "stride", dict(ld_gi=3), -1, "row strides must be >= dim and < 2^29 elements (ld_go=4 ld_arg=4 ld_gi=3 dim=4)"),
    ("scatter", "stride_2_29", dict(ld_go=ROWS_2_29), -1,
     "row strides must be >= dim and < 2^29 elements (ld_go=536870912 ld_arg=4 ld_gi=4 dim=4)"),
    ("scatter", "size", dict(n_out=-1), -1, "negative size (num_out_rows=-1 num_in_rows=2)"),
    ("scatter", "size_dim", dict(dim=0), -1, "dim must be >= 1 (got 0)"),
    ("scatter", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "unknown flag bits 0x80"),
    ("scatter", "rows_2_29", dict(n_out=ROWS_2_29), -3, "too many rows in one call (num_out_rows=536870912 num_in_rows=2)"),
    ("scatter", "null", dict(gi=None), -1, "null grad_in pointer"),
    ("scatter", "null_input", dict(arg=None), -1, "null pointer argument"),
    ("scatter", "alias", dict(gi=F[0]), -1, "grad_in must not alias grad_out"),
    ("scatter", "deterministic", DET, -3,
     "gnna_scatter_arg_ld_f32 has no deterministic schedule (gnna_tuning.deterministic = 1): its sums meet through float atomics"),
    ("x16", "stride", dict(ld_in=7), -1, "row strides must be >= dim and < 2^29 elements (ld_in=7 ld_out=8 dim=8)"),
    ("x16", "stride_2_29", dict(ld_out=ROWS_2_29), -1,
     "row strides must be >= dim and < 2^29 elements (ld_in=8 ld_out=536870912 dim=8)"),
    ("x16", "size", dict(P=-1), -1, "negative size (num_out_rows=2 dim=8 num_parts=-1)"),
    ("x16", "mode", dict(mode=3), -1, "unknown mode 3"),
    ("x16", "in_type", dict(in_type=0), -1, "in_type must be GNNA_BF16 or GNNA_F16 (got 0)"),
    ("x16", "out_type", dict(out_type=2), -1, "out_type must be GNNA_F32 or the input's type (in_type=1 out_type=2)"),
    ("x16", "partsize", dict(ps=0), -1, "partSize must be positive (got 0)"),
    ("x16", "accumulate", dict(flags=ACCUMULATE), -3,
     "GNNA_ACCUMULATE with a 16-bit output would round the sum twice: accumulate into an fp32 output"),
    ("x16", "unknown_flag", dict(flags=UNKNOWN_BIT), -1, "unknown flag bits 0x80"),
    ("x16", "rows_2_29", dict(n_out=ROWS_2_29), -3,
     "536870912 destination rows in one call (at most 536870911): shard the rows"),
    ("x16", "null", dict(out=None), -1, "null feature pointer"),
    ("x16", "null_index", dict(pp=None), -1, "null index pointer"),
    ("x16", "null_degrees", dict(mode=1), -1, "null degrees pointer"),
    ("x16", "alias", dict(out=F[0]), -1, "out must not alias input"),
    ("x16", "misaligned", dict(X=F[0] + 1), -1, "feature pointers must be aligned to their element size"),
    ("x16", "deterministic", DET, -3,
     "gnna_agg_ld_x16 has no deterministic schedule (gnna_tuning.deterministic = 1): its rows meet in fp32 through float atomics; "
     "use gnna_agg_ld_f32 on fp32 features"),
]


@pytest.mark.parametrize("entry, what, kw, rc, message", CASES, ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_refusal_keeps_its_code_and_text(entry, what, kw, rc, message):
    try:
        if kw == DET:
            _lib.set_tuning(deterministic=1)
            kw = {}
        got = ENTRIES[entry](**kw)
        text = _lib.load().gnna_last_error().decode()
    finally:
        _lib.reset_tuning()
    assert (got, text) == (rc, message)

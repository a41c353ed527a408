/*
 * gnna_dot_rows_x16.h -- the rows form of the fused scaled dot-product graph attention (gnna_dot_rows.h) over matrices STORED in
 * bfloat16 or float16 and ACCUMULATED in float32 (gnna_dot_rows_x16.hip).  The kernels own the rows they write, so the one rounding
 * of an output element is the one store of its one writer: no float atomics, no fp32 scratch of the size of an output, no finishing
 * kernel -- a 16-bit path that gives the same bits on every run and is accepted under gnna_tuning.deterministic = 1.
 *
 * Entries of libgnna.so added after gnna_dot_rows.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.  Bound
 * through this header's table in _lib.HEADERS.  Conventions (status codes, gnna_last_error, streams, scratch) are those of gnna.h.
 *
 * Types.  `type` is GNNA_BF16 or GNNA_F16 (gnna.h); any other value is GNNA_ERR_INVALID_ARGUMENT.  Q, K, V, out, Y, dY, dQ, dK and
 * dV of a call all have that type; leading dimensions are in ELEMENTS.  lse is float32, and so is the node-sized (lse, c) record
 * scratch of the backward (a scratch slot of its own).
 *
 * The function is that of gnna_dot_rows.h, word for word, the mask rule (gnna_ext.h) included:
 *
 *     z          = scale * sum_d Q[i,h,d] * K[j,h,d]
 *     lse[i,h]   = logsumexp_j z, over the un-dropped scores                         0 for a row without counted edges
 *     alpha      = exp(z - lse[i,h])
 *     k          = the dropout factor, a function of (rng_seed, i, j, h); 1 when attn_drop = 0
 *     out[i,h,:] = sum_j alpha * k * V[j,h,:]                                        0 for a row without counted edges
 *
 *     c[i,h]     = <dY[i,h,:], Y[i,h,:]>          dalpha = <dY[i,h,:], V[j,h,:]>
 *     dz         = alpha * (k * dalpha - c)
 *     dQ[i,h,:]  = scale * sum_j dz * K[j,h,:]
 *     dK[j,h,:]  = scale * sum_i dz * Q[i,h,:]
 *     dV[j,h,:]  = sum_i alpha * k * dY[i,h,:]
 *
 * Arithmetic.  Every input element is widened exactly (bf16 by a shift, fp16 by v_cvt_f32_f16).  Every product, score,
 * exponential and sum is float32 in a fixed order, as in the float32 kernels; no 16-bit dot instruction is used.  Each output
 * element is rounded ONCE, to nearest even, at its one store.  c is made from the Y the caller passes -- the rounded output of the
 * forward, not the float32 value it was rounded from -- as flash-attention backward passes make it: dQ and dK carry that rounding
 * of Y (at most u * sum |terms| with u = 2^-8 for bf16, 2^-11 for fp16) beyond their own.
 *
 * Shapes, the structure arguments, the rules for ids out of range, rows without edges, GNNA_EPILOGUE_RELU (forward only),
 * GNNA_ACCUMULATE (refused), NULL column_index and NULL outputs are those of gnna_dot_rows.h.  Q, K and V may overlap or be
 * column slices of one projection matrix.  heads <= 64, dim <= 256.
 *
 * The contract of the family carries over unchanged:
 *   - plain stores only, one writer per output element;
 *   - the order of every sum is a function of the structure and (heads, dim) only: the same bits on every run;
 *   - every element of the heads * dim (heads) columns of every row of every non-NULL output is written, so outputs pre-filled
 *     with NaN come back clean; there is no zero-fill launch; columns from heads * dim to the leading dimension are never touched;
 *   - accepted under gnna_tuning.deterministic = 1;
 *   - no tensor of the size of the edge list is read, written or allocated beyond the index arrays themselves;
 *   - library scratch is node-sized: num_out_rows * heads * 8 bytes (float32 records), backward only;
 *   - no synchronisation: a captured call consists of kernel nodes once that scratch exists (it is the capture's own).
 *
 * Ownership and data movement.  A lane holds 8 elements; LPH = next_pow2(ceil(dim / 8)) lanes cover a head, LPR = LPH * (whole
 * heads that fit) <= 64 lanes a row of a column block, and the 64 / LPR slots of a wavefront each own one of 64 / LPR consecutive
 * rows (dim = 64, one head: 8 rows per wavefront).  A row of up to 8 edges is walked by its own slot; a longer row of up to
 * (64 / LPR) * 128 edges by the slots of its wavefront, which meet by a butterfly; a row beyond that by the four wavefronts of its
 * workgroup, which meet through LDS in the order of the wavefronts.  A lane's piece of a row is ONE 16-byte access when every base
 * pointer of the call is 16-byte aligned, every leading dimension is a multiple of 8 and dim % 8 == 0; otherwise the whole call
 * moves its pieces by 16-bit loads and stores.  Both ways widen exactly and sum in the same order: they give the same bits.
 *
 * Checks, before any device work: the type, then those of gnna_dot_rows.h with the same texts under these entries' names
 * (GNNA_ACCUMULATE, unknown flag bits, sizes, row counts < 2^29, dim <= 256, heads <= 64, attn_drop in [0, 1) and not NaN, a finite
 * scale, row strides >= heads * dim and < 2^29 elements, no null pointer that would be used, no output that is an input or another
 * output).
 *
 * Out of scope: 16-bit storage for the atomic dot-product entries (gnna_dotattn.h), for the GAT rows form and for GATv2; a
 * per-edge score term.
 */
#ifndef GNNA_DOT_ROWS_X16_H_
#define GNNA_DOT_ROWS_X16_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_dot_attn_forward_rows_x16(
        int type, const void *Q, int64_t ld_q, const void *K, int64_t ld_k, const void *V, int64_t ld_v, int64_t num_in_rows,
        const int32_t *row_pointers, const int32_t *column_index,
        float scale, float attn_drop, uint64_t rng_seed,
        void *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream);

GNNA_API int gnna_dot_attn_backward_rows_x16(
        int type, const void *Q, int64_t ld_q, const void *K, int64_t ld_k, const void *V, int64_t ld_v, int64_t num_in_rows,
        const float *lse, const void *Y, int64_t ld_y, const void *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index,
        const int32_t *t_row_pointers, const int32_t *t_column_index,
        float scale, float attn_drop, uint64_t rng_seed,
        void *dQ, int64_t ld_dq, void *dK, int64_t ld_dk, void *dV, int64_t ld_dv,
        int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_DOT_ROWS_X16_H_ */

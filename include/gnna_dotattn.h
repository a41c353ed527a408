/*
 * gnna_dotattn.h -- fused scaled dot-product graph attention of libgnna.so (gnna_dotattn.hip).
 *
 * gnna.h (the pinned 601 surface), gnna_ext.h and gnna_gatv2.h are compared entry for entry by the test suite and stay as they
 * are; these entries are declared here and bound through this header's table in _lib.HEADERS, which the loader applies the
 * same way.  Conventions (status codes, gnna_last_error, streams,
 * scratch) are those of gnna.h; gnna_version() stays 601.
 *
 * The function is the attention of graph transformers (TransformerConv / UniMP, DotGatConv, the inner step of HGT and GPS
 * layers).  Q [num_out_rows, heads * dim] is the query of the destination rows, K and V [num_in_rows, heads * dim] the key and
 * the message of the source rows (the value head has the width of the key head).  For an edge i <- j (destination row i, column
 * id j; duplicate edges count twice) and head h:
 *
 *     z        = scale * sum_d Q[i,h,d] * K[j,h,d]
 *     lse[i,h] = logsumexp_j z                              (0 for a row without edges)
 *     alpha    = exp(z - lse[i,h])
 *     k        = the dropout factor of gnna_ext.h's rule, a function of (rng_seed, i, j, h); 1 when attn_drop = 0
 *     out[i,h,:] = sum_j alpha * k * V[j,h,:]
 *
 * Every pass recomputes z from the K row it gathers (the source side of the backward: from the Q row) and the walked row's own
 * piece.  No buffer of the size of the edge list exists anywhere; lse (and Y) is all the backward needs from the forward.
 *
 * Backward, with c[i,h] = <dY[i,h,:], Y[i,h,:]> and dalpha = <dY[i,h,:], V[j,h,:]>:
 *
 *     dz         = alpha * (k * dalpha - c)
 *     dQ[i,h,:]  = scale * sum_j dz * K[j,h,:]
 *     dK[j,h,:]  = scale * sum_i dz * Q[i,h,:]
 *     dV[j,h,:]  = sum_i alpha * k * dY[i,h,:]
 *
 * There is no parameter gradient.  Rectangular form with dropout only, as the entries of gnna_gatv2.h: the square case is both
 * counts equal, attn_drop = 0 is the plain function, and a symmetric undirected graph passes its own structure as the transposed
 * one.  Q, K and V each have a row stride of their own: they MAY overlap, be the same pointer, or be column slices of one
 * projection matrix [rows, 3 * heads * dim].  Everything gnna_gatv2_forward_f32 / gnna_gatv2_backward_f32 promise holds here
 * too, with messages prefixed by the entry's name:
 *   - ids outside [0, num_in_rows) (the transposed structure: [0, num_out_rows)), neighbor-groups without edges, with a negative
 *     range or with a row outside their side's rows are skipped, in every pass alike; num_in_rows = 0 gives out = 0, lse = 0;
 *   - the outputs are zero-filled first and every element is written -- out and lse; dQ, dK and dV;
 *   - GNNA_EPILOGUE_RELU on the forward only; GNNA_ACCUMULATE gives GNNA_ERR_UNSUPPORTED;
 *   - heads <= 64, dim <= 256, fewer than 2^29 rows on either side, row strides in [heads * dim, 2^29);
 *   - GNNA_ERR_UNSUPPORTED under gnna_tuning.deterministic = 1 (the gathered rows meet through float atomics); lse alone has one
 *     writer per (row, head) and the same bits on every run;
 *   - attn_drop outside [0, 1) or NaN gives GNNA_ERR_INVALID_ARGUMENT before any device work;
 *   - a scale that is NaN or infinite gives GNNA_ERR_INVALID_ARGUMENT before any device work (scale = 0 is uniform attention);
 *   - an output must not alias an input or another output.
 * Y is the out of the forward call with the same scale, attn_drop and rng_seed.  The backward keeps 8 bytes per (destination
 * row, head) of library scratch.  row_pointers is [num_out_rows + 1] (the lse pass walks it); the backward reads the
 * neighbor-groups only.
 */
#ifndef GNNA_DOTATTN_H_
#define GNNA_DOTATTN_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_dot_attn_forward_f32(const float *Q, int64_t ld_q, const float *K, int64_t ld_k, const float *V, int64_t ld_v,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float scale, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize,
        unsigned flags, void *stream);
GNNA_API int gnna_dot_attn_backward_f32(const float *Q, int64_t ld_q, const float *K, int64_t ld_k, const float *V, int64_t ld_v,
        const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        int64_t num_parts,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
        int64_t t_num_parts,
        float scale, float attn_drop, uint64_t rng_seed, float *dQ, int64_t ld_dq, float *dK, int64_t ld_dk,
        float *dV, int64_t ld_dv, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags,
        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_DOTATTN_H_ */

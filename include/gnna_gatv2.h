/*
 * gnna_gatv2.h -- fused GATv2 ("dynamic") attention of libgnna.so (gnna_gatv2.hip).
 *
 * gnna.h (the pinned 601 surface) and gnna_ext.h are compared entry for entry by the test suite and stay as they are; these
 * entries are declared here and bound through this header's table in _lib.HEADERS, which the loader applies the same way.
 * Conventions (status codes, gnna_last_error, streams, scratch) are those of gnna.h;
 * gnna_version() stays 601.
 *
 * The function (Brody et al., "How Attentive are Graph Attention Networks?").  Hs [num_in_rows, heads * dim] is the source side
 * and the message, Hd [num_out_rows, heads * dim] the destination side, att [heads * dim] the attention vector, s the slope.
 * For an edge i <- j (destination row i, column id j; duplicate edges count twice) and head h:
 *
 *     t[d]     = Hs[j,h,d] + Hd[i,h,d]
 *     z        = sum_d att[h,d] * lrelu(t[d])              lrelu(x) = x > 0 ? x : s * x
 *     lse[i,h] = logsumexp_j z                              (0 for a row without edges)
 *     alpha    = exp(z - lse[i,h])
 *     k        = the dropout factor of gnna_ext.h's rule, a function of (rng_seed, i, j, h); 1 when attn_drop = 0
 *     out[i,h,:] = sum_j alpha * k * Hs[j,h,:]
 *
 * The non-linearity sits inside the dot product, so the score is not a sum of two node-sized scalars as in gnna_gat_forward_f32:
 * every pass recomputes z from the row it gathers anyway and the row's own Hd piece.  No buffer of the size of the edge list
 * exists anywhere; lse (and Y) is all the backward needs from the forward.
 *
 * Backward, with c[i,h] = <dY[i,h,:], Y[i,h,:]> and dalpha = <dY[i,h,:], Hs[j,h,:]>:
 *
 *     dz         = alpha * (k * dalpha - c)
 *     g[d]       = dz * att[h,d] * (t[d] > 0 ? 1 : s)
 *     dHd[i,h,:] = sum_j g
 *     dHs[j,h,:] = sum_i (alpha * k * dY[i,h,:] + g)
 *     d_att[h,d] = sum_edges dz * lrelu(t[d])
 *
 * Rectangular form with dropout only, as the entries of gnna_ext.h: the square case is both counts equal, attn_drop = 0 is the
 * plain function, and a symmetric undirected graph passes its own structure as the transposed one.  Hs and Hd MAY be the same
 * pointer (shared weights on a square graph).  Everything gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32 and the drop
 * entries promise holds here too, with messages prefixed by the entry's name:
 *   - ids outside [0, num_in_rows) (the transposed structure: [0, num_out_rows)), neighbor-groups without edges, with a negative
 *     range or with a row outside their side's rows are skipped, in every pass alike; num_in_rows = 0 gives out = 0, lse = 0;
 *   - the outputs are zero-filled first and every element is written -- out and lse; dHs, dHd and d_att (d_att on every call that
 *     passes the checks, also with no row on either side);
 *   - GNNA_EPILOGUE_RELU on the forward; GNNA_ACCUMULATE gives GNNA_ERR_UNSUPPORTED;
 *   - heads <= 64, dim <= 256, fewer than 2^29 rows on either side, row strides in [heads * dim, 2^29);
 *   - GNNA_ERR_UNSUPPORTED under gnna_tuning.deterministic = 1 (the gathered rows meet through float atomics); lse alone has one
 *     writer per (row, head) and the same bits on every run;
 *   - attn_drop outside [0, 1) or NaN gives GNNA_ERR_INVALID_ARGUMENT before any device work;
 *   - an output must not alias an input or another output.
 * Y is the out of the forward call with the same attn_drop and rng_seed.  The backward keeps 8 bytes per (destination row, head)
 * of library scratch.  row_pointers is [num_out_rows + 1] (the lse pass walks it); the backward reads the neighbor-groups only.
 */
#ifndef GNNA_GATV2_H_
#define GNNA_GATV2_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_gatv2_forward_f32(const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float negative_slope, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize,
        unsigned flags, void *stream);
GNNA_API int gnna_gatv2_backward_f32(const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att,
        const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        int64_t num_parts,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
        int64_t t_num_parts,
        float negative_slope, float attn_drop, uint64_t rng_seed, float *dHs, int64_t ld_dhs, float *dHd, int64_t ld_dhd,
        float *d_att, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_GATV2_H_ */

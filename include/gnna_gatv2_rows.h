/*
 * gnna_gatv2_rows.h -- the "rows" form of the fused GATv2 ("dynamic") attention: the function of gnna_gatv2_forward_f32 /
 * gnna_gatv2_backward_f32 (gnna_gatv2.h), made by kernels that OWN the rows they write (gnna_gatv2_rows.hip).  No neighbor-group
 * partition, no float atomics, no zero-fill: the same bits on every run, accepted under gnna_tuning.deterministic = 1 -- and the
 * forward is ONE pass (an online softmax in the row's owner): Hs[j], the score's input and the message, is gathered once per
 * edge, where the atomic forward walks the ids twice and gathers it twice.
 *
 * Entries of libgnna.so added after gnna_dot_rows_x16.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are, and
 * so do the atomic entries (their code, their refusal under deterministic = 1 and its message).  Bound through this header's table
 * in _lib.HEADERS.  Conventions (status codes, gnna_last_error, streams, scratch) are those of gnna.h.
 *
 * The function, word for word that of gnna_gatv2.h.  Hs [num_in_rows, heads * dim] is the source side and the message, Hd
 * [num_out_rows, heads * dim] the destination side, att [heads * dim] the attention vector, s = negative_slope.  For an edge
 * i <- j (a position of row i of (row_pointers, column_index), j = column_index[e]; a duplicate edge counts twice) and head h:
 *
 *     t[d]       = Hs[j,h,d] + Hd[i,h,d]
 *     z          = sum_d att[h,d] * lrelu(t[d])                lrelu(x) = x > 0 ? x : s * x
 *     lse[i,h]   = logsumexp_j z, over the un-dropped scores                         0 for a row without counted edges
 *     alpha      = exp(z - lse[i,h])
 *     k          = the dropout factor of gnna_ext.h's rule, a function of (rng_seed, i, j, h); 1 when attn_drop = 0
 *     out[i,h,:] = sum_j alpha * k * Hs[j,h,:]                                       0 for a row without counted edges
 *
 *     c[i,h]     = <dY[i,h,:], Y[i,h,:]>          dalpha = <dY[i,h,:], Hs[j,h,:]>
 *     dz         = alpha * (k * dalpha - c)
 *     g[d]       = dz * att[h,d] * (t[d] > 0 ? 1 : s)
 *     dHd[i,h,:] = sum_j g
 *     dHs[j,h,:] = sum_i (alpha * k * dY[i,h,:] + g)
 *     d_att[h,d] = sum over the edges of dz * lrelu(t[d])
 *
 * Y is the out of the forward call with the same negative_slope, attn_drop and rng_seed.  Every matrix has a leading dimension of
 * its own; lse is [num_out_rows, heads] contiguous, att and d_att are [heads * dim] contiguous.  heads <= 64, dim <= 256.  Hs and
 * Hd MAY be the same pointer (shared weights) or overlap; dHs and dHd are separate outputs.  Entries are rectangular only: a
 * square graph is the call with both row counts equal.
 *
 * No partition arguments: the kernels walk CSR rows (row pointers are trusted to increase).  The backward entry ALWAYS takes the
 * transposed structure (t_row_pointers, t_column_index: num_in_rows rows whose ids are destination rows, e.g. from
 * gnna_transpose_csr_i32); a graph whose structure is symmetric passes its own arrays twice.  Each of dHs, dHd and d_att may be
 * NULL, and work that serves only unwanted outputs is not done: the source side runs for dHs alone; the destination side walks
 * the edges for dHd or d_att, and with both NULL it only leaves the (lse, c) records that the source side gathers -- no edge walk.
 * d_att is written on every call that passes the checks: zeros when either side has no row or no edge counts.
 *
 * Rules, in every pass alike:
 *   - a column id outside [0, num_in_rows) is skipped -- in the transposed structure: an id outside [0, num_out_rows);
 *   - a row without (counted) edges gives out = 0, lse = 0 and zero gradients;
 *   - GNNA_EPILOGUE_RELU applies to the forward only (inside the kernel: no second launch); GNNA_ACCUMULATE is refused;
 *   - column_index (t_column_index) may be NULL only when no row of its structure has an edge.
 *
 * The contract of this family (that of gnna_gat_rows.h and gnna_dot_rows.h):
 *   - plain stores only, one writer per output element;
 *   - the order of every sum is a function of the structure and (heads, dim) only: the same bits on every run, d_att included;
 *   - every element of the heads * dim (heads) columns of every row of every non-NULL output is written, so outputs pre-filled
 *     with NaN come back clean; there is no zero-fill launch; columns from heads * dim to the leading dimension are never touched;
 *   - accepted under gnna_tuning.deterministic = 1;
 *   - no tensor of the size of the edge list is read, written or allocated beyond the index arrays themselves;
 *   - library scratch is node-sized: num_out_rows * heads * 8 bytes, the (lse, c) record of every (destination row, head) that the
 *     destination-side pass of the backward writes and the source-side pass gathers (when dHs is wanted), and
 *     ceil(num_out_rows / rows per workgroup) * heads * dim * 4 bytes, one partial of d_att per workgroup of the destination side
 *     (when d_att is wanted; rows per workgroup = 4 * 64 / LPR, see below); the forward has none;
 *   - no synchronisation: a captured call consists of kernel nodes once that scratch exists (it is the capture's own).
 *
 * d_att.  The lanes of the destination side keep their share in registers across all the rows they walk; the slots of a wavefront
 * meet by a fixed butterfly, the wavefronts through LDS in the order of the wavefronts, and every workgroup stores ONE partial
 * [heads * dim] into the scratch.  A second small kernel sums the partials of each column: 64 strands add the workgroups
 * s, s + 64, ... in order and meet in a binary tree.  The grid of the destination side depends on (num_out_rows, heads, dim) only.
 *
 * Ownership.  LPR lanes of 4 floats hold a row of a column block (as many whole heads as fit in a wavefront); the 64 / LPR slots
 * of a wavefront each own one of 64 / LPR consecutive rows.  A row of up to 8 edges is walked by its own slot (wavefronts of more
 * than one slot); a longer row of up to (64 / LPR) * 128 edges by the slots of its wavefront, which then meet by a butterfly; a
 * row beyond that by the four wavefronts of its workgroup, which meet through LDS in the order of the wavefronts.  A row is owned
 * by at most one workgroup: there is no hub splitting.
 *
 * Out of scope: a per-edge score term, bfloat16 / float16 storage.
 *
 * Checks, before any device work: GNNA_ACCUMULATE, unknown flag bits, sizes >= 0 with heads, dim >= 1, row counts < 2^29,
 * dim <= 256, heads <= 64, attn_drop in [0, 1) and not NaN, a finite negative_slope, row strides >= heads * dim and < 2^29 floats,
 * no null pointer that would be used, no output that is an input or another output.
 */
#ifndef GNNA_GATV2_ROWS_H_
#define GNNA_GATV2_ROWS_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_gatv2_forward_rows_f32(
        const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att, int64_t num_in_rows,
        const int32_t *row_pointers, const int32_t *column_index,
        float negative_slope, float attn_drop, uint64_t rng_seed,
        float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream);

GNNA_API int gnna_gatv2_backward_rows_f32(
        const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att, int64_t num_in_rows,
        const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index,
        const int32_t *t_row_pointers, const int32_t *t_column_index,
        float negative_slope, float attn_drop, uint64_t rng_seed,
        float *dHs, int64_t ld_dhs, float *dHd, int64_t ld_dhd, float *d_att,
        int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_GATV2_ROWS_H_ */

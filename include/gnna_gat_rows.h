/*
 * gnna_gat_rows.h -- the "rows" form of the fused multi-head GAT attention: the function of gnna_gat_forward_rect_f32 /
 * gnna_gat_backward_rect_f32 (gnna.h), made by kernels that OWN the rows they write (gnna_gat_rows.hip).  No neighbor-group
 * partition, no float atomics, no zero-fill: the same bits on every run, accepted under gnna_tuning.deterministic = 1.
 *
 * Entries of libgnna.so added after gnna_spatial.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are, and so
 * do the atomic entries (their code, their refusal under deterministic = 1 and its message).  Bound through this header's table
 * in _lib.HEADERS.  Conventions (status codes, gnna_last_error, streams, scratch) are those of gnna.h.
 *
 * The function, word for word that of the rect entries.  For an edge i <- j (a position of row i of (row_pointers, column_index),
 * j = column_index[e]) and head h:
 *
 *     z(i,j,h)     = el[i,h] + er[j,h]
 *     s            = z > 0 ? z : negative_slope * z
 *     lse[i,h]     = log sum over the edges of row i of exp(s)                       0 for a row without edges
 *     alpha        = exp(s - lse[i,h])
 *     out[i,h,:]   = sum over the edges of row i of alpha * H[j,h,:]                 0 for a row without edges
 *
 *     c[i,h]       = <dY[i,h,:], Y[i,h,:]>
 *     dz           = alpha * (<dY[i,h,:], H[j,h,:]> - c[i,h]) * (z > 0 ? 1 : negative_slope)
 *     d_el[i,h]    = sum over the edges of row i of dz
 *     d_er[j,h]    = sum over the edges with source j of dz
 *     dH[j,h,:]    = sum over the edges with source j of alpha * dY[i,h,:]           (the attention part only)
 *
 * Shapes: H and dH [num_in_rows, heads * dim] with a leading dimension; er and d_er [num_in_rows, heads] contiguous; out, Y and dY
 * [num_out_rows, heads * dim] with a leading dimension; el, lse and d_el [num_out_rows, heads] contiguous.  heads <= 64,
 * dim <= 256.  Entries are rectangular only: a square graph is the call with both row counts equal.  A duplicate edge counts twice.
 *
 * No partition arguments: the kernels walk CSR rows (row pointers are trusted to increase).  The backward entry ALWAYS takes the
 * transposed structure (t_row_pointers, t_column_index: num_in_rows rows whose ids are destination rows, e.g. from
 * gnna_transpose_csr_i32); a graph whose structure is symmetric passes its own arrays twice.  Each of dH, d_el and d_er may be
 * NULL, and a pass none of whose outputs is wanted is not launched.
 *
 * Rules, in every pass alike:
 *   - a column id outside [0, num_in_rows) is skipped -- in the transposed structure: an id outside [0, num_out_rows);
 *   - a row without (counted) edges gives out = 0, lse = 0 and zero gradients;
 *   - GNNA_EPILOGUE_RELU applies to the forward only (inside the kernel: no second launch); GNNA_ACCUMULATE is refused;
 *   - column_index (t_column_index) may be NULL only when no row of its structure has an edge.
 *
 * The contract of this family:
 *   - plain stores only, one writer per output element;
 *   - the order of every sum is a function of the structure and (heads, dim) only: the same bits on every run;
 *   - every element of the heads * dim (heads) columns of every row of every non-NULL output is written, so outputs pre-filled
 *     with NaN come back clean; there is no zero-fill launch; columns from heads * dim to the leading dimension are never touched;
 *   - accepted under gnna_tuning.deterministic = 1;
 *   - no tensor of the size of the edge list is read, written or allocated beyond the index arrays themselves;
 *   - library scratch is node-sized: num_out_rows * heads * 16 bytes, the (el, lse, c, 0) record of every (destination row, head)
 *     that the destination-side pass of the backward writes and the source-side pass gathers (as the atomic backward has); the
 *     forward has none;
 *   - no synchronisation: a captured call consists of kernel nodes once that scratch exists (it is the capture's own).
 *
 * Ownership.  LPR lanes of 4 floats hold a row of a column block (as many whole heads as fit in a wavefront); the 64 / LPR slots
 * of a wavefront each own one of 64 / LPR consecutive rows.  A row of up to 8 edges is walked by its own slot (wavefronts of more
 * than one slot); a longer row of up to (64 / LPR) * 128 edges by the slots of its wavefront, which then meet by a butterfly; a
 * row beyond that by the four wavefronts of its workgroup, which meet through LDS in the order of the wavefronts.  A row is owned
 * by at most one workgroup: there is no hub splitting.
 *
 * Out of scope, and left to the atomic entries: attention dropout (gnna_ext.h), a per-edge score term (gnna_gat_edge.h), GATv2
 * (gnna_gatv2.h) and dot-product attention (gnna_dotattn.h), 16-bit storage.
 *
 * Checks, before any device work (those of the rect entries, without the partition): GNNA_ACCUMULATE, unknown flag bits, sizes
 * >= 0 with heads, dim >= 1, row counts < 2^29, dim <= 256, heads <= 64, row strides >= heads * dim and < 2^29 floats, no null
 * pointer that would be used, no output that is an input or another output.
 */
#ifndef GNNA_GAT_ROWS_H_
#define GNNA_GAT_ROWS_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_gat_forward_rows_f32(const float *H, int64_t ld_h, int64_t num_in_rows, const float *el, const float *er,
        const int32_t *row_pointers, const int32_t *column_index, float negative_slope,
        float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream);

GNNA_API int gnna_gat_backward_rows_f32(const float *H, int64_t ld_h, int64_t num_in_rows, const float *el, const float *er,
        const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index,
        const int32_t *t_row_pointers, const int32_t *t_column_index, float negative_slope,
        float *dH, int64_t ld_dh, float *d_el, float *d_er,
        int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_GAT_ROWS_H_ */

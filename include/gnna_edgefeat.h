/*
 * gnna_edgefeat.h -- message passing with a feature ROW per edge: the sum over a row's edges of act(x_j (+ | *) e_ij), made in
 * ONE gather that streams the edge rows, and its two backward passes (gnna_edgefeat.hip).  It is the aggregation of GINE
 * (relu(x_j + e_ij), Hu et al.) and of SchNet's continuous-filter convolution (x_j * W(e_ij)).
 *
 * Entries of libgnna.so added after gnna_walk.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes, gnna_last_error,
 * streams, scratch) are those of gnna.h.
 *
 * The function.  For position e of column_index in destination row i (row_pointers[i] <= e < row_pointers[i + 1]), with source
 * j = column_index[e] and column f:
 *
 *     pre[e,f] = x[j,f] + E[e,f]                     combine = GNNA_EDGE_ADD
 *              = x[j,f] * E[e,f]                     combine = GNNA_EDGE_MUL
 *     msg[e,f] = pre                                 act = GNNA_EDGE_ACT_NONE
 *              = pre > 0 ? pre : 0                   act = GNNA_EDGE_ACT_RELU: the mask is `pre > 0` evaluated in fp32, and the
 *                                                    gradient at pre == 0 is 0
 *     out[i,f] = sum over the edges of row i of msg[e,f]                          0 for a row without edges
 *
 *     d_input[j,f] = sum over the edges with source j of dY[i,f] * mask * (1 | E[e,f])          (ADD | MUL)
 *     d_edge[e,f]  = dY[i,f] * mask * (1 | x[j,f])                                              0 for a skipped edge
 *
 * with mask = 1 without an activation.  E (edge_feat) and d_edge are [num_edges, dim] fp32 with a leading dimension, EDGE-MAJOR in
 * the order of column_index; input is [num_in_rows, dim], out and dY [num_out_rows, dim], d_input [num_in_rows, dim].  A duplicate
 * edge counts twice (each position has its own E row).  num_in_rows != num_out_rows is the normal rectangular case; any dim >= 1.
 * NaN or infinite values in x, E or dY give whatever IEEE arithmetic gives (a NaN pre fails `pre > 0`); that behaviour is not
 * pinned.
 *
 * The backward entry.  d_input and d_edge may each be NULL, and a NULL output's pass is not launched.  d_edge is made on the
 * destination side: a walk over the rows of (row_pointers, column_index) that holds dY[i].  d_input is made on the source side: a
 * walk over row j of A^T (t_row_pointers, t_column_index: num_in_rows rows whose ids are destination rows) that holds x[j] and
 * gathers dY[i] and E[e], where e = t_edge_pos[p] is the position in column_index of the edge that transposed position p stands
 * for.  t_edge_pos has the meaning it has in gnna_gat_edge.h: `perm` of gnna_transpose_csr_i32, or the reverse-edge map of a
 * structure that is symmetric.  The three transposed arrays are needed only when d_input is wanted.  Nothing of the size of the
 * edge list is saved or made beyond E (an input) and d_edge (an output): the mask is recomputed from x and E in every pass.  The
 * source-side pass needs no scratch and does no zero-fill.
 *
 * Rules, in every pass alike (row pointers are trusted to increase):
 *   - a column id outside [0, num_in_rows) is skipped -- in the transposed structure: an id outside [0, num_out_rows);
 *   - a position >= num_edges is skipped (a row's range in row_pointers is cut to [0, num_edges]);
 *   - in the source-side pass a t_edge_pos outside [0, num_edges) is skipped;
 *   - every element of the `dim` columns of every row of every non-NULL output is written: a row without edges gets 0, a skipped
 *     edge's d_edge row is 0, and so is a d_edge row at or beyond row_pointers[num_out_rows]; columns from `dim` to the leading
 *     dimension are never touched;
 *   - num_edges = 0 gives zero outputs, and reads no index.
 *
 * One writer per output element, plain stores, a fixed order of every sum: the same bits on every run, and both entries are
 * accepted under gnna_tuning.deterministic = 1.  No synchronisation, no plan, no library scratch: a captured call consists of
 * kernel nodes.
 *
 * Checks, before any device work: flags == 0 (GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning here: the activation is
 * `act`), dim >= 1, sizes >= 0, combine and act in range, row counts < 2^29, num_edges < 2^31, strides >= dim and < 2^29 elements,
 * 4-byte alignment, no output that is an input or another output, no null pointer that would be used.
 */
#ifndef GNNA_EDGEFEAT_H_
#define GNNA_EDGEFEAT_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GNNA_EDGE_ADD 0
#define GNNA_EDGE_MUL 1
#define GNNA_EDGE_ACT_NONE 0
#define GNNA_EDGE_ACT_RELU 1

GNNA_API int gnna_agg_edge_feat_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const float *edge_feat, int64_t ld_e, int64_t num_edges,
        const int32_t *row_pointers, const int32_t *column_index,
        float *out, int64_t ld_out,
        int64_t num_out_rows, int dim, int combine, int act, unsigned flags, void *stream);

GNNA_API int gnna_agg_edge_feat_backward_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const float *edge_feat, int64_t ld_e, int64_t num_edges, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_edge_pos,
        float *d_input, int64_t ld_din, float *d_edge, int64_t ld_de,
        int64_t num_out_rows, int dim, int combine, int act, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_EDGEFEAT_H_ */

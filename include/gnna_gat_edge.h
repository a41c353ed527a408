/*
 * gnna_gat_edge.h -- fused GAT attention with a per-edge score term (gnna_gat.hip), and the attention coefficients edge for edge.
 *
 * Entries of libgnna.so added after gnna_dotattn.h; gnna.h, gnna_ext.h, gnna_gatv2.h, gnna_dotattn.h and GNNA_VERSION stay as
 * they are.  Bound through this header's table in _lib.HEADERS.  Conventions (status codes,
 * gnna_last_error, streams, scratch) are those of gnna.h.
 *
 * The function.  For the edge at position e of column_index, in destination row i (row_pointers[i] <= e < row_pointers[i + 1]),
 * with source j = column_index[e], and head h:
 *
 *     z[e,h]     = el[i,h] + er[j,h] + ee[e,h]
 *     lse[i,h]   = logsumexp over the edges of row i of leaky_relu(z)          (0 for a row without edges)
 *     alpha[e,h] = exp(leaky_relu(z) - lse[i,h])
 *     out[i,h,:] = sum_e alpha * k * H[j,h,:]            (k = 1, or the dropout factor k(rng_seed, i, j, h) of gnna_ext.h)
 *
 *   Backward, with c[i,h] = <dY[i,h,:], Y[i,h,:]> and dalpha = <dY[i,h,:], H[j,h,:]>:
 *     dz[e,h]    = alpha * (k * dalpha - c) * (z > 0 ? 1 : negative_slope)
 *     d_el[i,h]  = sum over the edges of row i of dz
 *     d_er[j,h]  = sum over the edges from source j of dz
 *     d_ee[e,h]  = dz[e,h]
 *     dH[j,h,:]  = sum over the edges from source j of alpha * k * dY[i,h,:]
 *
 * ee and d_ee are [num_edges, heads] fp32, contiguous, edge-major: row e belongs to position e of column_index -- the result of
 * a [num_edges, edge_dim] x [edge_dim, heads] product as it stands.  Nothing else of the size of the edge list exists: alpha is
 * recomputed where it is used, as in the entries without the term.
 *
 * Positions.  The lse pass, the forward and the destination-side pass of the backward walk the structure itself, so an edge's
 * position is where they read its id.  The source-side pass walks the transposed structure (row j, id i); t_edge_pos [num_edges]
 * gives, for every position p of t_column_index, the position e in column_index of that same edge i <- j:
 *     a directed graph or a sampled block: the `perm` of gnna_transpose_csr_i32;
 *     a symmetric graph that passes its own structure as the transposed one: the reverse-edge map of gnna_reverse_edges_i32.
 *
 * Skipping.  An edge whose id lies outside the source rows is skipped in every pass, as in the other entries; so is a position
 * >= num_edges, and, in the source-side pass, a transposed edge whose t_edge_pos lies outside [0, num_edges): it is never read
 * through (it is then missing from d_er and dH only).  A skipped edge's d_ee row and alpha row are 0.  Every element of every
 * output is written.
 *
 * d_ee has one writer per element (the destination-side pass, plain stores): two calls with the same inputs give the same
 * bits.  dH, d_el, d_er and out are added with float atomics as in the other entries.
 *
 * Checks, before any device work: those of gnna_gat_forward_drop_f32 / gnna_gat_backward_drop_f32 (sizes, strides, null
 * pointers, attn_drop in [0, 1), GNNA_ACCUMULATE refused for every gradient, d_ee included, GNNA_ERR_UNSUPPORTED under
 * gnna_tuning.deterministic = 1), and
 *     num_edges >= 0 (and < 2^31);
 *     ee -- and in the backward d_ee and t_edge_pos -- non-null when num_edges > 0;
 *     no output (out, lse; dH, d_el, d_er, d_ee; alpha) is an input (ee and t_edge_pos included) or another output.
 * num_edges = 0 means that no edge exists: the outputs are 0.
 */
#ifndef GNNA_GAT_EDGE_H_
#define GNNA_GAT_EDGE_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gnna_gat_forward_drop_f32 (gnna_ext.h) with ee after er and num_edges after the row counts. */
GNNA_API int gnna_gat_edge_forward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *ee,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float negative_slope, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int64_t num_in_rows, int64_t num_edges, int heads, int dim, int64_t num_parts, int partSize,
        unsigned flags, void *stream);

/* gnna_gat_backward_drop_f32 (gnna_ext.h) with ee after er, t_edge_pos after the transposed structure, d_ee after d_er and
 * num_edges after the row counts.  Y is the out of the forward call with the same ee, attn_drop and rng_seed. */
GNNA_API int gnna_gat_edge_backward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *ee,
        const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        int64_t num_parts,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
        int64_t t_num_parts, const int32_t *t_edge_pos,
        float negative_slope, float attn_drop, uint64_t rng_seed, float *dH, int64_t ld_dh, float *d_el, float *d_er, float *d_ee,
        int64_t num_out_rows, int64_t num_in_rows, int64_t num_edges, int heads, int dim, int partSize, unsigned flags,
        void *stream);

/* alpha[e,h] (undropped; 0 for a skipped edge and for a position outside [row_pointers[0], row_pointers[num_out_rows])) from the
 * node-sized values and lse of a forward call.  alpha is [num_edges, heads], edge-major like ee.  ee may be NULL: alpha of the
 * entries without the term (gnna_gat_forward_f32 and its kin).  An edge-parallel kernel of its own: one writer per element, plain
 * stores, allowed under gnna_tuning.deterministic = 1.  heads <= 64, rows < 2^29, num_edges < 2^31. */
GNNA_API int gnna_gat_alpha_f32(const float *el, const float *er, const float *ee, const float *lse,
        const int32_t *row_pointers, const int32_t *column_index, float negative_slope, float *alpha,
        int64_t num_out_rows, int64_t num_in_rows, int64_t num_edges, int heads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_GAT_EDGE_H_ */

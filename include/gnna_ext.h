/*
 * gnna_ext.h -- entries of libgnna.so added after the pinned 601 surface of gnna.h.
 *
 * gnna.h, GNNA_VERSION (601) and the binding table that restates it are compared entry for entry by the test suite and stay as
 * they are; an entry added since is declared here and bound through this header's table in _lib.HEADERS, which the loader
 * applies the same way.  Conventions (status codes, gnna_last_error, streams, scratch) are those of gnna.h.
 */
#ifndef GNNA_EXT_H_
#define GNNA_EXT_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Attention dropout inside the fused GAT attention (gnna_gat.hip): gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32 with a
 * dropout mask on the attention coefficients that is a pure function of (rng_seed, destination row, source row, head).  Every
 * pass computes the mask where it computes alpha: nothing of the size of the edge list is written, saved or read back, and the
 * forward and both passes of the backward see the same bits.
 *
 * The rule.  For an edge i <- j (destination row i, source row j; local ids on a block) and head h, all arithmetic mod 2^64:
 *
 *     u   = (i << 35) | (j << 6) | h          (rows < 2^29 and heads <= 64 are already enforced, so u is unique)
 *     key = splitmix64 finaliser of  z = rng_seed + 0x9E3779B97F4A7C15 * (u + 1)     -- the sampler's key function
 *               z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  key = z ^ (z >> 31)
 *     thr = (uint32) floor((double)attn_drop * 2^32)
 *     kept(i, j, h) = (key >> 32) >= thr
 *     k   = kept ? 1.0f / (1.0f - attn_drop) : 0        (fp32)
 *
 *   Forward: out[i,h,:] = sum_e alpha * k * H[j,h,:].  lse is unchanged; it is the softmax of the undropped scores.
 *   Backward: with c[i,h] = <dY[i,h,:], Y[i,h,:]> and dalpha = <dY[i,h,:], H[j,h,:]>:
 *       dz = alpha * (k * dalpha - c) * (z > 0 ? 1 : slope)
 *       d_el[i,h] = sum_j dz
 *       d_er[j,h] = sum_i dz
 *       dH[j,h,:] = sum_i alpha * k * dY[i,h,:]
 *   A dropped edge still contributes -alpha * c to dz.
 *   (Dropout acts after the softmax, alpha' = alpha * k, so Y = sum alpha' H and sum_e alpha_e dalpha_e = sum_e alpha'_e <dY, H_j>
 *   = <dY, Y>: the per-row constant c of the plain backward stays what it is, computed from the Y the forward returned.)
 *   The key depends on (i, j, h), not on an edge position.  The source-side pass walks the transposed structure, or the graph
 *   itself when it is symmetric, with row j and id i.  It computes the same key with no perm array and no reverse-edge map.
 *   Consequence: duplicate edges (i, j) are kept or dropped together.
 *   attn_drop must lie in [0, 1).  A NaN, a negative value or a value >= 1 gives GNNA_ERR_INVALID_ARGUMENT before any device
 *   work.  attn_drop = 0 keeps everything and equals the plain call.
 *
 * Rectangular form only.  The square case is both counts equal; a symmetric undirected graph passes its own structure as the
 * transposed one, as gnna_gat_backward_f32 does internally.  Everything else -- argument meanings, checks, skipping rules,
 * zero-filled outputs and every element written, flags, limits, scratch, GNNA_ERR_UNSUPPORTED under
 * gnna_tuning.deterministic = 1 -- is that of gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32 (gnna.h).  Y is the out of
 * the forward call with the same attn_drop and rng_seed. */
GNNA_API int gnna_gat_forward_drop_f32(const float *H, int64_t ld_h, const float *el, const float *er,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float negative_slope, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize,
        unsigned flags, void *stream);
GNNA_API int gnna_gat_backward_drop_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse,
        const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        int64_t num_parts,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
        int64_t t_num_parts,
        float negative_slope, float attn_drop, uint64_t rng_seed, float *dH, int64_t ld_dh, float *d_el, float *d_er,
        int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_EXT_H_ */

/*
 * gnna_segnorm.h -- per-graph normalisation on a batch of graphs (GraphNorm; with the mean scale fixed at 1, instance
 * normalisation): the centred moments of the rows of every graph from ONE read of the feature matrix, the normalising pass, and
 * the backward pass (gnna_segnorm.hip).
 *
 * Entries of libgnna.so added after gnna_topk.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes, gnna_last_error,
 * streams, scratch) are those of gnna.h.
 *
 * The segments are those of gnna_pool.h: graph_pointers, int32 [num_segments + 1] in DEVICE memory, the rows of graph g are
 * [graph_pointers[g], graph_pointers[g + 1]).  The pointers must not descend; that is not checked on the device.  A segment with
 * p[g + 1] < p[g] is taken as empty, every pointer is clamped to [0, num_rows], and the rows before p[0] or from p[num_segments]
 * on belong to no graph.
 *
 * The function.  Over the rows r of segment g (n rows), per column f, with x = input[r, f], the parameters weight[f], bias[f],
 * alpha[f] (the mean scale) and eps > 0:
 *
 *     mean[g,f] = (1/n) sum_r x
 *     m2[g,f]   = sum_r (x - mean)^2                        centred, >= 0
 *     var[g,f]  = m2 / n + (1 - alpha)^2 mean^2             (= (1/n) sum_r (x - alpha mean)^2)
 *     rstd[g,f] = 1 / sqrt(var + eps)                       IEEE square root and division, once per (g, f)
 *     xhat[r,f] = (x - alpha mean) rstd
 *     out[r,f]  = weight xhat + bias
 *
 * A NULL weight / bias / alpha means 1 / 0 / 1.  An empty segment gets mean = m2 = rstd = 0.  A row of no graph gets out = 0 and
 * d_input = 0.  mean and m2 are never made from raw sums of x and x^2: a lane keeps (count, mean, m2) of the rows it has seen --
 * the rows of a step enter as their own mean and centred sum -- and every meeting of two such states, between the slots of a
 * wavefront, the pieces of a segment and the wavefronts of a workgroup, is the pairwise merge
 *
 *     d = mean_b - mean_a,   mean = mean_a + d n_b / n,   m2 = m2_a + m2_b + d^2 n_a n_b / n,   n = n_a + n_b.
 *
 * With u = 2^-24 max|x| over the segment, |mean - exact| <= 4 u and |m2 / n - exact| <= 1e-5 exact + 4 u sqrt(exact), whatever
 * offset the values sit on.
 *
 * gnna_segment_moments_ld_f32 writes mean and m2.  gnna_segment_norm_ld_f32 runs the same pass, writes mean and rstd -- what the
 * backward needs -- and then reads input once more and writes every element of the `dim` columns of all num_rows rows of `out`
 * once; `out` must not be `input`.  Every element of the `dim` columns of all num_segments rows of the [G, dim] outputs is
 * written; columns from `dim` to a leading dimension are not touched.
 *
 * The backward entry.  With A[g,f] = sum_r d_out and B[g,f] = sum_r d_out xhat over the rows of segment g:
 *
 *     d_input[r,f] = weight rstd ( d_out - xhat B / n - alpha ( A / n - (1 - alpha) mean rstd B / n ) )
 *
 * One pass over d_out and input writes seg_a = A and seg_b = B [G, dim] (always); a second writes every element of d_input once,
 * with no zero-fill before it, unless d_input is NULL (only the parameter gradients are wanted).  Those are [G, dim] arithmetic
 * on the caller's side:
 *
 *     d_bias[f] = sum_g A,   d_weight[f] = sum_g B,   d_alpha[f] = - sum_g mean weight rstd ( A - (1 - alpha) mean rstd B ).
 *
 * How.  The tiles, the search for a tile's first segment, the two open pieces of a tile in library scratch and the join of the
 * pieces in tile order are those of gnna_pool.h (GNNA_POOL_TILE_ROWS rows per wavefront; a segment of more than
 * GNNA_POOL_LONG_STEPS join steps goes to the whole workgroup).  An open piece is kept as (mean, m2); its count follows from the
 * pointers.  The two writing passes walk the same tiles; a lane carries the segment of its row and reloads the segment's
 * constants only when the segment changes.
 *
 * No atomics, one writer per element, the order of every addition and merge fixed by (num_rows, dim, graph_pointers): the same
 * bits on every run, and the three entries are accepted under gnna_tuning.deterministic = 1.  No synchronisation, no read-back: a
 * captured call consists of kernel nodes, and its scratch is its capture's own.
 *
 * Checks, before any device work: unknown flag bits (there are no flags yet), dim >= 1, sizes >= 0, num_segments < 2^29,
 * num_rows < 2^31, strides >= dim and < 2^29 elements, eps finite and > 0, 4-byte alignment, no output that is an input or another
 * output, no null pointer that would be used.
 */
#ifndef GNNA_SEGNORM_H_
#define GNNA_SEGNORM_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_segment_moments_ld_f32(const float *input, int64_t ld_in, int64_t num_rows,
        const int32_t *graph_pointers, int64_t num_segments,
        float *mean, int64_t ld_mean, float *m2, int64_t ld_m2,
        int dim, unsigned flags, void *stream);

GNNA_API int gnna_segment_norm_ld_f32(const float *input, int64_t ld_in, int64_t num_rows,
        const int32_t *graph_pointers, int64_t num_segments,
        const float *weight, const float *bias, const float *alpha, float eps,
        float *out, int64_t ld_out, float *mean, int64_t ld_mean, float *rstd, int64_t ld_rstd,
        int dim, unsigned flags, void *stream);

GNNA_API int gnna_segment_norm_backward_ld_f32(const float *d_out, int64_t ld_do, const float *input, int64_t ld_in,
        const float *mean, int64_t ld_mean, const float *rstd, int64_t ld_rstd,
        const float *weight, const float *alpha,
        const int32_t *graph_pointers, int64_t num_segments,
        float *d_input, int64_t ld_din, float *seg_a, int64_t ld_a, float *seg_b, int64_t ld_b,
        int64_t num_rows, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_SEGNORM_H_ */

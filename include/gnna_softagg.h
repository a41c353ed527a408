/*
 * gnna_softagg.h -- softmax neighbor aggregation with a temperature, per channel, from ONE numerically stable gather, and its
 * backward pass (gnna_softagg.hip): the learnable aggregator of DeeperGCN's GENConv (PyG's aggr.SoftmaxAggregation).
 *
 * Entries of libgnna.so added after gnna_stats.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes,
 * gnna_last_error, streams, scratch) are those of gnna.h.
 *
 * The function.  Over the edges i <- j of destination row i (a duplicate edge counts twice), per channel f, with
 * t = temp[f] (temp[0] when temp_len is 1) and x = input[j, f]:
 *
 *     s        = t * x
 *     lse[i,f] = log sum_j exp(s)                              0 for a row without edges
 *     alpha    = exp(s - lse[i,f])
 *     out[i,f] = sum_j alpha * x
 *     sq[i,f]  = sum_j alpha * x * x                           optional (sq may be NULL): what the gradient of t needs,
 *                                                              dt[f] = sum_i dY[i,f] * (sq[i,f] - out[i,f]^2)
 *
 * t = 0 is the mean, t -> +inf approaches the max, t < 0 is a soft min.  exp is only ever taken of s - m with m a running
 * maximum of s, or of s - lse: no value of t * x overflows as long as it is finite.  NaN or infinite features and a non-finite
 * temperature give whatever IEEE arithmetic gives; that behaviour is not pinned.  `temp` is a DEVICE pointer and is not inspected.
 *
 * The backward entry computes, over the transposed edges j <- i of source row j (A^T as a CSR of num_in_rows rows whose ids are
 * destination rows),
 *
 *     d_input[j,f] = sum_i alpha_ij,f * dY[i,f] * (1 + t * (x[j,f] - Y[i,f])),     alpha_ij,f = exp(t * x[j,f] - lse[i,f])
 *
 * from the forward's `lse` and `out` (Y).  alpha is computed per edge inside the gather; the entry never forms exp(-lse).
 *
 * Both entries walk the rows of a CSR (row_pointers, trusted; no neighbor-group partition).  A column id outside
 * [0, num_in_rows) -- in the transposed structure: outside [0, num_out_rows) -- is skipped in every pass alike.  A row without
 * edges left gets out = lse = sq = 0, a source row without transposed edges d_input = 0.  Every element of the `dim` columns of
 * every row of every non-NULL output is written; columns from `dim` to the leading dimension are not touched.
 * num_in_rows != num_out_rows is the normal rectangular case; any dim >= 1.
 *
 * Checks, before any device work: flags == 0 (GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning here), dim >= 1,
 * sizes >= 0, temp_len 1 or dim, row counts < 2^29, strides >= dim and < 2^29 elements, 4-byte alignment, no output that is an
 * input or another output, no null pointer that would be used.
 *
 * One writer per output element, plain stores, a fixed order of every sum: the same bits on every run, and both entries are
 * accepted under gnna_tuning.deterministic = 1.  No synchronisation, no plan: a captured call consists of kernel nodes.  The
 * backward entry keeps 3 floats per (destination row, channel) in library scratch; no buffer of edge-list size exists.
 */
#ifndef GNNA_SOFTAGG_H_
#define GNNA_SOFTAGG_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_agg_softmax_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const float *temp, int temp_len,
        const int32_t *row_pointers, const int32_t *column_index,
        float *out, int64_t ld_out, float *lse, int64_t ld_lse, float *sq, int64_t ld_sq,
        int64_t num_out_rows, int dim, unsigned flags, void *stream);

GNNA_API int gnna_agg_softmax_backward_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const float *temp, int temp_len,
        const float *lse, int64_t ld_lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *t_row_pointers, const int32_t *t_column_index,
        float *d_input, int64_t ld_din,
        int64_t num_out_rows, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_SOFTAGG_H_ */

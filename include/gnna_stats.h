/*
 * gnna_stats.h -- sum, sum of squares, max and min over a node's neighbours from ONE walk over the ids and ONE load of every
 * source row (gnna_stats.hip): what a layer with several aggregators (PNA: mean, max, min, std) needs of the same X.
 *
 * An entry of libgnna.so added after gnna_gat_edge.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes,
 * gnna_last_error, streams, scratch, the neighbor-group partition) are those of gnna.h.
 *
 * The function.  Over the edges e of row i, with x = input[column_index[e], f]:
 *
 *     sum[i,f]     = sum_e x                                   fp32, in any order
 *     sumsq[i,f]   = sum_e x * x                               fp32, in any order
 *     max_out[i,f], argmax[i,f]                                the bits gnna_agg_reduce_ld_f32(GNNA_REDUCE_MAX, ...) writes:
 *     min_out[i,f], argmin[i,f]                                the same total order on bit patterns, the same tie rule (the
 *                                                              smallest edge position), the same treatment of NaN and -0
 *
 * Any of sum, sumsq, max_out and min_out may be NULL (at least one is not): what is not asked for is not computed when the
 * other member of its pair (sum / sumsq, max / min) is not asked for either.  argmax / argmin may be NULL; one that is given
 * without its value pointer is GNNA_ERR_INVALID_ARGUMENT.
 *
 * Rows without edges, and rows that no group names, get sum = sumsq = max = min = 0 and arg = -1.  Every element of the `dim`
 * columns of all num_out_rows rows of every non-NULL output is written; columns from `dim` to the leading dimension are not
 * touched.  A column id outside [0, num_in_rows) is skipped in every statistic alike.
 *
 * The partition is any that gnna_agg_reduce_ld_f32 takes: rows split over groups and chunks, shuffled groups, groups with
 * part_pointers[p + 1] < part_pointers[p] (taken as empty), num_in_rows != num_out_rows, any dim >= 1.
 *
 * Checks, before any device work: dim >= 1, sizes >= 0, partSize > 0, num_out_rows < 2^29, strides >= dim and < 2^29 elements,
 * flags == 0 (GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning here), 4-byte alignment, no output that is `input` or
 * another output.  sum and sumsq meet through float atomics: under gnna_tuning.deterministic = 1 a call that asks for either is
 * GNNA_ERR_UNSUPPORTED; a call for extrema only runs, and gives the same bits every time.
 *
 * No synchronisation, no plan: a captured call consists of kernel nodes.  The keys of the extrema (num_out_rows * dim 64-bit
 * words per extreme asked for) live in library scratch.
 */
#ifndef GNNA_STATS_H_
#define GNNA_STATS_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_agg_stats_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float *sum, int64_t ld_sum, float *sumsq, int64_t ld_sumsq,
        float *max_out, int64_t ld_max, int32_t *argmax, int64_t ld_argmax,
        float *min_out, int64_t ld_min, int32_t *argmin, int64_t ld_argmin,
        int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_STATS_H_ */

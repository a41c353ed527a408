/*
 * gnna_pool.h -- graph-level readout: sum / mean / max / min over the rows of every graph of a batch, with the rows of the
 * winning elements, from ONE read of the feature matrix, and the backward pass (gnna_pool.hip).
 *
 * Entries of libgnna.so added after gnna_softagg.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes,
 * gnna_last_error, streams, scratch) are those of gnna.h.
 *
 * A batch of graphs is a block-diagonal CSR plus graph_pointers, int32 [num_segments + 1] in DEVICE memory: the rows of graph g
 * are [graph_pointers[g], graph_pointers[g + 1]).  The pointers must not descend; that is not checked on the device.  A segment
 * with p[g + 1] < p[g] is taken as empty, every pointer is clamped to [0, num_rows], and the rows before p[0] or from
 * p[num_segments] on belong to no graph.
 *
 * The function.  Over the rows r of segment g, with x = input[r, f] and count = the rows of the segment:
 *
 *     sum[g,f]                   = sum_r x    in fp32; with GNNA_POOL_MEAN that sum divided by (float)count, one IEEE
 *                                  division; 0 for an empty segment
 *     max_out[g,f], argmax[g,f]  = the largest x and the smallest row r that holds it
 *     min_out[g,f], argmin[g,f]  = the smallest x and the smallest row r that holds it
 *
 * max / min follow gnna_agg_reduce_ld_f32: the same total order on the bit patterns (-0 < +0; a NaN with a clear sign bit is
 * above +inf, one with the sign bit set below -inf), ties go to the smallest row, an empty segment gives the value 0 and the
 * arg -1.  Any of sum, max_out, min_out may be NULL, at least one is not; an arg pointer needs its value pointer.  Every element
 * of the `dim` columns of all num_segments rows of every non-NULL output is written; columns from `dim` to the leading
 * dimension are not touched.
 *
 * The backward entry writes every element of the `dim` columns of all num_rows rows of d_input exactly once, with no zero-fill
 * before it.  For a row r of segment g
 *
 *     d_input[r,f] = s * d_sum[g,f] + (argmax[g,f] == r ? d_max[g,f] : 0) + (argmin[g,f] == r ? d_min[g,f] : 0)
 *
 * with s = 1, or 1 / (float)count under GNNA_POOL_MEAN, the terms added in this order in fp32; a NULL d_sum / d_max / d_min
 * leaves its term out (d_max comes with argmax, d_min with argmin), and at least one is given.  A row of no graph gets 0.
 *
 * How.  The work is split by rows, not by segments: the host does not know the segment sizes, and the launch geometry depends on
 * num_rows, num_segments and dim alone.  A wavefront owns GNNA_POOL_TILE_ROWS consecutive rows, finds the segment of its first
 * row by binary search in graph_pointers and walks its rows.  A segment that lies inside one tile is written at once.  The
 * pieces of a segment that crosses a tile's first or last row -- two per tile at most -- go to library scratch (sum, max key and
 * min key per column), and a second kernel with one wavefront per segment (the whole workgroup for a segment of many tiles)
 * joins them in tile order and writes the empty segments.  The backward is one kernel over the same tiles.
 *
 * No atomics, one writer per element, a fixed order of the additions for a given (num_rows, dim, graph_pointers): the same bits
 * on every run, and both entries are accepted under gnna_tuning.deterministic = 1.  No synchronisation, no read-back: a captured
 * call consists of kernel nodes, and its scratch is its capture's own.
 *
 * Checks, before any device work: unknown flag bits, dim >= 1, sizes >= 0, num_segments < 2^29, num_rows < 2^31 (the pointers
 * are int32), strides >= dim and < 2^29 elements, 4-byte alignment, no output that is the input or another output, no null
 * pointer that would be used.
 */
#ifndef GNNA_POOL_H_
#define GNNA_POOL_H_

#include "gnna.h"

/* rows of a tile: the unit the rows are split by (one wavefront walks a tile) */
#define GNNA_POOL_TILE_ROWS 256
/* a segment of more than GNNA_POOL_LONG_STEPS * (64 / lanes per row) tiles is joined by a whole workgroup instead of a wavefront;
 * lanes per row = the smallest power of two >= ceil(dim / 4), 64 at most */
#define GNNA_POOL_LONG_STEPS 16

/* flags of both entries */
#define GNNA_POOL_MEAN 1u      /* sum -> mean; in the backward d_sum counts 1 / count */

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_segment_pool_ld_f32(const float *input, int64_t ld_in, int64_t num_rows,
        const int32_t *graph_pointers, int64_t num_segments,
        float *sum, int64_t ld_sum,
        float *max_out, int64_t ld_max, int32_t *argmax, int64_t ld_argmax,
        float *min_out, int64_t ld_min, int32_t *argmin, int64_t ld_argmin,
        int dim, unsigned flags, void *stream);

GNNA_API int gnna_segment_pool_backward_ld_f32(const float *d_sum, int64_t ld_dsum,
        const float *d_max, int64_t ld_dmax, const int32_t *argmax, int64_t ld_argmax,
        const float *d_min, int64_t ld_dmin, const int32_t *argmin, int64_t ld_argmin,
        const int32_t *graph_pointers, int64_t num_segments,
        float *d_input, int64_t ld_din, int64_t num_rows, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_POOL_H_ */

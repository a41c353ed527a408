/*
 * gnna_attnpool.h -- attention readout: the softmax-weighted sum of the rows of every graph of a batch, with a gate per row or
 * per element, from ONE read of the feature matrix, and the backward pass (gnna_attnpool.hip).
 *
 * Entries of libgnna.so added after gnna_pool.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.  Bound
 * through this header's table in _lib.HEADERS.  Conventions (status codes,
 * gnna_last_error, streams, scratch) are those of gnna.h; the segments are those of gnna_pool.h: graph_pointers, int32
 * [num_segments + 1] in DEVICE memory, the rows of graph g are [graph_pointers[g], graph_pointers[g + 1]).  The pointers must not
 * descend; that is not checked on the device.  A segment with p[g + 1] < p[g] is taken as empty, every pointer is clamped to
 * [0, num_rows], and the rows before p[0] or from p[num_segments] on belong to no graph.
 *
 * The function.  gate_dim is 1 (a score per row) or dim (a score per element).  For row r of segment g and column f, with
 * c = 0 when gate_dim == 1 and c = f otherwise, s = gate[r, c] and x = input[r, f]:
 *
 *     lse[g, c] = log sum_r exp(s)                 [num_segments, gate_dim]; 0 for an empty segment
 *     alpha     = exp(s - lse[g, c])
 *     out[g, f] = sum_r alpha * x                  [num_segments, dim];      0 for an empty segment
 *
 * lse may be NULL (the caller wants out only), out may not.  The backward entry takes the forward's lse and out (Y):
 *
 *     d_input[r, f] = alpha * dY[g, f]
 *     d_gate[r, c]  = alpha * dY[g, f] * (x - Y[g, f])                    gate_dim == dim
 *     d_gate[r, 0]  = alpha * sum_f dY[g, f] * (x[r, f] - Y[g, f])        gate_dim == 1
 *
 * A row of no graph gets 0 in both.  Either of d_input and d_gate may be NULL, not both; a NULL output is neither computed nor
 * written.  Every element of the dim (gate_dim) columns of every row of every non-NULL output is written exactly once, columns
 * from there to the leading dimension are not touched, and nothing is zero-filled first.
 *
 * exp is only ever taken of s - m with m a running maximum of the scores met so far, or of s - lse: a finite gate never
 * overflows, and gates near +100 or -100 give what gates near 0 give.  The backward never forms exp(-lse).  Non-finite inputs
 * give whatever IEEE arithmetic gives; that is not pinned.
 *
 * input and gate may be the same pointer (softmax aggregation as a readout: the gate is a view of the features).  An output
 * that is an input or another output is refused.
 *
 * How.  The geometry of gnna_pool.h: a wavefront owns GNNA_POOL_TILE_ROWS consecutive rows, finds the segment of its first row
 * by binary search and walks its rows, 64 / LPR rows at a time with LPR = next_pow2(ceil(dim / 4)) lanes per row and 16-byte
 * loads.  A lane keeps the online softmax state of its columns -- the running maximum m, l = sum exp(s - m) and
 * a = sum exp(s - m) * x; with gate_dim == 1 one (m, l) per partial row and one exp per row -- and rescales it once per step of
 * rows in flight.  The partial rows of a wavefront meet by a butterfly of state merges.  A segment inside one tile is written at
 * once (out = a / l, lse = m + log l); the pieces of a segment that crosses a tile's first or last row -- two per tile at most --
 * go to library scratch as (a [dim], m [gate_dim], l [gate_dim]), and a second kernel with one wavefront per segment (the whole
 * workgroup for a segment of more than GNNA_POOL_LONG_STEPS * (64 / LPR) tiles) merges them in tile order and writes the empty
 * segments.  input is read once, and so is gate, in the same walk.  The backward is one kernel over the same tiles: every lane
 * keeps the segment of its row; with gate_dim == 1 the dot product over f is summed over the lanes of the row and over the column
 * blocks of a row wider than 256 before one lane writes d_gate[r].
 *
 * No atomics, one writer per element, every order of additions and of state merges fixed by (num_rows, dim, gate_dim,
 * graph_pointers): the same bits on every run, and both entries are accepted under gnna_tuning.deterministic = 1.  No
 * synchronisation, no read-back: a captured call consists of kernel nodes, and its scratch is its capture's own.
 *
 * Checks, before any device work: flags == 0, dim >= 1, gate_dim 1 or dim, sizes >= 0, num_segments < 2^29, num_rows < 2^31
 * (the pointers are int32), strides >= the width they stride (dim; gate_dim for ld_gate, ld_lse and ld_dgate) and < 2^29
 * elements, 4-byte alignment, no output that is an input or another output, no null pointer that would be used.  The forward
 * with num_segments == 0 and the backward with num_rows == 0 return GNNA_OK without a launch.
 */
#ifndef GNNA_ATTNPOOL_H_
#define GNNA_ATTNPOOL_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_segment_attn_pool_ld_f32(const float *input, int64_t ld_in, int64_t num_rows,
        const float *gate, int64_t ld_gate, int gate_dim,
        const int32_t *graph_pointers, int64_t num_segments,
        float *out, int64_t ld_out, float *lse, int64_t ld_lse,
        int dim, unsigned flags, void *stream);

GNNA_API int gnna_segment_attn_pool_backward_ld_f32(const float *input, int64_t ld_in,
        const float *gate, int64_t ld_gate, int gate_dim,
        const float *lse, int64_t ld_lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *graph_pointers, int64_t num_segments,
        float *d_input, int64_t ld_din, float *d_gate, int64_t ld_dgate,
        int64_t num_rows, int dim, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_ATTNPOOL_H_ */

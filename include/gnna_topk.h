/*
 * gnna_topk.h -- hierarchical pooling on a batch of graphs: the best-scoring rows of every graph are selected on the device and
 * the induced sub-batch (rows, graph pointers, CSR, neighbor-group partition) is cut out in ONE call with one read-back
 * (gnna_segment_topk_i32), and the differentiable part: the scaled gather of the kept rows and its one-pass backward, which is
 * also the unpooling of a Graph U-Net (gnna_gather_rows_scale_ld_f32, gnna_gather_rows_scale_backward_ld_f32).  gnna_topk.hip.
 *
 * Entries of libgnna.so added after gnna_attnpool.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes, gnna_last_error,
 * streams, scratch) are those of gnna.h.
 *
 * ---- gnna_segment_topk_i32 -------------------------------------------------------------------------------------------------
 *
 * Inputs, all in DEVICE memory: score, float [num_rows]; graph_pointers, int32 [num_segments + 1]; optionally the CSR of the
 * batch, row_pointers int32 [num_rows + 1] and column_index int32 [nnz] (both or neither; nnz is the caller's).
 *
 * Segments are those of gnna_pool.h: every pointer is clamped to [0, num_rows], the rows of segment g are [p[g], p[g + 1]), a
 * descending pair is an empty segment, and rows before p[0] or from p[num_segments] on belong to no graph and are dropped.
 *
 * How many rows a segment of n rows keeps (gnna_topk_keep_count states the same rule on the host): exactly one of `ratio` and
 * `k_fixed` is active, the other is 0.
 *     k_fixed >= 1:      k = min(n, k_fixed)
 *     0 < ratio <= 1:    k = min(n, (int64) ceil(ratio * (double) n))       one IEEE double multiplication and one ceil
 *
 * Which rows: the k rows with the largest score in the total order of the neighbor max (gnna_agg_reduce_ld_f32, gnna_pool.h):
 * -0 < +0, a NaN with a clear sign bit is above +inf, one with the sign bit set is below -inf; ties go to the smaller row.  With
 * t the value for which count(> t) < k <= count(>= t): every row above t is kept, and the first k - count(> t) rows equal to t
 * in row order.  The kept rows stay in increasing row order, so the new batch is a filter of the old one: the rows of a graph
 * stay contiguous, column ids keep their relative order, and nothing is sorted.
 *
 * Outputs (device memory, caller-sized):
 *     new_id              int32 [num_rows]           the new row of a kept row, -1 otherwise
 *     perm                int32 [row_capacity]       the old row of every new row; N' entries are written
 *     new_graph_pointers  int32 [num_segments + 1]   new_graph_pointers[g] = the kept rows below (the clamped) p[g]
 *   with a CSR:
 *     new_row_pointers    int32 [row_capacity + 1]   N' + 1 entries
 *     new_column_index    int32 [edge_capacity]      nnz' entries: an edge survives when its row is kept and its column id lies in
 *                                                    [0, num_rows) and is kept; ids are relabelled by new_id; the order inside a
 *                                                    row is that of the input
 *     edge_ids            int32 [edge_capacity]      the position of every surviving edge in column_index; may be NULL
 *   with partSize > 0 (needs the CSR):
 *     partPtr             int32 [part_capacity + 1]  P + 1 entries and
 *     part2Node           int32 [part_capacity]      P entries: what gnna_build_part_device_i32 gives for new_row_pointers
 *     counts[3]           HOST memory: (N', nnz', P); nnz' and P are 0 where they are not asked for
 * N' <= num_rows, nnz' <= nnz and P <= nnz' always hold.  A capacity below its count is GNNA_ERR_INVALID_ARGUMENT; counts[] is
 * set all the same, nothing is written beyond a capacity, and what lies below it is unspecified.
 *
 * Malformed input.  Every index that comes from device memory is clamped or range-checked before it addresses anything.
 *   * graph_pointers: clamped as above.  Pointers that descend and then rise again can name a row twice; a row is then kept when
 *     any segment that holds it selects it, and new_graph_pointers is still "the kept rows below p[g]".
 *   * column ids outside [0, num_rows): those edges are dropped.
 *   * row_pointers that do not start at 0, ascend and end at nnz: GNNA_ERR_INVALID_ARGUMENT after the read-back (the message names
 *     an offending row); the outputs are unspecified, and every access stayed in bounds.
 *
 * The call synchronises the stream once (the read-back of counts) and refuses to run inside a stream capture.  Every position
 * is computed by counts and scans, no global atomic hands one out, the rule above decides the result: the same bits on every
 * run, and the entry is accepted under gnna_tuning.deterministic = 1.
 *
 * How.  The launch geometry depends on num_rows, num_segments and nnz alone.  A selection, not a sort: a radix select of the
 * 32-bit order key, most significant digit first.
 *   1. keep flags: one wavefront per segment of up to GNNA_TOPK_WAVE_ROWS rows holds the keys in registers and finds the k-th
 *      largest bit by bit with ballots and popcounts; a second launch of one workgroup per segment returns at once unless the
 *      segment is longer, and then makes four passes over its scores with a 256-bin LDS histogram (LDS integer atomics).  Both
 *      rank the rows equal to the threshold in row order by ballot prefixes.  One huge segment runs on ONE workgroup.
 *   2. an exclusive scan of the flags, then new_id / perm / new_graph_pointers.
 *   3. with a CSR: a survivor flag per edge (its row by binary search in row_pointers), a scan, and a fill of new_column_index,
 *      edge_ids and new_row_pointers; 4 bytes of library scratch per edge.
 *   4. with partSize > 0: the groups per row, a scan, and the fill of gnna_build_part_device_i32.
 *
 * Checks before any device work: counts not NULL; sizes >= 0; num_rows < 2^31, num_segments < 2^29, nnz < 2^31; exactly one of
 * ratio (in (0, 1], not NaN) and k_fixed (>= 1) -- never both, never neither; capacities >= 0; partSize >= 0; a partition needs
 * the CSR; row_pointers and column_index come together; null pointers that would be used; no output that is an input or another
 * output.
 *
 * ---- gnna_gather_rows_scale_ld_f32 / gnna_gather_rows_scale_backward_ld_f32 ---------------------------------------------------
 *
 * Forward:   out[i, f] = scale[perm[i]] * input[perm[i], f]            i < num_out_rows, f < dim; one fp32 multiplication
 * scale (float [num_in_rows]) may be NULL: a plain gather.  A perm[i] outside [0, num_in_rows) gives a row of zeros.
 *
 * Backward, with j = new_id[r] for r < num_in_rows; the row is kept when 0 <= j < num_out_rows:
 *     d_input[r, f] = scale[r] * d_out[j, f]              kept, else 0        (scale NULL: d_out[j, f])
 *     d_scale[r]    = sum_f d_out[j, f] * input[r, f]     kept, else 0
 * Either output may be NULL, not both; d_scale needs input.  Every element of the dim columns of all rows of every non-NULL
 * output is written exactly once, nothing is zero-filled first, there are no atomics, and the additions of d_scale run in a
 * fixed order (a lane's columns in increasing order, column blocks of 256 in order, then a butterfly over the lanes of the row).
 * With scale == NULL and d_scale == NULL the entry is the unpooling of a Graph U-Net: it places the coarse rows back and writes
 * zeros elsewhere.
 *
 * Both are bandwidth kernels in the lane layout of gnna_pool.h (lanes per row from ceil(dim / 4), 16-byte accesses on 4-byte
 * alignment, row offsets in 64 bits), consist of kernel nodes only (capturable, no read-back), give the same bits on every run
 * and are accepted under gnna_tuning.deterministic = 1.  Columns from dim to the leading dimension are not touched.
 *
 * Checks before any device work: dim >= 1; sizes >= 0; num_in_rows and num_out_rows < 2^31; strides >= dim and < 2^29 elements;
 * 4-byte alignment; no output that is an input or another output; no null pointer that would be used.  The forward with
 * num_out_rows == 0 and the backward with num_in_rows == 0 return GNNA_OK without a launch.
 */
#ifndef GNNA_TOPK_H_
#define GNNA_TOPK_H_

#include "gnna.h"

/* a segment of up to this many rows is selected by one wavefront, a longer one by one workgroup */
#define GNNA_TOPK_WAVE_ROWS 256

#ifdef __cplusplus
extern "C" {
#endif

/* the rows a segment of n rows keeps (the rule above, on the host); -1 for arguments the structure entry refuses */
GNNA_API int64_t gnna_topk_keep_count(int64_t n, double ratio, int64_t k_fixed);

GNNA_API int gnna_segment_topk_i32(const float *score, int64_t num_rows,
        const int32_t *graph_pointers, int64_t num_segments,
        double ratio, int64_t k_fixed,
        const int32_t *row_pointers, const int32_t *column_index, int64_t nnz, int partSize,
        int32_t *new_id, int32_t *perm, int32_t *new_graph_pointers,
        int32_t *new_row_pointers, int32_t *new_column_index, int32_t *edge_ids,
        int32_t *partPtr, int32_t *part2Node,
        int64_t row_capacity, int64_t edge_capacity, int64_t part_capacity,
        int64_t counts[3], void *stream);

GNNA_API int gnna_gather_rows_scale_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const int32_t *perm, const float *scale,
        float *out, int64_t ld_out, int64_t num_out_rows, int dim, void *stream);

GNNA_API int gnna_gather_rows_scale_backward_ld_f32(const float *d_out, int64_t ld_dout, int64_t num_out_rows,
        const int32_t *new_id, const float *input, int64_t ld_in, const float *scale,
        float *d_input, int64_t ld_din, float *d_scale,
        int64_t num_in_rows, int dim, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_TOPK_H_ */

/*
 * gnna_spatial.h -- graph construction from coordinates on a batch of point sets: the radius graph and, with an infinite radius
 * and a cap, the k-nearest-neighbour graph, built on the device as a CSR with its neighbor-group partition (gnna_spatial.hip).
 * It is what a SchNet-style model (edgeconv.CFConv) or a DGCNN-style model needs whenever positions change.
 *
 * Entries of libgnna.so added after gnna_edgefeat.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes, gnna_last_error,
 * streams, scratch) are those of gnna.h.
 *
 * ---- gnna_radius_graph_f32 -------------------------------------------------------------------------------------------------
 * Inputs (device): pos float [num_rows, dim] with row stride ld_pos >= dim, 1 <= dim <= 64; graph_pointers int32
 * [num_segments + 1].  The rule:
 *
 *   Segments are those of gnna_pool.h.  Every pointer is clamped to [0, num_rows].  Segment g is rows [p[g], p[g+1]).
 *   Rows before p[0] or from p[num_segments] on belong to no segment and get an empty row.
 *   Clamped pointers that decrease anywhere are GNNA_ERR_INVALID_ARGUMENT.  The refusal comes after the read-back, and the
 *   message names the first such segment.  Every access stays in bounds, and the outputs are then unspecified.
 *
 *   Distance.  For destination row i and candidate j of the same segment, d2(i,j) = sum over c of (pos[j,c] - pos[i,c])^2.
 *   The sum runs over c = 0 .. dim-1 in that order.
 *   Every subtraction, multiplication and addition is rounded to fp32.  No fused multiply-add is used.
 *   d2(i,j) == d2(j,i) to the bit.
 *   r2 = radius * radius is one fp32 multiplication on the host.
 *   radius must be >= 0 or +inf.  A NaN or negative radius is GNNA_ERR_INVALID_ARGUMENT.
 *
 *   Candidates of row i.  The rows j of its segment with d2(i,j) <= r2 are candidates.  A point exactly at the cutoff is a
 *   neighbour.
 *   A NaN d2 compares false, so that row is not a candidate.
 *   j == i is a candidate only if loop != 0.  Its d2 is +0 unless the row holds NaN or inf; then it is NaN and the row is not
 *   its own neighbour.
 *   Coincident distinct points are neighbours at d2 = 0.
 *
 *   Cap on neighbours.  max_neighbors = 0 keeps every candidate.
 *   1 <= max_neighbors <= 64 keeps the max_neighbors candidates with the smallest key.
 *   The key is (uint64(bits(d2)) << 32) | uint32(j).  d2 is non-negative and not NaN here, so its bits order as its value.
 *   Ties in distance go to the smaller row id.
 *   A value outside [0, 64] is GNNA_ERR_INVALID_ARGUMENT.
 *   radius = +inf with a cap is a k-nearest-neighbour graph.
 *
 *   Order and outputs (device).  The kept neighbours of a row are stored in increasing j.  Nothing is sorted.
 *   row_pointers: [num_rows + 1].
 *   column_index: [edge_capacity], global row ids of the batch.  The structure is block-diagonal over the segments.
 *   dist2: [edge_capacity], the d2 bits of every kept pair.  May be NULL.
 *   partPtr [edge_capacity + 1] and part2Node [edge_capacity]: both or neither, with partSize > 0.  They are exactly what
 *   gnna_build_part_i32(partSize, row_pointers, num_rows) writes, including the closing sentinel.
 *
 *   Counts and capacity.  counts (host int64 [3]) is (num_rows, nnz', num_parts).  It is always written once the record is back.
 *   edge_capacity < nnz' is GNNA_ERR_INVALID_ARGUMENT with the needed sizes in counts.
 *   In that case row_pointers is written and nothing else.  Nothing is ever written beyond a capacity.  This is the protocol of
 *   gnna_induced_subgraph_i32.
 *   nnz' is accumulated in 64 bits.
 *   nnz' >= 2^31 is GNNA_ERR_UNSUPPORTED with counts[1] set (row_pointers is then unspecified, counts[2] is 0).
 *
 * Consequence.  With max_neighbors = 0 the structure is symmetric: (i,j) is kept iff (j,i) is, because d2 is symmetric to the bit.
 * With a cap it is in general not symmetric: it is a directed structure in the library's sense (the backward pass of an
 * aggregation over it needs its transpose).
 *
 * Call properties.  It is a prepare-time call: one read-back, one stream synchronisation, GNNA_ERR_UNSUPPORTED inside a capture.
 * Positions come from counts and scans.  No global atomic hands one out (the only atomics are integer sums and maxima into the
 * record).  The result is the same bits on every run and for every launch shape.  It is accepted under
 * gnna_tuning.deterministic = 1.  The scratch slot is its own (8 bytes per row).  num_rows = 0 and num_segments = 0 are fine.
 * Argument checks happen before any device work: non-NULL counts, sizes >= 0, num_rows < 2^31, no output aliasing an input.
 *
 * How.  A count pass, the shared exclusive scan, a fill pass; both passes recompute the distances, and neither keys nor
 * distances are stored anywhere but in dist2.  Rows of a segment of at most GNNA_SPATIAL_LONG_ROWS rows are walked by L = 4 .. 64
 * lanes per row (L from the average segment), many segments to a workgroup: candidates are counted with a ballot and a popcount
 * over the row's lane group and placed by the ballot's prefix.  Rows of a longer segment go to a workgroup per tile of 256
 * destination rows, one row per lane, which stages tiles of GNNA_SPATIAL_SOURCE_TILE / dim source rows in LDS as
 * structure-of-arrays, so that all lanes read the same j as a broadcast.  Under a cap, a row with more candidates than the cap
 * finds its max_neighbors-th smallest key most-significant-bit first over recomputed keys.  Work is brute force inside a segment:
 * O(sum of n_g^2 * dim), times up to 64 under a cap.  One huge point cloud wants a cell grid, which this is not.
 */
#ifndef GNNA_SPATIAL_H_
#define GNNA_SPATIAL_H_

#include "gnna.h"

/* a segment of more rows than this is taken by the tile kernel (one destination row per lane, source tiles in LDS) */
#define GNNA_SPATIAL_LONG_ROWS 256
/* floats of one staged source tile: GNNA_SPATIAL_SOURCE_TILE / dim source rows (256 at the most) */
#define GNNA_SPATIAL_SOURCE_TILE 8192
/* the tile kernel keeps a destination row of up to this many columns in registers; a wider one is re-read from memory */
#define GNNA_SPATIAL_REGISTER_DIM 4
/* the largest dim and the largest max_neighbors */
#define GNNA_SPATIAL_MAX_DIM 64
#define GNNA_SPATIAL_MAX_NEIGHBORS 64

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_radius_graph_f32(const float *pos, int64_t ld_pos, int64_t num_rows, int dim,
        const int32_t *graph_pointers, int64_t num_segments,
        float radius, int max_neighbors, int loop, int partSize,
        int32_t *row_pointers, int32_t *column_index, float *dist2,
        int32_t *partPtr, int32_t *part2Node, int64_t edge_capacity, int64_t counts[3], void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_SPATIAL_H_ */

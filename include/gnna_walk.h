/*
 * gnna_walk.h -- subgraph sampling on one large graph: uniform random walks on the device and the induced subgraph of an arbitrary
 * node set, cut out on the device as a square CSR with its neighbor-group partition (gnna_walk.hip).  Together they are the
 * GraphSAINT random-walk sampler; the second alone takes the node lists of Cluster-GCN partitions and k-hop ego nets.
 *
 * Entries of libgnna.so added after gnna_segnorm.h; gnna.h, the headers before this one and GNNA_VERSION stay as they are.
 * Bound through this header's table in _lib.HEADERS.  Conventions (status codes, gnna_last_error,
 * streams, scratch) are those of gnna.h.
 *
 * The graph is a CSR in DEVICE memory: row_pointers int32 [num_nodes + 1], column_index int32 [nnz].  Neither entry trusts it: a
 * row whose pointers decrease or leave [0, nnz] has no positions, and a column id outside [0, num_nodes) is never followed and
 * never kept.
 *
 * ---- gnna_random_walk_i32: uniform first-order walks -------------------------------------------------------------------------
 * All pointers are device int32: roots [num_roots], walks [num_roots, walk_length + 1], edge_ids [num_roots, walk_length]
 * (may be NULL).  The walk rule:
 *
 *   walks[w, 0] = roots[w].
 *   Step t of walk w stands at v = walks[w, t] with candidate positions [lo, hi) = [rp[v], rp[v+1]) and d = hi - lo.
 *   A row whose pointers decrease, or leave [0, nnz], has d = 0.
 *   If d = 0, the walk stays: walks[w, t+1] = v and edge_ids[w, t] = -1.
 *   Otherwise compute, in uint64 arithmetic:
 *     u = w * walk_length + t
 *     key = key_of_position(rng_seed, u), the splitmix64 finaliser of gnna.h's sampling rule with e = u, all arithmetic mod 2^64:
 *       z = rng_seed + 0x9E3779B97F4A7C15 * (u + 1)
 *       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *       z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *       key = z ^ (z >> 31)
 *     j = floor(key * d / 2^64)      (the high 64 bits of the 128-bit product: __umul64hi(key, d))
 *     e = lo + j and c = column_index[e]
 *   If c is outside [0, num_nodes), the edge is a dead end and is never followed: the walk stays and the edge id is -1.
 *   Else walks[w, t+1] = c and edge_ids[w, t] = e.
 *   A root outside [0, num_nodes) gives a row of -1 in both outputs.
 *
 * The result is a function of (rng_seed, w, t) and the graph only.  It is the same bits on every run and for every launch shape.
 * There are no atomics.  The call reads nothing back, so it does not synchronise, is a kernel node inside a capture, and is
 * accepted under gnna_tuning.deterministic = 1.  It uses no library scratch.  walk_length = 0 and num_roots = 0 are fine.
 * Negative sizes, and null pointers with non-zero sizes, give GNNA_ERR_INVALID_ARGUMENT.  num_roots * (walk_length + 1) < 2^31
 * (else GNNA_ERR_UNSUPPORTED).
 *
 * ---- gnna_induced_subgraph_i32: the subgraph a node list induces -----------------------------------------------------------------
 * nodes int32 [num_ids] (device).  The subgraph rule:
 *
 *   Kept set: S = the distinct values of nodes[0 .. num_ids) that lie in [0, num_nodes), in INCREASING GLOBAL ID.  Duplicates are
 *   expected, because a walk revisits nodes.
 *   A nodes entry of -1 is skipped silently.  It is what a bad root leaves.
 *   Any other nodes id outside the range is GNNA_ERR_INVALID_ARGUMENT, with gnna_last_error() naming the first such index seen.
 *   sub_nodes = S.
 *   new_id[v] = rank of v in S, or -1.
 *   Row a of the result holds the positions e of row S[a] whose column_index[e] is in S, IN INCREASING e:
 *     sub_column_index = the rank of that column;
 *     sub_edge_ids = e.
 *   Column ids outside [0, num_nodes) are dropped.  Duplicate edges and self loops are kept.
 *   A row whose pointers decrease or leave [0, nnz] is empty.
 *   partPtr and part2Node are exactly what gnna_build_part_i32(partSize, sub_row_pointers, |S|) writes, including the closing
 *   sentinel.
 *   counts = (|S|, nnz', num_parts).  It is always written once the record is back.
 *   A capacity that is too small returns GNNA_ERR_INVALID_ARGUMENT with the needed sizes in counts.  Nothing is written beyond a
 *   capacity.  This is the protocol of gnna_sample_neighbors_i32.
 *
 * Outputs (device int32 unless noted): sub_nodes [node_capacity], new_id [num_nodes] (may be NULL), sub_row_pointers
 * [node_capacity + 1], sub_column_index [edge_capacity], sub_edge_ids [edge_capacity] (may be NULL), partPtr [edge_capacity + 1]
 * and part2Node [edge_capacity] (both or neither; partSize > 0 with them), counts HOST int64 [3].  When a capacity is too small
 * the edge arrays and the partition are not written at all; sub_nodes and new_id are, up to their sizes.
 *
 * It is a prepare-time call: it makes one read-back, synchronises the stream, and returns GNNA_ERR_UNSUPPORTED inside a capture.
 * No atomic hands out a position, so the result is the same bits on every run.
 *
 * How.  The kept nodes are marked with plain stores of 1 and the marks are scanned: that gives sub_nodes and a new_id table in
 * library scratch.  A count pass and a fill pass then visit the KEPT ROWS ONLY, L = 4 .. 64 lanes per row (a whole workgroup for a
 * row beyond 2048 positions): column_index is read coalesced, every id is looked up in new_id, the survivors are counted with a
 * ballot and a popcount over the row's lane segment and placed by the ballot's prefix, so position order is kept without a sort.
 * Work is O(num_nodes) for the marks and the scan plus twice the degree sum of the kept rows, never O(nnz).  Scratch (a slot of
 * its own) is 8 bytes per node plus 4 per id.
 */
#ifndef GNNA_WALK_H_
#define GNNA_WALK_H_

#include "gnna.h"

#ifdef __cplusplus
extern "C" {
#endif

GNNA_API int gnna_random_walk_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes, int64_t nnz,
        const int32_t *roots, int64_t num_roots, int walk_length, uint64_t rng_seed,
        int32_t *walks, int32_t *edge_ids, void *stream);

GNNA_API int gnna_induced_subgraph_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes, int64_t nnz,
        const int32_t *nodes, int64_t num_ids, int partSize,
        int32_t *sub_nodes, int32_t *new_id, int32_t *sub_row_pointers, int32_t *sub_column_index, int32_t *sub_edge_ids,
        int32_t *partPtr, int32_t *part2Node, int64_t node_capacity, int64_t edge_capacity, int64_t counts[3], void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GNNA_WALK_H_ */

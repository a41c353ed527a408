/*
 * gnna.h -- C ABI of libgnna.so, the MI355X (gfx950) neighbor-group aggregation runtime.
 *
 * This is the drop-in boundary for GNNAdvisor's aggregation hot path.  Every entry point
 * replaces one symbol the reference's extension binds (paths relative to
 * GNNAdvisor/GNNConv/ in the reference):
 *
 *   gnna_sag_f32            <- SAG_cuda                  GNNAdvisor_kernel.cu:110-184 (+ kernel :186-259)
 *   gnna_agg_gcn_f32        <- the aggregation half of spmm_forward_cuda   .cu:282-322 (+ kernel :324-415)
 *                              and of spmm_backward_cuda                   .cu:436-470 (+ kernel :478-552)
 *   gnna_agg_gin_f32        <- the aggregation half of spmm_forward_cuda_gin  .cu:575-603 (+ kernel :620-689)
 *                              and of spmm_backward_cuda_gin               .cu:712-744 (+ kernel :749-814)
 *   gnna_count_parts /
 *   gnna_build_part_i32     <- build_part                GNNAdvisor.cpp:210-251
 *
 * The dense update (torch::mm at .cu:280,472,473,605,710,711) stays with the caller's
 * BLAS exactly as in the reference; the pybind module `GNNAdvisor` shipped in
 * gnnadvisor_osdi21_amd/csrc/gnna_torch.cpp composes both and re-exports the reference's
 * six Python-visible functions (GNNAdvisor.cpp:253-263) with identical signatures.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / STL types.
 *   - feature matrices: float32, row-major, contiguous, `dim` floats per row
 *     (rows need only 4-byte alignment; 16-byte aligned bases and dim % 4 == 0 take the
 *     vectorised path).
 *   - index arrays: int32 (packed_accessor32<int,1> in the reference).
 *   - all pointers passed to gnna_sag/agg_* are DEVICE pointers; build_part pointers are HOST.
 *   - inputs are borrowed and never written; `out` is fully overwritten (the reference
 *     returns a fresh zeros_like + accumulate, .cu:121).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only
 *     enqueue work.  One exception: the first aggregation on a partition the library has not
 *     seen yet (and that is large enough to be worth slicing) runs a counting pass over the
 *     column ids and synchronises `stream` once to read its statistics; never while the stream
 *     is being captured.  Library scratch (the staged or pre-scaled copy of the gathered rows, the
 *     deterministic schedule's partial rows, the weight-gradient slabs) is allocated on first use:
 *     eager calls share one grow-only buffer per (stream, slot).  A call that is being captured
 *     gets buffers of its own capture instead, keyed by (capture id, stream, slot), allocated with
 *     hipMalloc at capture time (in relaxed capture mode, so a global-mode capture accepts it) and
 *     never freed: each captured graph keeps its scratch -- up to the size of the staged input
 *     matrix per aggregation width, plus the partial rows or slabs -- for the life of the process,
 *     and no eager call and no other capture is ever handed it.  So a path needs no warm-up on the
 *     capture stream (torch.cuda.make_graphed_callables captures with none), and graphs captured on
 *     one stream may be replayed concurrently with each other and with eager calls on that stream.
 *     gnna_runtime_counters_ex [9] counts these allocations.  gnna_prepare_graph() once per graph:
 *     after it no eager aggregation on that graph synchronises, allocates or frees, and a captured
 *     call takes the same schedule as an eager one.  Captured calls also keep a block of per-call
 *     device scratch (step counters, lists) of their own for good; the library holds 160 such
 *     blocks per device -- graphs whose calls were captured after those are used up share a ring
 *     and must not be replayed concurrently with each other.
 *   - return value: GNNA_OK or a negative gnna_status; gnna_last_error() gives the
 *     message for the calling thread.  (The reference printf()s and exit(-1)s on launch
 *     failure, .cu:177-181; this library reports instead.)
 *   - partSize / dimWorker / warpPerBlock keep the reference's argument positions and
 *     are validated (> 0).  On CDNA4 they are scheduling hints: a 64-lane wavefront
 *     always covers the whole feature row, so dimWorker cannot drop dimensions the way
 *     dimWorker < 32 lanes strides them in the reference (.cu:246).
 */
#ifndef GNNA_H_
#define GNNA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNA_VERSION 601 /* 0.6.1: gnna_agg_ld_x16 + gnna_prepare_x16 (bf16 / fp16 storage, fp32 accumulation; GNNA_F32 / GNNA_BF16 / GNNA_F16), gnna_agg_edge_ld_f32 (caller-supplied edge weights), gnna_edge_softmax_f32, gnna_edge_softmax_backward_f32, gnna_reverse_edges_i32; per-capture library scratch, full hashes of a packed copy ordered across streams, gnna_debug_untrusted_copies, counter [9]; 0.6.0: gnna_tuning.ids_check_every (full hash of the ids behind a packed copy), gnna_device_cus, gnna_host_threads; 0.5.0: gnna_tuning opens with struct_size (checked by gnna_set_tuning, which now returns a status), gnna_build_id; 0.4.1: gnna_sddmm_ld_f32 (leading dimensions for both SDDMM sides); 0.4.0: gnna_agg_ld_f32 (leading dimensions, ReLU epilogue), gnna_forget_graph, chunk-walk kernel retired; 0.3.1: gnna_tuning grew (pack_ids); 0.3.0: sweep, sweep_slack, graph lifecycle, 64-bit CSR builder */
#define GNNA_API __attribute__((visibility("default")))

typedef enum gnna_status {
    GNNA_OK = 0,
    GNNA_ERR_INVALID_ARGUMENT = -1,
    GNNA_ERR_HIP = -2,
    GNNA_ERR_UNSUPPORTED = -3
} gnna_status;

GNNA_API int gnna_version(void);
/* "<major>.<minor>.<patch>+<16 hex digits>": the digits are the SHA-256 prefix of the library's sources (every file of
 * csrc/ and include/ that goes into libgnna.so and the GNNAdvisor module) as the build script hashed them -- a run can
 * prove that the binary it loaded was built from the sources beside it (gnnadvisor_osdi21_amd/build.py: source_hash). */
GNNA_API const char *gnna_build_id(void);
GNNA_API const char *gnna_last_error(void);

/* What the planners size their work for (param.py:4-164 reads the SM count and shared memory of "a GPU" from constants;
 * here the Decider asks): compute units of the calling thread's current device (256 on MI355X; 0 when no device is visible --
 * never an error) and the host threads the native builders / the renumbering may use (the CPUs this process is allowed:
 * affinity mask, cgroup quota on the way up from its own cgroup, GNNA_HOST_THREADS overrides; at most 64). */
GNNA_API int gnna_device_cus(void);
GNNA_API int gnna_host_threads(void);

/* ---- partitioner (host) --------------------------------------------------------------
 * Neighbor-group partition of a CSR: row i with degree d_i yields ceil(d_i / partSize)
 * groups of at most partSize consecutive neighbors; group p covers edge offsets
 * [partPtr[p], partPtr[p+1]) and belongs to row part2Node[p].
 * Replaces build_part (GNNAdvisor.cpp:210-251).  Deliberate divergences:
 * exact int32 storage instead of float32, and partPtr[P] = indptr[N] is always written.
 */
GNNA_API int64_t gnna_count_parts(int partSize, const int32_t *indptr, int64_t num_nodes);
GNNA_API int gnna_build_part_i32(int partSize, const int32_t *indptr, int64_t num_nodes,
                        int32_t *partPtr /* [num_parts + 1] */,
                        int32_t *part2Node /* [num_parts] */, int64_t num_parts);

/* ---- structure builders (device; gnna_transpose.hip) -----------------------------------
 * What a backward pass on a DIRECTED graph needs -- the transposed CSR, its partition and the edge permutation -- built on the
 * device from device arrays; nothing is copied to the host but one count per call.  All pointers are DEVICE pointers.  They are
 * prepare-time calls: each reads a count back and so SYNCHRONISES `stream`, and inside a stream capture each returns
 * GNNA_ERR_UNSUPPORTED.  Scratch is library scratch in a slot of their own (grow-only, per stream, like every other).
 *
 * gnna_transpose_csr_i32: the CSR of A^T for the CSR of a rectangular A [num_out_rows x num_in_rows] (the two may differ).
 *   Row j of the result lists the destination rows i of the edges i <- j, in increasing position e of the edge in column_index
 *   (a STABLE order), and t_perm[p] is that position: t_perm = numpy.argsort(column_index, kind="stable") and
 *   t_column_index = the row of every edge, in that order.  The same bits on every run and for every launch shape (a stable
 *   radix sort over the ids: integer counts, no position is handed out by an atomic).  Rows need not be sorted; duplicates and
 *   self loops are kept as they are.  Column ids outside [0, num_in_rows) are DROPPED, as every gather skips them:
 *   t_row_pointers[num_in_rows] is the number of edges kept, and t_column_index / t_perm are -1 from there to nnz =
 *   row_pointers[num_out_rows] (the count that is read back).  t_perm may be NULL.  nnz = 0 and num_out_rows = 0 are fine
 *   (t_row_pointers is all zeros).  row_pointers must start at 0 and not decrease (not checked).  Fewer than 2^31 - 1 rows on
 *   either side.  Scratch: 8 bytes per edge (12 without t_perm) + 1 KiB per 4,096 edges.
 * gnna_count_parts_device_i32 / gnna_build_part_device_i32: gnna_count_parts / gnna_build_part_i32 for DEVICE row pointers and
 *   device outputs -- the same part_pointers and part2Node, element for element, closing sentinel included.  The count call
 *   reads its result back (it synchronises); the build call counts again to check num_parts (it synchronises too) and writes
 *   nothing when num_parts is not the count.  A row whose pointers decrease counts as empty (the host call refuses it). */
GNNA_API int gnna_transpose_csr_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_out_rows,
        int64_t num_in_rows, int32_t *t_row_pointers /* [num_in_rows + 1] */, int32_t *t_column_index /* [nnz] */,
        int32_t *t_perm /* [nnz], may be NULL */, void *stream);
GNNA_API int64_t gnna_count_parts_device_i32(int partSize, const int32_t *indptr, int64_t num_nodes, void *stream);
GNNA_API int gnna_build_part_device_i32(int partSize, const int32_t *indptr, int64_t num_nodes,
        int32_t *partPtr /* [num_parts + 1] */, int32_t *part2Node /* [num_parts] */, int64_t num_parts, void *stream);

/* ---- neighbor sampling (device; gnna_sample.hip) -----------------------------------------
 * gnna_sample_neighbors_i32 builds one mini-batch BLOCK: the sampled edges of `num_seeds` destination rows as a rectangular
 * CSR [num_seeds x num_src] over LOCAL source ids, the global id of every local source, and (optionally) the neighbor-group
 * partition of the block -- what gnna_agg_ld_f32 / gnna_agg_reduce_ld_f32 / gnna_scatter_arg_ld_f32 take with
 * num_out_rows = num_seeds and num_in_rows = num_src.  All pointers are DEVICE pointers except `counts`.  A prepare-time call
 * like the structure builders above: ONE record (counts and an error word) is read back per call, which SYNCHRONISES `stream`
 * once, and inside a stream capture the call returns GNNA_ERR_UNSUPPORTED.
 *
 * The sampling rule.
 *   Destination row i of the block is node r = seeds[i].
 *   Its candidate edges are the positions e in [row_pointers[r], row_pointers[r+1]).  Let d be their number.
 *   If fanout <= 0 or d <= fanout, all of them are taken.
 *   Otherwise the `fanout` positions with the smallest 64-bit key are taken, and a tie goes to the smaller e.
 *   The key of position e is the splitmix64 finaliser, with all arithmetic mod 2^64:
 *     z = rng_seed + 0x9E3779B97F4A7C15 * (e + 1)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     key = z ^ (z >> 31)
 *   The taken positions are written in increasing e.
 *   Random priorities give a uniform sample without replacement.
 *   The result depends on nothing but (rng_seed, e).  It is the same bits for every launch shape and run.  No atomic ever
 *   hands out a position.
 *
 * Local ids.
 *   Local ids 0 .. num_seeds-1 are the seeds, in the order given: src_nodes[i] = seeds[i].  The destination features of a block
 *   are therefore the first num_seeds rows of its source features.
 *   Every other sampled source id gets a local id from num_seeds upwards, in increasing global id.
 *   blk_column_index[p] is the local id of column_index[blk_edge_ids[p]].
 *   Duplicate edges and self loops are kept as they are.
 *
 * Partition.  When partPtr and part2Node are given, they hold exactly what gnna_build_part_i32(partSize, blk_row_pointers,
 *   num_seeds) writes, closing sentinel included (num_parts <= nnz of the block, so edge_capacity bounds both).
 *
 * counts (HOST, always written once the record is back): nnz of the block, num_src, num_parts (0 without a partition).
 * Errors found on the device, returned as GNNA_ERR_INVALID_ARGUMENT with gnna_last_error() naming the cause: a seed outside
 *   [0, num_nodes); a duplicate seed; a selected column id outside [0, num_nodes); a capacity that is too small -- then `counts`
 *   still holds the needed sizes and the outputs are unspecified (nothing is written beyond a capacity).
 * partSize <= 0 together with partition outputs, and negative sizes: GNNA_ERR_INVALID_ARGUMENT.  num_seeds = 0 is fine.
 *   row_pointers must not decrease along the seeds' rows (a row whose pointers decrease counts as empty).
 * Cost: the relabelling marks and scans one flag per node of the graph, so a call is O(num_nodes) work on top of the seeds'
 *   rows; scratch (library scratch in a slot of its own, grow-only per stream) is 8 bytes per node + 4 per seed. */
GNNA_API int gnna_sample_neighbors_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes,
        const int32_t *seeds, int64_t num_seeds /* distinct ids in [0, num_nodes) */, int fanout /* >= 1; <= 0: every neighbour */,
        uint64_t rng_seed, int partSize, int32_t *blk_row_pointers /* [num_seeds + 1] */,
        int32_t *blk_column_index /* [edge_capacity], LOCAL source ids */,
        int32_t *blk_edge_ids /* [edge_capacity], positions in column_index; may be NULL */,
        int32_t *src_nodes /* [src_capacity], global id of every local source */,
        int32_t *partPtr /* [edge_capacity + 1] */, int32_t *part2Node /* [edge_capacity] */ /* both may be NULL */,
        int64_t edge_capacity, int64_t src_capacity, int64_t counts[3] /* HOST: nnz of the block, num_src, num_parts */,
        void *stream);

/* ---- graph inputs (host) --------------------------------------------------------------
 * Native counterparts of the reference loader's CSR construction
 * (GNNAdvisor/dataset.py:99-122) and of the renumbering hook (rabbit.reorder,
 * rabbit_module/src/reorder.cpp:235-295).  All pointers are HOST pointers.
 */

/* Edge list -> CSR with scipy coo->csr semantics (dataset.py:108-118): duplicate edges
 * merged, column indices sorted per row.  column_index must have room for num_edges
 * entries; the return value is nnz (>= 0) or a negative gnna_status. */
GNNA_API int64_t gnna_csr_from_edges_i32(const int32_t *src, const int32_t *dst, int64_t num_edges,
                                int64_t num_nodes, int32_t *row_pointers /* [num_nodes + 1] */,
                                int32_t *column_index /* [num_edges] */);

/* Sharded ingestion (multi-GPU, SURVEY 8e "index width"; extends dataset.py:99-122, which builds one int32 CSR):
 * the edge LIST may hold more than 2^31 entries (papers100M symmetrised: 3.2e9) and is counted with 64-bit
 * arithmetic; every rank then builds only the CSR rows of its own destination range, whose edge count must fit
 * int32 (GNNA_ERR_UNSUPPORTED otherwise: use more ranks).
 *   gnna_row_counts_i64: counts[r] += number of list entries with rows[e] == r (accumulates, so a list can be fed
 *     in pieces; raw entries -- duplicates are merged later, per shard);
 *   gnna_row_splits_i64: global 64-bit row pointers of those counts (row_pointers may be NULL) and `world` + 1
 *     row bounds that cut the rows into contiguous blocks of about equal edge count;
 *   gnna_csr_from_edges_range_i32: the CSR of rows [row_lo, row_hi) only -- local int32 row_pointers
 *     [row_hi - row_lo + 1] rebased to 0, GLOBAL column ids, duplicates merged, columns sorted per row (the
 *     semantics of gnna_csr_from_edges_i32); returns the shard's nnz (<= capacity) or a negative gnna_status. */
GNNA_API int gnna_row_counts_i64(const int32_t *rows, int64_t num_edges, int64_t num_nodes, int64_t *counts /* [num_nodes] */);
GNNA_API int gnna_row_splits_i64(const int64_t *counts, int64_t num_nodes, int world, int64_t *bounds /* [world + 1] */,
                                 int64_t *row_pointers /* [num_nodes + 1] or NULL */);
GNNA_API int64_t gnna_csr_from_edges_range_i32(const int32_t *src, const int32_t *dst, int64_t num_edges,
                                               int64_t num_nodes, int64_t row_lo, int64_t row_hi,
                                               int32_t *row_pointers, int32_t *column_index, int64_t capacity);

/* degrees[i] = sqrt(max(row_pointers[i+1] - row_pointers[i], 1))  (dataset.py:11-18,121-122) */
GNNA_API int gnna_degrees_f32(const int32_t *row_pointers, int64_t num_nodes, float *degrees);

/* avg_edge_span = mean |src - dst| over the raw edge list (dataset.py:100; Decider input) */
GNNA_API int gnna_edge_span(const int32_t *src, const int32_t *dst, int64_t num_edges, double *avg_edge_span);

/* Locality renumbering: writes new_id[old_id] (a permutation of 0..num_nodes-1) computed by
 * a deterministic reverse Cuthill-McKee sweep over the symmetrised graph (components in
 * order of their lowest-degree seed).  Same role as rabbit.reorder -- shrink the average
 * edge span -- but a different, single-threaded, reproducible algorithm. */
GNNA_API int gnna_reorder_rcm_i32(const int32_t *src, const int32_t *dst, int64_t num_edges,
                         int64_t num_nodes, int32_t *new_id /* [num_nodes] */);

/* Locality renumbering by communities: writes new_id[old_id] (a permutation).  On the symmetrised graph
 * (multi-threaded, deterministic): the triangle-supported backbone of the graph (edges whose end points share
 * neighbours), a breadth-first order over it in which a node is discovered once several of its backbone neighbours
 * have been walked (unfolded when the walk runs on two fronts), then median sweeps -- the role of rabbit.reorder
 * (community-based Rabbit Order, rabbit_module/src/reorder.cpp:235-295) with a different, reproducible algorithm
 * (gnna_reorder.cpp).  Node ids are int32; the edge list may hold any number of entries (64-bit
 * offsets inside: papers100M symmetrised has 3.2e9). */
GNNA_API int gnna_reorder_community_i32(const int32_t *src, const int32_t *dst, int64_t num_edges,
                               int64_t num_nodes, int32_t *new_id /* [num_nodes] */);

/* The same renumbering from the loader's CSR (sorted, duplicate-free rows; checked): a symmetric CSR is used as the adjacency
 * as it stands -- no second counting sort (1.2 of 4.6 s at 1.1e8 edges); a directed one goes through the edge-list form.
 * The permutation is the one gnna_reorder_community_i32 returns for the same graph. */
GNNA_API int gnna_reorder_community_csr_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes,
                                            int32_t *new_id /* [num_nodes] */);

/* Applying a renumbering to what the loader holds (dataset.py:147-172 relabels the edge list, then rebuilds CSR and degrees from
 * it): the edge list in place (+ the new mean |src - dst|, the Decider's statistic), and the relabelled graph's CSR straight from
 * the old CSR -- row new_id[u] = the ids of row u mapped and sorted; no global sort (a permutation keeps rows duplicate-free). */
GNNA_API int gnna_relabel_edges_i32(int32_t *src, int32_t *dst, int64_t num_edges, const int32_t *new_id, int64_t num_nodes,
                                    double *avg_edge_span /* may be NULL */);
GNNA_API int gnna_relabel_csr_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes,
                                  const int32_t *new_id, int32_t *out_row_pointers /* [num_nodes + 1] */,
                                  int32_t *out_column_index /* [nnz] */);

/* ---- aggregation (device) ------------------------------------------------------------
 * out[i, :] = sum over groups p with part2Node[p] == i, over e in [part_pointers[p],
 *             part_pointers[p+1]):  coef(i, column_index[e]) * input[column_index[e], :]
 *   sag : coef = 1
 *   gcn : coef = degrees[i] * degrees[column_index[e]]     (a product, as in the reference)
 *   gin : coef = 1, the row sum is scaled by epsilon
 * row_pointers and (for sag) degrees are accepted for signature parity and unused, as
 * in the reference kernels.
 */
/* Limits of one call (GNNA_ERR_UNSUPPORTED beyond them): fewer than 2^29 destination rows, fewer than 2^31 edges
 * (int32 CSR), source matrices of any size (64-bit row offsets above 4 GiB). */
GNNA_API int gnna_sag_f32(const float *input, const int32_t *row_pointers, const int32_t *column_index,
                 const float *degrees, const int32_t *part_pointers, const int32_t *part2Node,
                 float *out, int64_t num_nodes, int dim, int64_t num_parts,
                 int partSize, int dimWorker, int warpPerBlock, void *stream);

GNNA_API int gnna_agg_gcn_f32(const float *input, const int32_t *row_pointers, const int32_t *column_index,
                     const float *degrees, const int32_t *part_pointers, const int32_t *part2Node,
                     float *out, int64_t num_nodes, int dim, int64_t num_parts,
                     int partSize, int dimWorker, int warpPerBlock, void *stream);

GNNA_API int gnna_agg_gin_f32(const float *input, const int32_t *row_pointers, const int32_t *column_index,
                     float epsilon, const int32_t *part_pointers, const int32_t *part2Node,
                     float *out, int64_t num_nodes, int dim, int64_t num_parts,
                     int partSize, int dimWorker, int warpPerBlock, void *stream);

/* Rectangular form for a destination-range shard (multi-GPU; no counterpart in
 * the single-GPU reference): `out` has num_out_rows rows (the shard's destination nodes),
 * `input` has num_in_rows rows (all source nodes, e.g. the all-gathered feature matrix) and
 * column_index holds ids into `input`.  mode: 0 = sag, 1 = gcn, 2 = gin.  For gcn,
 * degrees_out is indexed by destination row and degrees_in by source row.
 * accumulate != 0 adds into the existing contents of `out` instead of overwriting it (used to
 * aggregate local-source edges while the all-gather of remote features is still in flight,
 * then add the remote-source part).
 */
GNNA_API int gnna_agg_rect_f32(int mode, const float *input, int64_t num_in_rows,
                      const int32_t *column_index, const float *degrees_out, const float *degrees_in,
                      float epsilon, const int32_t *part_pointers, const int32_t *part2Node,
                      float *out, int64_t num_out_rows, int dim, int64_t num_parts, int partSize,
                      int accumulate, void *stream);

/* General form: gnna_agg_rect_f32 with leading dimensions and an epilogue.
 *   ld_in / ld_out: floats between the starts of consecutive rows of `input` / `out` (>= dim; == dim: the contiguous
 *     layout every other entry point assumes -- the reference insists on contiguous tensors, GNNAdvisor.cpp:71-73).
 *     With them a producer can write the layout the gather likes best itself -- rows of 17..64 floats that start at
 *     multiples of 2 x ceil(4 dim / 128) x 128 bytes (stride 64 / 128 / 128 floats for dim 32 / 41 / 64), rows padded
 *     to a 128-byte-line-friendly stride (41 -> 48) -- and the library then gathers from `input` directly instead of
 *     staging a copy per call; a column block of a wider matrix (dim = 64, ld = 256) can be aggregated in place, and
 *     the result can land in a slice of a wider buffer (concatenated layer outputs).
 *   flags: GNNA_ACCUMULATE     add into the existing contents of `out` (the `accumulate` of gnna_agg_rect_f32);
 *          GNNA_EPILOGUE_RELU  out = max(out, 0) after the aggregation (and the accumulate): fused into the store wherever a
 *                              row is written once (sweep kernel, owned rows of a single pass), a small pass over the rows
 *                              that several work items add to otherwise.  Reference call sites: F.relu(conv(...)) after
 *                              every layer, GNNA_main.py:151,166-169.
 * mode, degrees_out / degrees_in, epsilon as for gnna_agg_rect_f32. */
#define GNNA_ACCUMULATE 1u
#define GNNA_EPILOGUE_RELU 2u
GNNA_API int gnna_agg_ld_f32(int mode, const float *input, int64_t ld_in, int64_t num_in_rows,
                      const int32_t *column_index, const float *degrees_out, const float *degrees_in,
                      float epsilon, const int32_t *part_pointers, const int32_t *part2Node,
                      float *out, int64_t ld_out, int64_t num_out_rows, int dim, int64_t num_parts, int partSize,
                      unsigned flags, void *stream);

/* Edge-weighted aggregation: out[i, :] (+)= sum over the neighbor-groups p of row i of sum_{e in p} w[e] * input[column_index[e], :],
 * with `edge_weight` [nnz] indexed like column_index (attention coefficients, learned edge weights, a normalised adjacency).
 * Arguments, limits, flags (GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU), leading dimensions and the prepared-graph contract are those
 * of gnna_agg_ld_f32: on a graph prepared for `dim` the call neither synchronises nor allocates.  A column-blocked call applies
 * the same weights to every block.  Runs on the streaming kernel (never the sweep kernel), per-edge like MODE_GCN.
 * Backward on a graph whose structure is symmetric: dX = the same call on dY with the weights w[rev] (gnna_reverse_edges_i32),
 * dw = gnna_sddmm_ld_f32(dY, X). */
GNNA_API int gnna_agg_edge_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows,
        const int32_t *column_index, const float *edge_weight /* [nnz], indexed like column_index */,
        const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out,
        int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags, void *stream);

/* 16-bit storage, fp32 arithmetic: gnna_agg_ld_f32 over features STORED as bfloat16 or IEEE half and ACCUMULATED in fp32.
 *   in_type:  GNNA_BF16 or GNNA_F16 -- the element type of `input`;
 *   out_type: GNNA_F32 (`out` is float) or in_type (`out` has the input's type); anything else: GNNA_ERR_INVALID_ARGUMENT;
 *   ld_in / ld_out: ELEMENTS between the starts of consecutive rows (>= dim).  Source rows that can be read 16 bytes at a time
 *     -- base 16-byte aligned, ld_in and dim multiples of 8 -- are gathered in place; any other layout (dim 1, 3, 7, 41, 100 ...)
 *     is first copied into library scratch with the width padded to a multiple of 8;
 *   degrees_out / degrees_in / epsilon: fp32, as for gnna_agg_ld_f32.  GCN is deg_out[i] * sum_j deg_in[j] * float(x[j]): every
 *     product and every sum is fp32 and the library never makes a pre-scaled 16-bit copy of `input`;
 *   a 16-bit output element is rounded exactly once, to nearest-even, after its whole sum (row factor and ReLU included) is
 *     known: the sums meet in fp32 library scratch (num_out_rows x dim floats; a captured call gets its capture's own) and a small
 *     epilogue converts them.  fp16 output beyond +-65504 becomes +-inf, as IEEE rounding says -- the GCN coefficients are
 *     products of sqrt-degrees and reach 1e3 - 1e5 on hub rows, so take GNNA_BF16 or GNNA_F32 output for GCN;
 *   flags: GNNA_EPILOGUE_RELU with both output types; GNNA_ACCUMULATE with fp32 output only (GNNA_ERR_UNSUPPORTED with a 16-bit
 *     output: adding into it would round twice).
 * Correct for every partition gnna_agg_ld_f32 accepts (every row is added with float atomics: no validation pass, no plan, no
 * synchronisation).  For the same reason there is no deterministic schedule: with gnna_tuning.deterministic = 1 the call returns
 * GNNA_ERR_UNSUPPORTED.  Limits of one call as for gnna_agg_ld_f32.  Scratch is allocated on first use like every other library
 * scratch; gnna_prepare_x16 sizes it up front for the given widths on `stream` (not inside a capture), after which eager calls
 * of those widths from num_in_rows source rows into num_out_rows destination rows on that stream never allocate or free. */
#define GNNA_F32 0   /* output only */
#define GNNA_BF16 1
#define GNNA_F16 2
GNNA_API int gnna_agg_ld_x16(int mode, int in_type, const void *input, int64_t ld_in, int64_t num_in_rows,
        const int32_t *column_index, const float *degrees_out, const float *degrees_in, float epsilon,
        const int32_t *part_pointers, const int32_t *part2Node,
        void *out, int out_type, int64_t ld_out, int64_t num_out_rows, int dim, int64_t num_parts, int partSize,
        unsigned flags, void *stream);
GNNA_API int gnna_prepare_x16(int64_t num_in_rows, int64_t num_out_rows, const int *dims, int num_dims, void *stream);

/* Element-wise max / min over the neighbours of every destination row, with the edge that supplied each element:
 *   out[i, f] = max (GNNA_REDUCE_MAX) or min (GNNA_REDUCE_MIN) over the edges e of row i of input[column_index[e], f];
 *   arg[i, f] = the position e in column_index that supplied it (arg may be NULL: values only).
 * Values are exact: a max does not round, so `out` is bit-identical to an fp32 reference for every partition, schedule and run.
 * Ties: arg is the SMALLEST edge position among the edges that hold the extreme value -- with a CSR whose column ids are
 *   unique and ascending within a row, also the smallest source id.  arg is therefore reproducible too, for every partition,
 *   and the call works unchanged under gnna_tuning.deterministic = 1.
 * Rows without edges, and rows that no neighbor-group names: out = 0, arg = -1.  Every element of the `dim` columns of out and
 *   arg of all num_out_rows rows is written.
 * Partitions: whatever gnna_agg_ld_f32 accepts -- rows split over many groups, groups in any order, part2Node in any order,
 *   groups with part_pointers[p + 1] < part_pointers[p] taken as empty, column ids outside [0, num_in_rows) skipped.
 *   num_in_rows != num_out_rows, any dim >= 1, leading dimensions (elements between row starts) >= dim on input, out and arg.
 * flags: GNNA_EPILOGUE_RELU gives max(out, 0) and leaves arg as it is; GNNA_ACCUMULATE: GNNA_ERR_UNSUPPORTED.  op other than the
 *   two above, dim < 1, a leading dimension < dim: GNNA_ERR_INVALID_ARGUMENT.
 * NaN and signed zero: elements are compared by the TOTAL order of their bit patterns (IEEE totalOrder), not by `<`:
 *   -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  So max prefers +0 to -0 (min the reverse), a NaN with a clear sign bit wins
 *   every max and loses every min, a NaN with the sign bit set the reverse.  out holds the bits of the selected element
 *   unchanged and arg points at exactly that element.
 * No synchronisation, no plan.  The partial rows of different wavefronts meet in library scratch (num_out_rows x dim 64-bit
 * keys, allocated on first use like every other library scratch; a captured call gets scratch of its capture) through 64-bit
 * integer atomic maxima, and a small epilogue kernel writes out and arg.  Limits of one call as for gnna_agg_ld_f32. */
#define GNNA_REDUCE_MAX 0
#define GNNA_REDUCE_MIN 1
GNNA_API int gnna_agg_reduce_ld_f32(int op, const float *input, int64_t ld_in, int64_t num_in_rows,
        const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float *out, int64_t ld_out, int32_t *arg /* may be NULL */, int64_t ld_arg,
        int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags, void *stream);

/* Backward of the above: grad_in[column_index[arg[i, f]], f] += grad_out[i, f] for every arg[i, f] >= 0 (arg as written by
 * gnna_agg_reduce_ld_f32 over the same column_index; a position whose column id is outside [0, num_in_rows) is skipped).
 * grad_in [num_in_rows, dim] is cleared first unless flags has GNNA_ACCUMULATE.  num_out_rows x dim work, one float atomic per
 * non-negative arg: the sums depend on arrival order, so with gnna_tuning.deterministic = 1 the call returns
 * GNNA_ERR_UNSUPPORTED (as gnna_agg_ld_x16 does).  Makes no assumption about the structure of the graph. */
GNNA_API int gnna_scatter_arg_ld_f32(const float *grad_out, int64_t ld_go, const int32_t *arg, int64_t ld_arg,
        const int32_t *column_index, int64_t num_out_rows, float *grad_in, int64_t ld_gi, int64_t num_in_rows,
        int dim, unsigned flags, void *stream);

/* Edge softmax over the edges of every destination row, per head; scores are head-major [num_heads, num_edges]:
 *   probs[h, e] = exp(s[h, e] - max_row) / sum_row exp(s - max_row),  e in [row_pointers[i], row_pointers[i + 1]).
 * Backward: grad_scores[h, e] = probs[h, e] * (grad_probs[h, e] - sum_row probs * grad_probs).
 * Empty rows write nothing.  No atomics: the same inputs give the same bits whatever the launch order.  Device pointers. */
GNNA_API int gnna_edge_softmax_f32(const float *scores, const int32_t *row_pointers, int64_t num_rows,
        int64_t num_edges, int num_heads, float *probs, void *stream);
GNNA_API int gnna_edge_softmax_backward_f32(const float *probs, const float *grad_probs,
        const int32_t *row_pointers, int64_t num_rows, int64_t num_edges, int num_heads,
        float *grad_scores, void *stream);

/* Fused multi-head GAT attention (gnna_gat.hip): the attention coefficient of an edge i <- j,
 *   alpha(i, j, h) = exp(leaky_relu(el[i, h] + er[j, h], negative_slope) - lse[i, h]),  lse[i, h] = logsumexp over the edges of row i,
 * is computed from node-sized values wherever a pass gathers a row: no buffer of the size of the edge list is read, written or
 * allocated, all heads run in one call and every pass reads column_index once (once per column block of whole heads when
 * heads * dim exceeds one wave-wide load of 256 floats; the lse pass once per 8 heads).
 *   H, out, Y, dY, dH: [num_nodes, heads * dim] fp32 with leading dimensions in floats (>= heads * dim); el, er, lse, d_el, d_er:
 *   contiguous [num_nodes, heads].  Square graph: num_nodes destination = source rows.  The partition arguments are the output of
 *   gnna_build_part_i32 for row_pointers (the lse pass walks the rows, the gathers walk the neighbor-groups); column ids outside
 *   [0, num_nodes) are skipped in every pass alike.
 * forward:  out[i, h dim + f] = sum_{e in row i} alpha(e, h) * H[col(e), h dim + f], and lse.  A row without edges: out = 0, lse = 0.
 *   The row maximum is subtracted before any exponential: finite inputs give finite outputs.  lse is computed without atomics,
 *   by one writer per row in a fixed order: the same bits on every run.  flags: GNNA_EPILOGUE_RELU (out = max(out, 0)).
 * backward (Y = the forward's out, dY = its gradient; the STRUCTURE of the graph must be symmetric -- the edges of row j stand for
 *   the edges j -> i; the caller checks, gnna_reverse_edges_i32 does): with c[i, h] = <dY[i, h, :], Y[i, h, :]> (computed inside
 *   the call, library scratch of num_nodes x heads x 16 bytes), z = el[i, h] + er[j, h], dalpha = <dY[i, h, :], H[j, h, :]> and
 *   dz = alpha * (dalpha - c[i, h]) * (z > 0 ? 1 : negative_slope):
 *     d_el[i, h] = sum_{j in row i} dz,  d_er[j, h] = sum_{i in row j} dz,  dH[j, h, :] = sum_{i in row j} alpha * dY[i, h, :].
 *   dH is the attention part only: the terms through el = <H, a_l> and er = <H, a_r> are the caller's (autograd).  A row without
 *   edges: d_el = d_er = 0, dH = 0.  flags: none.
 * Both: GNNA_ACCUMULATE: GNNA_ERR_UNSUPPORTED.  The gathered rows are added with float atomics (any partition gnna_agg_ld_f32
 *   accepts is correct, no validation pass, no plan, no synchronisation), so with gnna_tuning.deterministic = 1 the calls return
 *   GNNA_ERR_UNSUPPORTED, as gnna_agg_ld_x16 does.  heads <= 64 and dim <= 256 (GNNA_ERR_UNSUPPORTED beyond), otherwise the limits
 *   of gnna_agg_ld_f32.  Bad sizes, null pointers, outputs that alias an input or each other: GNNA_ERR_INVALID_ARGUMENT.  Scratch is
 *   allocated on first use like every other library scratch (a captured call gets its capture's own). */
GNNA_API int gnna_gat_forward_f32(const float *H, int64_t ld_h, const float *el, const float *er,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float negative_slope, float *out, int64_t ld_out, float *lse, int64_t num_nodes, int heads, int dim,
        int64_t num_parts, int partSize, unsigned flags, void *stream);
GNNA_API int gnna_gat_backward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse,
        const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_nodes, int heads, int dim,
        int64_t num_parts, int partSize, unsigned flags, void *stream);
/* gnna_gat_backward_f32 for a DIRECTED graph: the source-side pass (row j gathers dY[i] over the edges j -> i: d_er, dH) walks a
 * second structure, the transposed CSR of the first with its own partition (gnna_transpose_csr_i32 +
 * gnna_build_part_device_i32 at the same partSize; t_row_pointers is not read, like row_pointers); the destination-side pass
 * (d_el) walks the graph itself.  No symmetry is assumed.  gnna_gat_backward_f32 is this call with the same structure given
 * twice.  Everything else as above. */
GNNA_API int gnna_gat_backward_dir_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse,
        const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        int64_t num_parts,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
        int64_t t_num_parts,
        float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_nodes, int heads, int dim,
        int partSize, unsigned flags, void *stream);
/* The fused GAT attention on a RECTANGULAR structure (a sampled block): num_out_rows destination rows gather from num_in_rows
 * source rows.  Formulas, skipping rules, flags, limits (each row count < 2^29), scratch and error rules are those of
 * gnna_gat_forward_f32 / gnna_gat_backward_dir_f32 above; the square entries are these calls with both counts = num_nodes.
 * The differences:
 *   H, dH: [num_in_rows, heads * dim];  er, d_er: [num_in_rows, heads];  out, Y, dY: [num_out_rows, heads * dim];
 *   el, lse, d_el: [num_out_rows, heads] (scratch of the backward: num_out_rows x heads x 16 bytes).
 *   The forward structure (row_pointers, column_index and its partition) has num_out_rows rows and ids in [0, num_in_rows); the
 *   transposed structure has num_in_rows rows and ids in [0, num_out_rows): what gnna_transpose_csr_i32(row_pointers,
 *   column_index, num_out_rows, num_in_rows, ...) and gnna_build_part_device_i32 at the same partSize produce.  The backward
 *   always takes it: a rectangular structure is never its own transpose (null t_ pointers with t_num_parts > 0:
 *   GNNA_ERR_INVALID_ARGUMENT).
 *   An id >= num_in_rows is skipped in the lse pass, the forward pass and the d_el pass; an id >= num_out_rows is skipped in the
 *   source-side pass (d_er, dH); a neighbor-group whose row is outside its side's row count contributes nothing.
 *   Every element of every output is written: rows of dH / d_er that no edge reaches are 0, rows of out / lse / d_el without
 *   edges are 0.  num_out_rows = 0 or num_in_rows = 0: GNNA_OK after zero-filling whatever output has rows (no input is read). */
GNNA_API int gnna_gat_forward_rect_f32(const float *H, int64_t ld_h, const float *el, const float *er,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        float negative_slope, float *out, int64_t ld_out, float *lse,
        int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize,
        unsigned flags, void *stream);
GNNA_API int gnna_gat_backward_rect_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse,
        const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
        const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
        int64_t num_parts,
        const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
        int64_t t_num_parts,
        float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er,
        int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags, void *stream);

/* Relation-typed aggregation (gnna_typed.hip): what an R-GCN layer in basis form, W_r = sum_b C[r, b] V_b, needs around its one
 * GEMM.  Every edge position e (indexed like column_index) has a type edge_type[e] in [0, num_types) and a factor edge_norm[e]
 * (fp32; NULL: 1); coef is the table C [num_types, num_bases], contiguous fp32.  The weight of an edge for basis b,
 * edge_norm[e] * C[edge_type[e], b], is made where the edge's row is gathered: no buffer of the size of the edge list is
 * allocated, read or written by the library, and edge_type is read once per pass (once per column block of 256 floats when
 * dim > 256).  All matrices are fp32 device pointers with leading dimensions in floats; the calls are rectangular
 * (num_in_rows: rows gathered from; num_out_rows: rows of the structure, i.e. the values of part2Node) and take every partition
 * gnna_agg_ld_f32 accepts (rows split over many groups, groups in any order, groups with decreasing pointers taken as empty).
 *   expand:    out[i, b dim + f] = sum_{e in row i} edge_norm[e] C[edge_type[e], b] X[column_index[e], f]
 *              X [num_in_rows, dim] (ld_x >= dim), out [num_out_rows, num_bases * dim] (ld_out >= num_bases * dim).  A source row is
 *              gathered once per edge and feeds the num_bases accumulators of a lane.
 *   contract:  out[i, f] = sum_{e in row i} edge_norm[e] sum_b C[edge_type[e], b] G[column_index[e], b dim + f]
 *              G [num_in_rows, num_bases * dim] (ld_g >= num_bases * dim), out [num_out_rows, dim] (ld_out >= dim).  Runs over whatever
 *              structure it is given: for the backward of expand the caller passes the transposed structure
 *              (gnna_transpose_csr_i32 + gnna_build_part_device_i32) with edge_type / edge_norm permuted by t_perm.
 *   coef grad: dcoef[r, b] = sum_{e: edge_type[e] = r} edge_norm[e] <X[column_index[e], :], G[row(e), b dim : (b + 1) dim]>
 *              over the forward structure; X [num_in_rows, dim], G [num_out_rows, num_bases * dim], dcoef [num_types, num_bases]
 *              contiguous.  Partial sums are kept per workgroup in an LDS table while num_types * (num_bases rounded up to a power
 *              of two) <= 4096 cells, with one float atomic per non-zero cell and workgroup to dcoef; a larger table is added to
 *              dcoef edge by edge.  dcoef is cleared first unless flags has GNNA_ACCUMULATE.
 * An edge whose column id is outside [0, num_in_rows) or whose type is outside [0, num_types) counts for nothing, in all three
 * alike: its row is not read and no entry of coef enters a sum on its behalf (a non-finite row of coef reaches only the edges of
 * that type).  Outputs are zero-filled and rows meet through float atomics: no plan,
 * no validation pass, no synchronisation, no library scratch (the calls work inside a stream capture as they stand) -- and no
 * deterministic schedule: with gnna_tuning.deterministic = 1 the calls return GNNA_ERR_UNSUPPORTED, as gnna_agg_ld_x16 does.
 * Limits (GNNA_ERR_UNSUPPORTED beyond): 1 <= num_bases <= 16, num_types >= 1, any dim >= 1 (dim % 4 != 0 and rows wider than one
 * wave-wide load are handled inside the call), otherwise those of gnna_agg_ld_f32.  flags: GNNA_ACCUMULATE on the coef grad only
 * (expand / contract: GNNA_ERR_UNSUPPORTED, as the GAT entries); GNNA_EPILOGUE_RELU is not accepted.  Sizes < 1 (num_types,
 * num_bases, dim, partSize) or negative, null pointers, a leading dimension below the row width, an output that aliases an input:
 * GNNA_ERR_INVALID_ARGUMENT, before any device work.  The aliasing check compares the output's address with those of the feature
 * matrices, coef and edge_norm, as the neighbouring entries do: ranges that overlap at other addresses, or an output placed over
 * one of the int32 arrays, are the caller's to avoid. */
GNNA_API int gnna_agg_typed_expand_ld_f32(const float *X, int64_t ld_x, int64_t num_in_rows, const int32_t *column_index,
        const int32_t *edge_type, const float *edge_norm, const float *coef, int num_types, int num_bases,
        const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out, int64_t num_out_rows, int dim,
        int64_t num_parts, int partSize, unsigned flags, void *stream);
GNNA_API int gnna_agg_typed_contract_ld_f32(const float *G, int64_t ld_g, int64_t num_in_rows, const int32_t *column_index,
        const int32_t *edge_type, const float *edge_norm, const float *coef, int num_types, int num_bases,
        const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out, int64_t num_out_rows, int dim,
        int64_t num_parts, int partSize, unsigned flags, void *stream);
GNNA_API int gnna_typed_coef_grad_ld_f32(const float *X, int64_t ld_x, int64_t num_in_rows, const float *G, int64_t ld_g,
        int64_t num_out_rows, const int32_t *column_index, const int32_t *edge_type, const float *edge_norm,
        const int32_t *part_pointers, const int32_t *part2Node, float *dcoef, int num_types, int num_bases, int dim,
        int64_t num_parts, int partSize, unsigned flags, void *stream);

/* Reverse-edge map of a CSR whose structure is symmetric (host pointers): rev[e] is the position of the edge col(e) -> row(e)
 * that matches e; the k-th (i, j) of row i pairs with the k-th (j, i) of row j (positions in increasing order), a self loop
 * may pair with itself, rows need not be sorted.  gnna_host_threads() threads; the result does not depend on their number.
 * GNNA_ERR_INVALID_ARGUMENT, naming the first unmatched edge, when the structure is not symmetric. */
GNNA_API int gnna_reverse_edges_i32(const int32_t *row_pointers, const int32_t *column_index,
        int64_t num_nodes, int32_t *rev);

/* The row stride (in floats, >= dim) the library would stage `dim`-float source rows into before gathering them
 * `num_edges` times from `num_in_rows` rows -- dim itself when it would gather from the contiguous layout.  A producer
 * that writes its output with this leading dimension into a buffer aligned to (stride x 4) bytes (torch::mm into
 * buf[:, :dim] of a [N, stride] allocation) and calls gnna_agg_ld_f32 saves the library's staging copy per call. */
GNNA_API int64_t gnna_preferred_ld(int dim, int64_t num_in_rows, int64_t num_edges);

/* Windowed form of gnna_agg_rect_f32, for pipelining the aggregation with a chunked feature
 * exchange (multi-GPU: the all-gather is issued in `num_windows` pieces and each piece is
 * aggregated as soon as it has arrived).  The source rows are cut into `num_windows` (1..16) equal
 * windows of ceil(num_in_rows / num_windows) rows; this call aggregates the edges whose source
 * lies in windows [window_begin, window_end) and must only read those rows of `input`.
 * Contract: the calls of one aggregation cover every window exactly once, in increasing window order, with
 * identical other arguments; the call with window_begin == 0 overwrites `out` unless accumulate != 0, later calls
 * add.  The column ids of every neighbor-group must be in non-decreasing order (the loader's CSR; checked -- once per
 * graph, by the counting pass that builds the per-window counts -- and refused with GNNA_ERR_UNSUPPORTED otherwise:
 * a window call takes the id POSITIONS of its windows, which are its ids only when the ids are sorted).  Stateless
 * between the calls (0.4.0: runs on the streaming kernel; the per-run cursors of the earlier implementation are gone);
 * the first call of a sequence on a graph the library has not seen synchronises the stream once (not inside a stream
 * capture: GNNA_ERR_UNSUPPORTED there -- run the sequence once before capturing it).
 */
GNNA_API int gnna_agg_rect_windows_f32(int mode, const float *input, int64_t num_in_rows,
                      const int32_t *column_index, const float *degrees_out, const float *degrees_in,
                      float epsilon, const int32_t *part_pointers, const int32_t *part2Node,
                      float *out, int64_t num_out_rows, int dim, int64_t num_parts, int partSize,
                      int accumulate, int num_windows, int window_begin, int window_end, void *stream);

/* SDDMM over the same neighbor-group partition -- a build-defined extension: the reference
 * contains no SDDMM kernel, BASELINE.json's north star asks for one.
 *   edge_out[e] = < dst_feat[part2Node[p], :], src_feat[column_index[e], :] >
 * for every group p and every e in [part_pointers[p], part_pointers[p+1]); edge_out is indexed like
 * column_index.  dim >= 4.  Parity is defined by the dense formula only (no reference behaviour).
 */
GNNA_API int gnna_sddmm_f32(const float *dst_feat, const float *src_feat, const int32_t *column_index,
                   const int32_t *part_pointers, const int32_t *part2Node, float *edge_out,
                   int64_t num_out_rows, int64_t num_in_rows, int dim, int64_t num_parts, int partSize,
                   void *stream);

/* The same with leading dimensions (floats, >= dim) for both feature matrices: row r of dst_feat starts at
 * dst_feat + r * ld_dst, row r of src_feat at src_feat + r * ld_src -- a column block of a wider matrix (one attention
 * head of [N, heads * dim]) or the gapped layout gnna_preferred_ld names for the gathered side (src_feat). */
GNNA_API int gnna_sddmm_ld_f32(const float *dst_feat, int64_t ld_dst, const float *src_feat, int64_t ld_src,
                   const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, float *edge_out,
                   int64_t num_out_rows, int64_t num_in_rows, int dim, int64_t num_parts, int partSize,
                   void *stream);

/* Weight gradient of the dense update: dW[K, N] = X^T[K, M] * G[M, N], X = [num_rows, K] and
 * G = [num_rows, N] row-major fp32 (reference: torch::mm(X.transpose(0,1), d_input_prime),
 * GNNAdvisor_kernel.cu:473 and :710).  A reduction over the node dimension on the MFMA units
 * (v_mfma_f32_16x16x4_f32, fp32 in / fp32 accumulate); deterministic (no global atomics).
 * dW is overwritten.  Uses library scratch of the stream (first use allocates).
 */
GNNA_API int gnna_xtg_f32(const float *X, const float *G, float *dW, int64_t num_rows, int K, int N,
                 void *stream);

/* ---- scheduling knobs (not part of the reference API; used by the tuner and bench) ----
 * Any field <= 0 (or < 0 where 0 is meaningful) keeps the built-in choice.
 */
typedef struct gnna_tuning {
    int struct_size;      /* sizeof(gnna_tuning) of the caller's header: gnna_set_tuning refuses any other value (fields came
                             and went between 0.3 and 0.4 without a check; a caller built against another layout now gets
                             GNNA_ERR_INVALID_ARGUMENT instead of silently shifted knobs).  gnna_get_tuning fills it in. */
    int groups_per_chunk; /* neighbor-groups a wavefront walks per work item (1..64)      */
    int loads_in_flight;  /* wave-wide row loads issued before the first add (4, 8, 16)   */
    int blocks_per_cu;    /* sweep kernel only: workgroups per CU (1: one 16-wavefront workgroup with all of the
                             CU's LDS, 2: two); the streaming kernel's grid is hardware scheduled            */
    int xcd_remap;        /* 1: consecutive work items stay on one XCD's L2; 0: off       */
    int trust_canonical;  /* 1: skip the partition validation pass (build_part output)    */
    int column_phases;    /* 1: single pass; 2..32: gather X in that many source-id ranges (cache-resident
                             slices, all in one launch); 0: automatic, from the library's own statistics of
                             the partition */
    int avg_degree;       /* hint: average edges per destination row (0 = unknown)           */
    int nonlocal_ids;     /* hint: 1 = source ids of a row are scattered over the whole id
                             range (no community ordering), 0 = unknown / locality-ordered  */
    int gcn_prescale;     /* gnna_agg_gcn_f32: 1 = scale the source rows by their degree norm
                             once (library workspace) and gather unweighted, 2 = per-edge
                             coefficients as the reference computes them, 0 = automatic
                             (pre-scale when a source row is gathered >= ~32 times)          */
    int pad_rows;         /* 1 = gather from a staged copy of the source rows whose row stride is
                             padded to a 128-byte-line-friendly size when the width calls for
                             it (e.g. 41 -> 48, 56 -> 64 floats), 2 = never, 0 = automatic (when
                             a source row is gathered >= ~32 times; rows of 17..64 floats then start at
                             multiples of twice their 128-byte lines -- stride 64 / 128 / 128 floats for
                             32 / 41 / 64 -- while the copy stays Infinity-Cache sized: 2-6 % off the
                             gather), > 2 = this stride in floats (experiments) */
    int zero_fill;        /* what the prologue clears before a single pass of the streaming kernel that overwrites
                             `out`: 1 = only the rows that pass does not store (rows without edges, rows shared by
                             two work items), 2 = the whole output, 0 = automatic (1 once `out` is >= 32 MiB).
                             Every other schedule adds into `out` and always clears all of it */
    int sweep;            /* destination-blocked sweep kernel (gnna_sweep.hip): persistent wavefronts keep the partial
                             rows of their groups in LDS while every XCD walks the source slices in step, and write
                             each row once.  1 = wherever it applies (sliced schedule, unweighted or pre-scaled gather,
                             rows of >= 4 floats <= 128 wide, source matrix <= 4 GiB), 2 = never, 0 = automatic: where it
                             measures faster than the streaming kernel -- rows of 33..64 floats, a sliced schedule over a
                             square, Infinity-Cache-sized problem, long rows (>= 300 edges on average) and few enough of
                             them that a workgroup's share fits its LDS accumulators in two sets.  While it is selected by 1 two other knobs are read in its terms:
                             blocks_per_cu = workgroups per CU (1: one 16-wavefront workgroup with all of the CU's LDS,
                             else two), groups_per_chunk > 64 = 64 x (sets per workgroup) instead of the automatic count */
    int sweep_slack;      /* sweep kernel: how many slice steps a wavefront may run ahead of the slowest wavefront of
                             its XCD (soft barrier on a per-XCD counter, bounded spin: only locality depends on it).
                             0 = built-in, n > 0 = n steps, >= 1000 = no synchronisation at all */
    int deterministic;    /* 1 = bit-reproducible results of the streaming kernel for a canonical partition: the phases
                             of the sliced schedule run as separate launches in order, a row owned by one work item is
                             read-modify-written, and the partial sums of a row shared between work items are parked in
                             library scratch and added in work-item order by a small second kernel -- no float atomics,
                             so the association order of every output element is fixed.  Costs the per-phase launches
                             and the read-back of the rows; 0 = the default schedule (atomics: reproducible to fp32
                             rounding, exact where the sums are exactly representable) */
    int pack_ids;         /* prepared graphs (gnna_prepare_graph) only: keep, per phase count in use, a copy of the column
                             ids in the order the sliced schedule consumes them, so that a work item reads its ids once
                             and contiguously instead of one cache line per neighbor-group and phase (nnz x 4 bytes per
                             copy, up to 4 copies per graph).  0 = automatic (on for prepared graphs), 2 = off,
                             (every call compares 1024 samples of column_index with the copy's checksum and reads
                             column_index itself on a mismatch: a rewritten buffer is noticed, a few changed ids are not);
                             1 = on for EVERY graph, prepared or not: the caller promises that no column_index is
                             rewritten in place while the library holds a plan for it (the reference's own call sequence
                             never does; without the promise a stale copy would give wrong results, which is why it is
                             not the default) */
    int ids_check_every;  /* packed ids: every n-th aggregation that reads a packed copy also compares a 64-bit hash of ALL of
                             column_index and part_pointers (one read of both: ~0.1 ms per 114 M ids) with the hash taken when the
                             copy was made; on a mismatch that call and every later one read column_index itself (the copy is
                             marked on the device and never trusted again: gnna_forget_graph / gnna_prepare_graph make a new one).
                             Closes what the 2 x 1,024 samples leave open -- a few ids rewritten in place -- within n calls.
                             <= 0 = built-in (64: < 0.2 % of the aggregation time), 1 = every call (GNNA_DEBUG_FULL_CHECKSUM=1 sets it:
                             the test suite), n > 1 = every n-th, >= 2^30 = never.  Not inside a stream capture (samples only there) */
    int wide_blocks;      /* wide rows in 64-float column blocks (one call per block, leading dimensions): 0 = automatic (rows of
                             >= 100 floats of long-row graphs, >= 192 otherwise, when every source row is gathered >= ~32 times
                             and the matrix is Infinity-Cache sized), 1 = whenever dim >= 72, 2 = never */
} gnna_tuning;

GNNA_API int gnna_set_tuning(const gnna_tuning *t); /* NULL restores the defaults; GNNA_ERR_INVALID_ARGUMENT on a struct_size mismatch */
GNNA_API void gnna_get_tuning(gnna_tuning *t);

/* Per-graph form of the two hints: remembers (avg_degree, nonlocal_ids) for the graph whose
 * column_index array starts at this device address; aggregation calls on that array use them
 * instead of the process-wide gnna_tuning values.  avg_degree <= 0 forgets the graph,
 * column_index == NULL forgets all graphs.  At most 64 graphs are remembered (least recently used
 * is replaced).  A stale entry can only cost performance, never correctness. */
GNNA_API int gnna_set_graph_hints(const int32_t *column_index, int avg_degree, int nonlocal_ids);

/* Measured schedule: aggregations of `dim`-wide features on the graph whose column_index array
 * starts at this device address use `column_phases` (1..32) column phases instead of the rule
 * based on the hints; 0 removes the entry.  Up to 8 widths per graph.  An explicit process-wide
 * gnna_tuning.column_phases >= 1 still wins.  (decider.inputProperty.calibrate() measures and
 * registers these.) */
GNNA_API int gnna_set_graph_phases(const int32_t *column_index, int dim, int column_phases);

/* ---- graph lifecycle (optional) ----------------------------------------------------------
 * gnna_prepare_graph does, up front and on `stream`, everything an aggregation call would otherwise do at first
 * sight of a partition: the counting pass over the column ids, the read-back of its statistics (ONE
 * synchronisation of `stream`, here instead of inside the first aggregation), the choice of the phase count for
 * every feature width in dims[0 .. num_dims) (written to phases_out when not NULL) and the sizing of the stream's
 * scratch (row staging for widths that want it).  The plan is pinned: it is not subject to the library's
 * least-recently-used replacement and lives until gnna_release_graph.  After a successful prepare, aggregation
 * calls on (column_index, part_pointers, part2Node) gathering from `num_in_rows` source rows never synchronise,
 * allocate or free, and a call inside a stream capture takes the sliced schedule like an eager call.
 * num_out_rows: destination rows (rows of `out`); partSize as passed to the aggregation calls.
 * All pointers are DEVICE pointers and must stay valid (and unchanged in content) until the release.
 * gnna_release_graph forgets every plan, hint and measured schedule keyed by this column_index address
 * (NULL: all graphs); it waits for the device before freeing. */
GNNA_API int gnna_prepare_graph(const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                                int64_t num_parts, int64_t num_in_rows, int64_t num_out_rows, int partSize,
                                const int *dims, int num_dims, int *phases_out, void *stream);
GNNA_API int gnna_release_graph(const int32_t *column_index);
/* The same for callers that cannot choose their moment -- finalizers, garbage collectors, another thread while a stream is
 * being captured: the graph's plans, hints and schedules are unlinked at once (no later call finds them), but nothing is
 * freed and nothing synchronises here; the device buffers go at the next gnna_prepare_graph / gnna_release_graph, or when
 * the library next allocates a plan, and never while another thread's aggregation call is between looking a plan up
 * and enqueueing its kernels. */
GNNA_API int gnna_forget_graph(const int32_t *column_index);
/* gnna_forget_graph without touching what the CALLER registered for the graph: the plans and packed id copies go (deferred, as
 * above), the hints (gnna_set_graph_hints) and measured schedules (gnna_set_graph_phases) stay.  For a layer that pinned plans
 * on the caller's behalf and has to take them back -- the GNNAdvisor module's automatic lifecycle -- while the graph lives on. */
GNNA_API int gnna_forget_plans(const int32_t *column_index);

/* Events of the library's launch path since load (for tests and monitoring):
 *   [0] counting passes run, [1] stream / device synchronisations inside aggregation calls, [2] hipFree and
 *   [3] hipMalloc inside aggregation calls, [4] counting passes skipped by the back-off for partitions that are
 *   never seen twice, [5] launches of the sweep kernel, [6] packed-id copies built, [7] aggregation launches that
 *   read packed ids. */
GNNA_API void gnna_runtime_counters(int64_t out[8]);
/* The same list, open-ended: fills out[0 .. min(capacity, count)) and returns the number of counters this library keeps.
 *   [8] full hashes of the ids behind a packed copy run at a launch (gnna_tuning.ids_check_every), [9] scratch buffers
 *   allocated for calls that were being captured (kept for good: see "stream" under Conventions). */
GNNA_API int gnna_runtime_counters_ex(int64_t *out, int capacity);
/* For tests: waits for the device, then returns how many packed id copies of the graph whose column_index starts at this
 * device address are marked "never trust again" by a full hash (gnna_tuning.ids_check_every), or a negative gnna_status.
 * The full hashes of one copy run one after the other, whichever streams the calls come from, so only a column_index that
 * really changed marks its copy. */
GNNA_API int gnna_debug_untrusted_copies(const int32_t *column_index);

/* Number of column phases the calling thread's most recent aggregation call used (>= 1). */
GNNA_API int gnna_last_num_phases(void);
/* Number of aggregation-kernel launches that call issued (the sliced schedule of the streaming kernel is one
 * launch whatever its number of phases; the chunk-walk kernel launches once per phase). */
GNNA_API int gnna_last_num_launches(void);

/* ---- kernel timing (HIP events on the caller's stream; used by bench.py) ---------------
 * Between gnna_profile_begin() and gnna_profile_end() every aggregation call records HIP
 * events around its prologue kernel and around its main kernel on the stream it was
 * given.  gnna_profile_end() synchronises those events and returns the average
 * durations in milliseconds over the recorded calls (at most max_calls are recorded).
 */
GNNA_API int gnna_profile_begin(int max_calls);
GNNA_API int gnna_profile_end(double *avg_main_ms, double *avg_prologue_ms, int *num_calls);

#ifdef __cplusplus
}
#endif
#endif /* GNNA_H_ */

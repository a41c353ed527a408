// gnna_walk.hip -- subgraph sampling on one large graph (gnna_walk.h has both rules word for word):
//   gnna_random_walk_i32        uniform first-order walks, one lane per walk; kernel nodes only, no scratch, no read-back
//   gnna_induced_subgraph_i32   the square CSR a node list induces, with its neighbor-group partition; a prepare-time call like
//                               gnna_sample_neighbors_i32: ONE read-back, refuses to run inside a stream capture
//
// The cut, in launch order (rank / new_id / kept are library scratch: 8 bytes per node + 4 per id):
//   clear_kernel        (gnna_transpose.hip) the record and rank[N + 1]
//   mark_kernel         rank[nodes[i]] = 1 (plain stores: equal ids write the same value)
//   scan_* kernels      (gnna_transpose.hip) exclusive scan of the marks = the rank of every kept node in increasing global id
//   ids_kernel          new_id[N] (the table the passes below look ids up in), kept[a] = S[a], sub_nodes, the caller's new_id
//   cut_rows_kernel<0>  count pass over the KEPT rows, L = 4 .. 64 lanes per row: column_index coalesced, every id looked up in
//   cut_long_kernel<0>  new_id, survivors counted by ballot + popcount (a whole block for a row beyond kLongRow positions, up to
//                       64 blocks sharing the long rows of 256 kept rows);
//                       the counts go where the marks were (rank[] is free once ids_kernel has run)
//   scan_* kernels      exclusive scan of the counts = the result's row pointers
//   cut_rows_kernel<1>  fill pass: the same walk, every survivor placed by the ballot's prefix -- position order without a sort.
//   cut_long_kernel<1>  Both return at once when a capacity is too small: nothing is written beyond one
//   part_count_kernel   (gnna_transpose.hip), the scan, part_fill_kernel: the partition of the result's row pointers by the one
//                       rule of gnna_parts.h, as gnna_build_part_i32 writes it (groups per row where kept[] was), sizes read on
//                       the device
// Unlike the edge-parallel cut of gnna_topk.hip (a flag and a binary search per edge of the WHOLE graph) nothing here is O(nnz).
#include <algorithm>

#include "gnna_device.h"
#include "gnna_internal.h"
#include "gnna_parts.h"
#include "gnna_walk.h"

namespace gnna {
namespace {

constexpr int kSlotWalk = 17;         // library scratch: the record, rank[N + 1], new_id[N], kept[M + 1], scan partials
constexpr int kLongRow = 2048;        // rows with more positions get a whole block
// the record that is read back: 4 x int64
enum { REC_NODES = 0, REC_NNZ = 1, REC_PARTS = 2, REC_BAD_ID = 3, REC_WORDS = 4 };

// positions of row v: [*start, *start + d); d = 0 for a row whose pointers decrease or leave [0, nnz]
__device__ __forceinline__ int row_extent(const int32_t *__restrict__ rp, int32_t v, int64_t nnz, int64_t *start)
{
    const int32_t lo = rp[v], hi = rp[v + 1];
    *start = lo;
    return (lo >= 0 && (int64_t)hi <= nnz && hi > lo) ? hi - lo : 0;
}

// ---- walks --------------------------------------------------------------------------------------------------------------------

// One lane per walk: a step needs ONE position of a row (two row pointers, one column id), never a scan of it, so there is
// nothing for further lanes to share.  The steps of a walk depend on each other; the walks of a wavefront do not.
__global__ void __launch_bounds__(kBlock)
walk_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, uint32_t num_nodes, int64_t nnz,
            const int32_t *__restrict__ roots, int64_t num_roots, int walk_length, uint64_t rng_seed, int32_t *__restrict__ walks,
            int32_t *__restrict__ edge_ids)
{
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < num_roots; w += (int64_t)gridDim.x * kBlock) {
        int32_t *row = walks + w * ((int64_t)walk_length + 1);
        int32_t *eid = edge_ids ? edge_ids + w * (int64_t)walk_length : nullptr;
        int32_t v = roots[w];
        if ((uint32_t)v >= num_nodes) {
            for (int t = 0; t <= walk_length; t++) row[t] = -1;
            if (eid)
                for (int t = 0; t < walk_length; t++) eid[t] = -1;
            continue;
        }
        row[0] = v;
        for (int t = 0; t < walk_length; t++) {
            int64_t lo;
            const int d = row_extent(rp, v, nnz, &lo);
            int32_t taken = -1;
            if (d > 0) {
                const uint64_t u = (uint64_t)w * (uint64_t)walk_length + (uint64_t)t;
                const int64_t e = lo + (int64_t)__umul64hi(key_of_position(rng_seed, u), (uint64_t)d);
                const int32_t c = ci[e];
                if ((uint32_t)c < num_nodes) {            // (else a dead end: the walk stays)
                    v = c;
                    taken = (int32_t)e;
                }
            }
            row[t + 1] = v;
            if (eid) eid[t] = taken;
        }
    }
}

// ---- the induced subgraph -----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock)
mark_kernel(const int32_t *__restrict__ nodes, int64_t num_ids, uint32_t num_nodes, int32_t *__restrict__ mark,
            long long *__restrict__ rec)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < num_ids; i += (int64_t)gridDim.x * kBlock) {
        const int32_t v = nodes[i];
        if ((uint32_t)v < num_nodes) mark[v] = 1;
        else if (v != -1) rec[REC_BAD_ID] = i + 1;
    }
}

// rank[v] (the scanned marks) = kept ids below v; rank[v + 1] > rank[v]: v is kept.
__global__ void __launch_bounds__(kBlock)
ids_kernel(const int32_t *__restrict__ rank, int64_t num_nodes, int32_t *__restrict__ new_id, int32_t *__restrict__ new_id_out,
           int32_t *__restrict__ kept, int32_t *__restrict__ sub_nodes, int64_t node_capacity, long long *__restrict__ rec)
{
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (first == 0) rec[REC_NODES] = rank[num_nodes];
    for (int64_t v = first; v < num_nodes; v += (int64_t)gridDim.x * kBlock) {
        const int32_t before = rank[v];
        const bool is_kept = rank[v + 1] > before;
        const int32_t id = is_kept ? before : -1;
        new_id[v] = id;
        if (new_id_out) new_id_out[v] = id;
        if (is_kept) {
            kept[before] = (int32_t)v;
            if (before < node_capacity) sub_nodes[before] = (int32_t)v;
        }
    }
}

struct CutArgs {
    const int32_t *rp, *ci;
    uint32_t num_nodes;
    int64_t nnz;
    const int32_t *kept, *new_id;
    int64_t max_rows;                  // M = min(num_ids, num_nodes) >= |S|: what the grids are sized for
    int32_t *sub_rp;                   // scratch [M + 1]: the count pass writes the counts, the fill pass reads the scanned counts
    int32_t *out_rp, *out_ci, *out_eid;
    int64_t node_capacity, edge_capacity;
    long long *rec;
};

// fill pass: do the results fit?  (uniform over the grid; rec[REC_NODES] was written by ids_kernel, a launch before)
__device__ __forceinline__ bool cut_fits(const CutArgs &a, int64_t num_kept)
{
    return num_kept <= a.node_capacity && (int64_t)a.sub_rp[num_kept] <= a.edge_capacity;
}

// the local id of position e's column, or -1
__device__ __forceinline__ int32_t local_of(const CutArgs &a, int64_t e)
{
    const int32_t c = a.ci[e];
    return (uint32_t)c < a.num_nodes ? a.new_id[c] : -1;
}

__device__ __forceinline__ void emit_edge(const CutArgs &a, int64_t pos, int32_t local, int64_t e)
{
    if ((uint64_t)pos < (uint64_t)a.edge_capacity) {
        a.out_ci[pos] = local;
        if (a.out_eid) a.out_eid[pos] = (int32_t)e;
    }
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// L lanes per row (a power of two, 4 .. 64), 256 / L rows per block, rows 0 .. M.  Every loop bound is uniform over the
// wavefront: all 64 lanes reach every ballot.  FILL = false: sub_rp[i] = survivors of row i (0 from |S| on; a long row is
// cut_long_kernel's).  FILL = true: the survivors, and the caller's row pointers.
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
cut_rows_kernel(const CutArgs a, int L)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int lis = lane & (L - 1);
    const unsigned long long segmask = (L == kWave ? ~0ull : ((1ull << L) - 1ull)) << (lane & ~(L - 1));
    const unsigned long long below = segmask & ((1ull << lane) - 1ull);
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / L;
    const int64_t num_kept = a.rec[REC_NODES];
    if (FILL) {
        if (i == 0 && lis == 0) a.rec[REC_NNZ] = a.sub_rp[num_kept];
        if (!cut_fits(a, num_kept)) return;
    }
    int64_t start = 0, out0 = 0;
    int d = 0;
    bool is_long = false;
    if (i < num_kept) {
        d = row_extent(a.rp, a.kept[i], a.nnz, &start);
        is_long = d > kLongRow;
        if (is_long) d = 0;
    }
    if (FILL && i <= num_kept) {
        out0 = a.sub_rp[i];
        if (lis == 0) a.out_rp[i] = (int32_t)out0;
    }
    const int rounds = wave_max((d + L - 1) / L);
    int written = 0;
    for (int j = 0; j < rounds; j++) {
        const int t = j * L + lis;
        const int32_t local = t < d ? local_of(a, start + t) : -1;
        const unsigned long long picks = __ballot(local >= 0) & segmask;
        if (FILL && local >= 0) emit_edge(a, out0 + written + __popcll(picks & below), local, start + t);
        written += __popcll(picks);
    }
    if (!FILL && lis == 0 && i <= a.max_rows && !is_long) a.sub_rp[i] = written;
}

// `split` blocks look at rows [256 g, 256 g + 256) and share the rows among them that have more than kLongRow positions: block
// (g, s) cuts every split-th of them, one after another with all 256 threads, every wavefront one contiguous quarter of the row.
// (A walk visits nodes in proportion to their degree, so a sampled node set is rich in hubs: one block per 256 rows would leave
// a few thousand kept rows, many of them long, to a few dozen blocks.)
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
cut_long_kernel(const CutArgs a, int split)
{
    __shared__ unsigned long long s_long[kWavesPerBlock];
    __shared__ int s_cnt[kWavesPerBlock];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t num_kept = a.rec[REC_NODES];
    if (FILL && !cut_fits(a, num_kept)) return;
    const int64_t group = blockIdx.x / split;
    const int share = blockIdx.x % split;
    {
        const int64_t i = group * kBlock + tid;
        bool is_long = false;
        if (i < num_kept) {
            int64_t start;
            is_long = row_extent(a.rp, a.kept[i], a.nnz, &start) > kLongRow;
        }
        const unsigned long long mine = __ballot(is_long);
        if (lane == 0) s_long[wave] = mine;
    }
    __syncthreads();
    int ordinal = 0;                                           // (uniform over the block, like everything that steers it)
    for (int w = 0; w < kWavesPerBlock; w++) {
        unsigned long long todo = s_long[w];
        while (todo) {
            const int bitpos = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            if (ordinal++ % split != share) continue;
            const int64_t i = group * kBlock + w * kWave + bitpos;
            int64_t start;
            const int d = row_extent(a.rp, a.kept[i], a.nnz, &start);
            const int chunk = ((d + kBlock - 1) / kBlock) * kWave;
            const int lo = min(d, wave * chunk), hi = min(d, lo + chunk);
            int mine = 0;
            for (int base = lo; base < hi; base += kWave) {
                const int t = base + lane;
                mine += __popcll(__ballot(t < hi && local_of(a, start + t) >= 0));
            }
            __syncthreads();                                   // (the previous readers of s_cnt are done)
            if (lane == 0) s_cnt[wave] = mine;
            __syncthreads();
            if (!FILL) {
                if (tid == 0) a.sub_rp[i] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
                continue;
            }
            int64_t pos = a.sub_rp[i];
#pragma unroll
            for (int v = 0; v < kWavesPerBlock; v++)
                if (v < wave) pos += s_cnt[v];
            for (int base = lo; base < hi; base += kWave) {
                const int t = base + lane;
                const int32_t local = t < hi ? local_of(a, start + t) : -1;
                const unsigned long long picks = __ballot(local >= 0);
                if (local >= 0) emit_edge(a, pos + __popcll(picks & below), local, start + t);
                pos += __popcll(picks);
            }
        }
    }
}
static_assert(kWavesPerBlock == 4, "cut_long_kernel sums four wavefront counts");

// The partition of the result's row pointers (gnna_parts.h), with the number of rows (ids_kernel left it in the record) and of
// groups read on the device.  sub_rp is a scan: sub_rp[0] = 0, so the closing entry is sub_rp[rows] for no rows as well.
__global__ void __launch_bounds__(kBlock)
part_fill_kernel(const int32_t *__restrict__ sub_rp, const int32_t *__restrict__ first_part, int partSize, int64_t node_capacity,
                 int64_t edge_capacity, int32_t *__restrict__ pp, int32_t *__restrict__ p2n, long long *__restrict__ rec)
{
    const CsrRows rows{sub_rp, rec[REC_NODES]};
    const int64_t num_parts = first_part[rows.n];
    if (blockIdx.x == 0 && threadIdx.x == 0) rec[REC_PARTS] = num_parts;
    if (rows.n > node_capacity || (int64_t)sub_rp[rows.n] > edge_capacity) return;           // (groups <= edges: they fit as well)
    fill_parts(rows, first_part, partSize, num_parts, pp, p2n);
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_random_walk_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes, int64_t nnz,
                         const int32_t *roots, int64_t num_roots, int walk_length, uint64_t rng_seed, int32_t *walks,
                         int32_t *edge_ids, void *stream_v)
{
    const char *what = "gnna_random_walk_i32";
    if (num_nodes < 0 || nnz < 0 || num_roots < 0 || walk_length < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_nodes=%lld nnz=%lld num_roots=%lld walk_length=%d)", what,
                    (long long)num_nodes, (long long)nnz, (long long)num_roots, walk_length);
    if ((num_roots > 0 && (!roots || !walks)) || (num_roots > 0 && num_nodes > 0 && !row_pointers) || (nnz > 0 && !column_index))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (num_nodes >= 0x7fffffffLL || nnz > 0x7fffffffLL) return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 rows or 2^31 - 1 edges", what);
    if (num_roots * ((int64_t)walk_length + 1) >= 0x80000000LL)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: num_roots * (walk_length + 1) must stay below 2^31 (got %lld * %lld)", what,
                    (long long)num_roots, (long long)walk_length + 1);
    if (num_roots == 0) return GNNA_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    const int rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    hipLaunchKernelGGL(walk_kernel, dim3(elementwise_grid(num_roots, ds->num_cus, 16)), dim3(kBlock), 0, stream, row_pointers,
                       column_index, (uint32_t)num_nodes, nnz, roots, num_roots, walk_length, rng_seed, walks, edge_ids);
    return launch_ok("%s: launch", what);
}

int gnna_induced_subgraph_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes, int64_t nnz,
                              const int32_t *nodes, int64_t num_ids, int partSize, int32_t *sub_nodes, int32_t *new_id,
                              int32_t *sub_row_pointers, int32_t *sub_column_index, int32_t *sub_edge_ids, int32_t *partPtr,
                              int32_t *part2Node, int64_t node_capacity, int64_t edge_capacity, int64_t counts[3], void *stream_v)
{
    const char *what = "gnna_induced_subgraph_i32";
    if (num_nodes < 0 || nnz < 0 || num_ids < 0 || node_capacity < 0 || edge_capacity < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT,
                    "%s: negative size (num_nodes=%lld nnz=%lld num_ids=%lld node_capacity=%lld edge_capacity=%lld)", what,
                    (long long)num_nodes, (long long)nnz, (long long)num_ids, (long long)node_capacity, (long long)edge_capacity);
    if (!counts || !sub_row_pointers || (num_ids > 0 && !nodes) || (num_nodes > 0 && !row_pointers) || (nnz > 0 && !column_index) ||
        (node_capacity > 0 && !sub_nodes) || (edge_capacity > 0 && !sub_column_index))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((part2Node && !partPtr) || (partPtr && !part2Node && edge_capacity > 0))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partPtr and part2Node come together", what);
    if (partPtr && partSize <= 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must be positive when a partition is asked for (got %d)", what, partSize);
    if (num_nodes >= 0x7fffffffLL || nnz > 0x7fffffffLL || num_ids >= 0x7fffffffLL)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 rows or ids, or 2^31 - 1 edges", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = refuse_capture(what, stream);
    if (rc != GNNA_OK) return rc;
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    node_capacity = std::min<int64_t>(node_capacity, 0x7fffffffLL);       // positions are int32
    edge_capacity = std::min<int64_t>(edge_capacity, 0x7fffffffLL);
    const int64_t M = std::min(num_ids, num_nodes);                       // |S| <= M

    // scratch: [record][rank: N + 1] (cleared together) [new_id: N][kept: M + 1][scan partials]
    Carver c;
    const size_t o_rec = c.add(REC_WORDS * sizeof(long long)), o_rank = c.add((size_t)(num_nodes + 1) * 4), cleared_bytes = c.bytes;
    const size_t o_id = c.add((size_t)num_nodes * 4), o_kept = c.add((size_t)(M + 1) * 4);
    const size_t o_partial = c.add((size_t)scan_tiles(num_nodes + 1) * 4);
    void *ws = nullptr;
    rc = get_workspace(ds, stream, kSlotWalk, c.bytes, &ws);
    if (rc != GNNA_OK) return rc;
    long long *rec = Carver::at<long long>(ws, o_rec);
    int32_t *rank = Carver::at<int32_t>(ws, o_rank);          // marks -> ranks -> the result's row pointers
    int32_t *table = Carver::at<int32_t>(ws, o_id);
    int32_t *kept = Carver::at<int32_t>(ws, o_kept);          // S -> groups before every result row
    int32_t *partial = Carver::at<int32_t>(ws, o_partial);

    const dim3 block(kBlock);
    launch_clear_words(ds, stream, static_cast<int32_t *>(ws), (int64_t)(cleared_bytes / 4));
    hipLaunchKernelGGL(mark_kernel, dim3(elementwise_grid(num_ids, ds->num_cus, 16)), block, 0, stream, nodes, num_ids,
                       (uint32_t)num_nodes, rank, rec);
    rc = launch_exclusive_scan(stream, rank, num_nodes + 1, partial);
    if (rc != GNNA_OK) return rc;
    hipLaunchKernelGGL(ids_kernel, dim3(elementwise_grid(num_nodes, ds->num_cus, 16)), block, 0, stream, rank, num_nodes, table,
                       new_id, kept, sub_nodes, node_capacity, rec);
    // lanes per row from the edges an average row has: the graph's hint, else nnz / num_nodes
    const int L = lanes_per_row(column_index, num_nodes > 0 ? nnz / num_nodes : 0);
    CutArgs a{row_pointers, column_index, (uint32_t)num_nodes, nnz, kept, table, M, rank, sub_row_pointers, sub_column_index,
              sub_edge_ids, node_capacity, edge_capacity, rec};
    const int64_t rows_per_block = kBlock / L;
    // blocks per 256 rows of the long-row kernels: enough to fill the device when the kept rows are few (the results do not
    // depend on it)
    const int64_t groups = (M + kBlock - 1) / kBlock;
    const int split = (int)std::max<int64_t>(1, std::min<int64_t>(64, (int64_t)ds->num_cus * 8 / std::max<int64_t>(groups, 1)));
    const dim3 row_grid((unsigned)((M + 1 + rows_per_block - 1) / rows_per_block)), long_grid((unsigned)(groups * split));
    hipLaunchKernelGGL(cut_rows_kernel<false>, row_grid, block, 0, stream, a, L);
    if (M > 0) hipLaunchKernelGGL(cut_long_kernel<false>, long_grid, block, 0, stream, a, split);
    rc = launch_exclusive_scan(stream, rank, M + 1, partial);
    if (rc != GNNA_OK) return rc;
    hipLaunchKernelGGL(cut_rows_kernel<true>, row_grid, block, 0, stream, a, L);
    if (M > 0) hipLaunchKernelGGL(cut_long_kernel<true>, long_grid, block, 0, stream, a, split);
    if (partPtr) {
        launch_part_count(ds, stream, rank, M, rec + REC_NODES, partSize, kept);
        rc = launch_exclusive_scan(stream, kept, M + 1, partial);
        if (rc != GNNA_OK) return rc;
        hipLaunchKernelGGL(part_fill_kernel, dim3(elementwise_grid(edge_capacity + 1, ds->num_cus, 16)), block, 0, stream, rank,
                           kept, partSize, node_capacity, edge_capacity, partPtr, part2Node, rec);
    }
    long long host[REC_WORDS] = {0};
    rc = read_record(what, stream, rec, host, REC_WORDS);
    if (rc != GNNA_OK) return rc;
    counts[0] = host[REC_NODES];
    counts[1] = host[REC_NNZ];
    counts[2] = partPtr ? host[REC_PARTS] : 0;
    if (host[REC_BAD_ID])
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: nodes[%lld] is outside [0, num_nodes = %lld) and is not -1", what,
                    host[REC_BAD_ID] - 1, (long long)num_nodes);
    if (counts[0] > node_capacity || counts[1] > edge_capacity)
        return fail(GNNA_ERR_INVALID_ARGUMENT,
                    "%s: capacity too small: the subgraph has %lld nodes and %lld edges, node_capacity=%lld edge_capacity=%lld", what,
                    (long long)counts[0], (long long)counts[1], (long long)node_capacity, (long long)edge_capacity);
    return GNNA_OK;
}

#pragma GCC visibility pop
}  // extern "C"

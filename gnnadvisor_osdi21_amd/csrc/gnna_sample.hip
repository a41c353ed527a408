// gnna_sample.hip -- device-side neighbor sampling: gnna_sample_neighbors_i32 builds one mini-batch "block" (the sampled
// edges of a set of seed rows as a rectangular CSR over local source ids, the list of its source nodes and its neighbor-group
// partition) from device arrays, with ONE read-back per call.  A prepare-time call like the builders of gnna_transpose.hip:
// it synchronises the stream and refuses to run inside a stream capture.  DESIGN.md 7f.
//
// The rule (include/gnna.h has it word for word): a row with more than `fanout` candidate positions keeps the `fanout`
// positions whose key = splitmix64(rng_seed, position) is smallest.  Keys are COMPUTED from positions, never loaded or stored.
//   clear_kernel        (gnna_transpose.hip, like every kernel named so below) the record, seedpos[] and mark[]
//   seed_kernel         seedpos[seeds[i]] = i + 1 (plain stores: of two equal seeds one loses, which the sampling kernels see),
//                       blk_row_pointers[i] = min(degree, fanout)
//   scan_* kernels      (gnna_transpose.hip) exclusive scan of those counts = where every row's picks start
//   sample_rows_kernel  one segment of L = 4 .. 64 lanes per row: the fanout-th smallest key by a most-significant-bit-first
//                       search (per bit: ballot + popcount of "agrees with the prefix and has this bit clear", keys recomputed),
//                       then the picks in position order by a ballot prefix; only the picks read column_index.  Marks the
//                       picked global ids that are not seeds in mark[].
//   sample_long_kernel  the same for rows beyond kLongRow positions, a whole block per row (counts through LDS)
//   scan_* kernels      exclusive scan of mark[] = the rank of every non-seed source in increasing global id
//   relabel_kernel      src_nodes, global -> local ids in place, counts
//   part_count_kernel   (gnna_transpose.hip), the scan, part_fill_kernel: the partition of blk_row_pointers by the one rule of
//                       gnna_parts.h, as gnna_build_part_i32 writes it; its size stays on the device
// The splitmix64 finaliser is a bijection and z = rng_seed + odd * (e + 1) is injective in e, so two positions never share a
// key: the tie rule of the contract (the smaller position wins) never has to act, and "key <= the fanout-th smallest key" picks
// exactly `fanout` positions.  No position is handed out by an atomic; the result is the same bits for every launch shape.
#include <algorithm>

#include "gnna_device.h"
#include "gnna_internal.h"
#include "gnna_parts.h"

namespace gnna {
namespace {

constexpr int kSlotSample = 8;        // library scratch: the record, seedpos[N], mark[N + 1], scan partials, parts per row
constexpr int kLongRow = 2048;        // rows with more candidate positions get a whole block
// the record that is read back: 8 x int64
enum { REC_NNZ = 0, REC_SRC = 1, REC_PARTS = 2, REC_BAD_SEED = 3, REC_DUP_SEED = 4, REC_BAD_COLUMN = 5, REC_WORDS = 8 };

// candidate positions of a seed row: [*start, *start + d), d = 0 for a row whose pointers decrease
__device__ __forceinline__ int row_extent(const int32_t *__restrict__ rp, int32_t r, int64_t *start)
{
    const int32_t lo = rp[r], hi = rp[r + 1];
    *start = lo;
    return hi > lo ? hi - lo : 0;
}

__global__ void __launch_bounds__(kBlock)
seed_kernel(const int32_t *__restrict__ rp, uint32_t num_nodes, const int32_t *__restrict__ seeds, int64_t num_seeds, int fanout,
            int32_t *__restrict__ seedpos, int32_t *__restrict__ blk_rp, long long *__restrict__ rec)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= num_seeds; i += (int64_t)gridDim.x * kBlock) {
        int count = 0;
        if (i < num_seeds) {
            const int32_t r = seeds[i];
            if ((uint32_t)r < num_nodes) {
                seedpos[r] = (int32_t)(i + 1);
                int64_t start;
                const int d = row_extent(rp, r, &start);
                count = (fanout <= 0 || d <= fanout) ? d : fanout;
            } else {
                rec[REC_BAD_SEED] = i + 1;
            }
        }
        blk_rp[i] = count;        // (entry num_seeds: 0, which the scan turns into the block's nnz)
    }
}

struct SampleArgs {
    const int32_t *rp, *ci, *seeds;
    uint32_t num_nodes;
    int64_t num_seeds;
    int fanout;
    uint64_t rng_seed;
    const int32_t *seedpos;
    int32_t *mark;
    const int32_t *blk_rp;
    int32_t *blk_ci, *blk_eid;
    int64_t edge_capacity;
    long long *rec;
};

// One picked position e of the block's slot `pos`: the global id for now (relabel_kernel translates it in place).
__device__ __forceinline__ void emit_pick(const SampleArgs &a, int64_t pos, int64_t e)
{
    const int32_t c = a.ci[e];
    if ((uint64_t)pos < (uint64_t)a.edge_capacity) {       // (beyond it the call fails with "capacity too small" -- but still
        a.blk_ci[pos] = c;                                 // counts the sources the block needs)
        if (a.blk_eid) a.blk_eid[pos] = (int32_t)e;
    }
    if ((uint32_t)c < a.num_nodes) {
        if (a.seedpos[c] == 0) a.mark[c] = 1;
    } else {
        a.rec[REC_BAD_COLUMN] = e + 1;
    }
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// L lanes per row (a power of two, 4 .. 64), 256 / L rows per block.  Every loop bound is uniform over the wavefront: all 64
// lanes reach every ballot.
__global__ void __launch_bounds__(kBlock)
sample_rows_kernel(const SampleArgs a, int L)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int lis = lane & (L - 1);
    const unsigned long long segmask = (L == kWave ? ~0ull : ((1ull << L) - 1ull)) << (lane & ~(L - 1));
    const unsigned long long below = segmask & ((1ull << lane) - 1ull);
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / L;
    int64_t start = 0, out0 = 0;
    int d = 0;
    if (i < a.num_seeds) {
        const int32_t r = a.seeds[i];
        if ((uint32_t)r < a.num_nodes) {
            if (lis == 0 && a.seedpos[r] != (int32_t)(i + 1)) a.rec[REC_DUP_SEED] = i + 1;
            d = row_extent(a.rp, r, &start);
            out0 = a.blk_rp[i];
            if (d > kLongRow) d = 0;                          // sample_long_kernel's
        }
    }
    const bool select = a.fanout > 0 && d > a.fanout;
    // the fanout-th smallest key of the row: after bit b, `m` keys agree with `prefix` on bits 63 .. b and the wanted key is
    // the k-th smallest of them; m == 1: it is found, and the picks are the keys with (key >> b) <= (prefix >> b)
    uint64_t prefix = 0;
    int k = a.fanout, m = select ? d : 0, sh = 0;
    const int rounds_sel = wave_max(select ? (d + L - 1) / L : 0);
    for (int b = 63; b >= 0; b--) {
        const bool act = m > 1;
        if (!__any(act)) break;
        int c0 = 0;
        for (int j = 0; j < rounds_sel; j++) {
            const int t = j * L + lis;
            bool p = false;
            if (act && t < d) p = ((key_of_position(a.rng_seed, start + t) ^ prefix) >> b) == 0;
            c0 += __popcll(__ballot(p) & segmask);
        }
        if (act) {
            if (k <= c0) {
                m = c0;
            } else {
                k -= c0;
                m -= c0;
                prefix |= 1ull << b;
            }
            sh = b;
        }
    }
    const int rounds = wave_max((d + L - 1) / L);
    int written = 0;
    for (int j = 0; j < rounds; j++) {
        const int t = j * L + lis;
        bool p = false;
        if (t < d) p = !select || (key_of_position(a.rng_seed, start + t) >> sh) <= (prefix >> sh);
        const unsigned long long picks = __ballot(p) & segmask;
        if (p) emit_pick(a, out0 + written + __popcll(picks & below), start + t);
        written += __popcll(picks);
    }
}

// Block b looks at seeds [256 b, 256 b + 256) and samples the rows among them that have more than kLongRow positions, one
// after another with all 256 threads.
__global__ void __launch_bounds__(kBlock)
sample_long_kernel(const SampleArgs a)
{
    __shared__ unsigned long long s_long[kWavesPerBlock];
    __shared__ int s_cnt[kWavesPerBlock];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    {
        const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
        bool is_long = false;
        if (i < a.num_seeds) {
            const int32_t r = a.seeds[i];
            if ((uint32_t)r < a.num_nodes) {
                int64_t start;
                is_long = row_extent(a.rp, r, &start) > kLongRow;
            }
        }
        const unsigned long long mine = __ballot(is_long);
        if (lane == 0) s_long[wave] = mine;
    }
    __syncthreads();
    for (int w = 0; w < kWavesPerBlock; w++) {
        unsigned long long todo = s_long[w];
        while (todo) {
            const int bitpos = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t i = (int64_t)blockIdx.x * kBlock + w * kWave + bitpos;
            const int32_t r = a.seeds[i];
            if (tid == 0 && a.seedpos[r] != (int32_t)(i + 1)) a.rec[REC_DUP_SEED] = i + 1;
            int64_t start;
            const int d = row_extent(a.rp, r, &start);
            const int64_t out0 = a.blk_rp[i];
            const bool select = a.fanout > 0 && d > a.fanout;
            uint64_t prefix = 0;
            int sh = 0;
            if (select) {
                int k = a.fanout, m = d;
                for (int b = 63; b >= 0 && m > 1; b--) {
                    int c = 0;
                    for (int base = 0; base < d; base += kBlock) {
                        const int t = base + tid;
                        const bool p = t < d && ((key_of_position(a.rng_seed, start + t) ^ prefix) >> b) == 0;
                        c += __popcll(__ballot(p));
                    }
                    __syncthreads();                           // (the previous readers of s_cnt are done)
                    if (lane == 0) s_cnt[wave] = c;
                    __syncthreads();
                    int c0 = 0;
#pragma unroll
                    for (int v = 0; v < kWavesPerBlock; v++) c0 += s_cnt[v];
                    if (k <= c0) {
                        m = c0;
                    } else {
                        k -= c0;
                        m -= c0;
                        prefix |= 1ull << b;
                    }
                    sh = b;
                }
            }
            // every wavefront compacts one contiguous quarter of the row: count, exchange, write
            const int chunk = ((d + kBlock - 1) / kBlock) * kWave;
            const int lo = min(d, wave * chunk), hi = min(d, lo + chunk);
            int mine = hi - lo;
            if (select) {
                mine = 0;
                for (int base = lo; base < hi; base += kWave) {
                    const int t = base + lane;
                    const bool p = t < hi && (key_of_position(a.rng_seed, start + t) >> sh) <= (prefix >> sh);
                    mine += __popcll(__ballot(p));
                }
            }
            __syncthreads();
            if (lane == 0) s_cnt[wave] = mine;
            __syncthreads();
            int64_t pos = out0;
#pragma unroll
            for (int v = 0; v < kWavesPerBlock; v++)
                if (v < wave) pos += s_cnt[v];
            for (int base = lo; base < hi; base += kWave) {
                const int t = base + lane;
                const bool p = t < hi && (!select || (key_of_position(a.rng_seed, start + t) >> sh) <= (prefix >> sh));
                const unsigned long long picks = __ballot(p);
                if (p) emit_pick(a, pos + __popcll(picks & below), start + t);
                pos += __popcll(picks);
            }
        }
    }
}

// rank[v] (the scanned mark[]) = picked non-seed ids below v; rank[v + 1] > rank[v]: v is one of them.
__global__ void __launch_bounds__(kBlock)
relabel_kernel(const int32_t *__restrict__ seeds, int64_t num_seeds, int64_t num_nodes, const int32_t *__restrict__ seedpos,
               const int32_t *__restrict__ rank, const int32_t *__restrict__ blk_rp, int32_t *__restrict__ blk_ci,
               int32_t *__restrict__ src_nodes, int64_t edge_capacity, int64_t src_capacity, long long *__restrict__ rec)
{
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
    const int64_t nnz = blk_rp[num_seeds];
    if (first == 0) {
        rec[REC_NNZ] = nnz;
        rec[REC_SRC] = num_seeds + rank[num_nodes];
    }
    for (int64_t i = first; i < num_seeds && i < src_capacity; i += step) src_nodes[i] = seeds[i];
    for (int64_t v = first; v < num_nodes; v += step) {
        const int32_t before = rank[v];
        if (rank[v + 1] > before && num_seeds + before < src_capacity) src_nodes[num_seeds + before] = (int32_t)v;
    }
    const int64_t edges = std::min(nnz, edge_capacity);
    for (int64_t p = first; p < edges; p += step) {
        const int32_t c = blk_ci[p];
        int32_t local = -1;                                   // an id outside the graph (the call fails)
        if ((uint32_t)c < (uint64_t)num_nodes) {
            const int32_t s = seedpos[c];
            local = s > 0 ? s - 1 : (int32_t)(num_seeds + rank[c]);
        }
        blk_ci[p] = local;
    }
}

// The partition of the block's row pointers (gnna_parts.h); the number of groups is read on the device.
__global__ void __launch_bounds__(kBlock)
part_fill_kernel(const CsrRows rows, const int32_t *__restrict__ first_part, int partSize, int64_t capacity,
                 int32_t *__restrict__ pp, int32_t *__restrict__ p2n, long long *__restrict__ rec)
{
    const int64_t num_parts = first_part[rows.n];
    if (blockIdx.x == 0 && threadIdx.x == 0) rec[REC_PARTS] = num_parts;
    if (num_parts > capacity) return;                         // (then the edges do not fit either: the call fails)
    fill_parts(rows, first_part, partSize, num_parts, pp, p2n);
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_sample_neighbors_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_nodes, const int32_t *seeds,
                              int64_t num_seeds, int fanout, uint64_t rng_seed, int partSize, int32_t *blk_row_pointers,
                              int32_t *blk_column_index, int32_t *blk_edge_ids, int32_t *src_nodes, int32_t *partPtr,
                              int32_t *part2Node, int64_t edge_capacity, int64_t src_capacity, int64_t counts[3], void *stream_v)
{
    const char *what = "gnna_sample_neighbors_i32";
    if (num_nodes < 0 || num_seeds < 0 || edge_capacity < 0 || src_capacity < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_nodes=%lld num_seeds=%lld edge_capacity=%lld src_capacity=%lld)",
                    what, (long long)num_nodes, (long long)num_seeds, (long long)edge_capacity, (long long)src_capacity);
    if (!counts || !blk_row_pointers || (num_seeds > 0 && (!seeds || !row_pointers)) || (edge_capacity > 0 && !blk_column_index) ||
        (src_capacity > 0 && !src_nodes))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((part2Node && !partPtr) || (partPtr && !part2Node && edge_capacity > 0))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partPtr and part2Node come together", what);
    if (partPtr && partSize <= 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must be positive when a partition is asked for (got %d)", what, partSize);
    if (num_nodes >= 0x7fffffffLL || num_seeds >= 0x7fffffffLL) return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 rows", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = refuse_capture(what, stream);
    if (rc != GNNA_OK) return rc;
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    edge_capacity = std::min<int64_t>(edge_capacity, 0x7fffffffLL);       // positions are int32
    src_capacity = std::min<int64_t>(src_capacity, 0x7fffffffLL);

    // scratch: [record][seedpos: N][mark: N + 1] (cleared together) [scan partials][parts before every block row: S + 1]
    Carver c;
    const size_t o_rec = c.add(REC_WORDS * sizeof(long long)), o_pos = c.add((size_t)num_nodes * 4);
    const size_t o_mark = c.add((size_t)(num_nodes + 1) * 4), cleared_bytes = c.bytes;
    const size_t o_partial = c.add((size_t)scan_tiles(std::max(num_nodes, num_seeds) + 1) * 4);
    const size_t o_parts = c.add((size_t)(num_seeds + 1) * 4);
    void *ws = nullptr;
    rc = get_workspace(ds, stream, kSlotSample, c.bytes, &ws);
    if (rc != GNNA_OK) return rc;
    long long *rec = Carver::at<long long>(ws, o_rec);
    int32_t *seedpos = Carver::at<int32_t>(ws, o_pos), *mark = Carver::at<int32_t>(ws, o_mark);
    int32_t *partial = Carver::at<int32_t>(ws, o_partial), *first_part = Carver::at<int32_t>(ws, o_parts);

    const dim3 block(kBlock);
    launch_clear_words(ds, stream, static_cast<int32_t *>(ws), (int64_t)(cleared_bytes / 4));
    hipLaunchKernelGGL(seed_kernel, dim3(elementwise_grid(num_seeds + 1, ds->num_cus, 16)), block, 0, stream, row_pointers,
                       (uint32_t)num_nodes, seeds, num_seeds, fanout, seedpos, blk_row_pointers, rec);
    rc = launch_exclusive_scan(stream, blk_row_pointers, num_seeds + 1, partial);
    if (rc != GNNA_OK) return rc;
    if (num_seeds > 0) {
        // lanes per row from the edges an average row has: the graph's hint, else what the fanout suggests
        const int L = lanes_per_row(column_index, fanout > 0 ? 2 * (int64_t)fanout : kWave);
        SampleArgs a{row_pointers, column_index, seeds, (uint32_t)num_nodes, num_seeds, fanout, rng_seed, seedpos, mark,
                     blk_row_pointers, blk_column_index, blk_edge_ids, edge_capacity, rec};
        const int64_t rows_per_block = kBlock / L;
        hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)((num_seeds + rows_per_block - 1) / rows_per_block)), block, 0, stream,
                           a, L);
        hipLaunchKernelGGL(sample_long_kernel, dim3((unsigned)((num_seeds + kBlock - 1) / kBlock)), block, 0, stream, a);
    }
    rc = launch_exclusive_scan(stream, mark, num_nodes + 1, partial);
    if (rc != GNNA_OK) return rc;
    const int64_t relabel_items = std::max(std::max(num_nodes, num_seeds), edge_capacity);
    hipLaunchKernelGGL(relabel_kernel, dim3(elementwise_grid(relabel_items, ds->num_cus, 16)), block, 0, stream, seeds, num_seeds,
                       num_nodes, seedpos, mark, blk_row_pointers, blk_column_index, src_nodes, edge_capacity, src_capacity, rec);
    if (partPtr) {
        launch_part_count(ds, stream, blk_row_pointers, num_seeds, nullptr, partSize, first_part);
        rc = launch_exclusive_scan(stream, first_part, num_seeds + 1, partial);
        if (rc != GNNA_OK) return rc;
        hipLaunchKernelGGL(part_fill_kernel, dim3(elementwise_grid(edge_capacity + 1, ds->num_cus, 16)), block, 0, stream,
                           CsrRows{blk_row_pointers, num_seeds}, first_part, partSize, edge_capacity, partPtr, part2Node, rec);
    }
    long long host[REC_WORDS] = {0};
    rc = read_record(what, stream, rec, host, REC_WORDS);
    if (rc != GNNA_OK) return rc;
    counts[0] = host[REC_NNZ];
    counts[1] = host[REC_SRC];
    counts[2] = partPtr ? host[REC_PARTS] : 0;
    if (host[REC_BAD_SEED])
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: seeds[%lld] is outside [0, num_nodes = %lld)", what, host[REC_BAD_SEED] - 1,
                    (long long)num_nodes);
    if (host[REC_DUP_SEED])
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: duplicate seed: seeds[%lld] appears more than once", what, host[REC_DUP_SEED] - 1);
    if (host[REC_BAD_COLUMN])
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: column_index[%lld] is outside [0, num_nodes = %lld)", what,
                    host[REC_BAD_COLUMN] - 1, (long long)num_nodes);
    if (counts[0] < 0) return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 sampled edges", what);
    if (counts[0] > edge_capacity || counts[1] > src_capacity)
        return fail(GNNA_ERR_INVALID_ARGUMENT,
                    "%s: capacity too small: the block has %lld edges and %lld source nodes, edge_capacity=%lld src_capacity=%lld", what,
                    (long long)counts[0], (long long)counts[1], (long long)edge_capacity, (long long)src_capacity);
    return GNNA_OK;
}

#pragma GCC visibility pop
}  // extern "C"

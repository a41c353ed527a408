// gnna_spatial.hip -- graph construction from coordinates (gnna_spatial.h has the rule word for word):
//   gnna_radius_graph_f32   the radius graph / k-nearest-neighbour graph of every point set of a batch as a CSR with its
//                           neighbor-group partition; a prepare-time call like gnna_induced_subgraph_i32: ONE read-back, refuses
//                           to run inside a stream capture
//
// In launch order (the record, counts[N + 1] and groups per row [N + 1] are library scratch: 8 bytes per row):
//   clear_kernel            (gnna_transpose.hip) the record and counts[N + 1]
//   check_segments_kernel   the first segment whose clamped pointers decrease, into the record
//   radius_rows_kernel<0>   count pass over the rows of segments of up to kLongRows rows, L = 4 .. 64 lanes per row: the
//                           candidates of a lane group's row counted by ballot + popcount
//   radius_tiles_kernel<0>  count pass over the rows of longer segments: a workgroup per tile of 256 destination rows, a row per
//                           lane, source tiles staged in LDS as structure-of-arrays (returns at once when no segment is long)
//   total_kernel            nnz' in 64 bits (an integer sum: the same whatever the order)
//   scan_* kernels          (gnna_transpose.hip) exclusive scan of the counts = the row pointers
//   radius_rows_kernel<1>   fill pass: the same walks; under a cap a row with more candidates than the cap first finds its
//   radius_tiles_kernel<1>  cap-th smallest key most-significant-bit first over recomputed keys; every kept neighbour is placed by
//                           the ballot's prefix (rows kernel) or the lane's own counter (tiles kernel): increasing j, no sort.
//                           Both write nothing but row_pointers when the capacity is too small
//   part_count_kernel       (gnna_transpose.hip), the scan, part_fill_kernel: the partition by the one rule of gnna_parts.h
// Distances and keys are recomputed by every pass and stored nowhere but in dist2.  The library is compiled with
// -ffp-contract=off: a subtraction, a multiplication and an addition per column, each rounded to fp32.
#include <algorithm>
#include <cmath>

#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::check_alias
#include "gnna_internal.h"
#include "gnna_parts.h"
#include "gnna_segments.h"
#include "gnna_spatial.h"

namespace gnna {
namespace {

constexpr int kSlotSpatial = 19;                          // library scratch: the record, counts[N + 1], groups per row [N + 1], scan partials
constexpr int kLongRows = GNNA_SPATIAL_LONG_ROWS;         // a segment of more rows goes to radius_tiles_kernel
constexpr int kSourceTile = GNNA_SPATIAL_SOURCE_TILE;     // floats of a staged source tile
constexpr int kMaxDim = GNNA_SPATIAL_MAX_DIM;
constexpr int kRegisterDim = GNNA_SPATIAL_REGISTER_DIM;                         // radius_tiles_kernel keeps a destination row of up to this width in registers
constexpr uint64_t kNoKey = ~0ull;                        // no candidate (a key's high word is the bits of a non-negative float)
// the record that is read back: int64 words
enum { REC_NNZ = 0, REC_PARTS = 1, REC_BAD_SEG = 2, REC_LONG = 3, REC_WORDS = 4 };

struct SpatialArgs {
    const float *pos;
    int64_t ld, N;
    int dim;
    const int32_t *gp;
    int64_t G;
    float r2;
    int cap, loop;
    int32_t *cnt;                      // scratch [N + 1]: the count passes write the counts, the fill passes read the scanned counts
    int32_t *out_rp, *out_ci;
    float *out_d2;
    int64_t edge_capacity;
    long long *rec;
};

// d2(i, j) of gnna_spatial.h: column by column, every operation rounded to fp32
__device__ __forceinline__ float dist2_of(const float *__restrict__ pi, const float *__restrict__ pj, int dim)
{
#pragma clang fp contract(off)
    float acc = 0.0f;                  // (+0 + t == t for every t that is a square or NaN)
    for (int c = 0; c < dim; c++) {
        const float diff = pj[c] - pi[c];
        acc = acc + diff * diff;
    }
    return acc;
}

__device__ __forceinline__ uint64_t key_of(float d2, int64_t j) { return ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)j; }

// the key of candidate j of row i, or kNoKey when j is no candidate
__device__ __forceinline__ uint64_t candidate_key(const SpatialArgs &a, int64_t i, int64_t j)
{
    const float d2 = dist2_of(a.pos + i * a.ld, a.pos + j * a.ld, a.dim);
    return (d2 <= a.r2 && (j != i || a.loop)) ? key_of(d2, j) : kNoKey;
}

// fill passes: do the results fit?  (uniform over the grid; total_kernel wrote the word launches before)
__device__ __forceinline__ bool fits(const SpatialArgs &a) { return a.rec[REC_NNZ] <= a.edge_capacity; }

__device__ __forceinline__ void emit_neighbor(const SpatialArgs &a, int64_t at, uint64_t key)
{
    if ((uint64_t)at < (uint64_t)a.edge_capacity) {
        a.out_ci[at] = (int32_t)(uint32_t)key;
        if (a.out_d2) a.out_d2[at] = __uint_as_float((uint32_t)(key >> 32));
    }
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// One step of the most-significant-bit-first search for the k-th smallest of m keys that agree with `prefix` above bit b, c0 of
// them with bit b clear (sample_rows_kernel's step).
__device__ __forceinline__ void select_step(int b, int c0, int *k, int *m, uint64_t *prefix)
{
    if (*k <= c0) {
        *m = c0;
    } else {
        *k -= c0;
        *m -= c0;
        *prefix |= 1ull << b;
    }
}

__global__ void __launch_bounds__(kBlock)
check_segments_kernel(const int32_t *__restrict__ gp, int64_t G, int64_t N, long long *__restrict__ rec)
{
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < G; g += (int64_t)gridDim.x * kBlock)
        if (seg::seg_ptr(gp, N, g + 1) < seg::seg_ptr(gp, N, g))          // the first such g = the largest G - g
            atomicMax(reinterpret_cast<unsigned long long *>(rec + REC_BAD_SEG), (unsigned long long)(G - g));
}

// rec[REC_NNZ] += the counts (cleared before): integers, so the order of the additions does not show
__global__ void __launch_bounds__(kBlock)
total_kernel(const int32_t *__restrict__ cnt, int64_t N, long long *__restrict__ rec)
{
    long long mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) mine += cnt[i];
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
    if ((threadIdx.x & (kWave - 1)) == 0 && mine)
        atomicAdd(reinterpret_cast<unsigned long long *>(rec + REC_NNZ), (unsigned long long)mine);
}

// ---- short segments: L lanes per row ------------------------------------------------------------------------------------------

// L lanes per row (a power of two, 4 .. 64), 256 / L rows per block, rows 0 .. N: many segments share a workgroup.  Every loop
// bound is uniform over the wavefront: all 64 lanes reach every ballot.  FILL = false: cnt[i] = the neighbours row i keeps (0 for
// row N; a row of a long segment is radius_tiles_kernel's).  FILL = true: the neighbours, and the caller's row pointers.
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
radius_rows_kernel(const SpatialArgs a, int L)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int lis = lane & (L - 1);
    const unsigned long long segmask = (L == kWave ? ~0ull : ((1ull << L) - 1ull)) << (lane & ~(L - 1));
    const unsigned long long below = segmask & ((1ull << lane) - 1ull);
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / L;
    int64_t out0 = 0;
    if (FILL) {
        if (i <= a.N) {
            out0 = a.cnt[i];
            if (lis == 0) a.out_rp[i] = (int32_t)out0;
        }
        if (!fits(a)) return;
    }
    // the segment [s, s + d) of row i
    int64_t s = 0;
    int d = 0;
    bool is_long = false;
    if (i < a.N) {
        const int64_t g = seg::first_segment(a.gp, a.G, a.N, i);
        if (g < a.G) {
            const int64_t lo = seg::seg_ptr(a.gp, a.N, g), hi = seg::seg_ptr(a.gp, a.N, g + 1);
            if (lo <= i && i < hi) {
                s = lo;
                d = (int)(hi - lo);
                is_long = d > kLongRows;
                if (is_long) d = 0;
            }
        }
    }
    if (!FILL && is_long && lis == 0) a.rec[REC_LONG] = 1;      // (plain stores of one value)
    const int rounds = wave_max((d + L - 1) / L);
    // the first round's key stays in a register: a segment of up to L rows computes every distance once per pass
    const uint64_t key0 = lis < d ? candidate_key(a, i, s + lis) : kNoKey;
    auto key_at = [&](int j) -> uint64_t {
        if (j == 0) return key0;
        const int t = j * L + lis;
        return t < d ? candidate_key(a, i, s + t) : kNoKey;
    };
    int cnt = 0;
    if (!FILL || a.cap > 0)
        for (int j = 0; j < rounds; j++) cnt += __popcll(__ballot(key_at(j) != kNoKey) & segmask);
    if (!FILL) {
        if (lis == 0 && i <= a.N && !is_long) a.cnt[i] = a.cap > 0 ? min(cnt, a.cap) : cnt;
        return;
    }
    // the cap-th smallest key of the row: after bit b, `m` keys agree with `prefix` on bits 63 .. b and the wanted key is the
    // k-th smallest of them; m == 1: it is found, and the kept keys are those with (key >> b) <= (prefix >> b)
    const bool select = a.cap > 0 && cnt > a.cap;
    uint64_t prefix = 0;
    int k = a.cap, m = select ? cnt : 0, sh = 0;
    const int rounds_sel = wave_max(select ? (d + L - 1) / L : 0);
    for (int b = 63; b >= 0; b--) {
        const bool act = m > 1;
        if (!__any(act)) break;
        int c0 = 0;
        for (int j = 0; j < rounds_sel; j++) {
            const uint64_t key = act ? key_at(j) : kNoKey;
            c0 += __popcll(__ballot(key != kNoKey && ((key ^ prefix) >> b) == 0) & segmask);
        }
        if (act) {
            select_step(b, c0, &k, &m, &prefix);
            sh = b;
        }
    }
    int written = 0;
    for (int j = 0; j < rounds; j++) {
        const uint64_t key = key_at(j);
        const bool p = key != kNoKey && (!select || (key >> sh) <= (prefix >> sh));
        const unsigned long long picks = __ballot(p) & segmask;
        if (p) emit_neighbor(a, out0 + written + __popcll(picks & below), key);
        written += __popcll(picks);
    }
}

// ---- long segments: a destination row per lane, source tiles in LDS -----------------------------------------------------------

// f(key) for every candidate j of row i in increasing j, for the lanes with `mine`; [s, e) is the row's segment.  The whole block
// stages T source rows at a time as structure-of-arrays (column c of tile row jj at s_pos[c * (T + 1) + jj]: the odd stride keeps
// the staging stores off one bank, and every lane reading the same jj is a broadcast).  Uniform over the block: every thread
// reaches every barrier.
template <class F>
__device__ __forceinline__ void sweep_segment(const SpatialArgs &a, float *__restrict__ s_pos, int64_t s, int64_t e, int64_t i,
                                              bool mine, F &&f)
{
#pragma clang fp contract(off)
    const int dim = a.dim;
    const int T = min(kBlock, kSourceTile / dim), TS = T + 1;
    const bool in_registers = dim <= kRegisterDim;
    float own[kRegisterDim] = {};
    const float *__restrict__ pi = a.pos + (mine ? i : s) * a.ld;
    if (mine && in_registers) {
#pragma unroll
        for (int c = 0; c < kRegisterDim; c++)
            if (c < dim) own[c] = pi[c];
    }
    for (int64_t base = s; base < e; base += T) {
        const int rows = (int)min((int64_t)T, e - base);
        __syncthreads();                                       // (the readers of the tile before are done)
        for (int idx = threadIdx.x; idx < rows * dim; idx += kBlock) {
            const int jj = idx / dim, c = idx - jj * dim;
            s_pos[c * TS + jj] = a.pos[(base + jj) * a.ld + c];
        }
        __syncthreads();
        if (!mine) continue;
        for (int jj = 0; jj < rows; jj++) {
            float d2 = 0.0f;
            if (in_registers) {
#pragma unroll
                for (int c = 0; c < kRegisterDim; c++)
                    if (c < dim) {
                        const float diff = s_pos[c * TS + jj] - own[c];
                        d2 = d2 + diff * diff;
                    }
            } else {
                for (int c = 0; c < dim; c++) {
                    const float diff = s_pos[c * TS + jj] - pi[c];
                    d2 = d2 + diff * diff;
                }
            }
            const int64_t j = base + jj;
            if (d2 <= a.r2 && (j != i || a.loop)) f(key_of(d2, j));
        }
    }
}

// Block b looks at rows [256 b, 256 b + 256) and takes, one after another, the segments of more than kLongRows rows that reach
// into them: lane t owns row 256 b + t while the block is at that row's segment.
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
radius_tiles_kernel(const SpatialArgs a)
{
    __shared__ float s_pos[kSourceTile + kMaxDim];             // T + 1 floats per column
    if (a.rec[REC_LONG] == 0) return;                          // (uniform over the grid)
    if (FILL && !fits(a)) return;
    const int64_t tile0 = (int64_t)blockIdx.x * kBlock, tile1 = min(a.N, tile0 + kBlock);
    const int64_t i = tile0 + threadIdx.x;
    int64_t r = tile0;                                         // (uniform over the block, like everything that steers it)
    while (r < tile1) {
        const int64_t g = seg::first_segment(a.gp, a.G, a.N, r);
        if (g >= a.G) break;
        const int64_t s = seg::seg_ptr(a.gp, a.N, g), e = seg::seg_ptr(a.gp, a.N, g + 1);
        const int64_t lo = max(s, r), hi = min(e, tile1);
        r = max(e, r + 1);
        if (e - s <= kLongRows || lo >= hi) continue;
        const bool mine = i >= lo && i < hi;
        int cnt = 0;
        if (!FILL || a.cap > 0) sweep_segment(a, s_pos, s, e, i, mine, [&](uint64_t) { cnt++; });
        if (!FILL) {
            if (mine) a.cnt[i] = a.cap > 0 ? min(cnt, a.cap) : cnt;
            continue;
        }
        const bool select = mine && a.cap > 0 && cnt > a.cap;
        uint64_t prefix = 0;
        int k = a.cap, m = select ? cnt : 0, sh = 0;
        for (int b = 63; b >= 0; b--) {
            const bool act = m > 1;
            if (!__syncthreads_or(act)) break;
            int c0 = 0;
            sweep_segment(a, s_pos, s, e, i, act, [&](uint64_t key) { c0 += ((key ^ prefix) >> b) == 0; });
            if (act) {
                select_step(b, c0, &k, &m, &prefix);
                sh = b;
            }
        }
        int64_t at = mine ? (int64_t)a.cnt[i] : 0;
        sweep_segment(a, s_pos, s, e, i, mine, [&](uint64_t key) {
            if (!select || (key >> sh) <= (prefix >> sh)) emit_neighbor(a, at++, key);
        });
    }
}

// The partition of the result's row pointers (gnna_parts.h); the number of groups is read on the device.
__global__ void __launch_bounds__(kBlock)
part_fill_kernel(const SpatialArgs a, const int32_t *__restrict__ first_part, int partSize, int32_t *__restrict__ pp,
                 int32_t *__restrict__ p2n)
{
    const CsrRows rows{a.cnt, a.N};
    const int64_t num_parts = first_part[a.N];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.rec[REC_PARTS] = num_parts;
    if (!fits(a)) return;                                                                    // (groups <= edges: they fit as well)
    fill_parts(rows, first_part, partSize, num_parts, pp, p2n);
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_radius_graph_f32(const float *pos, int64_t ld_pos, int64_t num_rows, int dim, const int32_t *graph_pointers,
                          int64_t num_segments, float radius, int max_neighbors, int loop, int partSize, int32_t *row_pointers,
                          int32_t *column_index, float *dist2, int32_t *partPtr, int32_t *part2Node, int64_t edge_capacity,
                          int64_t counts[3], void *stream_v)
{
    const char *what = "gnna_radius_graph_f32";
    if (!counts) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null counts", what);
    if (dim < 1 || dim > kMaxDim) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dim must be in [1, %d] (got %d)", what, kMaxDim, dim);
    if (edge_capacity < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (edge_capacity=%lld)", what, (long long)edge_capacity);
    int rc = seg::check_counts(what, num_rows, num_segments);
    if (rc != GNNA_OK) return rc;
    if (num_rows >= 0x7fffffffLL) return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 rows", what);
    if (bad_ld(ld_pos, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: ld_pos must be in [dim, 2^29) (ld_pos=%lld dim=%d)", what, (long long)ld_pos, dim);
    if (!(radius >= 0.0f)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: radius must be >= 0 or +inf (got %g)", what, (double)radius);
    if (max_neighbors < 0 || max_neighbors > GNNA_SPATIAL_MAX_NEIGHBORS)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: max_neighbors must be in [0, %d] (got %d)", what, GNNA_SPATIAL_MAX_NEIGHBORS,
                    max_neighbors);
    if (!row_pointers || !graph_pointers || (num_rows > 0 && !pos) || (edge_capacity > 0 && !column_index))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((part2Node && !partPtr) || (partPtr && !part2Node && edge_capacity > 0))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partPtr and part2Node come together", what);
    if (partPtr && partSize <= 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must be positive when a partition is asked for (got %d)", what, partSize);
    {
        const void *const ins[2] = {pos, graph_pointers};
        const void *const outs[5] = {row_pointers, column_index, dist2, partPtr, part2Node};
        if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if ((rc = refuse_capture(what, stream)) != GNNA_OK) return rc;
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    edge_capacity = std::min<int64_t>(edge_capacity, 0x7fffffffLL);       // positions are int32
    const int64_t N = num_rows;

    // scratch: [record][counts: N + 1] (cleared together) [groups per row: N + 1][scan partials]
    Carver c;
    const size_t o_rec = c.add(REC_WORDS * sizeof(long long)), o_cnt = c.add((size_t)(N + 1) * 4), cleared_bytes = c.bytes;
    const size_t o_parts = c.add((size_t)(N + 1) * 4), o_partial = c.add((size_t)scan_tiles(N + 1) * 4);
    void *ws = nullptr;
    if ((rc = get_workspace(ds, stream, kSlotSpatial, c.bytes, &ws)) != GNNA_OK) return rc;
    long long *rec = Carver::at<long long>(ws, o_rec);
    int32_t *cnt = Carver::at<int32_t>(ws, o_cnt);            // counts -> the result's row pointers
    int32_t *first_part = Carver::at<int32_t>(ws, o_parts);
    int32_t *partial = Carver::at<int32_t>(ws, o_partial);

    const float r2 = radius * radius;
    SpatialArgs a{pos, ld_pos, N, dim, graph_pointers, num_segments, r2, max_neighbors, loop != 0 ? 1 : 0, cnt, row_pointers,
                  column_index, dist2, edge_capacity, rec};
    // lanes per row from the rows an average segment has
    const int L = std::max(4, std::min<int>(kWave, pow2_at_least(num_segments > 0 ? (N + num_segments - 1) / num_segments : 1)));
    const int64_t rows_per_block = kBlock / L;
    const dim3 block(kBlock), row_grid((unsigned)((N + 1 + rows_per_block - 1) / rows_per_block)),
        tile_grid((unsigned)((N + kBlock - 1) / kBlock));
    launch_clear_words(ds, stream, static_cast<int32_t *>(ws), (int64_t)(cleared_bytes / 4));
    hipLaunchKernelGGL(check_segments_kernel, dim3(elementwise_grid(num_segments, ds->num_cus, 16)), block, 0, stream, graph_pointers,
                       num_segments, N, rec);
    hipLaunchKernelGGL(radius_rows_kernel<false>, row_grid, block, 0, stream, a, L);
    if (N > kLongRows) hipLaunchKernelGGL(radius_tiles_kernel<false>, tile_grid, block, 0, stream, a);
    hipLaunchKernelGGL(total_kernel, dim3(elementwise_grid(N, ds->num_cus, 16)), block, 0, stream, cnt, N, rec);
    if ((rc = launch_exclusive_scan(stream, cnt, N + 1, partial)) != GNNA_OK) return rc;
    hipLaunchKernelGGL(radius_rows_kernel<true>, row_grid, block, 0, stream, a, L);
    if (N > kLongRows) hipLaunchKernelGGL(radius_tiles_kernel<true>, tile_grid, block, 0, stream, a);
    if (partPtr) {
        launch_part_count(ds, stream, cnt, N, nullptr, partSize, first_part);
        if ((rc = launch_exclusive_scan(stream, first_part, N + 1, partial)) != GNNA_OK) return rc;
        hipLaunchKernelGGL(part_fill_kernel, dim3(elementwise_grid(edge_capacity + 1, ds->num_cus, 16)), block, 0, stream, a,
                           first_part, partSize, partPtr, part2Node);
    }
    long long host[REC_WORDS] = {0};
    if ((rc = read_record(what, stream, rec, host, REC_WORDS)) != GNNA_OK) return rc;
    counts[0] = N;
    counts[1] = host[REC_NNZ];
    counts[2] = partPtr ? host[REC_PARTS] : 0;
    if (host[REC_BAD_SEG]) {
        const long long g = (long long)num_segments - host[REC_BAD_SEG];
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: graph_pointers decreases at segment %lld (clamped to [0, num_rows = %lld])", what,
                    g, (long long)N);
    }
    if (counts[1] >= 0x80000000LL) {
        counts[2] = 0;
        return fail(GNNA_ERR_UNSUPPORTED, "%s: the graph has %lld edges (at most 2^31 - 1: positions are int32)", what,
                    (long long)counts[1]);
    }
    if (counts[1] > edge_capacity)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: capacity too small: the graph has %lld edges, edge_capacity=%lld", what,
                    (long long)counts[1], (long long)edge_capacity);
    return GNNA_OK;
}

#pragma GCC visibility pop
}  // extern "C"

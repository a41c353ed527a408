// gnna_topk.hip -- hierarchical pooling on a batch of graphs (include/gnna_topk.h): gnna_segment_topk_i32 selects the
// best-scoring rows of every graph and cuts the induced sub-batch out on the device with ONE read-back, a prepare-time call like
// gnna_sample_neighbors_i32 (it synchronises the stream and refuses to run inside a stream capture);
// gnna_gather_rows_scale_ld_f32 / gnna_gather_rows_scale_backward_ld_f32 are the differentiable part.  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its models never change the number of rows).
//
//   clear_kernel        (gnna_transpose.hip) keep[0 .. N] = 0 and the record
//   select_wave_kernel  one wavefront per segment of up to GNNA_TOPK_WAVE_ROWS rows: the order keys (gnna_keys.h) of the segment in
//                       registers, the k-th largest key bit by bit from the top (per bit: ballots + popcounts of "agrees with the
//                       prefix and has this bit set"), then keep[] = 1 for the keys above it and for the first rows equal to it, in
//                       row order by a ballot prefix
//   select_block_kernel one workgroup per segment, which returns at once unless the segment is longer: four passes over the scores
//                       with a 256-bin histogram in LDS (integer atomics), the digit by a block scan from the top bin down; then
//                       every wavefront ranks the equal rows of one contiguous quarter (count, exchange, write)
//   scan_* kernels      (gnna_transpose.hip) keep[] -> the kept rows below every row
//   ids_kernel          new_id, perm, new_graph_pointers
//   edge_flag_kernel    flag[e] = the edge's row (binary search in row_pointers) and its column are kept; checks row_pointers
//   scan_* kernels      flag[] -> where every surviving edge goes
//   edge_fill_kernel    new_column_index, edge_ids, new_row_pointers, and the neighbor-groups of every kept row
//   scan_* kernels      -> the first group of every row
//   part_fill_kernel    partPtr / part2Node of new_row_pointers by the one rule of gnna_parts.h, over the OLD rows
// Only ones are stored into keep[] after the clear, every other position is computed from counts and scans, and no global atomic
// hands a position out: the same bits on every run and for every launch shape.
//
//   gather_rows_kernel / gather_rows_bwd_kernel: the lane layout of gnna_pool.hip -- LPR = next_pow2(ceil(D / 4)) lanes per row
//   with 16-byte accesses, 64 / LPR rows per wavefront and step, kRowsInFlight steps in flight, column blocks of 256 floats for
//   wider rows.  One writer per element, plain stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gnna_topk.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::load_piece, gat::head_sum, gat::check_alias
#include "gnna_internal.h"
#include "gnna_keys.h"
#include "gnna_parts.h"
#include "gnna_segments.h"

namespace gnna {
namespace {

using gat::VT;
using gat::load_piece;
using seg::seg_ptr;
using seg::store_piece;
using seg::uniform64;

constexpr int kSlotTopk = 15;        // library scratch: the record, keep[N + 1], groups per row [N + 1], flag[nnz + 1], scan partials
constexpr int kWaveRows = GNNA_TOPK_WAVE_ROWS;
constexpr int kKeysPerLane = kWaveRows / kWave;
constexpr int kRowsInFlight = 4;     // 16-byte loads in flight per lane in the gathers
// the record that is read back: 4 x int64
enum { REC_ROWS = 0, REC_EDGES = 1, REC_PARTS = 2, REC_BAD_ROW = 3, REC_WORDS = 4 };

// The rows a segment of n rows keeps (include/gnna_topk.h); the arguments have passed the entry's checks.
__host__ __device__ __forceinline__ int64_t keep_count(int64_t n, double ratio, int64_t k_fixed)
{
    if (k_fixed > 0) return n < k_fixed ? n : k_fixed;
    const int64_t k = (int64_t)ceil(ratio * (double)n);
    return n < k ? n : k;
}

struct SelectArgs {
    const float *score;
    const int32_t *gp;
    int64_t N, G;
    double ratio;
    int64_t k_fixed;
    int32_t *keep;           // [N + 1], cleared
};

__global__ void __launch_bounds__(kBlock)
select_wave_kernel(const SelectArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t g = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= a.G) return;                                            // (the whole wavefront)
    const int64_t S = uniform64(seg_ptr(a.gp, a.N, g)), E = uniform64(seg_ptr(a.gp, a.N, g + 1));
    if (E <= S || E - S > kWaveRows) return;                         // empty, or select_block_kernel's
    const int n = (int)(E - S);
    int k = (int)keep_count(n, a.ratio, a.k_fixed);
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t key[kKeysPerLane];
    bool in[kKeysPerLane];
#pragma unroll
    for (int j = 0; j < kKeysPerLane; j++) {
        const int t = j * kWave + lane;
        in[j] = t < n;
        key[j] = in[j] ? order_of<GNNA_REDUCE_MAX>(a.score[S + t]) : 0u;
    }
    // after bit b, `prefix` holds the bits 31 .. b of the k-th largest key among those that agree with it above b
    uint32_t prefix = 0;
    if (k < n) {
        for (int b = 31; b >= 0; b--) {
            const uint32_t cand = prefix | (1u << b), mask = ~0u << b;
            int c1 = 0;
#pragma unroll
            for (int j = 0; j < kKeysPerLane; j++) c1 += __popcll(__ballot(in[j] && ((key[j] ^ cand) & mask) == 0u));
            if (k <= c1) prefix = cand;
            else k -= c1;
        }
    }
    // k: the rows equal to the threshold that are kept, the first in row order (k >= n: every row)
    int seen = 0;
#pragma unroll
    for (int j = 0; j < kKeysPerLane; j++) {
        const bool eq = in[j] && key[j] == prefix, gt = in[j] && key[j] > prefix;
        const unsigned long long eqs = __ballot(eq);
        if (gt || (eq && seen + __popcll(eqs & below) < k)) a.keep[S + j * kWave + lane] = 1;
        seen += __popcll(eqs);
    }
}

// Inclusive prefix of `v` over the block's threads.  All threads must call it; s_wave: kWavesPerBlock ints.
__device__ __forceinline__ int block_inclusive_scan(int v, int *s_wave)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int incl = wave_inclusive_scan(v);
    __syncthreads();                                                 // (the previous readers of s_wave are done)
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++)
        if (w < wave) before += s_wave[w];
    return before + incl;
}

__global__ void __launch_bounds__(kBlock)
select_block_kernel(const SelectArgs a)
{
    __shared__ int s_hist[kBlock];
    __shared__ int s_wave[kWavesPerBlock];
    __shared__ int s_pick[2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t g = blockIdx.x;
    const int64_t S = seg_ptr(a.gp, a.N, g), E = seg_ptr(a.gp, a.N, g + 1);
    if (E - S <= kWaveRows) return;                                  // (the whole block) select_wave_kernel's, or empty
    const int64_t n = E - S;
    const float *__restrict__ sc = a.score + S;
    int32_t *__restrict__ keep = a.keep + S;
    int k = (int)keep_count(n, a.ratio, a.k_fixed);
    if (k >= n) {
        for (int64_t t = tid; t < n; t += kBlock) keep[t] = 1;
        return;
    }
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const uint32_t himask = pass == 0 ? 0u : ~0u << (shift + 8);
        s_hist[tid] = 0;
        __syncthreads();
        for (int64_t base = 0; base < n; base += 4 * kBlock) {
            uint32_t key[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t t = base + u * kBlock + tid;
                in[u] = t < n;
                key[u] = in[u] ? order_of<GNNA_REDUCE_MAX>(sc[t]) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (in[u] && ((key[u] ^ prefix) & himask) == 0u) atomicAdd(&s_hist[(key[u] >> shift) & 255u], 1);
        }
        __syncthreads();
        // thread t looks at bin 255 - t: the digit whose bin holds the k-th largest of the keys counted
        const int h = s_hist[kBlock - 1 - tid];
        const int incl = block_inclusive_scan(h, s_wave);
        if (incl - h < k && k <= incl) { s_pick[0] = kBlock - 1 - tid; s_pick[1] = k - (incl - h); }
        __syncthreads();
        prefix |= (uint32_t)s_pick[0] << shift;
        k = s_pick[1];
        __syncthreads();                                             // (before the next pass clears the bins and picks again)
    }
    // every wavefront takes one contiguous quarter of the segment: count the rows equal to the threshold, exchange, write
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t chunk = ((n + kBlock - 1) / kBlock) * kWave;
    const int64_t lo = std::min<int64_t>(n, wave * chunk), hi = std::min<int64_t>(n, lo + chunk);
    int mine = 0;
    for (int64_t base = lo; base < hi; base += kWave) {
        const int64_t t = base + lane;
        mine += __popcll(__ballot(t < hi && order_of<GNNA_REDUCE_MAX>(sc[t]) == prefix));
    }
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    int seen = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++)
        if (w < wave) seen += s_wave[w];
    for (int64_t base = lo; base < hi; base += kWave) {
        const int64_t t = base + lane;
        uint32_t key = 0;
        if (t < hi) key = order_of<GNNA_REDUCE_MAX>(sc[t]);
        const bool eq = t < hi && key == prefix, gt = t < hi && key > prefix;
        const unsigned long long eqs = __ballot(eq);
        if (gt || (eq && seen + __popcll(eqs & below) < k)) keep[t] = 1;
        seen += __popcll(eqs);
    }
}

// rank[r] (the scanned keep[]) = kept rows below r; rank[r + 1] > rank[r]: r is kept.
__global__ void __launch_bounds__(kBlock)
ids_kernel(const int32_t *__restrict__ rank, int64_t N, const int32_t *__restrict__ gp, int64_t G, int32_t *__restrict__ new_id,
           int32_t *__restrict__ perm, int32_t *__restrict__ new_gp, int64_t row_capacity, long long *__restrict__ rec)
{
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
    if (first == 0) rec[REC_ROWS] = rank[N];
    for (int64_t r = first; r < N; r += step) {
        const int32_t before = rank[r];
        const bool kept = rank[r + 1] > before;
        new_id[r] = kept ? before : -1;
        if (kept && before < row_capacity) perm[before] = (int32_t)r;
    }
    for (int64_t g = first; g <= G; g += step) new_gp[g] = rank[seg_ptr(gp, N, g)];
}

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// flag[e] = 1 for an edge whose row and column are kept, flag[nnz] = 0 (which the scan turns into nnz'); the first row whose
// pointers break the contract goes to the record
__global__ void __launch_bounds__(kBlock)
edge_flag_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, int64_t N, int64_t nnz,
                 const int32_t *__restrict__ new_id, int32_t *__restrict__ flag, long long *__restrict__ rec)
{
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
    for (int64_t r = first; r <= N; r += step) {
        const int64_t v = rp[r];
        bool bad = v < 0 || v > nnz || (r == 0 && v != 0) || (r == N && v != nnz);
        if (r < N && (int64_t)rp[r + 1] < v) bad = true;
        if (bad) rec[REC_BAD_ROW] = r + 1;
    }
    for (int64_t e = first; e <= nnz; e += step) {
        int32_t f = 0;
        if (e < nnz && N > 0) {
            const int32_t c = ci[e];
            if ((uint32_t)c < (uint64_t)N && new_id[c] >= 0) {
                // the last row i with rp[i] <= e (rows without edges share their start with the next row)
                int64_t lo = 0, hi = N - 1;
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if (rp[mid] <= e) lo = mid; else hi = mid - 1;
                }
                f = new_id[lo] >= 0 ? 1 : 0;
            }
        }
        flag[e] = f;
    }
}

struct FillArgs {
    const int32_t *rp, *ci;
    int64_t N, nnz;
    const int32_t *new_id, *rank, *pos;      // pos: the scanned flag[]
    int32_t *new_rp, *new_ci, *eid;
    int64_t row_capacity, edge_capacity;
    int32_t *groups;                         // [N + 1] or null: the neighbor-groups of every OLD row (0 for one that is dropped)
    int partSize;
    long long *rec;
};

__global__ void __launch_bounds__(kBlock)
edge_fill_kernel(const FillArgs a)
{
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
    const int64_t rows = a.rank[a.N], edges = a.pos[a.nnz];
    if (first == 0) {
        a.rec[REC_EDGES] = edges;
        if (rows <= a.row_capacity) a.new_rp[rows] = (int32_t)edges;
    }
    for (int64_t e = first; e < a.nnz; e += step) {
        const int32_t p = a.pos[e];
        if (a.pos[e + 1] > p && p < a.edge_capacity) {
            a.new_ci[p] = a.new_id[a.ci[e]];                 // (a surviving edge: its id was range-checked by edge_flag_kernel)
            if (a.eid) a.eid[p] = (int32_t)e;
        }
    }
    for (int64_t r = first; r <= a.N; r += step) {
        int32_t count = 0;
        if (r < a.N) {
            const int32_t i = a.new_id[r];
            if (i >= 0) {
                const int32_t b = a.pos[clamp_to(a.rp[r], a.nnz)], e = a.pos[clamp_to(a.rp[r + 1], a.nnz)];
                if (i < a.row_capacity) a.new_rp[i] = b;
                if (a.groups) count = groups_of((int64_t)e - b, a.partSize);
            }
        }
        if (a.groups) a.groups[r] = count;
    }
}

// The OLD rows, of which only the kept ones own groups (a group's owner is then a kept row): old row i starts where its first
// edge goes (pos: the scanned flag[]) and is called by its new id.
struct KeptRows {
    const int32_t *rp, *pos, *new_id;
    int64_t N, nnz;
    __device__ int64_t rows() const { return N; }
    __device__ int32_t start(int64_t i) const { return pos[clamp_to(rp[i], nnz)]; }
    __device__ int32_t id(int64_t i) const { return new_id[i]; }
    __device__ int32_t end() const { return pos[nnz]; }
};

// The partition of new_row_pointers (gnna_parts.h); the number of groups is read on the device.
__global__ void __launch_bounds__(kBlock)
part_fill_kernel(const KeptRows rows, const int32_t *__restrict__ first_part, int partSize, int64_t capacity,
                 int32_t *__restrict__ pp, int32_t *__restrict__ p2n, long long *__restrict__ rec)
{
    const int64_t num_parts = first_part[rows.N];
    if (blockIdx.x == 0 && threadIdx.x == 0) rec[REC_PARTS] = num_parts;
    if (num_parts > capacity) return;                         // (the call fails)
    fill_parts(rows, first_part, partSize, num_parts, pp, p2n);
}

// ---- the gathers ---------------------------------------------------------------------------------------------------------------

struct GatherArgs {
    const float *X;              // forward: the rows; backward: the saved input (d_scale) or null
    size_t ldx;
    const int32_t *idx;          // forward: perm [M]; backward: new_id [N]
    const float *scale;          // [N] or null
    const float *dY;             // backward: [M, D]
    size_t lddy;
    float *out;                  // forward: [M, D]; backward: d_input [N, D] or null
    size_t ldo;
    float *d_scale;              // backward: [N] or null
    int64_t N, M;                // input rows, gathered rows
    int D;
};

template <int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
gather_rows_kernel(const GatherArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, U = kRowsInFlight;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t base = wave * (R * U); base < p.M; base += waves * (R * U)) {
        int64_t src[U];
        float s[U];
        bool in[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int64_t i = base + k * R + sub;
            in[k] = i < p.M;
            src[k] = -1;
            s[k] = 1.f;
            if (in[k]) {
                const int32_t r = p.idx[i];
                if ((uint32_t)r < (uint64_t)p.N) {
                    src[k] = r;
                    if (p.scale) s[k] = p.scale[r];
                }
            }
        }
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            if (n4 <= 0) continue;
            VT v[U];
#pragma unroll
            for (int k = 0; k < U; k++) {
                v[k] = (VT)(0.f);
                if (src[k] >= 0) v[k] = load_piece(p.X + (size_t)src[k] * p.ldx + (size_t)mycol, n4);
            }
#pragma unroll
            for (int k = 0; k < U; k++) {
                if (!in[k]) continue;
                if (p.scale && src[k] >= 0) v[k] = s[k] * v[k];
                store_piece(p.out + (size_t)(base + k * R + sub) * p.ldo + (size_t)mycol, v[k], n4);
            }
        }
    }
}

template <int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
gather_rows_bwd_kernel(const GatherArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, U = kRowsInFlight;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * kWavesPerBlock;
    const bool want_scale = p.d_scale != nullptr;
    // (every lane of a wavefront makes the same steps: the sum over the lanes of a row is wave-wide)
    for (int64_t base = wave * (R * U); base < p.N; base += waves * (R * U)) {
        int64_t j[U];
        float s[U], dot[U];
        bool in[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int64_t r = base + k * R + sub;
            in[k] = r < p.N;
            j[k] = -1;
            s[k] = 1.f;
            dot[k] = 0.f;
            if (in[k]) {
                const int32_t t = p.idx[r];
                if ((uint32_t)t < (uint64_t)p.M) {
                    j[k] = t;
                    if (p.scale) s[k] = p.scale[r];
                }
            }
        }
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            if (n4 <= 0) continue;
            VT d[U], x[U];
#pragma unroll
            for (int k = 0; k < U; k++) {
                d[k] = (VT)(0.f);
                x[k] = (VT)(0.f);
                if (j[k] >= 0) {
                    d[k] = load_piece(p.dY + (size_t)j[k] * p.lddy + (size_t)mycol, n4);
                    if (want_scale) x[k] = load_piece(p.X + (size_t)(base + k * R + sub) * p.ldx + (size_t)mycol, n4);
                }
            }
#pragma unroll
            for (int k = 0; k < U; k++) {
                if (want_scale) {
#pragma unroll
                    for (int q = 0; q < 4; q++) dot[k] += d[k][q] * x[k][q];      // (columns past the row hold 0)
                }
                if (!in[k] || !p.out) continue;
                if (p.scale && j[k] >= 0) d[k] = s[k] * d[k];
                store_piece(p.out + (size_t)(base + k * R + sub) * p.ldo + (size_t)mycol, d[k], n4);
            }
        }
        if (want_scale) {
#pragma unroll
            for (int k = 0; k < U; k++) {
                const float sum = gat::head_sum<LPR>(dot[k]);
                if (in[k] && cl == 0) p.d_scale[base + k * R + sub] = j[k] >= 0 ? sum : 0.f;
            }
        }
    }
}

int launch_gather(bool backward, DeviceState *ds, hipStream_t stream, const GatherArgs &a)
{
    const int log_lpr = log2_lanes(a.D, 4);
    const int64_t rows = backward ? a.N : a.M;
    const int64_t per_wave = (int64_t)(kWave >> log_lpr) * kRowsInFlight;
    const int64_t waves = (rows + per_wave - 1) / per_wave;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((waves + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ds->num_cus * 16));
    dispatch_lpr(log_lpr, [&](auto L) {
        if (backward) hipLaunchKernelGGL((gather_rows_bwd_kernel<decltype(L)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, a);
        else hipLaunchKernelGGL((gather_rows_kernel<decltype(L)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, a);
    });
    return launch_ok(backward ? "row gather backward launch" : "row gather launch");
}

// what both gather entries check alike, before any device work
int check_gather_sizes(const char *what, int64_t num_in_rows, int64_t num_out_rows, int dim)
{
    if (dim < 1) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dim must be >= 1 (got %d)", what, dim);
    if (num_in_rows < 0 || num_out_rows < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_in_rows=%lld num_out_rows=%lld)", what, (long long)num_in_rows,
                    (long long)num_out_rows);
    if (num_in_rows > 0x7fffffffll || num_out_rows > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 2147483647: the row ids are int32)", what,
                    (long long)std::max(num_in_rows, num_out_rows));
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int64_t gnna_topk_keep_count(int64_t n, double ratio, int64_t k_fixed)
{
    const bool by_ratio = ratio > 0.0 && ratio <= 1.0 && k_fixed == 0, by_k = ratio == 0.0 && k_fixed >= 1;
    if (n < 0 || !(by_ratio || by_k)) return -1;
    return keep_count(n, ratio, k_fixed);
}

int gnna_segment_topk_i32(const float *score, int64_t num_rows, const int32_t *graph_pointers, int64_t num_segments, double ratio,
                          int64_t k_fixed, const int32_t *row_pointers, const int32_t *column_index, int64_t nnz, int partSize,
                          int32_t *new_id, int32_t *perm, int32_t *new_graph_pointers, int32_t *new_row_pointers,
                          int32_t *new_column_index, int32_t *edge_ids, int32_t *partPtr, int32_t *part2Node, int64_t row_capacity,
                          int64_t edge_capacity, int64_t part_capacity, int64_t counts[3], void *stream_v)
{
    static const char what[] = "gnna_segment_topk_i32";
    if (!counts) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null counts", what);
    counts[0] = counts[1] = counts[2] = 0;
    if (num_rows < 0 || num_segments < 0 || nnz < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_rows=%lld num_segments=%lld nnz=%lld)", what, (long long)num_rows,
                    (long long)num_segments, (long long)nnz);
    if (num_segments >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld segments in one call (at most 536870911): shard the batch", what,
                    (long long)num_segments);
    if (num_rows > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 2147483647: graph_pointers is int32)", what,
                    (long long)num_rows);
    if (nnz > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld edges in one call (at most 2147483647: row_pointers is int32)", what, (long long)nnz);
    if (ratio != 0.0 && k_fixed != 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: ratio and k_fixed are both given (ratio=%g k_fixed=%lld): one of them is 0", what, ratio,
                    (long long)k_fixed);
    if (ratio == 0.0 && k_fixed == 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: neither ratio nor k_fixed is given", what);
    if (k_fixed < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: k_fixed must be >= 1 (got %lld)", what, (long long)k_fixed);
    if (k_fixed == 0 && !(ratio > 0.0 && ratio <= 1.0))         // (a NaN fails the first comparison)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: ratio must be in (0, 1] (got %g)", what, ratio);
    if (row_capacity < 0 || edge_capacity < 0 || part_capacity < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative capacity (row_capacity=%lld edge_capacity=%lld part_capacity=%lld)", what,
                    (long long)row_capacity, (long long)edge_capacity, (long long)part_capacity);
    if (partSize < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must not be negative (got %d)", what, partSize);
    if ((row_pointers != nullptr) != (column_index != nullptr) && (nnz > 0 || !row_pointers))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row_pointers and column_index come together", what);
    const bool csr = row_pointers != nullptr, parts = partSize > 0;
    if (parts && !csr) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: a partition (partSize=%d) needs row_pointers and column_index", what, partSize);
    if (!new_graph_pointers || !graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers or new_graph_pointers", what);
    if (num_rows > 0 && (!score || !new_id)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null score or new_id", what);
    if (row_capacity > 0 && !perm) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null perm", what);
    if (csr && (!new_row_pointers || (edge_capacity > 0 && !new_column_index)))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null new_row_pointers or new_column_index", what);
    if (parts && (!partPtr || (part_capacity > 0 && !part2Node))) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null partPtr or part2Node", what);
    {
        const void *const ins[4] = {score, graph_pointers, row_pointers, column_index};
        const void *const outs[8] = {new_id, perm, new_graph_pointers, csr ? new_row_pointers : nullptr, csr ? new_column_index : nullptr,
                                     csr ? edge_ids : nullptr, parts ? partPtr : nullptr, parts ? part2Node : nullptr};
        const int rc = gat::check_alias(what, ins, outs);
        if (rc != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = refuse_capture(what, stream);
    if (rc != GNNA_OK) return rc;
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    row_capacity = std::min<int64_t>(row_capacity, 0x7fffffffll);            // positions are int32
    edge_capacity = std::min<int64_t>(edge_capacity, 0x7fffffffll);
    part_capacity = std::min<int64_t>(part_capacity, 0x7fffffffll);

    // scratch: [record][keep: N + 1] (cleared together) [groups per row: N + 1][flag: nnz + 1][scan partials]
    Carver c;
    const size_t o_rec = c.add(REC_WORDS * sizeof(long long)), o_keep = c.add((size_t)(num_rows + 1) * 4), cleared_bytes = c.bytes;
    const size_t o_groups = parts ? c.add((size_t)(num_rows + 1) * 4) : 0, o_flag = csr ? c.add((size_t)(nnz + 1) * 4) : 0;
    const size_t o_partial = c.add((size_t)scan_tiles(std::max(num_rows, csr ? nnz : 0) + 1) * 4);
    void *ws = nullptr;
    if ((rc = get_workspace(ds, stream, kSlotTopk, c.bytes, &ws)) != GNNA_OK) return rc;
    long long *rec = Carver::at<long long>(ws, o_rec);
    int32_t *keep = Carver::at<int32_t>(ws, o_keep), *groups = parts ? Carver::at<int32_t>(ws, o_groups) : nullptr;
    int32_t *flag = csr ? Carver::at<int32_t>(ws, o_flag) : nullptr, *partial = Carver::at<int32_t>(ws, o_partial);

    const dim3 block(kBlock);
    launch_clear_words(ds, stream, static_cast<int32_t *>(ws), (int64_t)(cleared_bytes / 4));
    if (num_segments > 0 && num_rows > 0) {
        const SelectArgs sa{score, graph_pointers, num_rows, num_segments, ratio, k_fixed, keep};
        hipLaunchKernelGGL(select_wave_kernel, dim3((unsigned)((num_segments + kWavesPerBlock - 1) / kWavesPerBlock)), block, 0, stream, sa);
        hipLaunchKernelGGL(select_block_kernel, dim3((unsigned)num_segments), block, 0, stream, sa);
    }
    if ((rc = launch_exclusive_scan(stream, keep, num_rows + 1, partial)) != GNNA_OK) return rc;
    hipLaunchKernelGGL(ids_kernel, dim3(elementwise_grid(std::max(num_rows, num_segments + 1), ds->num_cus, 16)), block, 0, stream, keep,
                       num_rows, graph_pointers, num_segments, new_id, perm, new_graph_pointers, row_capacity, rec);
    if (csr) {
        hipLaunchKernelGGL(edge_flag_kernel, dim3(elementwise_grid(std::max(num_rows, nnz) + 1, ds->num_cus, 16)), block, 0, stream,
                           row_pointers, column_index, num_rows, nnz, new_id, flag, rec);
        if ((rc = launch_exclusive_scan(stream, flag, nnz + 1, partial)) != GNNA_OK) return rc;
        const FillArgs fa{row_pointers, column_index, num_rows, nnz, new_id, keep, flag, new_row_pointers, new_column_index, edge_ids,
                          row_capacity, edge_capacity, groups, partSize, rec};
        hipLaunchKernelGGL(edge_fill_kernel, dim3(elementwise_grid(std::max(num_rows, nnz) + 1, ds->num_cus, 16)), block, 0, stream, fa);
        if (parts) {
            if ((rc = launch_exclusive_scan(stream, groups, num_rows + 1, partial)) != GNNA_OK) return rc;
            hipLaunchKernelGGL(part_fill_kernel, dim3(elementwise_grid(part_capacity + 1, ds->num_cus, 16)), block, 0, stream,
                               KeptRows{row_pointers, flag, new_id, num_rows, nnz}, groups, partSize, part_capacity, partPtr, part2Node, rec);
        }
    }
    long long host[REC_WORDS] = {0};
    if ((rc = read_record(what, stream, rec, host, REC_WORDS)) != GNNA_OK) return rc;
    counts[0] = host[REC_ROWS];
    counts[1] = csr ? host[REC_EDGES] : 0;
    counts[2] = parts ? host[REC_PARTS] : 0;
    if (csr && host[REC_BAD_ROW])
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row_pointers must start at 0, ascend and end at nnz = %lld (row_pointers[%lld] does not)",
                    what, (long long)nnz, host[REC_BAD_ROW] - 1);
    if (counts[0] > row_capacity || counts[1] > edge_capacity || counts[2] > part_capacity)
        return fail(GNNA_ERR_INVALID_ARGUMENT,
                    "%s: capacity too small: the selection has %lld rows, %lld edges and %lld neighbor-groups, row_capacity=%lld "
                    "edge_capacity=%lld part_capacity=%lld", what, (long long)counts[0], (long long)counts[1], (long long)counts[2],
                    (long long)row_capacity, (long long)edge_capacity, (long long)part_capacity);
    return GNNA_OK;
}

int gnna_gather_rows_scale_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows, const int32_t *perm, const float *scale,
                                  float *out, int64_t ld_out, int64_t num_out_rows, int dim, void *stream_v)
{
    static const char what[] = "gnna_gather_rows_scale_ld_f32";
    int rc = check_gather_sizes(what, num_in_rows, num_out_rows, dim);
    if (rc != GNNA_OK) return rc;
    if (bad_ld(ld_in, dim) || bad_ld(ld_out, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_out=%lld dim=%d)", what,
                    (long long)ld_in, (long long)ld_out, dim);
    const void *const ins[3] = {input, perm, scale};
    const void *const outs[1] = {out};
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(out);
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, scale, row id and output pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;
    if (!out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer", what);
    if (!perm) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null perm", what);
    if (num_in_rows > 0 && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    GatherArgs a{};
    a.X = input; a.ldx = (size_t)ld_in; a.idx = perm; a.scale = num_in_rows > 0 ? scale : nullptr;
    a.out = out; a.ldo = (size_t)ld_out; a.N = num_in_rows; a.M = num_out_rows; a.D = dim;
    return launch_gather(false, ds, static_cast<hipStream_t>(stream_v), a);
}

int gnna_gather_rows_scale_backward_ld_f32(const float *d_out, int64_t ld_dout, int64_t num_out_rows, const int32_t *new_id,
                                           const float *input, int64_t ld_in, const float *scale, float *d_input, int64_t ld_din,
                                           float *d_scale, int64_t num_in_rows, int dim, void *stream_v)
{
    static const char what[] = "gnna_gather_rows_scale_backward_ld_f32";
    int rc = check_gather_sizes(what, num_in_rows, num_out_rows, dim);
    if (rc != GNNA_OK) return rc;
    if (!d_input && !d_scale) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointers: d_input and d_scale are both null", what);
    // (a null pointer leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_dout, dim) || (d_input ? bad_ld(ld_din, dim) : ld_din >= ((int64_t)1 << 29)) ||
        (d_scale ? bad_ld(ld_in, dim) : ld_in >= ((int64_t)1 << 29)))
        return fail(GNNA_ERR_INVALID_ARGUMENT,
                    "%s: row strides must be >= dim and < 2^29 elements (ld_dout=%lld ld_in=%lld ld_din=%lld dim=%d)", what,
                    (long long)ld_dout, (long long)ld_in, (long long)ld_din, dim);
    const void *const ins[4] = {d_out, new_id, input, scale};
    const void *const outs[2] = {d_input, d_scale};
    uintptr_t low_bits = 0;
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    for (const void *q : outs) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: gradient, feature, scale and row id pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_in_rows == 0) return GNNA_OK;
    if (!new_id) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null new_id", what);
    if (d_scale && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: d_scale needs the feature pointer", what);
    if (num_out_rows > 0 && !d_out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null gradient pointer", what);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    GatherArgs a{};
    a.X = d_scale ? input : nullptr; a.ldx = (size_t)ld_in; a.idx = new_id; a.scale = scale;
    a.dY = d_out; a.lddy = (size_t)ld_dout; a.out = d_input; a.ldo = (size_t)ld_din; a.d_scale = d_scale;
    a.N = num_in_rows; a.M = num_out_rows; a.D = dim;
    return launch_gather(true, ds, static_cast<hipStream_t>(stream_v), a);
}

}  // extern "C"

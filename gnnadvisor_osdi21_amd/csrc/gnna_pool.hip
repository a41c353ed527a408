// gnna_pool.hip -- graph-level readout: sum / mean / max / min over the rows of every graph of a batch, and the backward pass
// (gnna_segment_pool_ld_f32, gnna_segment_pool_backward_ld_f32; include/gnna_pool.h).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its models stop at one row per node, GNNAdvisor/gnn_conv.py).
//
// The segments are contiguous row ranges whose sizes only the device knows, so the work is split by rows: a wavefront owns a tile
// of GNNA_POOL_TILE_ROWS consecutive rows, a workgroup four tiles.  The lane layout is that of the reduce / stats kernels:
// LPR = next_pow2(ceil(D / 4)) lanes per row with 16-byte loads, 64 / LPR partial rows ("slots") per wavefront, column blocks of
// 256 floats for wider rows, element-wise loads for a partial last vector.
//   * pool_tile_kernel: the wavefront finds the segment of its first row by binary search in graph_pointers and walks the
//     segments of its tile one after the other.  The slots stride over the rows of a piece, kRowsInFlight rows per slot and step;
//     per lane and element a running sum, a max key and a min key (gnna_keys.h, with the row as the position).  The slots meet by
//     the folds of the stats kernel.  A segment that lies inside the tile is written at once; a piece of a segment that crosses the
//     tile's first row goes to piece 0 of the tile in library scratch, one that only crosses its last row to piece 1.
//   * pool_finish_kernel: one wavefront per segment.  A segment inside one tile is done, an empty one gets its zeros, one that
//     spans the tiles tf .. tl joins piece 1 of tf and piece 0 of the others: slot t takes the tiles tf + t, tf + t + slots, ...
//     in order, then the slots meet as above.  A segment of more than kLongSteps steps goes to the whole workgroup after the short
//     ones, whose wavefronts meet through LDS in the order of the wavefronts.
//   * pool_bwd_kernel: the same tiles and search; every lane keeps the segment of its row and moves on as its rows rise.
// One writer per element, plain stores, every order fixed by (num_rows, dim, graph_pointers): the same bits on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gnna_pool.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::load_piece, gat::slots_sum, gat::check_alias
#include "gnna_internal.h"
#include "gnna_keys.h"
#include "gnna_segments.h"

namespace gnna {
namespace {

using gat::VT;
using gat::load_piece;
using seg::kTile;
using seg::kRowsInFlight;
using seg::kLongSteps;
using seg::seg_ptr;
using seg::first_segment;
using seg::uniform64;
using seg::store_piece;

struct PoolArgs {
    const float *X;             // forward: the rows
    size_t ldx;
    const int32_t *gp;          // graph_pointers [G + 1]
    int64_t N, G;               // rows (< 2^31), segments
    float *sum;                 // forward outputs, any may be null
    float *mx, *mn;
    int32_t *amx, *amn;
    size_t lds, ldmx, ldamx, ldmn, ldamn;
    float *Ps;                  // pieces in scratch: [tiles][2][D] sums, max keys, min keys
    u64 *Pmax, *Pmin;
    int D, mean;
};

// what a lane holds of a piece or a segment: four columns
struct Acc {
    VT sum;
    u64 hi[4], lo[4];
};

__device__ __forceinline__ void acc_clear(Acc &a)
{
    a.sum = (VT)(0.f);
#pragma unroll
    for (int q = 0; q < 4; q++) { a.hi[q] = 0ull; a.lo[q] = 0ull; }
}

// the 64 / LPR slots of a wavefront -> one, in every lane
template <bool SUM, bool EXT, int LPR>
__device__ __forceinline__ void acc_fold(Acc &a)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if constexpr (SUM) a.sum[q] = gat::slots_sum<LPR>(a.sum[q]);
        if constexpr (EXT) {
            a.hi[q] = partial_rows_max<kWave / LPR>(a.hi[q]);
            a.lo[q] = partial_rows_max<kWave / LPR>(a.lo[q]);
        }
    }
}

// the final values of segment g (count rows) from a lane's four columns at mycol, the first n4 (1 .. 4 and more) of them
template <bool SUM, bool EXT>
__device__ __forceinline__ void write_segment(const PoolArgs &p, int64_t g, int64_t count, int mycol, int n4, const Acc &a)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (q >= n4) break;
        const size_t c = (size_t)(mycol + q);
        if constexpr (SUM) {
            if (p.sum) {
                float v = a.sum[q];
                if (p.mean) v = count > 0 ? v / (float)count : 0.f;
                p.sum[(size_t)g * p.lds + c] = v;
            }
        }
        if constexpr (EXT) {
            float v;
            int32_t pos;
            if (p.mx) {
                key_result(a.hi[q], GNNA_REDUCE_MAX, &v, &pos);
                p.mx[(size_t)g * p.ldmx + c] = v;
                if (p.amx) p.amx[(size_t)g * p.ldamx + c] = pos;
            }
            if (p.mn) {
                key_result(a.lo[q], GNNA_REDUCE_MIN, &v, &pos);
                p.mn[(size_t)g * p.ldmn + c] = v;
                if (p.amn) p.amn[(size_t)g * p.ldamn + c] = pos;
            }
        }
    }
}

// ---- forward: the tiles ------------------------------------------------------------------------------------------------------

template <bool SUM, bool EXT, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
pool_tile_kernel(const PoolArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, U = kRowsInFlight;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t r0 = tile * kTile;
    if (r0 >= p.N) return;                                        // (the whole wavefront)
    const int64_t r1 = r0 + kTile < p.N ? r0 + kTile : p.N;
    for (int64_t g = uniform64(first_segment(p.gp, p.G, p.N, r0)); g < p.G; g++) {
        const int64_t S = uniform64(seg_ptr(p.gp, p.N, g)), E = uniform64(seg_ptr(p.gp, p.N, g + 1));
        if (S >= r1) break;
        const int64_t a = S > r0 ? S : r0, b = E < r1 ? E : r1;
        if (b <= a) continue;                                     // an empty segment, or one that descends: the finish kernel's
        const bool closed = S >= r0 && E <= r1;
        const size_t piece = (size_t)tile * 2 + (S < r0 ? 0 : 1);
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            const bool ok = n4 > 0;
            Acc acc;
            acc_clear(acc);
#pragma unroll 1
            for (int64_t base = a; base < b; base += R * U) {
                VT v[U];
                bool in[U];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const int64_t row = base + k * R + sub;
                    in[k] = row < b && ok;
                    v[k] = (VT)(0.f);
                    if (in[k]) v[k] = load_piece(p.X + (size_t)row * p.ldx + (size_t)mycol, n4);
                }
#pragma unroll
                for (int k = 0; k < U; k++) {
                    // (rows rise with k and base: the low word falls, so among equal values the first row stays)
                    const uint32_t npos = 0xFFFFFFFFu - (uint32_t)(base + k * R + sub);
                    if constexpr (SUM) acc.sum += v[k];           // (a row past the piece holds 0)
                    if constexpr (EXT) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            acc.hi[q] = umax64(acc.hi[q], in[k] ? pack(order_of<GNNA_REDUCE_MAX>(v[k][q]), npos) : 0ull);
                            acc.lo[q] = umax64(acc.lo[q], in[k] ? pack(order_of<GNNA_REDUCE_MIN>(v[k][q]), npos) : 0ull);
                        }
                    }
                }
            }
            acc_fold<SUM, EXT, LPR>(acc);
            if (sub != 0 || !ok) continue;
            if (closed) {
                write_segment<SUM, EXT>(p, g, E - S, mycol, n4, acc);
            } else {
                const size_t at = piece * (size_t)p.D + (size_t)mycol;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (q >= n4) break;
                    if constexpr (SUM) p.Ps[at + q] = acc.sum[q];
                    if constexpr (EXT) {
                        p.Pmax[at + q] = acc.hi[q];
                        p.Pmin[at + q] = acc.lo[q];
                    }
                }
            }
        }
    }
}

// ---- forward: the segments ---------------------------------------------------------------------------------------------------

template <bool SUM, bool EXT, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
pool_finish_kernel(const PoolArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR;
    __shared__ int s_long[kWavesPerBlock];
    __shared__ int s_nlong;
    __shared__ float s_sum[4][kWavesPerBlock][LPR];
    __shared__ u64 s_hi[4][kWavesPerBlock][LPR], s_lo[4][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    const int64_t g0 = (int64_t)blockIdx.x * kWavesPerBlock;
    const int64_t g = g0 + wib;
    const bool valid = g < p.G;
    int64_t S = 0, E = 0;
    if (valid) { S = uniform64(seg_ptr(p.gp, p.N, g)); E = uniform64(seg_ptr(p.gp, p.N, g + 1)); }
    const bool empty = E <= S;
    // a segment of the tiles tf .. tl; inside one tile: the tile kernel has written it
    const int64_t tf = empty ? 0 : S / kTile, tl = empty ? 0 : (E - 1) / kTile;
    const int64_t nt = tl > tf ? tl - tf + 1 : 0;
    const bool is_long = nt > (int64_t)R * kLongSteps;
    if (is_long && lane == 0) s_long[atomicAdd(&s_nlong, 1)] = wib;
    __syncthreads();
    // k = -1: the short segments (and the empty ones), a wavefront each; k >= 0: the long ones, the whole block, one after the
    // other (the list's order may vary; a segment's result does not depend on it)
    const int nlong = s_nlong;
    for (int k = -1; k < nlong; k++) {
        const bool whole = k >= 0;
        int64_t gg = g, cnt = empty ? 0 : E - S, first = tf, n = is_long ? 0 : nt;
        if (whole) {
            gg = g0 + s_long[k];
            const int64_t s2 = seg_ptr(p.gp, p.N, gg), e2 = seg_ptr(p.gp, p.N, gg + 1);
            cnt = e2 - s2;
            first = s2 / kTile;
            n = (e2 - 1) / kTile - first + 1;
        }
        const int t = whole ? wib * R + sub : sub, nl = whole ? kWavesPerBlock * R : R;
        const bool writer = whole ? wib == 0 : (valid && !is_long && (empty || nt > 0));
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            const bool ok = n4 > 0;
            Acc acc;
            acc_clear(acc);
            if (ok) {
#pragma unroll 2
                for (int64_t i = t; i < n; i += nl) {
                    // the first tile's piece is the one that crosses its last row, every other tile's crosses its first
                    const size_t at = ((size_t)(first + i) * 2 + (i == 0 ? 1 : 0)) * (size_t)p.D + (size_t)mycol;
                    if constexpr (SUM) acc.sum += load_piece(p.Ps + at, n4);
                    if constexpr (EXT) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            if (q >= n4) break;
                            acc.hi[q] = umax64(acc.hi[q], p.Pmax[at + q]);
                            acc.lo[q] = umax64(acc.lo[q], p.Pmin[at + q]);
                        }
                    }
                }
            }
            acc_fold<SUM, EXT, LPR>(acc);
            if (whole) {
                // the wavefronts meet through LDS, in the order of the wavefronts
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if constexpr (SUM) s_sum[q][wib][cl] = acc.sum[q];
                        if constexpr (EXT) { s_hi[q][wib][cl] = acc.hi[q]; s_lo[q][wib][cl] = acc.lo[q]; }
                    }
                }
                __syncthreads();
                acc_clear(acc);
#pragma unroll
                for (int w = 0; w < kWavesPerBlock; w++) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if constexpr (SUM) acc.sum[q] += s_sum[q][w][cl];
                        if constexpr (EXT) {
                            acc.hi[q] = umax64(acc.hi[q], s_hi[q][w][cl]);
                            acc.lo[q] = umax64(acc.lo[q], s_lo[q][w][cl]);
                        }
                    }
                }
            }
            if (writer && sub == 0 && ok) write_segment<SUM, EXT>(p, gg, cnt, mycol, n4, acc);
        }
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------

struct BwdArgs {
    const float *dsum, *dmax, *dmin;    // any may be null
    const int32_t *amx, *amn;
    size_t ldds, lddmx, ldamx, lddmn, ldamn;
    const int32_t *gp;
    int64_t N, G;
    float *dX;
    size_t lddx;
    int D, mean;
};

typedef int32_t i32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// the first n4 (<= 4) ints at q, the others -1
__device__ __forceinline__ i32x4 load_ipiece(const int32_t *__restrict__ q, int n4)
{
    if (n4 >= 4) return *reinterpret_cast<const i32x4u *>(q);
    i32x4 v = (i32x4)(-1);
    if (n4 > 0) v[0] = q[0];
    if (n4 > 1) v[1] = q[1];
    if (n4 > 2) v[2] = q[2];
    return v;
}

template <int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
pool_bwd_kernel(const BwdArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t r0 = tile * kTile;
    if (r0 >= p.N) return;
    const int64_t r1 = r0 + kTile < p.N ? r0 + kTile : p.N;
    // this lane's segment: the first whose end lies beyond its row; it moves on as the lane's rows rise
    int64_t g = first_segment(p.gp, p.G, p.N, r0);
    int64_t S = 0, E = 0;
    if (g < p.G) { S = seg_ptr(p.gp, p.N, g); E = seg_ptr(p.gp, p.N, g + 1); }
    for (int64_t row = r0 + sub; row < r1; row += R) {
        while (g < p.G && row >= E) {
            g++;
            if (g < p.G) { S = seg_ptr(p.gp, p.N, g); E = seg_ptr(p.gp, p.N, g + 1); }
        }
        const bool in = g < p.G && row >= S && row < E;
        const float s = p.mean && in ? 1.0f / (float)(E - S) : 1.0f;
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            if (n4 <= 0) continue;
            VT out = (VT)(0.f);
            if (in) {
                if (p.dsum) {
                    out = load_piece(p.dsum + (size_t)g * p.ldds + (size_t)mycol, n4);
                    if (p.mean) out = s * out;
                }
                if (p.dmax) {
                    const i32x4 am = load_ipiece(p.amx + (size_t)g * p.ldamx + (size_t)mycol, n4);
                    const VT d = load_piece(p.dmax + (size_t)g * p.lddmx + (size_t)mycol, n4);
#pragma unroll
                    for (int q = 0; q < 4; q++) out[q] += (int64_t)am[q] == row ? d[q] : 0.f;
                }
                if (p.dmin) {
                    const i32x4 am = load_ipiece(p.amn + (size_t)g * p.ldamn + (size_t)mycol, n4);
                    const VT d = load_piece(p.dmin + (size_t)g * p.lddmn + (size_t)mycol, n4);
#pragma unroll
                    for (int q = 0; q < 4; q++) out[q] += (int64_t)am[q] == row ? d[q] : 0.f;
                }
            }
            store_piece(p.dX + (size_t)row * p.lddx + (size_t)mycol, out, n4);
        }
    }
}

// Scratch of the forward entry: slot 13 = the pieces of the tiles (max keys, min keys, sums; seg::get_pieces).
constexpr int kSlotPoolPieces = 13;

// what both entries check alike, before any device work
int check_sizes(const char *what, int64_t num_rows, int64_t num_segments, int dim, unsigned flags)
{
    if (flags & ~GNNA_POOL_MEAN)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x (GNNA_POOL_MEAN is the only flag)", what, flags & ~GNNA_POOL_MEAN);
    const int rc = seg::check_dim(what, dim);
    return rc != GNNA_OK ? rc : seg::check_counts(what, num_rows, num_segments);
}

template <bool SUM, bool EXT>
int launch_forward(int log_lpr, hipStream_t stream, const PoolArgs &a)
{
    return seg::launch_tiles_then_finish("segment pooling", log_lpr, stream, a, [](auto L) {
        return std::make_pair(pool_tile_kernel<SUM, EXT, decltype(L)::value>, pool_finish_kernel<SUM, EXT, decltype(L)::value>);
    });
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_segment_pool_ld_f32(const float *input, int64_t ld_in, int64_t num_rows, const int32_t *graph_pointers, int64_t num_segments,
                             float *sum, int64_t ld_sum, float *max_out, int64_t ld_max, int32_t *argmax, int64_t ld_argmax,
                             float *min_out, int64_t ld_min, int32_t *argmin, int64_t ld_argmin, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_pool_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, flags);
    if (rc != GNNA_OK) return rc;
    if (!sum && !max_out && !min_out)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: no statistic asked for: sum, max_out and min_out are all null", what);
    if ((argmax && !max_out) || (argmin && !min_out))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: %s without %s: rows come with their values", what,
                    argmax && !max_out ? "argmax" : "argmin", argmax && !max_out ? "max_out" : "min_out");
    // (a null output leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld_of(sum, ld_sum, dim) || bad_ld_of(max_out, ld_max, dim) || bad_ld_of(argmax, ld_argmax, dim) ||
        bad_ld_of(min_out, ld_min, dim) || bad_ld_of(argmin, ld_argmin, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_sum=%lld ld_max=%lld "
                    "ld_argmax=%lld ld_min=%lld ld_argmin=%lld dim=%d)", what, (long long)ld_in, (long long)ld_sum, (long long)ld_max,
                    (long long)ld_argmax, (long long)ld_min, (long long)ld_argmin, dim);
    const void *const ins[2] = {input, graph_pointers};
    const void *const outs[5] = {sum, max_out, argmax, min_out, argmin};
    uintptr_t low_bits = 0;
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    for (const void *q : outs) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, pointer, statistic and arg pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_segments == 0) return GNNA_OK;
    if (!graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    if (num_rows > 0 && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    const bool want_sum = sum != nullptr, extrema = max_out || min_out;
    PoolArgs a;
    a.X = input; a.ldx = (size_t)ld_in; a.gp = graph_pointers; a.N = num_rows; a.G = num_segments;
    a.sum = sum; a.mx = max_out; a.mn = min_out; a.amx = argmax; a.amn = argmin;
    a.lds = (size_t)ld_sum; a.ldmx = (size_t)ld_max; a.ldamx = (size_t)ld_argmax; a.ldmn = (size_t)ld_min; a.ldamn = (size_t)ld_argmin;
    a.D = dim; a.mean = (flags & GNNA_POOL_MEAN) ? 1 : 0;
    // the keys first, so that they are 8-byte aligned
    const size_t key_bytes = extrema ? (size_t)dim * sizeof(u64) : 0;
    const size_t piece_bytes[3] = {key_bytes, key_bytes, want_sum ? (size_t)dim * sizeof(float) : 0};
    void *pieces[3];
    if ((rc = seg::get_pieces(ds, stream, kSlotPoolPieces, num_rows, piece_bytes, pieces)) != GNNA_OK) return rc;
    a.Pmax = static_cast<u64 *>(pieces[0]); a.Pmin = static_cast<u64 *>(pieces[1]); a.Ps = static_cast<float *>(pieces[2]);
    const int log_lpr = log2_lanes(dim, 4);
    if (want_sum && extrema) return launch_forward<true, true>(log_lpr, stream, a);
    if (want_sum) return launch_forward<true, false>(log_lpr, stream, a);
    return launch_forward<false, true>(log_lpr, stream, a);
}

int gnna_segment_pool_backward_ld_f32(const float *d_sum, int64_t ld_dsum, const float *d_max, int64_t ld_dmax, const int32_t *argmax,
                                      int64_t ld_argmax, const float *d_min, int64_t ld_dmin, const int32_t *argmin, int64_t ld_argmin,
                                      const int32_t *graph_pointers, int64_t num_segments, float *d_input, int64_t ld_din,
                                      int64_t num_rows, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_pool_backward_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, flags);
    if (rc != GNNA_OK) return rc;
    if (!d_sum && !d_max && !d_min)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: no gradient given: d_sum, d_max and d_min are all null", what);
    if ((d_max != nullptr) != (argmax != nullptr) || (d_min != nullptr) != (argmin != nullptr)) {
        const bool mx = (d_max != nullptr) != (argmax != nullptr);
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: %s and %s come together", what, mx ? "d_max" : "d_min", mx ? "argmax" : "argmin");
    }
    if (bad_ld(ld_din, dim) || bad_ld_of(d_sum, ld_dsum, dim) || bad_ld_of(d_max, ld_dmax, dim) || bad_ld_of(argmax, ld_argmax, dim) ||
        bad_ld_of(d_min, ld_dmin, dim) || bad_ld_of(argmin, ld_argmin, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_dsum=%lld ld_dmax=%lld "
                    "ld_argmax=%lld ld_dmin=%lld ld_argmin=%lld ld_din=%lld dim=%d)", what, (long long)ld_dsum, (long long)ld_dmax,
                    (long long)ld_argmax, (long long)ld_dmin, (long long)ld_argmin, (long long)ld_din, dim);
    const void *const ins[6] = {d_sum, d_max, argmax, d_min, argmin, graph_pointers};
    const void *const outs[1] = {d_input};
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(d_input);
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: gradient, arg and pointer pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_rows == 0) return GNNA_OK;
    if (!d_input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer", what);
    if (num_segments > 0 && !graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    BwdArgs a;
    a.dsum = d_sum; a.dmax = d_max; a.dmin = d_min; a.amx = argmax; a.amn = argmin;
    a.ldds = (size_t)ld_dsum; a.lddmx = (size_t)ld_dmax; a.ldamx = (size_t)ld_argmax; a.lddmn = (size_t)ld_dmin; a.ldamn = (size_t)ld_argmin;
    a.gp = graph_pointers; a.N = num_rows; a.G = num_segments; a.dX = d_input; a.lddx = (size_t)ld_din;
    a.D = dim; a.mean = (flags & GNNA_POOL_MEAN) ? 1 : 0;
    const int64_t tiles = (num_rows + kTile - 1) / kTile;
    const dim3 grid((unsigned)((tiles + kWavesPerBlock - 1) / kWavesPerBlock));
    dispatch_lpr(log2_lanes(dim, 4), [&](auto L) {
        hipLaunchKernelGGL((pool_bwd_kernel<decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("segment pooling backward launch");
}

}  // extern "C"

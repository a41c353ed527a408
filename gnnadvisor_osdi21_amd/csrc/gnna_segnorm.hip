// gnna_segnorm.hip -- per-graph normalisation on a batch of graphs (GraphNorm): the centred moments of the rows of every graph,
// the normalising pass and the backward pass (gnna_segment_moments_ld_f32, gnna_segment_norm_ld_f32,
// gnna_segment_norm_backward_ld_f32; gnna_segnorm.h).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its models have no normalisation layer, GNNAdvisor/gnn_conv.py).
//
// The tiles, the lane layout, the two open pieces of a tile and the join are those of gnna_pool.hip: a wavefront owns a tile of
// GNNA_POOL_TILE_ROWS rows, LPR = next_pow2(ceil(D / 4)) lanes per row with 16-byte loads, 64 / LPR slots per wavefront, column
// blocks of 256 floats for wider rows.  What a lane holds of a piece is a Part: (n, a, b) per column, n shared by its four columns.
//   * MOMENTS / NORM: (n, mean, m2).  The kRowsInFlight rows of a step enter as their own mean and centred sum; two parts meet by
//     the pairwise merge (d = mean_b - mean_a; mean_a + d n_b / n; m2_a + m2_b + d^2 n_a n_b / n).  No raw sum of x^2 exists.
//   * SUMS: (n, A, B) = (rows, sum dY, sum dY xhat) of the backward; two parts meet by addition.
//   * seg_tile_kernel: the walk of pool_tile_kernel.  The slots meet by a butterfly of the merge in which the lower lane is always
//     the left operand, so every lane ends with the same bits.  A closed segment is finished here, an open piece goes to scratch as (a, b): its
//     count follows from the pointers.
//   * seg_finish_kernel: one wavefront per segment joins the pieces (slot t takes the tiles tf + t, tf + t + slots, ... in order,
//     then the butterfly); a segment of more than kLongSteps steps goes to the whole workgroup through LDS, in wavefront order.
//     It writes the empty segments.  NORM turns m2 into rstd here, once per (g, f).
//   * seg_apply_kernel: the walk of pool_bwd_kernel over the same tiles, a column block at a time: a lane carries the segment of
//     its row and reloads the segment's constants only when the segment changes.  Forward: out = weight xhat + bias; backward:
//     d_input.  Streaming: kRowsInFlight loads per lane are issued before the first is used.
// One writer per element, plain stores, every order fixed by (num_rows, dim, graph_pointers): the same bits on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gnna_segnorm.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::load_piece, gat::check_alias
#include "gnna_internal.h"
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

enum Mode { MOMENTS = 0, NORM = 1, SUMS = 2 };

struct SegArgs {
    const float *X;             // the rows
    size_t ldx;
    const float *dY;            // SUMS, backward apply: the gradient of the output rows
    size_t lddy;
    const int32_t *gp;          // graph_pointers [G + 1]
    int64_t N, G;
    const float *weight, *bias, *alpha;     // [D], any may be null
    float eps;
    float *o1, *o2;             // [G, D] outputs of the tile and finish kernels: (mean, m2), (mean, rstd) or (A, B)
    size_t ld1, ld2;
    const float *mean, *rstd;   // [G, D] inputs of SUMS and of the apply kernels
    size_t ldm, ldr;
    const float *A, *B;         // [G, D] inputs of the backward apply
    size_t lda, ldb;
    float *P1, *P2;             // pieces in scratch: [tiles][2][D] each
    float *out;                 // the apply kernels' output rows
    size_t ldo;
    int D;
};

// what a lane holds of a piece or a segment: four columns and the rows behind them
struct Part {
    float n;
    VT a, b;
};

__device__ __forceinline__ Part part_zero() { return Part{0.f, (VT)(0.f), (VT)(0.f)}; }

// x then y.  SUMS: addition.  Otherwise the pairwise merge of (n, mean, m2); a part without rows changes nothing.
template <int MODE>
__device__ __forceinline__ Part part_merge(const Part &x, const Part &y)
{
    Part r;
    r.n = x.n + y.n;
    if constexpr (MODE == SUMS) {
        r.a = x.a + y.a;
        r.b = x.b + y.b;
    } else {
        const float w = r.n > 0.f ? y.n / r.n : 0.f;
        const VT d = y.a - x.a;
        r.a = x.a + d * w;
        r.b = (x.b + y.b) + (d * d) * (x.n * w);
    }
    return r;
}

// the 64 / LPR slots of a wavefront -> one, the same bits in every lane: at every stride the lower lane's part is `x`
template <int MODE, int LPR>
__device__ __forceinline__ Part part_fold(Part v, int lane)
{
#pragma unroll
    for (int d = kWave >> 1; d >= LPR; d >>= 1) {
        Part o;
        o.n = __shfl_xor(v.n, d);
#pragma unroll
        for (int q = 0; q < 4; q++) { o.a[q] = __shfl_xor(v.a[q], d); o.b[q] = __shfl_xor(v.b[q], d); }
        v = (lane & d) ? part_merge<MODE>(o, v) : part_merge<MODE>(v, o);
    }
    return v;
}

__device__ __forceinline__ VT param_or(const float *__restrict__ p, int mycol, int n4, float dflt)
{
    if (!p) return (VT)(dflt);
    return load_piece(p + mycol, n4);
}

// the final values of segment g (count rows; 0: an empty one) from a lane's four columns at mycol, the first n4 of them
template <int MODE>
__device__ __forceinline__ void write_segment(const SegArgs &p, int64_t g, int64_t count, int mycol, int n4, const Part &v)
{
    VT a = v.a, b = v.b;
    if (count <= 0) {
        a = (VT)(0.f);
        b = (VT)(0.f);
    } else if constexpr (MODE == NORM) {
        const VT al = param_or(p.alpha, mycol, n4, 1.f);
        const float nf = (float)count;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float t = (1.f - al[q]) * a[q];
            const float var = b[q] / nf + t * t;
            b[q] = 1.0f / sqrtf(var + p.eps);
        }
    }
    store_piece(p.o1 + (size_t)g * p.ld1 + (size_t)mycol, a, n4);
    store_piece(p.o2 + (size_t)g * p.ld2 + (size_t)mycol, b, n4);
}

// ---- the tiles ---------------------------------------------------------------------------------------------------------------

template <int MODE, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
seg_tile_kernel(const SegArgs p)
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
            VT am = (VT)(0.f), rs = (VT)(0.f);                    // SUMS: alpha * mean and rstd of this segment
            if constexpr (MODE == SUMS) {
                if (ok) {
                    am = param_or(p.alpha, mycol, n4, 1.f) * load_piece(p.mean + (size_t)g * p.ldm + (size_t)mycol, n4);
                    rs = load_piece(p.rstd + (size_t)g * p.ldr + (size_t)mycol, n4);
                }
            }
            Part acc = part_zero();
#pragma unroll 1
            for (int64_t base = a; base < b; base += R * U) {
                VT v[U], dy[U];
                bool in[U];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const int64_t row = base + k * R + sub;
                    in[k] = row < b && ok;
                    v[k] = (VT)(0.f);
                    dy[k] = (VT)(0.f);
                    if (in[k]) {
                        v[k] = load_piece(p.X + (size_t)row * p.ldx + (size_t)mycol, n4);
                        if constexpr (MODE == SUMS) dy[k] = load_piece(p.dY + (size_t)row * p.lddy + (size_t)mycol, n4);
                    }
                }
                if constexpr (MODE == SUMS) {
#pragma unroll
                    for (int k = 0; k < U; k++) {                 // (a row past the piece holds dY = 0)
                        acc.n += in[k] ? 1.f : 0.f;
                        acc.a += dy[k];
                        acc.b += dy[k] * ((v[k] - am) * rs);
                    }
                } else {
                    // the rows of this step as a part of their own: their mean, then the centred sum about it
                    Part st = part_zero();
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        st.n += in[k] ? 1.f : 0.f;
                        st.a += v[k];                             // (a row past the piece holds 0)
                    }
                    st.a = st.a * (st.n > 0.f ? 1.0f / st.n : 0.f);
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const VT d = v[k] - st.a;
                        st.b += in[k] ? d * d : (VT)(0.f);
                    }
                    acc = part_merge<MODE>(acc, st);
                }
            }
            acc = part_fold<MODE, LPR>(acc, lane);
            if (sub != 0 || !ok) continue;
            if (closed) {
                write_segment<MODE>(p, g, E - S, mycol, n4, acc);
            } else {
                const size_t at = piece * (size_t)p.D + (size_t)mycol;
                store_piece(p.P1 + at, acc.a, n4);
                store_piece(p.P2 + at, acc.b, n4);
            }
        }
    }
}

// ---- the segments ------------------------------------------------------------------------------------------------------------

template <int MODE, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
seg_finish_kernel(const SegArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR;
    __shared__ int s_long[kWavesPerBlock];
    __shared__ int s_nlong;
    __shared__ float s_n[kWavesPerBlock][LPR];
    __shared__ float s_a[4][kWavesPerBlock][LPR], s_b[4][kWavesPerBlock][LPR];
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
        int64_t gg = g, s2 = S, e2 = E, first = tf, n = is_long ? 0 : nt;
        if (whole) {
            gg = g0 + s_long[k];
            s2 = seg_ptr(p.gp, p.N, gg);
            e2 = seg_ptr(p.gp, p.N, gg + 1);
            first = s2 / kTile;
            n = (e2 - 1) / kTile - first + 1;
        }
        const int64_t cnt = e2 > s2 ? e2 - s2 : 0;
        const int t = whole ? wib * R + sub : sub, nl = whole ? kWavesPerBlock * R : R;
        const bool writer = whole ? wib == 0 : (valid && !is_long && (empty || nt > 0));
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            const bool ok = n4 > 0;
            Part acc = part_zero();
            if (ok) {
#pragma unroll 2
                for (int64_t i = t; i < n; i += nl) {
                    // the first tile's piece is the one that crosses its last row, every other tile's crosses its first; the rows
                    // of the piece: what of the segment lies in the tile
                    const int64_t lo = (first + i) * kTile, hi = lo + kTile;
                    const size_t at = ((size_t)(first + i) * 2 + (i == 0 ? 1 : 0)) * (size_t)p.D + (size_t)mycol;
                    Part pc;
                    pc.n = (float)((e2 < hi ? e2 : hi) - (s2 > lo ? s2 : lo));
                    pc.a = load_piece(p.P1 + at, n4);
                    pc.b = load_piece(p.P2 + at, n4);
                    acc = part_merge<MODE>(acc, pc);
                }
            }
            acc = part_fold<MODE, LPR>(acc, lane);
            if (whole) {
                // the wavefronts meet through LDS, in the order of the wavefronts
                __syncthreads();
                if (sub == 0) {
                    s_n[wib][cl] = acc.n;
#pragma unroll
                    for (int q = 0; q < 4; q++) { s_a[q][wib][cl] = acc.a[q]; s_b[q][wib][cl] = acc.b[q]; }
                }
                __syncthreads();
                acc = part_zero();
#pragma unroll
                for (int w = 0; w < kWavesPerBlock; w++) {
                    Part o;
                    o.n = s_n[w][cl];
#pragma unroll
                    for (int q = 0; q < 4; q++) { o.a[q] = s_a[q][w][cl]; o.b[q] = s_b[q][w][cl]; }
                    acc = part_merge<MODE>(acc, o);
                }
            }
            if (writer && sub == 0 && ok) write_segment<MODE>(p, gg, cnt, mycol, n4, acc);
        }
    }
}

// ---- the rows: out = weight xhat + bias, or d_input ---------------------------------------------------------------------------

template <bool BWD, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
seg_apply_kernel(const SegArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, U = kRowsInFlight;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t r0 = tile * kTile;
    if (r0 >= p.N) return;
    const int64_t r1 = r0 + kTile < p.N ? r0 + kTile : p.N;
    const int64_t gfirst = first_segment(p.gp, p.G, p.N, r0);
    for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
        const int mycol = c0 + cl * 4, n4 = p.D - mycol;
        if (n4 <= 0) continue;
        const VT al = param_or(p.alpha, mycol, n4, 1.f), w = param_or(p.weight, mycol, n4, 1.f);
        VT bias = (VT)(0.f);
        if constexpr (!BWD) bias = param_or(p.bias, mycol, n4, 0.f);
        // this lane's segment: the first whose end lies beyond its row; it moves on as the lane's rows rise.  Its constants:
        // forward xhat = (x - am) rs, out = w xhat + bias; backward d_input = c1 ((dY - xhat bn) - c2)
        int64_t g = gfirst, S = 0, E = 0, loaded = -1;
        if (g < p.G) { S = seg_ptr(p.gp, p.N, g); E = seg_ptr(p.gp, p.N, g + 1); }
        VT am = (VT)(0.f), rs = (VT)(0.f), c1 = (VT)(0.f), c2 = (VT)(0.f), bn = (VT)(0.f);
        for (int64_t base = r0 + sub; base < r1; base += R * U) {
            VT v[U], dy[U];
#pragma unroll
            for (int k = 0; k < U; k++) {
                const int64_t row = base + k * R;
                v[k] = (VT)(0.f);
                dy[k] = (VT)(0.f);
                if (row < r1) {
                    v[k] = load_piece(p.X + (size_t)row * p.ldx + (size_t)mycol, n4);
                    if constexpr (BWD) dy[k] = load_piece(p.dY + (size_t)row * p.lddy + (size_t)mycol, n4);
                }
            }
#pragma unroll
            for (int k = 0; k < U; k++) {
                const int64_t row = base + k * R;
                if (row >= r1) break;
                while (g < p.G && row >= E) {
                    g++;
                    if (g < p.G) { S = seg_ptr(p.gp, p.N, g); E = seg_ptr(p.gp, p.N, g + 1); }
                }
                const bool in = g < p.G && row >= S && row < E;
                VT o = (VT)(0.f);
                if (in) {
                    if (loaded != g) {
                        loaded = g;
                        const VT mean = load_piece(p.mean + (size_t)g * p.ldm + (size_t)mycol, n4);
                        rs = load_piece(p.rstd + (size_t)g * p.ldr + (size_t)mycol, n4);
                        am = al * mean;
                        if constexpr (BWD) {
                            const float nf = (float)(E - S);
                            const VT an = load_piece(p.A + (size_t)g * p.lda + (size_t)mycol, n4) / nf;
                            bn = load_piece(p.B + (size_t)g * p.ldb + (size_t)mycol, n4) / nf;
                            c1 = w * rs;
                            c2 = al * (an - (((VT)(1.f) - al) * mean) * rs * bn);
                        }
                    }
                    const VT xhat = (v[k] - am) * rs;
                    if constexpr (BWD) o = c1 * ((dy[k] - xhat * bn) - c2);
                    else o = w * xhat + bias;
                }
                store_piece(p.out + (size_t)row * p.ldo + (size_t)mycol, o, n4);
            }
        }
    }
}

// Scratch of the moments and of the backward sums: slot 16 = the pieces of the tiles, (a, b) per column (seg::get_pieces).
constexpr int kSlotSegnormPieces = 16;

// what the three entries check alike, before any device work
int check_sizes(const char *what, int64_t num_rows, int64_t num_segments, int dim, unsigned flags)
{
    if (flags) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x (the entry has no flags)", what, flags);
    const int rc = seg::check_dim(what, dim);
    return rc != GNNA_OK ? rc : seg::check_counts(what, num_rows, num_segments);
}

template <size_t K>
bool misaligned(const void *const (&ptrs)[K])
{
    uintptr_t low_bits = 0;
    for (const void *q : ptrs) low_bits |= reinterpret_cast<uintptr_t>(q);
    return (low_bits & 3) != 0;
}

// the pieces of a call's tiles in library scratch
int get_pieces(DeviceState *ds, hipStream_t stream, SegArgs *a)
{
    const size_t piece_bytes[2] = {(size_t)a->D * sizeof(float), (size_t)a->D * sizeof(float)};
    void *pieces[2];
    const int rc = seg::get_pieces(ds, stream, kSlotSegnormPieces, a->N, piece_bytes, pieces);
    a->P1 = static_cast<float *>(pieces[0]);
    a->P2 = static_cast<float *>(pieces[1]);
    return rc;
}

// the tile and finish kernels of a call with G > 0: every element of o1 and o2 [G, D] is written
template <int MODE>
int launch_segments(const char *noun, int log_lpr, hipStream_t stream, const SegArgs &a)
{
    return seg::launch_tiles_then_finish(noun, log_lpr, stream, a, [](auto L) {
        return std::make_pair(seg_tile_kernel<MODE, decltype(L)::value>, seg_finish_kernel<MODE, decltype(L)::value>);
    });
}

// the pass over the rows of a call with N > 0: every element of a.out [N, D] is written
template <bool BWD>
int launch_apply(const char *noun, int log_lpr, hipStream_t stream, const SegArgs &a)
{
    const int64_t tiles = (a.N + kTile - 1) / kTile;
    dispatch_lpr(log_lpr, [&](auto L) {
        hipLaunchKernelGGL((seg_apply_kernel<BWD, decltype(L)::value>), dim3((unsigned)((tiles + kWavesPerBlock - 1) / kWavesPerBlock)),
                           dim3(kBlock), 0, stream, a);
    });
    return launch_ok("%s: row launch", noun);
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_segment_moments_ld_f32(const float *input, int64_t ld_in, int64_t num_rows, const int32_t *graph_pointers, int64_t num_segments,
                                float *mean, int64_t ld_mean, float *m2, int64_t ld_m2, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_moments_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, flags);
    if (rc != GNNA_OK) return rc;
    if (bad_ld(ld_in, dim) || bad_ld(ld_mean, dim) || bad_ld(ld_m2, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_mean=%lld ld_m2=%lld "
                    "dim=%d)", what, (long long)ld_in, (long long)ld_mean, (long long)ld_m2, dim);
    const void *const ins[2] = {input, graph_pointers};
    const void *const outs[2] = {mean, m2};
    if (misaligned(ins) || misaligned(outs))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, pointer and statistic pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_segments == 0) return GNNA_OK;
    if (!graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    if (!mean || !m2) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer (mean and m2 are both written)", what);
    if (num_rows > 0 && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    SegArgs a{};       // (every pointer null, every size 0)
    a.X = input; a.ldx = (size_t)ld_in; a.gp = graph_pointers; a.N = num_rows; a.G = num_segments;
    a.o1 = mean; a.ld1 = (size_t)ld_mean; a.o2 = m2; a.ld2 = (size_t)ld_m2; a.D = dim;
    if ((rc = get_pieces(ds, stream, &a)) != GNNA_OK) return rc;
    return launch_segments<MOMENTS>("segment moments", log2_lanes(dim, 4), stream, a);
}

int gnna_segment_norm_ld_f32(const float *input, int64_t ld_in, int64_t num_rows, const int32_t *graph_pointers, int64_t num_segments,
                             const float *weight, const float *bias, const float *alpha, float eps, float *out, int64_t ld_out,
                             float *mean, int64_t ld_mean, float *rstd, int64_t ld_rstd, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_norm_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, flags);
    if (rc != GNNA_OK) return rc;
    if (!std::isfinite(eps) || !(eps > 0.f))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: eps must be finite and > 0 (got %g)", what, (double)eps);
    if (bad_ld(ld_in, dim) || bad_ld(ld_out, dim) || bad_ld(ld_mean, dim) || bad_ld(ld_rstd, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_out=%lld ld_mean=%lld "
                    "ld_rstd=%lld dim=%d)", what, (long long)ld_in, (long long)ld_out, (long long)ld_mean, (long long)ld_rstd, dim);
    const void *const ins[5] = {input, graph_pointers, weight, bias, alpha};
    const void *const outs[3] = {out, mean, rstd};
    if (misaligned(ins) || misaligned(outs))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, pointer, parameter and output pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_segments == 0 && num_rows == 0) return GNNA_OK;
    if (num_segments > 0 && !graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    if (num_segments > 0 && (!mean || !rstd))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null statistic pointer (mean and rstd are both written)", what);
    if (num_rows > 0 && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    if (num_rows > 0 && !out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    SegArgs a{};       // (every pointer null, every size 0)
    a.X = input; a.ldx = (size_t)ld_in; a.gp = graph_pointers; a.N = num_rows; a.G = num_segments;
    a.weight = weight; a.bias = bias; a.alpha = alpha; a.eps = eps;
    a.o1 = mean; a.ld1 = (size_t)ld_mean; a.o2 = rstd; a.ld2 = (size_t)ld_rstd;
    a.mean = mean; a.ldm = (size_t)ld_mean; a.rstd = rstd; a.ldr = (size_t)ld_rstd;
    a.out = out; a.ldo = (size_t)ld_out; a.D = dim;
    const int log_lpr = log2_lanes(dim, 4);
    if (num_segments > 0) {
        if ((rc = get_pieces(ds, stream, &a)) != GNNA_OK) return rc;
        if ((rc = launch_segments<NORM>("segment norm", log_lpr, stream, a)) != GNNA_OK) return rc;
    }
    if (num_rows == 0) return GNNA_OK;
    return launch_apply<false>("segment norm", log_lpr, stream, a);
}

int gnna_segment_norm_backward_ld_f32(const float *d_out, int64_t ld_do, const float *input, int64_t ld_in, const float *mean,
                                      int64_t ld_mean, const float *rstd, int64_t ld_rstd, const float *weight, const float *alpha,
                                      const int32_t *graph_pointers, int64_t num_segments, float *d_input, int64_t ld_din, float *seg_a,
                                      int64_t ld_a, float *seg_b, int64_t ld_b, int64_t num_rows, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_norm_backward_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, flags);
    if (rc != GNNA_OK) return rc;
    // (a null d_input leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_do, dim) || bad_ld(ld_in, dim) || bad_ld(ld_mean, dim) || bad_ld(ld_rstd, dim) || bad_ld(ld_a, dim) || bad_ld(ld_b, dim) ||
        (d_input ? bad_ld(ld_din, dim) : ld_din >= ((int64_t)1 << 29)))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_do=%lld ld_in=%lld ld_mean=%lld "
                    "ld_rstd=%lld ld_din=%lld ld_a=%lld ld_b=%lld dim=%d)", what, (long long)ld_do, (long long)ld_in, (long long)ld_mean,
                    (long long)ld_rstd, (long long)ld_din, (long long)ld_a, (long long)ld_b, dim);
    const void *const ins[7] = {d_out, input, mean, rstd, weight, alpha, graph_pointers};
    const void *const outs[3] = {d_input, seg_a, seg_b};
    if (misaligned(ins) || misaligned(outs))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: gradient, feature, statistic, parameter and pointer pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_segments == 0 && (num_rows == 0 || !d_input)) return GNNA_OK;
    if (num_segments > 0 && !graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    if (num_segments > 0 && (!seg_a || !seg_b))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer (seg_a and seg_b are always written)", what);
    if (num_segments > 0 && (!mean || !rstd)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null statistic pointer", what);
    if (num_rows > 0 && (!input || !d_out)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature or gradient pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    SegArgs a{};       // (every pointer null, every size 0)
    a.X = input; a.ldx = (size_t)ld_in; a.dY = d_out; a.lddy = (size_t)ld_do; a.gp = graph_pointers; a.N = num_rows; a.G = num_segments;
    a.weight = weight; a.alpha = alpha;
    a.mean = mean; a.ldm = (size_t)ld_mean; a.rstd = rstd; a.ldr = (size_t)ld_rstd;
    a.o1 = seg_a; a.ld1 = (size_t)ld_a; a.o2 = seg_b; a.ld2 = (size_t)ld_b;
    a.A = seg_a; a.lda = (size_t)ld_a; a.B = seg_b; a.ldb = (size_t)ld_b;
    a.out = d_input; a.ldo = (size_t)ld_din; a.D = dim;
    const int log_lpr = log2_lanes(dim, 4);
    if (num_segments > 0) {
        if ((rc = get_pieces(ds, stream, &a)) != GNNA_OK) return rc;
        if ((rc = launch_segments<SUMS>("segment norm backward", log_lpr, stream, a)) != GNNA_OK) return rc;
    }
    if (num_rows == 0 || !d_input) return GNNA_OK;
    return launch_apply<true>("segment norm backward", log_lpr, stream, a);
}

}  // extern "C"

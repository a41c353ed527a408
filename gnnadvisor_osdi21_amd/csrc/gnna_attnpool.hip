// gnna_attnpool.hip -- attention readout: the softmax-weighted sum of the rows of every graph of a batch, gated per row or per
// element, and the backward pass (gnna_segment_attn_pool_ld_f32, gnna_segment_attn_pool_backward_ld_f32;
// include/gnna_attnpool.h).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its models stop at one row per node, GNNAdvisor/gnn_conv.py).
//
// The tiles, the lane layout, the search and the two pieces per tile are those of gnna_pool.hip (gnna_segments.h holds what both
// share); what a lane keeps is the online softmax state of gnna_softagg.hip instead of (sum, max key, min key):
//   * CH (gate_dim == dim): (m, l, a) per column, 12 registers -- the running max of the scores, sum e and sum e * x with
//     e = exp(s - m).  Not CH (gate_dim == 1): one (m, l) per partial row ("slot") and a per column: one exp per row.
//   * attnpool_tile_kernel: the slots stride over the rows of a piece, kRowsInFlight rows per slot and step, the features and the
//     gate of a row loaded in the same step.  The rows of a step enter together: the max over their scores first, then one exp to
//     rescale the state and one per score.  The slots meet by a butterfly of state merges.  A segment inside the tile is written at
//     once (out = a / l, lse = m + log l); a piece that crosses the tile's first row goes to piece 0 of the tile in library
//     scratch, one that only crosses its last row to piece 1: a [dim], m [gate_dim], l [gate_dim].
//   * attnpool_finish_kernel: one wavefront per segment.  A segment inside one tile is done, an empty one gets its zeros, one that
//     spans the tiles tf .. tl merges piece 1 of tf and piece 0 of the others: slot t takes the tiles tf + t, tf + t + slots, ...
//     in order, then the slots meet as above.  A segment of more than kLongSteps steps goes to the whole workgroup after the short
//     ones, whose wavefronts meet through LDS in the order of the wavefronts.
//   * attnpool_bwd_kernel: the same tiles and search; every lane keeps the segment of its row and moves on as its rows rise.
//     alpha = exp(s - lse) per row (per element with CH), never exp(-lse).  Without CH the dot product over the columns is summed
//     over the column blocks in a lane, then over the lanes of the row, and lane 0 of the row writes d_gate[r].
// One writer per element, plain stores, every order fixed by (num_rows, dim, gate_dim, graph_pointers): the same bits on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gnna_attnpool.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::load_piece, gat::head_sum, gat::check_alias
#include "gnna_internal.h"
#include "gnna_segments.h"

namespace gnna {
namespace {

using gat::VT;
using gat::load_piece;
using seg::kTile;
using seg::kRowsInFlight;            // (two 16-byte loads per row in flight with CH)
using seg::kLongSteps;
using seg::seg_ptr;
using seg::first_segment;
using seg::uniform64;
using seg::store_piece;
using seg::exp_nonpos;

struct FwdArgs {
    const float *X;             // the rows
    size_t ldx;
    const float *gate;          // [N, gate_dim]
    size_t ldg;
    const int32_t *gp;          // graph_pointers [G + 1]
    int64_t N, G;               // rows (< 2^31), segments
    float *out, *lse;           // lse may be null
    size_t ldo, ldl;
    float *Pa, *Pm, *Pl;        // pieces in scratch: [tiles][2][D] a, [tiles][2][gate_dim] m and l
    int D;
};

// what a lane holds of a piece or a segment: four columns; with CH a score per column, else one for the row.  m = -inf: no row
// yet (l = a = 0)
template <bool CH>
struct State {
    static constexpr int NG = CH ? 4 : 1;
    float m[NG], l[NG];
    VT a;
};

template <bool CH>
__device__ __forceinline__ State<CH> state_empty()
{
    State<CH> s;
#pragma unroll
    for (int g = 0; g < State<CH>::NG; g++) { s.m[g] = -INFINITY; s.l[g] = 0.f; }
    s.a = (VT)(0.f);
    return s;
}

template <bool CH>
__device__ __forceinline__ void state_merge(State<CH> &s, const State<CH> &o)
{
#pragma unroll
    for (int g = 0; g < State<CH>::NG; g++) {
        const float m = fmaxf(s.m[g], o.m[g]);
        const float fa = s.m[g] == -INFINITY ? 0.f : exp_nonpos(s.m[g] - m);
        const float fb = o.m[g] == -INFINITY ? 0.f : exp_nonpos(o.m[g] - m);
        s.l[g] = s.l[g] * fa + o.l[g] * fb;
        if constexpr (CH) {
            s.a[g] = s.a[g] * fa + o.a[g] * fb;
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) s.a[c] = s.a[c] * fa + o.a[c] * fb;
        }
        s.m[g] = m;
    }
}

// U rows enter together (z = -inf: no row): the max first, then one rescale of the state per step and one exp per score
template <bool CH, int U>
__device__ __forceinline__ void state_add(State<CH> &s, const VT (&v)[U], const float (&z)[U][State<CH>::NG])
{
#pragma unroll
    for (int g = 0; g < State<CH>::NG; g++) {
        float m = s.m[g];
#pragma unroll
        for (int k = 0; k < U; k++) m = fmaxf(m, z[k][g]);
        const float r = s.m[g] == -INFINITY ? 0.f : exp_nonpos(s.m[g] - m);
        float l = s.l[g] * r;
        if constexpr (CH) s.a[g] = s.a[g] * r;
        else s.a = s.a * r;
#pragma unroll
        for (int k = 0; k < U; k++) {
            const float e = z[k][g] == -INFINITY ? 0.f : exp_nonpos(z[k][g] - m);
            l += e;
            if constexpr (CH) s.a[g] += e * v[k][g];
            else s.a += e * v[k];
        }
        s.m[g] = m;
        s.l[g] = l;
    }
}

// the 64 / LPR slots of a wavefront -> one, in every lane: a butterfly over the lanes that share lane % LPR
template <bool CH, int LOG_LPR>
__device__ __forceinline__ void state_fold(State<CH> &s)
{
#pragma unroll
    for (int d = kWave >> 1; d >= (1 << LOG_LPR); d >>= 1) {
        State<CH> o;
#pragma unroll
        for (int g = 0; g < State<CH>::NG; g++) {
            o.m[g] = __shfl_xor(s.m[g], d);
            o.l[g] = __shfl_xor(s.l[g], d);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) o.a[c] = __shfl_xor(s.a[c], d);
        state_merge<CH>(s, o);
    }
}

// the final values of segment g from a lane's four columns at mycol, the first n4 (1 .. 4 and more) of them
template <bool CH>
__device__ __forceinline__ void write_segment(const FwdArgs &p, int64_t g, int mycol, int n4, const State<CH> &s)
{
    VT o, ls;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int gi = CH ? c : 0;
        const bool any = s.m[gi] != -INFINITY;                      // an empty segment: out = lse = 0
        o[c] = any ? s.a[c] / s.l[gi] : 0.f;
        ls[c] = any ? s.m[gi] + logf(s.l[gi]) : 0.f;
    }
    store_piece(p.out + (size_t)g * p.ldo + (size_t)mycol, o, n4);
    if (p.lse) {
        if constexpr (CH) store_piece(p.lse + (size_t)g * p.ldl + (size_t)mycol, ls, n4);
        else if (mycol == 0) p.lse[(size_t)g * p.ldl] = ls[0];
    }
}

// ---- forward: the tiles ------------------------------------------------------------------------------------------------------

template <bool CH, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
attnpool_tile_kernel(const FwdArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, U = kRowsInFlight, NG = State<CH>::NG;
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
            State<CH> st = state_empty<CH>();
#pragma unroll 1
            for (int64_t base = a; base < b; base += R * U) {
                VT v[U];
                float z[U][NG];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const int64_t row = base + k * R + sub;
                    v[k] = (VT)(0.f);
#pragma unroll
                    for (int q = 0; q < NG; q++) z[k][q] = -INFINITY;
                    if (row < b && ok) {
                        v[k] = load_piece(p.X + (size_t)row * p.ldx + (size_t)mycol, n4);
                        if constexpr (CH) {
                            const VT s = load_piece(p.gate + (size_t)row * p.ldg + (size_t)mycol, n4);
#pragma unroll
                            for (int q = 0; q < 4; q++) z[k][q] = s[q];
                        } else {
                            z[k][0] = p.gate[(size_t)row * p.ldg];      // (the lanes of the row load one address)
                        }
                    }
                }
                state_add<CH, U>(st, v, z);
            }
            state_fold<CH, LOG_LPR>(st);
            if (sub != 0 || !ok) continue;
            if (closed) {
                write_segment<CH>(p, g, mycol, n4, st);
            } else {
                const size_t at = piece * (size_t)p.D + (size_t)mycol;
                store_piece(p.Pa + at, st.a, n4);
                if constexpr (CH) {
                    VT m, l;
#pragma unroll
                    for (int q = 0; q < 4; q++) { m[q] = st.m[q]; l[q] = st.l[q]; }
                    store_piece(p.Pm + at, m, n4);
                    store_piece(p.Pl + at, l, n4);
                } else if (mycol == 0) {
                    p.Pm[piece] = st.m[0];
                    p.Pl[piece] = st.l[0];
                }
            }
        }
    }
}

// ---- forward: the segments ---------------------------------------------------------------------------------------------------

template <bool CH, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
attnpool_finish_kernel(const FwdArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, NG = State<CH>::NG;
    __shared__ int s_long[kWavesPerBlock];
    __shared__ int s_nlong;
    __shared__ float s_red[4 + 2 * NG][kWavesPerBlock][LPR];     // a, m, l
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
        int64_t gg = g, first = tf, n = is_long ? 0 : nt;
        if (whole) {
            gg = g0 + s_long[k];
            const int64_t s2 = seg_ptr(p.gp, p.N, gg), e2 = seg_ptr(p.gp, p.N, gg + 1);
            first = s2 / kTile;
            n = (e2 - 1) / kTile - first + 1;
        }
        const int t = whole ? wib * R + sub : sub, nl = whole ? kWavesPerBlock * R : R;
        const bool writer = whole ? wib == 0 : (valid && !is_long && (empty || nt > 0));
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            const bool ok = n4 > 0;
            State<CH> st = state_empty<CH>();
            if (ok) {
#pragma unroll 2
                for (int64_t i = t; i < n; i += nl) {
                    // the first tile's piece is the one that crosses its last row, every other tile's crosses its first
                    const size_t piece = (size_t)(first + i) * 2 + (i == 0 ? 1 : 0);
                    const size_t at = piece * (size_t)p.D + (size_t)mycol;
                    State<CH> o;
                    o.a = load_piece(p.Pa + at, n4);
                    if constexpr (CH) {
                        const VT m = load_piece(p.Pm + at, n4), l = load_piece(p.Pl + at, n4);
#pragma unroll
                        for (int q = 0; q < 4; q++) { o.m[q] = m[q]; o.l[q] = l[q]; }
                    } else {
                        o.m[0] = p.Pm[piece];
                        o.l[0] = p.Pl[piece];
                    }
                    state_merge<CH>(st, o);
                }
            }
            state_fold<CH, LOG_LPR>(st);
            if (whole) {
                // the wavefronts meet through LDS, in the order of the wavefronts
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int c = 0; c < 4; c++) s_red[c][wib][cl] = st.a[c];
#pragma unroll
                    for (int q = 0; q < NG; q++) { s_red[4 + q][wib][cl] = st.m[q]; s_red[4 + NG + q][wib][cl] = st.l[q]; }
                }
                __syncthreads();
                st = state_empty<CH>();
#pragma unroll 1
                for (int w = 0; w < kWavesPerBlock; w++) {
                    State<CH> o;
#pragma unroll
                    for (int c = 0; c < 4; c++) o.a[c] = s_red[c][w][cl];
#pragma unroll
                    for (int q = 0; q < NG; q++) { o.m[q] = s_red[4 + q][w][cl]; o.l[q] = s_red[4 + NG + q][w][cl]; }
                    state_merge<CH>(st, o);
                }
            }
            if (writer && sub == 0 && ok) write_segment<CH>(p, gg, mycol, n4, st);
        }
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------

struct BwdArgs {
    const float *X, *gate, *lse, *Y, *dY;
    size_t ldx, ldg, ldl, ldy, lddy;
    const int32_t *gp;
    int64_t N, G;
    float *dX, *dG;             // either may be null
    size_t lddx, lddg;
    int D;
};

template <bool CH, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
attnpool_bwd_kernel(const BwdArgs p)
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
    // (every lane of the wavefront makes the same number of steps: the lanes of a row meet at the end of each)
    for (int64_t base = r0; base < r1; base += R) {
        const int64_t row = base + sub;
        const bool live = row < r1;
        while (live && g < p.G && row >= E) {
            g++;
            if (g < p.G) { S = seg_ptr(p.gp, p.N, g); E = seg_ptr(p.gp, p.N, g + 1); }
        }
        const bool in = live && g < p.G && row >= S && row < E;
        float alpha1 = 0.f, dot = 0.f;
        if constexpr (!CH) {
            if (in) alpha1 = exp_nonpos(p.gate[(size_t)row * p.ldg] - p.lse[(size_t)g * p.ldl]);
        }
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            if (n4 <= 0) continue;
            VT dx = (VT)(0.f), dg = (VT)(0.f);
            if (in) {
                const VT dy = load_piece(p.dY + (size_t)g * p.lddy + (size_t)mycol, n4);
                VT al = (VT)(alpha1);
                if constexpr (CH) {
                    const VT s = load_piece(p.gate + (size_t)row * p.ldg + (size_t)mycol, n4);
                    const VT ls = load_piece(p.lse + (size_t)g * p.ldl + (size_t)mycol, n4);
#pragma unroll
                    for (int q = 0; q < 4; q++) al[q] = exp_nonpos(s[q] - ls[q]);
                }
                dx = al * dy;
                if (p.dG) {
                    const VT x = load_piece(p.X + (size_t)row * p.ldx + (size_t)mycol, n4);
                    const VT y = load_piece(p.Y + (size_t)g * p.ldy + (size_t)mycol, n4);
                    const VT t = dy * (x - y);                      // (columns past the row hold 0)
                    if constexpr (CH) dg = al * t;
                    else dot += (t[0] + t[1]) + (t[2] + t[3]);
                }
            }
            if (live) {
                if (p.dX) store_piece(p.dX + (size_t)row * p.lddx + (size_t)mycol, dx, n4);
                if constexpr (CH) {
                    if (p.dG) store_piece(p.dG + (size_t)row * p.lddg + (size_t)mycol, dg, n4);
                }
            }
        }
        if constexpr (!CH) {
            if (p.dG) {                                             // (the same in every lane)
                dot = gat::head_sum<LPR>(dot);
                if (live && cl == 0) p.dG[(size_t)row * p.lddg] = alpha1 * dot;
            }
        }
    }
}

// Scratch of the forward entry: slot 14 = the pieces of the tiles (a, m, l; seg::get_pieces).
constexpr int kSlotAttnPoolPieces = 14;

// what both entries check alike, before any device work
int check_sizes(const char *what, int64_t num_rows, int64_t num_segments, int dim, int gate_dim, unsigned flags)
{
    if (flags != 0u) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s takes no flags (got 0x%x)", what, flags);
    const int rc = seg::check_dim(what, dim);
    if (rc != GNNA_OK) return rc;
    if (gate_dim != 1 && gate_dim != dim)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: gate_dim must be 1 or dim = %d (got %d)", what, dim, gate_dim);
    return seg::check_counts(what, num_rows, num_segments);
}

template <bool CH>
int launch_forward(int log_lpr, hipStream_t stream, const FwdArgs &a)
{
    return seg::launch_tiles_then_finish("attention pooling", log_lpr, stream, a, [](auto L) {
        return std::make_pair(attnpool_tile_kernel<CH, decltype(L)::value>, attnpool_finish_kernel<CH, decltype(L)::value>);
    });
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_segment_attn_pool_ld_f32(const float *input, int64_t ld_in, int64_t num_rows, const float *gate, int64_t ld_gate, int gate_dim,
                                  const int32_t *graph_pointers, int64_t num_segments, float *out, int64_t ld_out, float *lse,
                                  int64_t ld_lse, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_attn_pool_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, gate_dim, flags);
    if (rc != GNNA_OK) return rc;
    // (a null lse leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld(ld_gate, gate_dim) || bad_ld(ld_out, dim) || bad_ld_of(lse, ld_lse, gate_dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= the width they stride and < 2^29 elements (ld_in=%lld "
                    "ld_gate=%lld ld_out=%lld ld_lse=%lld dim=%d gate_dim=%d)", what, (long long)ld_in, (long long)ld_gate,
                    (long long)ld_out, (long long)ld_lse, dim, gate_dim);
    const void *const ins[3] = {input, gate, graph_pointers};
    const void *const outs[2] = {out, lse};
    uintptr_t low_bits = 0;
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    for (const void *q : outs) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, gate, pointer and output pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_segments == 0) return GNNA_OK;
    if (!out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer (out is always written)", what);
    if (!graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    if (num_rows > 0 && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    if (num_rows > 0 && !gate) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null gate pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    FwdArgs a;
    a.X = input; a.ldx = (size_t)ld_in; a.gate = gate; a.ldg = (size_t)ld_gate; a.gp = graph_pointers; a.N = num_rows; a.G = num_segments;
    a.out = out; a.lse = lse; a.ldo = (size_t)ld_out; a.ldl = (size_t)ld_lse;
    a.D = dim;
    const size_t piece_bytes[3] = {(size_t)dim * sizeof(float), (size_t)gate_dim * sizeof(float), (size_t)gate_dim * sizeof(float)};
    void *pieces[3];
    if ((rc = seg::get_pieces(ds, stream, kSlotAttnPoolPieces, num_rows, piece_bytes, pieces)) != GNNA_OK) return rc;
    a.Pa = static_cast<float *>(pieces[0]); a.Pm = static_cast<float *>(pieces[1]); a.Pl = static_cast<float *>(pieces[2]);
    const int log_lpr = log2_lanes(dim, 4);
    // (dim == 1: a score per element is a score per row)
    return gate_dim == 1 ? launch_forward<false>(log_lpr, stream, a) : launch_forward<true>(log_lpr, stream, a);
}

int gnna_segment_attn_pool_backward_ld_f32(const float *input, int64_t ld_in, const float *gate, int64_t ld_gate, int gate_dim,
                                           const float *lse, int64_t ld_lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
                                           const int32_t *graph_pointers, int64_t num_segments, float *d_input, int64_t ld_din,
                                           float *d_gate, int64_t ld_dgate, int64_t num_rows, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_segment_attn_pool_backward_ld_f32";
    int rc = check_sizes(what, num_rows, num_segments, dim, gate_dim, flags);
    if (rc != GNNA_OK) return rc;
    // (a null output leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld(ld_gate, gate_dim) || bad_ld(ld_lse, gate_dim) || bad_ld(ld_y, dim) || bad_ld(ld_dy, dim) ||
        bad_ld_of(d_input, ld_din, dim) || bad_ld_of(d_gate, ld_dgate, gate_dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= the width they stride and < 2^29 elements (ld_in=%lld "
                    "ld_gate=%lld ld_lse=%lld ld_y=%lld ld_dy=%lld ld_din=%lld ld_dgate=%lld dim=%d gate_dim=%d)", what, (long long)ld_in,
                    (long long)ld_gate, (long long)ld_lse, (long long)ld_y, (long long)ld_dy, (long long)ld_din, (long long)ld_dgate, dim,
                    gate_dim);
    const void *const ins[6] = {input, gate, lse, Y, dY, graph_pointers};
    const void *const outs[2] = {d_input, d_gate};
    uintptr_t low_bits = 0;
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    for (const void *q : outs) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, gate, lse, gradient and pointer pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_rows == 0) return GNNA_OK;
    if (!d_input && !d_gate)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointers: d_input and d_gate are both null", what);
    if (num_segments > 0 && !graph_pointers) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null graph_pointers", what);
    if (num_segments > 0 && (!input || !gate)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature or gate pointer", what);
    if (num_segments > 0 && (!lse || !Y || !dY)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null lse, Y or dY pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    BwdArgs a;
    a.X = input; a.gate = gate; a.lse = lse; a.Y = Y; a.dY = dY;
    a.ldx = (size_t)ld_in; a.ldg = (size_t)ld_gate; a.ldl = (size_t)ld_lse; a.ldy = (size_t)ld_y; a.lddy = (size_t)ld_dy;
    a.gp = graph_pointers; a.N = num_rows; a.G = num_segments;
    a.dX = d_input; a.dG = d_gate; a.lddx = (size_t)ld_din; a.lddg = (size_t)ld_dgate; a.D = dim;
    const int64_t tiles = (num_rows + kTile - 1) / kTile;
    const dim3 grid((unsigned)((tiles + kWavesPerBlock - 1) / kWavesPerBlock));
    dispatch_lpr(log2_lanes(dim, 4), [&](auto L) {
        if (gate_dim == 1) hipLaunchKernelGGL((attnpool_bwd_kernel<false, decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
        else hipLaunchKernelGGL((attnpool_bwd_kernel<true, decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("attention pooling backward launch");
}

}  // extern "C"

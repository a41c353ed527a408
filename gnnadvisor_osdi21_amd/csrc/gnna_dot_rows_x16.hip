// gnna_dot_rows_x16.hip -- the rows form of the fused scaled dot-product graph attention over matrices STORED in bf16 / fp16 and
// ACCUMULATED in fp32 (gnna_dot_attn_forward_rows_x16 / gnna_dot_attn_backward_rows_x16; include/gnna_dot_rows_x16.h).  CDNA4 /
// gfx950 only.  No counterpart in the reference (it has no attention layer and no 16-bit kernel).
//
// The function, the mask rule and the ownership are those of gnna_dot_rows.hip: R = 64 / LPR consecutive rows per wavefront, a row by
// its own slot (up to 8 edges), by the slots of its wavefront (up to R * 128 edges; the slots meet by a butterfly) or by the four
// wavefronts of its workgroup (beyond; they meet through LDS in the order of the wavefronts); ids one step ahead; no partition, no
// atomics, no zero-fill; limits and host side from gnna_ownrows.h.  What this file decides for itself is how the 16-bit rows move:
//   * a lane holds EIGHT elements: one 16-byte load is a lane's piece of a row, LPH = next_pow2(ceil(dim / 8)) lanes cover a head
//     (attn_layout with 8 elements per lane).  At 1 x 64 that is 8 lanes a row and 8 rows a wavefront where the fp32 kernels have 16
//     and 4, and every fold over a head is one DPP level shallower.
//   * the two pieces gathered per edge stay PACKED (4 VGPRs each) from the load to the one place that consumes them; they are widened
//     there (bf16: a shift / a mask, fp16: v_cvt_f32_f16 -- exact) and multiplied and added in fp32.  What the walked row itself
//     brings (Q[i] | K[j], dY[i] | V[j]) is widened once per row and column block and held as fp32.
//   * per lane the state is fp32: forward (m, s, acc[8]), destination side a[8], source side a[8] and b[8].  Nothing is rounded to
//     16 bits before the one store of an output element (round-to-nearest-even: v_cvt_pk_bf16_f32 / v_cvt_f16_f32); lse and the
//     (lse, c) records of the backward stay fp32.
//   * whether a piece is one 16-byte access or eight 16-bit ones is decided per CALL (every base 16-byte aligned, every stride a
//     multiple of 8, dim % 8 == 0) and is a uniform branch inside load_piece16 / store_piece16: the arithmetic around it is the same
//     code, so both paths give the same bits.
//   * the sum of a lane's 8 products is ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), then the DPP fold over the lanes of the
//     head (gat::head_sum); accumulators add one edge after the other.  No dot instruction with an internal rounding of its own.
// The LDS planes of the long rows are 10 (forward) / 8 (destination side) / 16 (source side) floats per lane.
//
// The mask constants sit in VGPRs as in gnna_dot_rows.hip (its in_vgpr / DropRegs, restated here because that file's compilation
// inputs stay as they are).  Row strides are 32-bit (the entries refuse a stride of 2^29 elements or more).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "gnna_dot_rows_x16.h"
#include "gnna_convert16.h"      // widen2, narrow1, narrow2
#include "gnna_device.h"
#include "gnna_gat_common.h"     // head_sum, slots_sum, set_drop, check_drop, check_alias
#include "gnna_internal.h"
#include "gnna_ownrows.h"        // the ownership limits, the host side of the rows entries
#include "gnna_rowwalk.h"        // wave_max
#include "gnna_segments.h"       // seg::exp_nonpos

namespace gnna {
namespace {

using cvt16::narrow1;
using cvt16::narrow2;
using cvt16::widen2;
using gat::head_sum;
using gat::slots_sum;
using seg::exp_nonpos;

constexpr int kEl = 8;                          // elements per lane: one 16-byte piece
typedef uint32_t Packed __attribute__((ext_vector_type(4)));        // a piece as it was loaded
typedef Packed PackedMem __attribute__((aligned(16)));

// edges per slot and step: the larger of {2, 4} at which no instance has a private segment or a spill (DESIGN: the table per pass)
constexpr int kEdges = 2;
using own::kSlotEdges;
constexpr int kLongSteps = own::kLongSteps<kEdges>;

constexpr int kSlotDotRowsX16Pack = 22;         // library scratch: (lse, c) per (destination row, head) of a backward call

enum Pass { kFwd = 0, kDst = 1, kSrc = 2 };

struct Args {
    const uint16_t *own; uint32_t ld_own;       // the walked row's side of z: Q (forward, destination side), K (source side)
    const uint16_t *own2; uint32_t ld_own2;     // the walked row's second piece: dY (destination side), V (source side)
    const uint16_t *gat; uint32_t ld_gat;       // the gathered side of z: K (forward, destination side), Q (source side)
    const uint16_t *gat2; uint32_t ld_gat2;     // the second row gathered per edge: V (forward, destination side), dY (source side)
    const uint16_t *Y; uint32_t ld_y;           // destination side: for c
    const float *lse;                           // destination side: [rows, heads]
    float2 *pack;                               // destination side: written (null: not wanted); source side: gathered by id
    const int32_t *rp, *col;                    // the CSR walked: A, or A^T on the source side
    uint16_t *out; uint32_t ld_out;             // out (forward) | dQ (destination side, may be null) | dK (source side, may be null)
    uint16_t *out2; uint32_t ld_out2;           // source side: dV (may be null)
    float *sc;                                  // forward: lse [rows, heads]
    int64_t rows;                               // rows walked
    uint32_t limit;                             // ids < limit
    int heads, dim;
    float scale;
    bool relu;                                  // forward: out = max(out, 0)
    bool walk;                                  // false: no edge can count, or no sum is wanted: the index arrays are not read
    bool hold;                                  // false: what the row itself brings is not read either
    bool vec;                                   // every piece of this call is one aligned 16-byte access
    uint64_t rng_seed;                          // attention dropout (gnna_ext.h: the mask rule), read by the DROP instances only
    uint32_t drop_thr;
    float keep_scale;
};

// ---- a lane's piece of a row ----------------------------------------------------------------------------------------------------

// the first n (1 .. 8, or more) elements at p, packed two to a word, the others 0.  vec is uniform over the call and means n >= 8 and
// p 16-byte aligned for every piece of the call.  Element by element, a position past n reads element 0 again and is then set to
// 0: selects, where a branch per element would keep eight lane masks in SGPRs across the sweep (the resource report showed 11 to
// 29 of them spilled).
__device__ __forceinline__ Packed load_piece16(const uint16_t *__restrict__ p, int n, bool vec)
{
    if (vec) return *reinterpret_cast<const PackedMem *>(p);
    Packed v;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const bool in0 = 2 * q < n, in1 = 2 * q + 1 < n;
        const uint32_t lo = p[in0 ? 2 * q : 0], hi = p[in1 ? 2 * q + 1 : 0];
        v[q] = (in0 ? lo : 0u) | ((in1 ? hi : 0u) << 16);
    }
    return v;
}

template <int TYPE>
__device__ __forceinline__ void widen8(const Packed v, float (&x)[kEl])
{
#pragma unroll
    for (int q = 0; q < 4; q++) widen2<TYPE>(v[q], x[2 * q], x[2 * q + 1]);
}

// each of the first n (<= 8) values rounded once, stored at q
template <int TYPE>
__device__ __forceinline__ void store_piece16(uint16_t *__restrict__ q, const float (&x)[kEl], int n, bool vec)
{
    if (vec) {
        Packed o;
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = narrow2<TYPE>(x[2 * w], x[2 * w + 1]);
        *reinterpret_cast<PackedMem *>(q) = o;
        return;
    }
#pragma unroll
    for (int c = 0; c < kEl; c++) {
        if (c < n) q[c] = narrow1<TYPE>(x[c]);
    }
}

// this lane's share of <a, b> over its (<= 8) elements; both are 0 beyond the head's elements.  The stated order.
template <int TYPE>
__device__ __forceinline__ float dot_part(const float (&a)[kEl], const Packed b)
{
    float x[kEl];
    widen8<TYPE>(b, x);
    return ((a[0] * x[0] + a[1] * x[1]) + (a[2] * x[2] + a[3] * x[3])) + ((a[4] * x[4] + a[5] * x[5]) + (a[6] * x[6] + a[7] * x[7]));
}

// acc += f * (the piece v)
template <int TYPE>
__device__ __forceinline__ void axpy(float (&acc)[kEl], float f, const Packed v)
{
    float x[kEl];
    widen8<TYPE>(v, x);
#pragma unroll
    for (int c = 0; c < kEl; c++) acc[c] += f * x[c];
}

// ---- attention dropout with its uniform operands in VGPRs (gnna_dot_rows.hip: why) -------------------------------------------------

__device__ __forceinline__ uint32_t in_vgpr(uint32_t x)
{
    uint32_t r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
__device__ __forceinline__ uint64_t in_vgpr64(uint64_t x) { return ((uint64_t)in_vgpr((uint32_t)(x >> 32)) << 32) | in_vgpr((uint32_t)x); }

struct DropRegs {
    uint64_t seed, c0, c1, c2;
    uint32_t thr, keep;         // keep: the bits of keep_scale
};

template <bool DROP>
__device__ __forceinline__ DropRegs drop_regs(uint64_t rng_seed, uint32_t drop_thr, float keep_scale)
{
    if constexpr (!DROP) return DropRegs{};
    else
        return DropRegs{in_vgpr64(rng_seed), in_vgpr64(0x9E3779B97F4A7C15ull), in_vgpr64(0xBF58476D1CE4E5B9ull),
                        in_vgpr64(0x94D049BB133111EBull), in_vgpr(drop_thr), in_vgpr(__float_as_uint(keep_scale))};
}

// gat::drop_factor's k(i, j, h), bit for bit
__device__ __forceinline__ float drop_factor(const DropRegs &d, uint32_t i, uint32_t j, int h)
{
    const uint64_t u = ((uint64_t)i << 35) | ((uint64_t)j << 6) | (uint64_t)(uint32_t)h;
    uint64_t z = d.seed + d.c0 * (u + 1ull);
    z = (z ^ (z >> 30)) * d.c1;
    z = (z ^ (z >> 27)) * d.c2;
    z ^= z >> 31;
    return (uint32_t)(z >> 32) >= d.thr ? __uint_as_float(d.keep) : 0.f;
}

// ---- the state of a slot ---------------------------------------------------------------------------------------------------------

// Forward: the online (max, sum e, sum e * k * V) of this lane's head and columns.  Destination side: a = sum dz * K.  Source side:
// a = sum dz * Q, b = sum alpha * k * dY.  (What a pass does not use is never live.)
struct State {
    float m, s;
    float a[kEl], b[kEl];
};

template <int PASS>
__device__ __forceinline__ State state_empty()
{
    State st;
    st.m = PASS == kFwd ? -INFINITY : 0.f;
    st.s = 0.f;
#pragma unroll
    for (int c = 0; c < kEl; c++) st.a[c] = st.b[c] = 0.f;
    return st;
}

template <int PASS>
__device__ __forceinline__ void state_merge(State &s, const State &o)
{
    if constexpr (PASS == kFwd) {
        const float m = fmaxf(s.m, o.m);
        const float fa = s.m == -INFINITY ? 0.f : exp_nonpos(s.m - m);
        const float fb = o.m == -INFINITY ? 0.f : exp_nonpos(o.m - m);
        s.s = s.s * fa + o.s * fb;
#pragma unroll
        for (int c = 0; c < kEl; c++) s.a[c] = s.a[c] * fa + o.a[c] * fb;
        s.m = m;
    } else {
#pragma unroll
        for (int c = 0; c < kEl; c++) s.a[c] += o.a[c];
        if constexpr (PASS == kSrc) {
#pragma unroll
            for (int c = 0; c < kEl; c++) s.b[c] += o.b[c];
        }
    }
}

// the 64 / LPR slots of a wavefront meet (lanes that share lane % LPR); the result in every slot.  Whole wavefronts only.
template <int PASS, int LPR>
__device__ __forceinline__ void slots_meet(State &st)
{
    if constexpr (PASS == kFwd) {
#pragma unroll
        for (int d = kWave >> 1; d >= LPR; d >>= 1) {
            State o = state_empty<kFwd>();
            o.m = __shfl_xor(st.m, d);
            o.s = __shfl_xor(st.s, d);
#pragma unroll
            for (int c = 0; c < kEl; c++) o.a[c] = __shfl_xor(st.a[c], d);
            state_merge<kFwd>(st, o);
        }
    } else {
#pragma unroll
        for (int c = 0; c < kEl; c++) st.a[c] = slots_sum<LPR>(st.a[c]);
        if constexpr (PASS == kSrc) {
#pragma unroll
            for (int c = 0; c < kEl; c++) st.b[c] = slots_sum<LPR>(st.b[c]);
        }
    }
}

// the floats of a state that the wavefronts of a long row exchange: a[8], then (m, s) forward or b[8] on the source side
template <int PASS>
constexpr int kPlanes = PASS == kFwd ? kEl + 2 : PASS == kSrc ? 2 * kEl : kEl;

template <int PASS, int LPR>
__device__ __forceinline__ void state_to_lds(float (&red)[kPlanes<PASS>][kWavesPerBlock][LPR], int w, int cl, const State &st)
{
#pragma unroll
    for (int c = 0; c < kEl; c++) red[c][w][cl] = st.a[c];
    if constexpr (PASS == kFwd) { red[kEl][w][cl] = st.m; red[kEl + 1][w][cl] = st.s; }
    if constexpr (PASS == kSrc) {
#pragma unroll
        for (int c = 0; c < kEl; c++) red[kEl + c][w][cl] = st.b[c];
    }
}

template <int PASS, int LPR>
__device__ __forceinline__ State state_from_lds(const float (&red)[kPlanes<PASS>][kWavesPerBlock][LPR], int w, int cl)
{
    State o = state_empty<PASS>();
#pragma unroll
    for (int c = 0; c < kEl; c++) o.a[c] = red[c][w][cl];
    if constexpr (PASS == kFwd) { o.m = red[kEl][w][cl]; o.s = red[kEl + 1][w][cl]; }
    if constexpr (PASS == kSrc) {
#pragma unroll
        for (int c = 0; c < kEl; c++) o.b[c] = red[kEl + c][w][cl];
    }
    return o;
}

// where a lane stands in its row's column block
struct Lane {
    int h;              // its head
    int n;              // elements of its piece (<= 0: the lane idles)
    bool ok, first;     // n > 0; the first lane of its head
    uint32_t colf;      // the column of its piece (< heads * dim <= 2^14)
};

// what the walked row itself brings, widened
struct Held {
    float own[kEl];     // Q[i] | K[j]
    float own2[kEl];    // backward: dY[i] | V[j]
    float lse, c;       // destination side
};

// Whole wavefronts only (the destination side folds c over the lanes of a head); on: this lane's slot has such a row.
template <int TYPE, int PASS, int LPH>
__device__ __forceinline__ Held load_held(const Args &p, int64_t row, bool on, const Lane &L)
{
    Held r;
    r.lse = r.c = 0.f;
    Packed a = (Packed)(0u), b = (Packed)(0u), y = (Packed)(0u);
    const bool ld = on && L.ok && p.hold;
    if (ld) {
        a = load_piece16(p.own + (size_t)row * p.ld_own + L.colf, L.n, p.vec);
        if constexpr (PASS != kFwd) b = load_piece16(p.own2 + (size_t)row * p.ld_own2 + L.colf, L.n, p.vec);
        if constexpr (PASS == kDst) {
            r.lse = p.lse[(size_t)row * (size_t)p.heads + (size_t)L.h];
            y = load_piece16(p.Y + (size_t)row * p.ld_y + L.colf, L.n, p.vec);
        }
    }
    widen8<TYPE>(a, r.own);
    widen8<TYPE>(b, r.own2);
    // c = <dY, Y> of the head, from the Y the caller passes (the rounded one)
    if constexpr (PASS == kDst) r.c = head_sum<LPH>(dot_part<TYPE>(r.own2, y));
    return r;
}

// The ids of the kEdges edges of slot t in the step at `base` (edges base + t + k * nl); -1 past the end of the row and for an id
// outside [0, limit): such an edge is skipped, in every pass alike.
__device__ __forceinline__ void load_ids(const Args &p, uint32_t base, uint32_t end, int t, int nl, int (&id)[kEdges])
{
#pragma unroll
    for (int k = 0; k < kEdges; k++) {
        const uint32_t ee = base + (uint32_t)(t + k * nl);      // (end < 2^31 and a step is < 2^13 edges: no wrap)
        id[k] = ee < end ? p.col[ee] : -1;
        if ((uint32_t)id[k] >= p.limit) id[k] = -1;
    }
}

// The edges [beg, end) of `row` swept by `nl` slots (this one: slot t) in `steps` steps of kEdges edges per slot.  Whole wavefronts
// only, and `steps` is uniform over the wavefront (every pass folds over the lanes of a head in every step); a lane whose row ended
// earlier, or has none, brings no edge.  -> this slot's state.
template <int TYPE, int PASS, int LPH, bool DROP>
__device__ __forceinline__ State sweep(const Args &p, const DropRegs &dr, uint32_t row, uint32_t beg, uint32_t end, int steps, int t,
                                       int nl, const Lane &L, const Held &r)
{
    State st = state_empty<PASS>();
    int next[kEdges];
    load_ids(p, beg, end, t, nl, next);
#pragma unroll 1
    for (int it = 0; it < steps; it++) {
        const uint32_t base = beg + (uint32_t)it * (uint32_t)(nl * kEdges);
        // 0 for an edge that counts, -inf for one that does not: added to the score, it makes e (alpha) exactly 0
        float dead[kEdges];
        Packed v[kEdges], w[kEdges];                    // the two gathered pieces of every edge, packed until they are consumed
        float2 rec[PASS == kSrc ? kEdges : 1];
        float kf[DROP ? kEdges : 1];
#pragma unroll
        for (int k = 0; k < kEdges; k++) {
            const int id = next[k];
            const bool live = id >= 0 && L.ok;
            dead[k] = live ? 0.f : -INFINITY;
            v[k] = (Packed)(0u);
            w[k] = (Packed)(0u);
            if constexpr (PASS == kSrc) rec[k] = make_float2(0.f, 0.f);
            if (live) {
                v[k] = load_piece16(p.gat + (size_t)(uint32_t)id * p.ld_gat + L.colf, L.n, p.vec);
                w[k] = load_piece16(p.gat2 + (size_t)(uint32_t)id * p.ld_gat2 + L.colf, L.n, p.vec);
                if constexpr (PASS == kSrc) rec[k] = p.pack[(size_t)(uint32_t)id * (size_t)p.heads + (size_t)L.h];
            }
            // (the LPH lanes of a head compute the same key, as they compute the same alpha; an idle lane's is unused)
            if constexpr (DROP)
                kf[k] = PASS == kSrc ? drop_factor(dr, (uint32_t)id, row, L.h) : drop_factor(dr, row, (uint32_t)id, L.h);
        }
        load_ids(p, base + (uint32_t)(nl * kEdges), end, t, nl, next);
        if constexpr (PASS == kFwd) {
            // the edges of a step enter together: one exp to rescale the state, one per edge
            float z[kEdges];
            float m = st.m;
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                z[k] = p.scale * head_sum<LPH>(dot_part<TYPE>(r.own, v[k])) + dead[k];
                m = fmaxf(m, z[k]);
            }
            const float f = st.m == -INFINITY ? 0.f : exp_nonpos(st.m - m);
            st.s *= f;
#pragma unroll
            for (int c = 0; c < kEl; c++) st.a[c] *= f;
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                const float e = z[k] == -INFINITY ? 0.f : exp_nonpos(z[k] - m);
                st.s += e;                                      // (lse is that of the un-dropped scores)
                axpy<TYPE>(st.a, DROP ? e * kf[k] : e, w[k]);
            }
            st.m = m;
        } else {
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                // z = scale * <Q[i], K[j]> and dalpha = <dY[i], V[j]>: of each pair one is the walked row's, one the gathered
                const float z = p.scale * head_sum<LPH>(dot_part<TYPE>(r.own, v[k])) + dead[k];
                float dalpha = head_sum<LPH>(dot_part<TYPE>(r.own2, w[k]));
                float lse_e = r.lse, c_e = r.c;
                if constexpr (PASS == kSrc) { lse_e = rec[k].x; c_e = rec[k].y; }
                const float alpha = __expf(z - lse_e);          // (exp(-inf) = 0 for an edge that does not count)
                if constexpr (DROP) dalpha *= kf[k];
                const float dz = alpha * (dalpha - c_e);        // (a dropped edge still contributes -alpha * c)
                axpy<TYPE>(st.a, dz, v[k]);
                if constexpr (PASS == kSrc) axpy<TYPE>(st.b, DROP ? alpha * kf[k] : alpha, w[k]);
            }
        }
    }
    return st;
}

// The one writer of a row's column block stores what the row's state gives: every column of the block, each rounded here and
// nowhere else, and the head's scalar by the first lane of the head.
template <int TYPE, int PASS>
__device__ __forceinline__ void write_row(const Args &p, int64_t row, const Lane &L, const Held &r, const State &st)
{
    if (!L.ok) return;
    const size_t sidx = (size_t)row * (size_t)p.heads + (size_t)L.h;
    float o[kEl];
    if constexpr (PASS == kFwd) {
        const bool any = st.m != -INFINITY;             // a row without counted edges: out = lse = 0
#pragma unroll
        for (int c = 0; c < kEl; c++) {
            o[c] = any ? st.a[c] / st.s : 0.f;
            if (p.relu) o[c] = o[c] < 0.f ? 0.f : o[c];      // (NaN stays NaN, as torch.relu)
        }
        store_piece16<TYPE>(p.out + (size_t)row * p.ld_out + L.colf, o, L.n, p.vec);
        if (L.first) p.sc[sidx] = any ? st.m + logf(st.s) : 0.f;
    } else {
        if (p.out) {
#pragma unroll
            for (int c = 0; c < kEl; c++) o[c] = p.scale * st.a[c];
            store_piece16<TYPE>(p.out + (size_t)row * p.ld_out + L.colf, o, L.n, p.vec);
        }
        if constexpr (PASS == kDst) {
            if (L.first && p.pack) p.pack[sidx] = make_float2(r.lse, r.c);
        } else {
            if (p.out2) store_piece16<TYPE>(p.out2 + (size_t)row * p.ld_out2 + L.colf, st.b, L.n, p.vec);
        }
    }
}

template <int TYPE, int PASS, int LOG_LPH, int LOG_LPR, bool DROP>
__global__ void __launch_bounds__(kBlock)
dot_rows_x16_kernel(const Args p)
{
    constexpr int LPH = 1 << LOG_LPH, LPR = 1 << LOG_LPR, HB = LPR / LPH, R = kWave / LPR, RB = R * kWavesPerBlock;
    constexpr uint32_t kLong = (uint32_t)(R * kEdges * kLongSteps);
    __shared__ int s_long[RB];
    __shared__ int s_nlong;
    __shared__ float s_red[kPlanes<PASS>][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    int hl = cl >> LOG_LPH;
    const int fl = (cl & (LPH - 1)) * kEl;
    // with one head per column block (LPR == LPH) hl is 0 and the head, its columns and its scalars' indices would all be uniform
    // and live in SGPRs, the short resource here; kept in a VGPR, they are vector arithmetic like in every other layout
    asm("" : "+v"(hl));
    const DropRegs dr = drop_regs<DROP>(p.rng_seed, p.drop_thr, p.keep_scale);
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    // this slot's row: R consecutive rows per wavefront, RB per block
    const int64_t r0 = (int64_t)blockIdx.x * RB;
    const int64_t row = r0 + wib * R + sub;
    const bool live = row < p.rows;
    uint32_t beg = 0, end = 0;
    if (live && p.walk) {
        beg = std::min((uint32_t)p.rp[row], 0x7fffffffu);
        end = std::min((uint32_t)p.rp[row + 1], 0x7fffffffu);
        if (beg > end) beg = end;
    }
    const uint32_t deg = end - beg;
    const bool is_long = deg > kLong;
    const bool is_short = R > 1 && deg <= (uint32_t)kSlotEdges;         // (a wavefront of one slot: the slot is the wavefront)
    if (is_long && cl == 0) s_long[atomicAdd(&s_nlong, 1)] = wib * R + sub;
    __syncthreads();

    // this lane's place in the column block at head hb0
    auto lane_at = [&](int hb0) {
        Lane L;
        const int h = hb0 + hl;
        L.n = h < p.heads ? p.dim - fl : 0;
        L.ok = L.n > 0;
        L.h = L.ok ? h : 0;
        L.first = fl == 0;
        L.colf = (uint32_t)(L.h * p.dim + (L.ok ? fl : 0));
        return L;
    };

    // ---- the short rows (and, in wavefronts of several slots, the rows without edges): every slot its own row -------------------
    if constexpr (R > 1) {
        const bool mine = live && is_short;
        if (__ballot(mine)) {
            const uint32_t sb = mine ? beg : 0u, se = mine ? end : 0u;
            // every slot makes the steps of the longest short row of the wavefront (at most kSlotEdges / kEdges, rounded up)
            const int steps = wave_max((int)((se - sb + (uint32_t)kEdges - 1u) / (uint32_t)kEdges));
            for (int hb0 = 0; hb0 < p.heads; hb0 += HB) {
                const Lane L = lane_at(hb0);
                const Held r = load_held<TYPE, PASS, LPH>(p, row, mine, L);
                const State st = sweep<TYPE, PASS, LPH, DROP>(p, dr, (uint32_t)row, sb, se, steps, 0, 1, L, r);
                if (mine) write_row<TYPE, PASS>(p, row, L, r, st);
            }
        }
    }

    // ---- the rows in between: the slots of the wavefront share one row after the other ------------------------------------------
    {
        constexpr uint64_t slot_lanes = LPR == 64 ? ~0ull : ((1ull << (LPR & 63)) - 1ull);
        uint64_t todo = __ballot(live && !is_long && !is_short);
        while (todo) {
            const int s = (__ffsll((unsigned long long)todo) - 1) >> LOG_LPR;
            todo &= ~(slot_lanes << (s * LPR));
            const int64_t rr = r0 + wib * R + s;
            const uint32_t lb = (uint32_t)__shfl((int)beg, s * LPR), le = (uint32_t)__shfl((int)end, s * LPR);
            const int steps = __builtin_amdgcn_readfirstlane((int)((le - lb + (uint32_t)(R * kEdges) - 1u) / (uint32_t)(R * kEdges)));
            for (int hb0 = 0; hb0 < p.heads; hb0 += HB) {
                const Lane L = lane_at(hb0);
                const Held r = load_held<TYPE, PASS, LPH>(p, rr, true, L);
                State st = sweep<TYPE, PASS, LPH, DROP>(p, dr, (uint32_t)rr, lb, le, steps, sub, R, L, r);
                slots_meet<PASS, LPR>(st);
                if (sub == 0) write_row<TYPE, PASS>(p, rr, L, r, st);
            }
        }
    }

    // ---- the long rows: the whole block, one after the other (the list's order may vary; a row's result does not depend on it) ---
    const int nlong = s_nlong;
    for (int k = 0; k < nlong; k++) {
        const int64_t rr = r0 + s_long[k];
        uint32_t lb = std::min((uint32_t)p.rp[rr], 0x7fffffffu);
        const uint32_t le = std::min((uint32_t)p.rp[rr + 1], 0x7fffffffu);
        if (lb > le) lb = le;
        const int steps = __builtin_amdgcn_readfirstlane((int)((le - lb + (uint32_t)(RB * kEdges) - 1u) / (uint32_t)(RB * kEdges)));
        for (int hb0 = 0; hb0 < p.heads; hb0 += HB) {
            const Lane L = lane_at(hb0);
            const Held r = load_held<TYPE, PASS, LPH>(p, rr, true, L);
            State st = sweep<TYPE, PASS, LPH, DROP>(p, dr, (uint32_t)rr, lb, le, steps, wib * R + sub, RB, L, r);
            slots_meet<PASS, LPR>(st);
            // the wavefronts meet through LDS, in the order of the wavefronts
            __syncthreads();
            if (sub == 0) state_to_lds<PASS, LPR>(s_red, wib, cl, st);
            __syncthreads();
            st = state_empty<PASS>();
#pragma unroll 1
            for (int w = 0; w < kWavesPerBlock; w++) state_merge<PASS>(st, state_from_lds<PASS, LPR>(s_red, w, cl));
            if (wib == 0 && sub == 0) write_row<TYPE, PASS>(p, rr, L, r, st);
        }
    }
}

// attn_drop = 0 keeps every edge with k = 1, so the call runs the instances without the mask (which carry no key computation)
template <int PASS>
int launch(int type, const Args &a, hipStream_t stream, const char *noun)
{
    const AttnLayout layout = attn_layout(a.heads, a.dim, kEl);             // (dim <= kMaxDim: log_lph <= 5)
    const dim3 grid = own::rows_grid(a.rows, layout);
    auto with = [&](auto T, auto D) {
        dispatch_layout(layout, [&](auto H, auto L) {
            if constexpr (decltype(H)::value <= 5)
                hipLaunchKernelGGL((dot_rows_x16_kernel<decltype(T)::value, PASS, decltype(H)::value, decltype(L)::value, decltype(D)::value>),
                                   grid, dim3(kBlock), 0, stream, a);
        });
    };
    auto with_type = [&](auto D) {
        if (type == GNNA_BF16) with(std::integral_constant<int, GNNA_BF16>(), D);
        else with(std::integral_constant<int, GNNA_F16>(), D);
    };
    if (a.drop_thr) with_type(std::true_type());
    else with_type(std::false_type());
    return launch_ok("%s launch", noun);
}

// what both entries check alike, before any device work: the type, the checks of every rows entry, then attn_drop and scale as the
// dot entries check them
int check_sizes(const char *what, int type, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, unsigned flags,
                unsigned allowed_flags, float attn_drop, float scale)
{
    if (type != GNNA_BF16 && type != GNNA_F16)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: type must be GNNA_BF16 or GNNA_F16 (got %d)", what, type);
    int rc = own::check_rows_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, allowed_flags);
    if (rc != GNNA_OK) return rc;
    if ((rc = gat::check_drop(what, attn_drop)) != GNNA_OK) return rc;
    // (0 is uniform attention, a negative scale is allowed)
    if (!std::isfinite(scale)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: scale must be finite (got %g)", what, (double)scale);
    return GNNA_OK;
}

// one operand of a call towards the choice of the 16-byte path: a null (unused) operand does not count
struct Aligned {
    bool ok = true;
    void add(const void *ptr, int64_t ld) { if (ptr) ok = ok && (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0 && ld % kEl == 0; }
};

const uint16_t *u16(const void *ptr) { return static_cast<const uint16_t *>(ptr); }
uint16_t *u16(void *ptr) { return static_cast<uint16_t *>(ptr); }

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_dot_attn_forward_rows_x16(int type, const void *Q, int64_t ld_q, const void *K, int64_t ld_k, const void *V, int64_t ld_v,
                                   int64_t num_in_rows, const int32_t *row_pointers, const int32_t *column_index, float scale,
                                   float attn_drop, uint64_t rng_seed, void *out, int64_t ld_out, float *lse, int64_t num_out_rows,
                                   int heads, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_dot_attn_forward_rows_x16";
    const int rc = check_sizes(what, type, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU, attn_drop,
                               scale);
    if (rc != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;                    // nothing to write
    const int64_t W = (int64_t)heads * dim;
    const bool no_in = num_in_rows == 0;                      // every id is out of range: out = 0, lse = 0, nothing else is read
    if ((!no_in && (bad_ld(ld_q, W) || bad_ld(ld_k, W) || bad_ld(ld_v, W))) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_q=%lld ld_k=%lld "
                    "ld_v=%lld ld_out=%lld)", what, (long long)ld_q, (long long)ld_k, (long long)ld_v, (long long)ld_out);
    if ((!no_in && (!Q || !K || !V || !row_pointers)) || !out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (out == Q || out == K || out == V || out == lse || lse == Q || lse == K || lse == V)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input or the other output", what);
    Args a{};
    a.own = u16(Q); a.ld_own = (uint32_t)ld_q; a.gat = u16(K); a.ld_gat = (uint32_t)ld_k; a.gat2 = u16(V); a.ld_gat2 = (uint32_t)ld_v;
    a.rp = row_pointers; a.col = column_index; a.out = u16(out); a.ld_out = (uint32_t)ld_out; a.sc = lse;
    a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim; a.scale = scale;
    a.relu = (flags & GNNA_EPILOGUE_RELU) != 0;
    a.walk = a.hold = !no_in && column_index != nullptr;
    Aligned al;
    if (!no_in) { al.add(Q, ld_q); al.add(K, ld_k); al.add(V, ld_v); }
    al.add(out, ld_out);
    a.vec = al.ok && dim % kEl == 0;
    gat::set_drop(&a, attn_drop, rng_seed);
    return launch<kFwd>(type, a, static_cast<hipStream_t>(stream_v), "dot-product attention (rows, 16-bit)");
}

int gnna_dot_attn_backward_rows_x16(int type, const void *Q, int64_t ld_q, const void *K, int64_t ld_k, const void *V, int64_t ld_v,
                                    int64_t num_in_rows, const float *lse, const void *Y, int64_t ld_y, const void *dY, int64_t ld_dy,
                                    const int32_t *row_pointers, const int32_t *column_index, const int32_t *t_row_pointers,
                                    const int32_t *t_column_index, float scale, float attn_drop, uint64_t rng_seed, void *dQ,
                                    int64_t ld_dq, void *dK, int64_t ld_dk, void *dV, int64_t ld_dv, int64_t num_out_rows, int heads,
                                    int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_dot_attn_backward_rows_x16";
    int rc = check_sizes(what, type, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE, attn_drop, scale);
    if (rc != GNNA_OK) return rc;
    const int64_t W = (int64_t)heads * dim;
    const bool want_dq = dQ && num_out_rows > 0, want_dk = dK && num_in_rows > 0, want_dv = dV && num_in_rows > 0;
    const bool want_src = want_dk || want_dv;
    if (!want_src && !want_dq) return GNNA_OK;
    const bool one_side = num_out_rows == 0 || num_in_rows == 0;      // no edge can exist: the outputs that have rows are 0
    if (bad_ld_of(dQ, ld_dq, W) || bad_ld_of(dK, ld_dk, W) || bad_ld_of(dV, ld_dv, W) ||
        (!one_side && (bad_ld(ld_q, W) || bad_ld(ld_k, W) || bad_ld(ld_v, W) || bad_ld(ld_y, W) || bad_ld(ld_dy, W))))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_q=%lld ld_k=%lld "
                    "ld_v=%lld ld_y=%lld ld_dy=%lld ld_dq=%lld ld_dk=%lld ld_dv=%lld)", what, (long long)ld_q, (long long)ld_k,
                    (long long)ld_v, (long long)ld_y, (long long)ld_dy, (long long)ld_dq, (long long)ld_dk, (long long)ld_dv);
    if (!one_side) {
        if (!Q || !K || !V || !lse || !Y || !dY) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        if ((want_dq && !row_pointers) || (want_src && !t_row_pointers))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer (the structure for dQ, the transposed structure for dK "
                        "and dV)", what);
        const void *const ins[] = {Q, K, V, lse, Y, dY}, *const outs[] = {dQ, dK, dV};
        if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    float2 *pack = nullptr;
    if (!one_side && want_src) {
        void *ws = nullptr;
        if ((rc = own::record_scratch(stream, kSlotDotRowsX16Pack, (size_t)num_out_rows * heads * sizeof(float2), &ws)) != GNNA_OK) return rc;
        pack = static_cast<float2 *>(ws);
    }
    // one choice for both passes of the call: every operand that either of them touches
    Aligned al;
    if (!one_side) { al.add(Q, ld_q); al.add(K, ld_k); al.add(V, ld_v); al.add(Y, ld_y); al.add(dY, ld_dy); }
    if (want_dq) al.add(dQ, ld_dq);
    if (want_dk) al.add(dK, ld_dk);
    if (want_dv) al.add(dV, ld_dv);
    Args a{};
    a.heads = heads; a.dim = dim; a.scale = scale;
    a.vec = al.ok && dim % kEl == 0;
    gat::set_drop(&a, attn_drop, rng_seed);
    if (want_dq || pack) {
        // destination side: row i holds Q[i], dY[i], (lse, c)[i] and pulls K[j], V[j] -> dQ, and the records of the source side
        a.own = u16(Q); a.ld_own = (uint32_t)ld_q; a.own2 = u16(dY); a.ld_own2 = (uint32_t)ld_dy;
        a.gat = u16(K); a.ld_gat = (uint32_t)ld_k; a.gat2 = u16(V); a.ld_gat2 = (uint32_t)ld_v;
        a.Y = u16(Y); a.ld_y = (uint32_t)ld_y; a.lse = lse; a.pack = pack; a.rp = row_pointers; a.col = column_index;
        a.out = want_dq ? u16(dQ) : nullptr; a.ld_out = (uint32_t)ld_dq;
        a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows;
        a.hold = !one_side; a.walk = !one_side && want_dq && column_index != nullptr;
        if ((rc = launch<kDst>(type, a, stream, "dot-product attention (rows, 16-bit) backward: destination side")) != GNNA_OK) return rc;
    }
    if (want_src) {
        // source side: row j of A^T holds K[j], V[j] and pulls Q[i], dY[i], (lse, c)[i] -> dK, dV
        a.own = u16(K); a.ld_own = (uint32_t)ld_k; a.own2 = u16(V); a.ld_own2 = (uint32_t)ld_v;
        a.gat = u16(Q); a.ld_gat = (uint32_t)ld_q; a.gat2 = u16(dY); a.ld_gat2 = (uint32_t)ld_dy;
        a.Y = nullptr; a.ld_y = 0; a.lse = nullptr; a.pack = pack; a.rp = t_row_pointers; a.col = t_column_index;
        a.out = want_dk ? u16(dK) : nullptr; a.ld_out = (uint32_t)ld_dk; a.out2 = want_dv ? u16(dV) : nullptr; a.ld_out2 = (uint32_t)ld_dv;
        a.rows = num_in_rows; a.limit = (uint32_t)num_out_rows;
        a.walk = a.hold = !one_side && t_column_index != nullptr;
        if ((rc = launch<kSrc>(type, a, stream, "dot-product attention (rows, 16-bit) backward: source side")) != GNNA_OK) return rc;
    }
    return GNNA_OK;
}

}  // extern "C"

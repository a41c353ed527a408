// gnna_dot_rows.hip -- the "rows" form of the fused scaled dot-product graph attention (gnna_dot_attn_forward_rows_f32 /
// gnna_dot_attn_backward_rows_f32; include/gnna_dot_rows.h): the function of gnna_dotattn.hip by kernels that own the rows they
// write.  CDNA4 / gfx950 only.  No counterpart in the reference (it has no attention layer).
//
// One kernel body, three passes, with or without the dropout mask.  Ownership is that of gnna_gat_rows.hip, restated here (the
// limits and the host side are shared, gnna_ownrows.h; one shared kernel skeleton is not yet: profiles/ownrows/README.md):
// R = 64 / LPR consecutive rows per wavefront, a row by its own
// slot, by the slots of its wavefront or by the whole workgroup, by its degree alone; ids one step ahead; no neighbor-group
// partition, no atomics, no zero-fill.  The lane layout is attn_layout's: LPH = next_pow2(ceil(dim / 4)) lanes of 4 floats cover a
// head, LPR = LPH * (heads of a column block) <= 64 lanes a row, rows wider than one wave-wide load go in column blocks of whole
// heads.  What is new is the data movement: the score needs the whole gathered row, so EVERY pass gathers two row pieces per edge
// and folds over the lanes of a head (DPP) for every edge.  What a row holds, gathers and writes:
//   * forward (rows of A):      holds Q[i] (registers, once per row and column block); gathers K[j], V[j]; z = scale *
//                               head_sum(q . k) is one fold per edge; per lane the online state (m, s, acc[4]) of its head and
//                               columns -- the running max of z, sum e over ALL counted edges, sum e * k * V with e = exp(z - m) and k
//                               the dropout factor -- rescaled once per step; exp is only ever taken of a score minus a maximum.
//                               ONE gather of K where the atomic path has two (lse pass, pull pass).  Writes out = acc / s (ReLU
//                               here when asked for) and lse = m + log s.
//   * destination side (A):     holds Q[i], dY[i], lse[i] and c[i] = <dY[i], Y[i]> (made here per head, DPP); gathers K[j], V[j];
//                               two independent folds per edge (z, dalpha); one accumulator sum dz * K[j]; writes dQ = scale * acc
//                               (scale once) and the 8-byte record (lse, c) of (i, h) into library scratch when the source side
//                               will run.
//   * source side (A^T):        holds K[j], V[j]; gathers Q[i], dY[i] and the record of (i, h); two accumulators, sum dz * Q[i] and
//                               sum alpha * k * dY[i]; writes dK = scale * acc and dV.  In the mask key i is the gathered id and j
//                               the walked row: the (i, j, h) of the other two passes.
// The slots of a wavefront meet by a butterfly (forward: the (max, sum e, sum e * x) merge; backward: sums), the wavefronts of a
// long row through LDS in the order of the wavefronts (6 planes forward, 4 destination side, 8 source side).  Path and order depend
// on the degree and (heads, dim) only: the same bits on every run.
//
// The two invariants of gnna_rowwalk.h hold because every sweep is entered by whole wavefronts with a step count that is uniform
// over the wavefront -- here every pass, the forward included, folds over the lanes of a head in every step -- and the barriers sit
// in loops whose bounds (s_nlong, heads) are uniform over the block, which no thread leaves early.
//
// The row strides are 32-bit (the entries refuse a stride of 2^29 floats or more): every pass carries four to six strided
// operands, and the atomic dot kernels needed the same to keep their last SGPRs on the source side with the mask.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "gnna_dot_rows.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // the lane-layout folds, load_piece, set_drop, check_drop, check_alias
#include "gnna_internal.h"
#include "gnna_ownrows.h"        // the ownership limits, the host side of the rows entries
#include "gnna_rowwalk.h"        // wave_max
#include "gnna_segments.h"       // seg::store_piece, seg::exp_nonpos

namespace gnna {
namespace {

using gat::VT;
using gat::head_sum;
using gat::load_piece;
using gat::slots_sum;
using seg::exp_nonpos;
using seg::store_piece;

// edges per slot and step: every pass holds two gathered row pieces per edge (the source side an 8-byte record beside them).
// The larger of {2, 4} at which no instance has a private segment or a spill: at 4 the backward passes spill 4 to 8 SGPRs (with
// and without the mask) and the source side with the mask drops to 3 waves per SIMD (the table per pass).
constexpr int kEdges = 2;
using own::kSlotEdges;                          // the two ownership limits: gnna_ownrows.h
constexpr int kLongSteps = own::kLongSteps<kEdges>;

constexpr int kSlotDotRowsPack = 21;    // library scratch: (lse, c) per (destination row, head) of a backward call

enum Pass { kFwd = 0, kDst = 1, kSrc = 2 };

struct Args {
    const float *own; uint32_t ld_own;      // the walked row's side of z: Q (forward, destination side), K (source side)
    const float *own2; uint32_t ld_own2;    // the walked row's second piece: dY (destination side), V (source side)
    const float *gat; uint32_t ld_gat;      // the gathered side of z: K (forward, destination side), Q (source side)
    const float *gat2; uint32_t ld_gat2;    // the second row gathered per edge: V (forward, destination side), dY (source side)
    const float *Y; uint32_t ld_y;          // destination side: for c
    const float *lse;                       // destination side: [rows, heads]
    float2 *pack;                           // destination side: written (null: not wanted); source side: gathered by id
    const int32_t *rp, *col;                // the CSR walked: A, or A^T on the source side
    float *out; uint32_t ld_out;            // out (forward) | dQ (destination side, may be null) | dK (source side, may be null)
    float *out2; uint32_t ld_out2;          // source side: dV (may be null)
    float *sc;                              // forward: lse [rows, heads]
    int64_t rows;                           // rows walked
    uint32_t limit;                         // ids < limit
    int heads, dim;
    float scale;
    bool relu;                              // forward: out = max(out, 0)
    bool walk;                              // false: no edge can count, or no sum is wanted: the index arrays are not read
    bool hold;                              // false: what the row itself brings is not read either
    uint64_t rng_seed;                      // attention dropout (gnna_ext.h: the mask rule), read by the DROP instances only
    uint32_t drop_thr;
    float keep_scale;
};

// this lane's share of <a, b> over its (<= 4) floats; both are 0 beyond the head's floats
__device__ __forceinline__ float dot_part(const VT a, const VT b)
{
    return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

// ---- attention dropout (gnna_ext.h: the mask rule) with its uniform operands in VGPRs ----------------------------------------
//
// k(i, j, h) is gat::drop_factor's, bit for bit.  Its three 64-bit multipliers, the seed, the threshold and the scale are uniform, so
// the compiler keeps them in ten SGPRs across the whole sweep (VOP3 takes no literal on gfx9) -- the SGPRs the passes with the mask
// do not have (the resource report showed 8 to 17 spilled before).  VGPRs are not short here: the values are moved there once per kernel
// through an opaque move, and the key arithmetic then reads vector registers only.
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

// (key_of_position of gnna_device.h on the position gat::drop_factor makes of (i, j, h))
__device__ __forceinline__ float drop_factor(const DropRegs &d, uint32_t i, uint32_t j, int h)
{
    const uint64_t u = ((uint64_t)i << 35) | ((uint64_t)j << 6) | (uint64_t)(uint32_t)h;
    uint64_t z = d.seed + d.c0 * (u + 1ull);
    z = (z ^ (z >> 30)) * d.c1;
    z = (z ^ (z >> 27)) * d.c2;
    z ^= z >> 31;
    return (uint32_t)(z >> 32) >= d.thr ? __uint_as_float(d.keep) : 0.f;
}

// Forward: the online (max, sum e, sum e * k * V) of this lane's head and columns.  Destination side: a = sum dz * K.  Source
// side: a = sum dz * Q, b = sum alpha * k * dY.  (What a pass does not use is never live.)
struct State {
    float m, s;
    VT a, b;
};

template <int PASS>
__device__ __forceinline__ State state_empty()
{
    return State{PASS == kFwd ? -INFINITY : 0.f, 0.f, (VT)(0.f), (VT)(0.f)};
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
        for (int c = 0; c < 4; c++) s.a[c] = s.a[c] * fa + o.a[c] * fb;
        s.m = m;
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) s.a[c] += o.a[c];
        if constexpr (PASS == kSrc) {
#pragma unroll
            for (int c = 0; c < 4; c++) s.b[c] += o.b[c];
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
            for (int c = 0; c < 4; c++) o.a[c] = __shfl_xor(st.a[c], d);
            state_merge<kFwd>(st, o);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) st.a[c] = slots_sum<LPR>(st.a[c]);
        if constexpr (PASS == kSrc) {
#pragma unroll
            for (int c = 0; c < 4; c++) st.b[c] = slots_sum<LPR>(st.b[c]);
        }
    }
}

// where a lane stands in its row's column block
struct Lane {
    int h;              // its head
    int n4;             // floats of its piece (<= 0: the lane idles)
    bool ok, first;     // n4 > 0; the first lane of its head
    uint32_t colf;      // the column of its piece (< heads * dim <= 2^14)
};

// what the walked row itself brings
struct Held {
    VT own;             // Q[i] | K[j]
    VT own2;            // backward: dY[i] | V[j]
    float lse, c;       // destination side
};

// Whole wavefronts only (the destination side folds c over the lanes of a head); on: this lane's slot has such a row.
template <int PASS, int LPH>
__device__ __forceinline__ Held load_held(const Args &p, int64_t row, bool on, const Lane &L)
{
    Held r{(VT)(0.f), (VT)(0.f), 0.f, 0.f};
    const bool ld = on && L.ok && p.hold;
    if (ld) {
        r.own = load_piece(p.own + (size_t)row * p.ld_own + L.colf, L.n4);
        if constexpr (PASS != kFwd) r.own2 = load_piece(p.own2 + (size_t)row * p.ld_own2 + L.colf, L.n4);
    }
    if constexpr (PASS == kDst) {
        VT y = (VT)(0.f);
        if (ld) {
            r.lse = p.lse[(size_t)row * (size_t)p.heads + (size_t)L.h];
            y = load_piece(p.Y + (size_t)row * p.ld_y + L.colf, L.n4);
        }
        r.c = head_sum<LPH>(dot_part(r.own2, y));
    }
    return r;
}

// The ids of the kEdges edges of slot t in the step at `base` (edges base + t + k * nl); -1 past the end of the row and for an id
// outside [0, limit): such an edge is skipped, in every pass alike.
__device__ __forceinline__ void load_ids(const Args &p, uint32_t base, uint32_t end, int t, int nl, int (&id)[kEdges])
{
#pragma unroll
    for (int k = 0; k < kEdges; k++) {
        const uint32_t ee = base + (uint32_t)(t + k * nl);      // (end < 2^31 and a step is < 2^12 edges: no wrap)
        id[k] = ee < end ? p.col[ee] : -1;
        if ((uint32_t)id[k] >= p.limit) id[k] = -1;
    }
}

// The edges [beg, end) of `row` swept by `nl` slots (this one: slot t) in `steps` steps of kEdges edges per slot.  Whole wavefronts
// only, and `steps` is uniform over the wavefront (every pass folds over the lanes of a head in every step); a lane whose row ended
// earlier, or has none, brings no edge.  -> this slot's state.
template <int PASS, int LPH, bool DROP>
__device__ __forceinline__ State sweep(const Args &p, const DropRegs &dr, uint32_t row, uint32_t beg, uint32_t end, int steps, int t,
                                       int nl, const Lane &L, const Held &r)
{
    State st = state_empty<PASS>();
    int next[kEdges];
    load_ids(p, beg, end, t, nl, next);
#pragma unroll 1
    for (int it = 0; it < steps; it++) {
        const uint32_t base = beg + (uint32_t)it * (uint32_t)(nl * kEdges);
        // 0 for an edge that counts, -inf for one that does not: added to the score, it makes e (alpha) exactly 0 without a lane
        // mask that would live in two SGPRs per edge across the step
        float dead[kEdges];
        VT v[kEdges], w[kEdges];
        float2 rec[PASS == kSrc ? kEdges : 1];
        float kf[DROP ? kEdges : 1];
#pragma unroll
        for (int k = 0; k < kEdges; k++) {
            const int id = next[k];
            const bool live = id >= 0 && L.ok;
            dead[k] = live ? 0.f : -INFINITY;
            v[k] = (VT)(0.f);
            w[k] = (VT)(0.f);
            if constexpr (PASS == kSrc) rec[k] = make_float2(0.f, 0.f);
            if (live) {
                v[k] = load_piece(p.gat + (size_t)(uint32_t)id * p.ld_gat + L.colf, L.n4);
                w[k] = load_piece(p.gat2 + (size_t)(uint32_t)id * p.ld_gat2 + L.colf, L.n4);
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
                z[k] = p.scale * head_sum<LPH>(dot_part(r.own, v[k])) + dead[k];
                m = fmaxf(m, z[k]);
            }
            const float f = st.m == -INFINITY ? 0.f : exp_nonpos(st.m - m);
            st.s *= f;
#pragma unroll
            for (int c = 0; c < 4; c++) st.a[c] *= f;
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                const float e = z[k] == -INFINITY ? 0.f : exp_nonpos(z[k] - m);
                st.s += e;                                      // (lse is that of the un-dropped scores)
                const float ek = DROP ? e * kf[k] : e;
#pragma unroll
                for (int c = 0; c < 4; c++) st.a[c] += ek * w[k][c];
            }
            st.m = m;
        } else {
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                // z = scale * <Q[i], K[j]> and dalpha = <dY[i], V[j]>: of each pair one is the walked row's, one the gathered
                const float z = p.scale * head_sum<LPH>(dot_part(r.own, v[k])) + dead[k];
                float dalpha = head_sum<LPH>(dot_part(r.own2, w[k]));
                float lse_e = r.lse, c_e = r.c;
                if constexpr (PASS == kSrc) { lse_e = rec[k].x; c_e = rec[k].y; }
                const float alpha = __expf(z - lse_e);          // (exp(-inf) = 0 for an edge that does not count)
                if constexpr (DROP) dalpha *= kf[k];
                const float dz = alpha * (dalpha - c_e);        // (a dropped edge still contributes -alpha * c)
#pragma unroll
                for (int c = 0; c < 4; c++) st.a[c] += dz * v[k][c];
                if constexpr (PASS == kSrc) {
                    const float ak = DROP ? alpha * kf[k] : alpha;
#pragma unroll
                    for (int c = 0; c < 4; c++) st.b[c] += ak * w[k][c];
                }
            }
        }
    }
    return st;
}

// The one writer of a row's column block stores what the row's state gives: every column of the block, and the head's scalar by
// the first lane of the head.
template <int PASS>
__device__ __forceinline__ void write_row(const Args &p, int64_t row, const Lane &L, const Held &r, const State &st)
{
    if (!L.ok) return;
    const size_t sidx = (size_t)row * (size_t)p.heads + (size_t)L.h;
    if constexpr (PASS == kFwd) {
        const bool any = st.m != -INFINITY;             // a row without counted edges: out = lse = 0
        VT o;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            o[c] = any ? st.a[c] / st.s : 0.f;
            if (p.relu) o[c] = o[c] < 0.f ? 0.f : o[c];      // (NaN stays NaN, as torch.relu)
        }
        store_piece(p.out + (size_t)row * p.ld_out + L.colf, o, L.n4);
        if (L.first) p.sc[sidx] = any ? st.m + logf(st.s) : 0.f;
    } else {
        if (p.out) {
            VT o;
#pragma unroll
            for (int c = 0; c < 4; c++) o[c] = p.scale * st.a[c];
            store_piece(p.out + (size_t)row * p.ld_out + L.colf, o, L.n4);
        }
        if constexpr (PASS == kDst) {
            if (L.first && p.pack) p.pack[sidx] = make_float2(r.lse, r.c);
        } else {
            if (p.out2) store_piece(p.out2 + (size_t)row * p.ld_out2 + L.colf, st.b, L.n4);
        }
    }
}

template <int PASS, int LOG_LPH, int LOG_LPR, bool DROP>
__global__ void __launch_bounds__(kBlock)
dot_rows_kernel(const Args p)
{
    constexpr int LPH = 1 << LOG_LPH, LPR = 1 << LOG_LPR, HB = LPR / LPH, R = kWave / LPR, RB = R * kWavesPerBlock;
    constexpr uint32_t kLong = (uint32_t)(R * kEdges * kLongSteps);
    constexpr int kPlanes = PASS == kFwd ? 6 : PASS == kSrc ? 8 : 4;    // floats of a state that the wavefronts exchange
    __shared__ int s_long[RB];
    __shared__ int s_nlong;
    __shared__ float s_red[kPlanes][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH, fl = (cl & (LPH - 1)) * 4;
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
        L.n4 = h < p.heads ? p.dim - fl : 0;
        L.ok = L.n4 > 0;
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
                const Held r = load_held<PASS, LPH>(p, row, mine, L);
                const State st = sweep<PASS, LPH, DROP>(p, dr, (uint32_t)row, sb, se, steps, 0, 1, L, r);
                if (mine) write_row<PASS>(p, row, L, r, st);
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
                const Held r = load_held<PASS, LPH>(p, rr, true, L);
                State st = sweep<PASS, LPH, DROP>(p, dr, (uint32_t)rr, lb, le, steps, sub, R, L, r);
                slots_meet<PASS, LPR>(st);
                if (sub == 0) write_row<PASS>(p, rr, L, r, st);
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
            const Held r = load_held<PASS, LPH>(p, rr, true, L);
            State st = sweep<PASS, LPH, DROP>(p, dr, (uint32_t)rr, lb, le, steps, wib * R + sub, RB, L, r);
            slots_meet<PASS, LPR>(st);
            // the wavefronts meet through LDS, in the order of the wavefronts
            __syncthreads();
            if (sub == 0) {
#pragma unroll
                for (int c = 0; c < 4; c++) s_red[c][wib][cl] = st.a[c];
                if constexpr (PASS == kFwd) { s_red[4][wib][cl] = st.m; s_red[5][wib][cl] = st.s; }
                if constexpr (PASS == kSrc) {
#pragma unroll
                    for (int c = 0; c < 4; c++) s_red[4 + c][wib][cl] = st.b[c];
                }
            }
            __syncthreads();
            st = state_empty<PASS>();
#pragma unroll 1
            for (int w = 0; w < kWavesPerBlock; w++) {
                State o = state_empty<PASS>();
#pragma unroll
                for (int c = 0; c < 4; c++) o.a[c] = s_red[c][w][cl];
                if constexpr (PASS == kFwd) { o.m = s_red[4][w][cl]; o.s = s_red[5][w][cl]; }
                if constexpr (PASS == kSrc) {
#pragma unroll
                    for (int c = 0; c < 4; c++) o.b[c] = s_red[4 + c][w][cl];
                }
                state_merge<PASS>(st, o);
            }
            if (wib == 0 && sub == 0) write_row<PASS>(p, rr, L, r, st);
        }
    }
}

// attn_drop = 0 keeps every edge with k = 1, so the call runs the instances without the mask (which carry no key computation)
template <int PASS>
int launch(const Args &a, hipStream_t stream, const char *noun)
{
    const AttnLayout layout = attn_layout(a.heads, a.dim);                  // (dim <= kMaxDim: log_lph is never capped)
    const dim3 grid = own::rows_grid(a.rows, layout);
    auto with_mask = [&](auto D) {
        dispatch_layout(layout, [&](auto H, auto L) {
            hipLaunchKernelGGL((dot_rows_kernel<PASS, decltype(H)::value, decltype(L)::value, decltype(D)::value>), grid, dim3(kBlock),
                               0, stream, a);
        });
    };
    if (a.drop_thr) with_mask(std::true_type());
    else with_mask(std::false_type());
    return launch_ok("%s launch", noun);
}

// what both entries check alike, before any device work: the checks of every rows entry, then attn_drop and scale as the dot
// entries check them
int check_sizes(const char *what, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, unsigned flags, unsigned allowed_flags,
                float attn_drop, float scale)
{
    int rc = own::check_rows_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, allowed_flags);
    if (rc != GNNA_OK) return rc;
    if ((rc = gat::check_drop(what, attn_drop)) != GNNA_OK) return rc;
    // (0 is uniform attention, a negative scale is allowed)
    if (!std::isfinite(scale)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: scale must be finite (got %g)", what, (double)scale);
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_dot_attn_forward_rows_f32(const float *Q, int64_t ld_q, const float *K, int64_t ld_k, const float *V, int64_t ld_v,
                                   int64_t num_in_rows, const int32_t *row_pointers, const int32_t *column_index, float scale,
                                   float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out, float *lse, int64_t num_out_rows,
                                   int heads, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_dot_attn_forward_rows_f32";
    const int rc = check_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU, attn_drop, scale);
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
    a.own = Q; a.ld_own = (uint32_t)ld_q; a.gat = K; a.ld_gat = (uint32_t)ld_k; a.gat2 = V; a.ld_gat2 = (uint32_t)ld_v;
    a.rp = row_pointers; a.col = column_index; a.out = out; a.ld_out = (uint32_t)ld_out; a.sc = lse;
    a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim; a.scale = scale;
    a.relu = (flags & GNNA_EPILOGUE_RELU) != 0;
    a.walk = a.hold = !no_in && column_index != nullptr;
    gat::set_drop(&a, attn_drop, rng_seed);
    return launch<kFwd>(a, static_cast<hipStream_t>(stream_v), "dot-product attention (rows)");
}

int gnna_dot_attn_backward_rows_f32(const float *Q, int64_t ld_q, const float *K, int64_t ld_k, const float *V, int64_t ld_v,
                                    int64_t num_in_rows, const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
                                    const int32_t *row_pointers, const int32_t *column_index, const int32_t *t_row_pointers,
                                    const int32_t *t_column_index, float scale, float attn_drop, uint64_t rng_seed, float *dQ,
                                    int64_t ld_dq, float *dK, int64_t ld_dk, float *dV, int64_t ld_dv, int64_t num_out_rows, int heads,
                                    int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_dot_attn_backward_rows_f32";
    int rc = check_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE, attn_drop, scale);
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
        if ((rc = own::record_scratch(stream, kSlotDotRowsPack, (size_t)num_out_rows * heads * sizeof(float2), &ws)) != GNNA_OK) return rc;
        pack = static_cast<float2 *>(ws);
    }
    Args a{};
    a.heads = heads; a.dim = dim; a.scale = scale;
    gat::set_drop(&a, attn_drop, rng_seed);
    if (want_dq || pack) {
        // destination side: row i holds Q[i], dY[i], (lse, c)[i] and pulls K[j], V[j] -> dQ, and the records of the source side
        a.own = Q; a.ld_own = (uint32_t)ld_q; a.own2 = dY; a.ld_own2 = (uint32_t)ld_dy;
        a.gat = K; a.ld_gat = (uint32_t)ld_k; a.gat2 = V; a.ld_gat2 = (uint32_t)ld_v;
        a.Y = Y; a.ld_y = (uint32_t)ld_y; a.lse = lse; a.pack = pack; a.rp = row_pointers; a.col = column_index;
        a.out = want_dq ? dQ : nullptr; a.ld_out = (uint32_t)ld_dq;
        a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows;
        a.hold = !one_side; a.walk = !one_side && want_dq && column_index != nullptr;
        if ((rc = launch<kDst>(a, stream, "dot-product attention (rows) backward: destination side")) != GNNA_OK) return rc;
    }
    if (want_src) {
        // source side: row j of A^T holds K[j], V[j] and pulls Q[i], dY[i], (lse, c)[i] -> dK, dV
        a.own = K; a.ld_own = (uint32_t)ld_k; a.own2 = V; a.ld_own2 = (uint32_t)ld_v;
        a.gat = Q; a.ld_gat = (uint32_t)ld_q; a.gat2 = dY; a.ld_gat2 = (uint32_t)ld_dy;
        a.Y = nullptr; a.ld_y = 0; a.lse = nullptr; a.pack = pack; a.rp = t_row_pointers; a.col = t_column_index;
        a.out = want_dk ? dK : nullptr; a.ld_out = (uint32_t)ld_dk; a.out2 = want_dv ? dV : nullptr; a.ld_out2 = (uint32_t)ld_dv;
        a.rows = num_in_rows; a.limit = (uint32_t)num_out_rows;
        a.walk = a.hold = !one_side && t_column_index != nullptr;
        if ((rc = launch<kSrc>(a, stream, "dot-product attention (rows) backward: source side")) != GNNA_OK) return rc;
    }
    return GNNA_OK;
}

}  // extern "C"

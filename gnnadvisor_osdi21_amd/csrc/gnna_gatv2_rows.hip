// gnna_gatv2_rows.hip -- the "rows" form of the fused GATv2 attention (gnna_gatv2_forward_rows_f32 / gnna_gatv2_backward_rows_f32;
// include/gnna_gatv2_rows.h): the function of gnna_gatv2.hip by kernels that own the rows they write.  CDNA4 / gfx950 only.  No
// counterpart in the reference (it has no attention layer).
//
// One kernel body, three passes, with or without the dropout mask.  Ownership is that of gnna_gat_rows.hip and gnna_dot_rows.hip
// (the limits and the host side are shared, gnna_ownrows.h; the skeleton is written out here as it is there): R = 64 / LPR
// consecutive rows per wavefront, a row by its own slot, by the slots of its wavefront or by the whole workgroup, by its degree
// alone; ids one step ahead; no neighbor-group partition, no atomics, no zero-fill.  The lane layout is attn_layout's: LPH =
// next_pow2(ceil(dim / 4)) lanes of 4 floats cover a head, LPR = LPH * (heads of a column block) <= 64 lanes a row, rows wider than
// one wave-wide load go in column blocks of whole heads.  Here the loop over the column blocks is the OUTER one in every pass: a
// lane's piece of att is loaded once per column block and kernel, and on the destination side a lane's share of d_att stays in
// registers across every row the lane walks.  In GATv2 the gathered row Hs[j] is the score's input AND the message, so the forward
// and the destination side gather ONE row piece per edge:
//   * forward (rows of A):      holds Hd[i] and att; gathers Hs[j] once (16 bytes per lane); z = head_sum(att . lrelu(Hs[j] + Hd[i]))
//                               is one fold per edge; per lane the online state (m, s, acc[4]) of its head and columns -- the
//                               running max of z, sum e over ALL counted edges, sum e * k * Hs[j] with e = exp(z - m) and k the
//                               dropout factor -- rescaled once per step, from the registers that made z.  Writes out = acc / s
//                               (ReLU here when asked for) and lse = m + log s.  The atomic forward walks the ids twice and gathers
//                               Hs[j] twice.
//   * destination side (A):     holds Hd[i], att, dY[i], lse[i] and c[i] = <dY[i], Y[i]> (made here per head, DPP); gathers Hs[j];
//                               two independent folds per edge (z, dalpha); accumulates dHd[i] = sum g and, across all its rows,
//                               the lane's share of d_att = sum dz * lrelu(t).  Writes dHd, the 8-byte record (lse, c) of (i, h)
//                               when the source side will run, and the workgroup's partial of d_att (below).
//   * source side (A^T):        holds Hs[j] and att; gathers Hd[i], dY[i] and the record of (i, h); one accumulator,
//                               sum (alpha * k * dY[i] + g); writes dHs.  In the mask key i is the gathered id and j the walked
//                               row: the (i, j, h) of the other two passes.
// with t = Hs[j] + Hd[i], dz = alpha * (k * dalpha - c), g = dz * att * (t > 0 ? 1 : slope).
//
// d_att without atomics.  At the end of a column block the lanes' registers meet over the slots of the wavefront (slots_sum: a fixed
// butterfly), the wavefronts through LDS in the order of the wavefronts, and the first wavefront stores the workgroup's partial
// [heads * dim] with plain stores into library scratch [blocks, heads * dim].  datt_finish_kernel then sums the partials of every
// column in an order fixed by the number of blocks: 64 strands take the blocks s, s + 64, ... in order, and the strands meet in a
// binary tree through LDS.  The grid of the destination side is a function of (num_out_rows, heads, dim), so the order is too.
//
// The slots of a wavefront meet by a butterfly (forward: the (max, sum e, sum e * x) merge; backward: sums), the wavefronts of a
// long row through LDS in the order of the wavefronts (6 planes forward, 4 backward).  Path and order depend on the degree and
// (heads, dim) only: the same bits on every run.
//
// The two invariants of gnna_rowwalk.h hold because every sweep is entered by whole wavefronts with a step count that is uniform
// over the wavefront -- every pass folds over the lanes of a head in every step -- and the barriers sit in loops whose bounds
// (the long rows of the block, heads) are uniform over the block, which no thread leaves early.  Row strides are 32-bit (the
// entries refuse a stride of 2^29 floats or more).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "gnna_gatv2_rows.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // the lane-layout folds, load_piece, leaky, set_drop, check_drop, check_alias
#include "gnna_internal.h"
#include "gnna_ownrows.h"        // the ownership limits, the host side of the rows entries
#include "gnna_rowwalk.h"        // wave_max
#include "gnna_segments.h"       // seg::store_piece, seg::exp_nonpos

namespace gnna {
namespace {

using gat::VT;
using gat::head_sum;
using gat::leaky;
using gat::load_piece;
using gat::slots_sum;
using seg::exp_nonpos;
using seg::store_piece;

// edges per slot and step: the first rung (gnna_dot_rows.hip spilled SGPRs at 4; 4 was not built here).  No instance has a private
// segment or a VGPR spill; the destination side of one-head column blocks spills 2 to 16 SGPRs (the table per pass)
constexpr int kEdges = 2;
using own::kSlotEdges;                          // the two ownership limits: gnna_ownrows.h
constexpr int kLongSteps = own::kLongSteps<kEdges>;

constexpr int kSlotGatv2RowsPack = 23;  // library scratch: (lse, c) per (destination row, head) of a backward call
constexpr int kSlotGatv2RowsAtt = 24;   // library scratch: the partial of d_att of every workgroup of the destination side

enum Pass { kFwd = 0, kDst = 1, kSrc = 2 };

struct Args {
    const float *own; uint32_t ld_own;      // the walked row's side of t: Hd (forward, destination side), Hs (source side)
    const float *own2; uint32_t ld_own2;    // destination side: dY, by the walked row
    const float *gat; uint32_t ld_gat;      // the gathered side of t: Hs (forward, destination side), Hd (source side)
    const float *gat2; uint32_t ld_gat2;    // source side: dY, the second row gathered per edge
    const float *att;                       // [heads * dim]
    const float *Y; uint32_t ld_y;          // destination side: for c
    const float *lse;                       // destination side: [rows, heads]
    float2 *pack;                           // destination side: written (null: not wanted); source side: gathered by id
    const int32_t *rp, *col;                // the CSR walked: A, or A^T on the source side
    float *out; uint32_t ld_out;            // out (forward) | dHd (destination side, may be null) | dHs (source side)
    float *sc;                              // forward: lse [rows, heads]
    float *part;                            // destination side: [blocks, heads * dim], the workgroups' partials of d_att (null: not wanted)
    int64_t rows;                           // rows walked
    uint32_t limit;                         // ids < limit
    int heads, dim;
    float slope;
    bool relu;                              // forward: out = max(out, 0)
    bool walk;                              // false: no edge can count, or no sum is wanted: the index arrays are not read
    bool hold;                              // false: what the row itself brings (and att) is not read either
    uint64_t rng_seed;                      // attention dropout (gnna_ext.h: the mask rule), read by the DROP instances only
    uint32_t drop_thr;
    float keep_scale;
};

// this lane's share of z: sum over its (<= 4) floats of att * lrelu(hs + hd); att is 0 beyond the head's floats
__device__ __forceinline__ float score_part(const VT hs, const VT hd, const VT at, float slope)
{
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) s = __builtin_fmaf(at[q], leaky(hs[q] + hd[q], slope), s);
    return s;
}

// this lane's share of <a, b> over its (<= 4) floats; both are 0 beyond the head's floats
__device__ __forceinline__ float dot_part(const VT a, const VT b)
{
    return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

// ---- attention dropout with its uniform operands in VGPRs (gnna_dot_rows.hip: why; restated here because that file's compilation
// unit keeps its own) -- k(i, j, h) is gat::drop_factor's, bit for bit -------------------------------------------------------------
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

// Forward: the online (max, sum e, sum e * k * Hs) of this lane's head and columns.  Destination side: a = sum g.  Source side:
// a = sum (alpha * k * dY + g).  (m and s are live in the forward only.)
struct State {
    float m, s;
    VT a;
};

template <int PASS>
__device__ __forceinline__ State state_empty()
{
    return State{PASS == kFwd ? -INFINITY : 0.f, 0.f, (VT)(0.f)};
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
    }
}

// a value that is the same in every lane, as the scalar it is
__device__ __forceinline__ uint64_t uniform64(uint64_t x)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

// where a lane stands in its row's column block, and its piece of att (the same for every row)
struct Lane {
    int h;              // its head
    int n4;             // floats of its piece (<= 0: the lane idles)
    bool ok, first;     // n4 > 0; the first lane of its head
    uint32_t colf;      // the column of its piece (< heads * dim <= 2^14)
    VT at;
};

// what the walked row itself brings
struct Held {
    VT own;             // Hd[i] | Hs[j]
    VT dy;              // destination side: dY[i]
    float lse, c;       // destination side
};

// Whole wavefronts only (the destination side folds c over the lanes of a head); on: this lane's slot has such a row.
template <int PASS, int LPH>
__device__ __forceinline__ Held load_held(const Args &p, int64_t row, bool on, const Lane &L)
{
    Held r{(VT)(0.f), (VT)(0.f), 0.f, 0.f};
    const bool ld = on && L.ok && p.hold;
    if (ld) r.own = load_piece(p.own + (size_t)row * p.ld_own + L.colf, L.n4);
    if constexpr (PASS == kDst) {
        VT y = (VT)(0.f);
        if (ld) {
            r.dy = load_piece(p.own2 + (size_t)row * p.ld_own2 + L.colf, L.n4);
            r.lse = p.lse[(size_t)row * (size_t)p.heads + (size_t)L.h];
            y = load_piece(p.Y + (size_t)row * p.ld_y + L.colf, L.n4);
        }
        r.c = head_sum<LPH>(dot_part(r.dy, y));
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
// earlier, or has none, brings no edge.  -> this slot's state; da: the destination side's share of d_att of this lane, added to.
template <int PASS, int LPH, bool DROP>
__device__ __forceinline__ State sweep(const Args &p, const DropRegs &dr, uint32_t row, uint32_t beg, uint32_t end, int steps, int t,
                                       int nl, const Lane &L, const Held &r, VT &da)
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
        VT v[kEdges];
        VT w[PASS == kSrc ? kEdges : 1];
        float2 rec[PASS == kSrc ? kEdges : 1];
        float kf[DROP ? kEdges : 1];
#pragma unroll
        for (int k = 0; k < kEdges; k++) {
            const int id = next[k];
            const bool live = id >= 0 && L.ok;
            dead[k] = live ? 0.f : -INFINITY;
            v[k] = (VT)(0.f);
            if constexpr (PASS == kSrc) { w[k] = (VT)(0.f); rec[k] = make_float2(0.f, 0.f); }
            if (live) {
                v[k] = load_piece(p.gat + (size_t)(uint32_t)id * p.ld_gat + L.colf, L.n4);
                if constexpr (PASS == kSrc) {
                    w[k] = load_piece(p.gat2 + (size_t)(uint32_t)id * p.ld_gat2 + L.colf, L.n4);
                    rec[k] = p.pack[(size_t)(uint32_t)id * (size_t)p.heads + (size_t)L.h];
                }
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
                z[k] = head_sum<LPH>(score_part(v[k], r.own, L.at, p.slope)) + dead[k];
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
                for (int c = 0; c < 4; c++) st.a[c] += ek * v[k][c];     // the message is the row that made the score
            }
            st.m = m;
        } else {
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                // t = Hs[j] + Hd[i], dalpha = <dY[i], Hs[j]>: the gathered row is Hs[j] (destination side) or Hd[i] (source side)
                VT hs, hd, dy;
                float lse_e, c_e;
                if constexpr (PASS == kSrc) { hs = r.own; hd = v[k]; dy = w[k]; lse_e = rec[k].x; c_e = rec[k].y; }
                else { hs = v[k]; hd = r.own; dy = r.dy; lse_e = r.lse; c_e = r.c; }
                const float z = head_sum<LPH>(score_part(hs, hd, L.at, p.slope)) + dead[k];
                float dalpha = head_sum<LPH>(dot_part(dy, hs));
                const float alpha = __expf(z - lse_e);          // (exp(-inf) = 0 for an edge that does not count)
                if constexpr (DROP) dalpha *= kf[k];
                const float dz = alpha * (dalpha - c_e);        // (a dropped edge still contributes -alpha * c)
                const float ak = DROP ? alpha * kf[k] : alpha;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float tq = hs[q] + hd[q];
                    const float g = dz * L.at[q] * (tq > 0.f ? 1.f : p.slope);
                    if constexpr (PASS == kDst) {
                        st.a[q] += g;
                        da[q] = __builtin_fmaf(dz, leaky(tq, p.slope), da[q]);
                    } else {
                        st.a[q] = __builtin_fmaf(ak, dy[q], st.a[q]) + g;
                    }
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
        if (p.out) store_piece(p.out + (size_t)row * p.ld_out + L.colf, st.a, L.n4);
        if constexpr (PASS == kDst)
            if (L.first && p.pack) p.pack[sidx] = make_float2(r.lse, r.c);
    }
}

template <int PASS, int LOG_LPH, int LOG_LPR, bool DROP>
__global__ void __launch_bounds__(kBlock)
gatv2_rows_kernel(const Args p)
{
    constexpr int LPH = 1 << LOG_LPH, LPR = 1 << LOG_LPR, HB = LPR / LPH, R = kWave / LPR, RB = R * kWavesPerBlock;
    constexpr uint32_t kLong = (uint32_t)(R * kEdges * kLongSteps);
    constexpr int kPlanes = PASS == kFwd ? 6 : 4;       // floats of a state that the wavefronts exchange
    __shared__ unsigned long long s_long[kWavesPerBlock];      // per wavefront: the first lanes of the slots whose row is long
    __shared__ float s_red[kPlanes][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH, fl = (cl & (LPH - 1)) * 4;
    const DropRegs dr = drop_regs<DROP>(p.rng_seed, p.drop_thr, p.keep_scale);

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
    const uint64_t long_slots = __ballot(is_long && cl == 0);
    if (lane == 0) s_long[wib] = long_slots;
    __syncthreads();
    const bool mine = live && is_short;
    const uint64_t mid = __ballot(live && !is_long && !is_short);

    // column blocks outside, rows inside: att once per block, and a lane's share of d_att in registers across its rows
    for (int hb0 = 0; hb0 < p.heads; hb0 += HB) {
        // this lane's place in the column block at head hb0
        Lane L;
        {
            const int h = hb0 + hl;
            L.n4 = h < p.heads ? p.dim - fl : 0;
            L.ok = L.n4 > 0;
            L.h = L.ok ? h : 0;
            L.first = fl == 0;
            L.colf = (uint32_t)(L.h * p.dim + (L.ok ? fl : 0));
            L.at = L.ok && p.hold ? load_piece(p.att + L.colf, L.n4) : (VT)(0.f);
        }
        VT da = (VT)(0.f);

        // ---- the short rows (and, in wavefronts of several slots, the rows without edges): every slot its own row ---------------
        if constexpr (R > 1) {
            if (__ballot(mine)) {
                const uint32_t sb = mine ? beg : 0u, se = mine ? end : 0u;
                // every slot makes the steps of the longest short row of the wavefront (at most kSlotEdges / kEdges, rounded up)
                const int steps = wave_max((int)((se - sb + (uint32_t)kEdges - 1u) / (uint32_t)kEdges));
                const Held r = load_held<PASS, LPH>(p, row, mine, L);
                const State st = sweep<PASS, LPH, DROP>(p, dr, (uint32_t)row, sb, se, steps, 0, 1, L, r, da);
                if (mine) write_row<PASS>(p, row, L, r, st);
            }
        }

        // ---- the rows in between: the slots of the wavefront share one row after the other --------------------------------------
        {
            constexpr uint64_t slot_lanes = LPR == 64 ? ~0ull : ((1ull << (LPR & 63)) - 1ull);
            uint64_t todo = mid;
            while (todo) {
                const int s = (__ffsll((unsigned long long)todo) - 1) >> LOG_LPR;
                todo &= ~(slot_lanes << (s * LPR));
                const int64_t rr = r0 + wib * R + s;
                const uint32_t lb = (uint32_t)__shfl((int)beg, s * LPR), le = (uint32_t)__shfl((int)end, s * LPR);
                const int steps = __builtin_amdgcn_readfirstlane((int)((le - lb + (uint32_t)(R * kEdges) - 1u) / (uint32_t)(R * kEdges)));
                const Held r = load_held<PASS, LPH>(p, rr, true, L);
                State st = sweep<PASS, LPH, DROP>(p, dr, (uint32_t)rr, lb, le, steps, sub, R, L, r, da);
                slots_meet<PASS, LPR>(st);
                if (sub == 0) write_row<PASS>(p, rr, L, r, st);
            }
        }

        // ---- the long rows: the whole block, one after the other, in the order of the rows (a lane's share of d_att is added to in
        // that order, so it must not vary from run to run) ------------------------------------------------------------------------
        for (int lw = 0; lw < kWavesPerBlock; lw++)
        for (uint64_t todo = uniform64(s_long[lw]); todo; todo &= todo - 1ull) {
            const int64_t rr = r0 + lw * R + ((__ffsll((unsigned long long)todo) - 1) >> LOG_LPR);
            uint32_t lb = std::min((uint32_t)p.rp[rr], 0x7fffffffu);
            const uint32_t le = std::min((uint32_t)p.rp[rr + 1], 0x7fffffffu);
            if (lb > le) lb = le;
            const int steps = __builtin_amdgcn_readfirstlane((int)((le - lb + (uint32_t)(RB * kEdges) - 1u) / (uint32_t)(RB * kEdges)));
            const Held r = load_held<PASS, LPH>(p, rr, true, L);
            State st = sweep<PASS, LPH, DROP>(p, dr, (uint32_t)rr, lb, le, steps, wib * R + sub, RB, L, r, da);
            slots_meet<PASS, LPR>(st);
            // the wavefronts meet through LDS, in the order of the wavefronts
            __syncthreads();
            if (sub == 0) {
#pragma unroll
                for (int c = 0; c < 4; c++) s_red[c][wib][cl] = st.a[c];
                if constexpr (PASS == kFwd) { s_red[4][wib][cl] = st.m; s_red[5][wib][cl] = st.s; }
            }
            __syncthreads();
            st = state_empty<PASS>();
#pragma unroll 1
            for (int w = 0; w < kWavesPerBlock; w++) {
                State o = state_empty<PASS>();
#pragma unroll
                for (int c = 0; c < 4; c++) o.a[c] = s_red[c][w][cl];
                if constexpr (PASS == kFwd) { o.m = s_red[4][w][cl]; o.s = s_red[5][w][cl]; }
                state_merge<PASS>(st, o);
            }
            if (wib == 0 && sub == 0) write_row<PASS>(p, rr, L, r, st);
        }

        // ---- the workgroup's partial of d_att for this column block: slots (butterfly), wavefronts (LDS, in order), one store ----
        if constexpr (PASS == kDst) {
            if (p.part) {                               // (uniform over the block)
#pragma unroll
                for (int q = 0; q < 4; q++) da[q] = slots_sum<LPR>(da[q]);
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int q = 0; q < 4; q++) s_red[q][wib][cl] = da[q];
                }
                __syncthreads();
                if (wib == 0 && sub == 0 && L.ok) {
                    VT t = (VT)(0.f);
#pragma unroll
                    for (int w = 0; w < kWavesPerBlock; w++) {
#pragma unroll
                        for (int q = 0; q < 4; q++) t[q] += s_red[q][w][cl];
                    }
                    store_piece(p.part + (size_t)blockIdx.x * (size_t)(p.heads * p.dim) + L.colf, t, L.n4);
                }
            }
        }
    }
}

// d_att[c] = the sum over the `blocks` partials of column c, in an order fixed by `blocks`: strand s of 64 adds the blocks
// s, s + 64, ... in order, then the strands meet in a binary tree.  blocks = 0: d_att = 0 (no edge, or no row).
constexpr int kFinCols = 4, kFinStrands = kBlock / kFinCols;
__global__ void __launch_bounds__(kBlock)
datt_finish_kernel(const float *__restrict__ part, int64_t blocks, int W, float *__restrict__ d_att)
{
    __shared__ float s_sum[kFinStrands][kFinCols];
    const int c = threadIdx.x & (kFinCols - 1), strand = threadIdx.x / kFinCols;
    const int col = (int)blockIdx.x * kFinCols + c;
    float t = 0.f;
    if (col < W) {
#pragma unroll 4
        for (int64_t b = strand; b < blocks; b += kFinStrands) t += part[(size_t)b * (size_t)W + (size_t)col];
    }
    s_sum[strand][c] = t;
    __syncthreads();
#pragma unroll
    for (int d = kFinStrands >> 1; d > 0; d >>= 1) {
        if (strand < d) s_sum[strand][c] += s_sum[strand + d][c];
        __syncthreads();
    }
    if (strand == 0 && col < W) d_att[col] = s_sum[0][c];
}

// attn_drop = 0 keeps every edge with k = 1, so the call runs the instances without the mask (which carry no key computation)
template <int PASS>
int launch(const Args &a, hipStream_t stream, const char *noun)
{
    const AttnLayout layout = attn_layout(a.heads, a.dim);                  // (dim <= kMaxDim: log_lph is never capped)
    const dim3 grid = own::rows_grid(a.rows, layout);
    auto with_mask = [&](auto D) {
        dispatch_layout(layout, [&](auto H, auto L) {
            hipLaunchKernelGGL((gatv2_rows_kernel<PASS, decltype(H)::value, decltype(L)::value, decltype(D)::value>), grid,
                               dim3(kBlock), 0, stream, a);
        });
    };
    if (a.drop_thr) with_mask(std::true_type());
    else with_mask(std::false_type());
    return launch_ok("%s launch", noun);
}

// what both entries check alike, before any device work: the checks of every rows entry, then attn_drop and the slope
int check_sizes(const char *what, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, unsigned flags, unsigned allowed_flags,
                float attn_drop, float negative_slope)
{
    int rc = own::check_rows_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, allowed_flags);
    if (rc != GNNA_OK) return rc;
    if ((rc = gat::check_drop(what, attn_drop)) != GNNA_OK) return rc;
    if (!std::isfinite(negative_slope))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative_slope must be finite (got %g)", what, (double)negative_slope);
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_gatv2_forward_rows_f32(const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att, int64_t num_in_rows,
                                const int32_t *row_pointers, const int32_t *column_index, float negative_slope, float attn_drop,
                                uint64_t rng_seed, float *out, int64_t ld_out, float *lse, int64_t num_out_rows, int heads, int dim,
                                unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_gatv2_forward_rows_f32";
    const int rc = check_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU, attn_drop,
                               negative_slope);
    if (rc != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;                    // nothing to write
    const int64_t W = (int64_t)heads * dim;
    const bool no_in = num_in_rows == 0;                      // every id is out of range: out = 0, lse = 0, nothing else is read
    if ((!no_in && (bad_ld(ld_hs, W) || bad_ld(ld_hd, W))) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_hs=%lld ld_hd=%lld "
                    "ld_out=%lld)", what, (long long)ld_hs, (long long)ld_hd, (long long)ld_out);
    if ((!no_in && (!Hs || !Hd || !att || !row_pointers)) || !out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (out == Hs || out == Hd || out == att || out == lse || lse == Hs || lse == Hd || lse == att)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input or the other output", what);
    Args a{};
    a.own = Hd; a.ld_own = (uint32_t)ld_hd; a.gat = Hs; a.ld_gat = (uint32_t)ld_hs; a.att = att;
    a.rp = row_pointers; a.col = column_index; a.out = out; a.ld_out = (uint32_t)ld_out; a.sc = lse;
    a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim; a.slope = negative_slope;
    a.relu = (flags & GNNA_EPILOGUE_RELU) != 0;
    a.walk = a.hold = !no_in && column_index != nullptr;
    gat::set_drop(&a, attn_drop, rng_seed);
    return launch<kFwd>(a, static_cast<hipStream_t>(stream_v), "GATv2 attention (rows)");
}

int gnna_gatv2_backward_rows_f32(const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att, int64_t num_in_rows,
                                 const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
                                 const int32_t *row_pointers, const int32_t *column_index, const int32_t *t_row_pointers,
                                 const int32_t *t_column_index, float negative_slope, float attn_drop, uint64_t rng_seed, float *dHs,
                                 int64_t ld_dhs, float *dHd, int64_t ld_dhd, float *d_att, int64_t num_out_rows, int heads, int dim,
                                 unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_gatv2_backward_rows_f32";
    int rc = check_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE, attn_drop, negative_slope);
    if (rc != GNNA_OK) return rc;
    const int64_t W = (int64_t)heads * dim;
    const bool want_dhs = dHs && num_in_rows > 0, want_dhd = dHd && num_out_rows > 0, want_att = d_att != nullptr;
    if (!want_dhs && !want_dhd && !want_att) return GNNA_OK;
    const bool one_side = num_out_rows == 0 || num_in_rows == 0;      // no edge can exist: the outputs that have rows are 0
    if (bad_ld_of(dHs, ld_dhs, W) || bad_ld_of(dHd, ld_dhd, W) ||
        (!one_side && (bad_ld(ld_hs, W) || bad_ld(ld_hd, W) || bad_ld(ld_y, W) || bad_ld(ld_dy, W))))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_hs=%lld ld_hd=%lld "
                    "ld_y=%lld ld_dy=%lld ld_dhs=%lld ld_dhd=%lld)", what, (long long)ld_hs, (long long)ld_hd, (long long)ld_y,
                    (long long)ld_dy, (long long)ld_dhs, (long long)ld_dhd);
    const bool want_dst = want_dhd || want_att;             // what walks the edges of the structure itself
    if (!one_side) {
        if (!Hs || !Hd || !att || !lse || !Y || !dY) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        if ((want_dst && !row_pointers) || (want_dhs && !t_row_pointers))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer (the structure for dHd and d_att, the transposed structure "
                        "for dHs)", what);
        const void *const ins[] = {Hs, Hd, att, lse, Y, dY}, *const outs[] = {dHs, dHd, d_att};
        if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const AttnLayout layout = attn_layout(heads, dim);
    float2 *pack = nullptr;
    float *part = nullptr;
    int64_t blocks = 0;                                     // partials of d_att that the destination side leaves
    if (!one_side && want_dhs) {
        void *ws = nullptr;
        if ((rc = own::record_scratch(stream, kSlotGatv2RowsPack, (size_t)num_out_rows * heads * sizeof(float2), &ws)) != GNNA_OK) return rc;
        pack = static_cast<float2 *>(ws);
    }
    if (!one_side && want_att) {
        void *ws = nullptr;
        blocks = (int64_t)own::rows_grid(num_out_rows, layout).x;
        if ((rc = own::record_scratch(stream, kSlotGatv2RowsAtt, (size_t)blocks * (size_t)W * sizeof(float), &ws)) != GNNA_OK) return rc;
        part = static_cast<float *>(ws);
    }
    Args a{};
    a.att = att; a.heads = heads; a.dim = dim; a.slope = negative_slope;
    gat::set_drop(&a, attn_drop, rng_seed);
    if (want_dhd || pack || part) {
        // destination side: row i holds Hd[i], dY[i], (lse, c)[i] and pulls Hs[j] -> dHd, the partials of d_att, and the records of
        // the source side (which alone need no edge walk)
        a.own = Hd; a.ld_own = (uint32_t)ld_hd; a.own2 = dY; a.ld_own2 = (uint32_t)ld_dy; a.gat = Hs; a.ld_gat = (uint32_t)ld_hs;
        a.Y = Y; a.ld_y = (uint32_t)ld_y; a.lse = lse; a.pack = pack; a.part = part; a.rp = row_pointers; a.col = column_index;
        a.out = want_dhd ? dHd : nullptr; a.ld_out = (uint32_t)ld_dhd;
        a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows;
        a.hold = !one_side; a.walk = !one_side && want_dst && column_index != nullptr;
        if ((rc = launch<kDst>(a, stream, "GATv2 attention (rows) backward: destination side")) != GNNA_OK) return rc;
    }
    if (want_att) {
        hipLaunchKernelGGL(datt_finish_kernel, dim3((unsigned)((W + kFinCols - 1) / kFinCols)), dim3(kBlock), 0, stream, part, blocks,
                           (int)W, d_att);
        if ((rc = launch_ok("%s launch", "GATv2 attention (rows) backward: d_att")) != GNNA_OK) return rc;
    }
    if (want_dhs) {
        // source side: row j of A^T holds Hs[j] and pulls Hd[i], dY[i], (lse, c)[i] -> dHs
        a.own = Hs; a.ld_own = (uint32_t)ld_hs; a.own2 = nullptr; a.ld_own2 = 0; a.gat = Hd; a.ld_gat = (uint32_t)ld_hd;
        a.gat2 = dY; a.ld_gat2 = (uint32_t)ld_dy; a.Y = nullptr; a.ld_y = 0; a.lse = nullptr; a.pack = pack; a.part = nullptr;
        a.rp = t_row_pointers; a.col = t_column_index; a.out = dHs; a.ld_out = (uint32_t)ld_dhs;
        a.rows = num_in_rows; a.limit = (uint32_t)num_out_rows;
        a.walk = a.hold = !one_side && t_column_index != nullptr;
        if ((rc = launch<kSrc>(a, stream, "GATv2 attention (rows) backward: source side")) != GNNA_OK) return rc;
    }
    return GNNA_OK;
}

}  // extern "C"

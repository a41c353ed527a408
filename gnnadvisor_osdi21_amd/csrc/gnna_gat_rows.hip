// gnna_gat_rows.hip -- the "rows" form of the fused multi-head GAT attention (gnna_gat_forward_rows_f32 / gnna_gat_backward_rows_f32;
// include/gnna_gat_rows.h): the function of gnna_gat.hip's rectangular entries by kernels that own the rows they write.
// CDNA4 / gfx950 only.  No counterpart in the reference (it has no attention layer).
//
// One kernel body, three passes.  Each walks the rows of a CSR the way gnna_edgefeat.hip does -- R = 64 / LPR consecutive rows per
// wavefront, a row by its own slot, by the slots of its wavefront or by the whole workgroup, by its degree alone; ids one step
// ahead; no neighbor-group partition, no atomics, no zero-fill -- with the lane layout of gnna_gat.hip: LPH = next_pow2(ceil(dim / 4))
// lanes of 4 floats cover a head, LPR = LPH * (heads of a column block) <= 64 lanes a row, so a lane's head is fixed and the
// per-head dot product of the backward is a sum over the LPH lanes of the head (DPP).  Rows wider than one wave-wide load are taken
// in column blocks of whole heads.  What a row holds, gathers and writes:
//   * forward (rows of A):       holds el[i]; gathers er[j], H[j]; per lane the online state (m, s, acc[4]) of its head -- the running
//                                max of z, sum e and sum e * H with e = exp(z - m) -- rescaled once per step of kEdges edges; exp is
//                                only ever taken of a score minus a maximum.  ONE pass over column_index where the atomic path has
//                                two (lse, then the gather).  Writes out = acc / s (ReLU here when asked for) and lse = m + log s.
//   * destination side (A):      holds dY[i], el[i], lse[i] and c[i] = <dY[i], Y[i]> (made here per head, DPP); gathers er[j], H[j];
//                                writes d_el[i] = sum dz and the 16-byte record (el, lse, c, 0) of (i, h) into library scratch.
//   * source side (A^T):         holds H[j], er[j]; gathers dY[i] and the record of (i, h) -- one 16-byte load beside the row piece;
//                                recomputing c from a gathered Y[i] would double the bytes gathered per edge, so the scratch it is
//                                (by that count, not by a timing: the other form was not built).  Writes dH[j] and d_er[j].
// The slots of a wavefront meet by a butterfly (forward: the (max, sum e, sum e * x) merge of gnna_softagg.hip; backward: sums), the
// wavefronts of a long row through LDS in the order of the wavefronts.  Path and order depend on the degree and (heads, dim) only:
// the same bits on every run.
//
// The two invariants of gnna_rowwalk.h hold here because every sweep is entered by whole wavefronts with a step count that is
// uniform over the wavefront -- the short rows of a wavefront all make wave_max steps, a row that ended earlier brings no edge --
// so every lane reaches every DPP fold and shuffle; and the barriers sit in loops whose bounds (s_nlong, heads) are uniform over the
// block, which no thread leaves early.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gnna_gat_rows.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // the lane-layout folds, load_piece, leaky, check_alias
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

// edges per slot and step = gathered row pieces in flight per lane (the source side gathers a 16-byte record beside each).  Not
// tuned: 4 is between gnna_edgefeat.hip's 2 (two row pieces per edge) and the 8 of the atomic gather.
constexpr int kEdges = 4;
using own::kSlotEdges;                          // the two ownership limits: gnna_ownrows.h
constexpr int kLongSteps = own::kLongSteps<kEdges>;

constexpr int kSlotGatRowsPack = 20;    // library scratch: (el, lse, c, 0) per (destination row, head) of a backward call

enum Pass { kFwd = 0, kDst = 1, kSrc = 2 };

struct Args {
    const float *gat;           // the rows gathered by id: H (forward, destination side), dY (source side)
    size_t ld_gat;
    const float *own;           // the row held while its edges are walked: dY (destination side), H (source side)
    size_t ld_own;
    const float *Y;             // destination side: for c
    size_t ld_y;
    const float *el, *lse;      // by row: forward (el), destination side (both)
    const float *er;            // by id (forward, destination side); by row (source side)
    VT *pack;                   // destination side: written (null: not wanted); source side: gathered by id
    const int32_t *rp, *col;    // the CSR walked: A, or A^T on the source side
    float *out;                 // out (forward) | dH (source side, may be null)
    size_t ld_out;
    float *sc;                  // [rows, heads]: lse (forward) | d_el (destination side, may be null) | d_er (source side, may be null)
    int64_t rows;               // rows walked
    uint32_t limit;             // ids < limit
    int heads, dim;
    float slope;
    bool relu;                  // forward: out = max(out, 0)
    bool walk;                  // false: no edge can count, or no sum is wanted: the index arrays are not read
    bool hold;                  // false: what the row itself brings is not read either
};

// Forward: the online (max, sum e, sum e * H) of this lane's head and columns.  Backward: s = sum dz, a = sum alpha * dY (m unused).
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
        s.s += o.s;
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
            State o;
            o.m = __shfl_xor(st.m, d);
            o.s = __shfl_xor(st.s, d);
#pragma unroll
            for (int c = 0; c < 4; c++) o.a[c] = __shfl_xor(st.a[c], d);
            state_merge<kFwd>(st, o);
        }
    } else {
        st.s = slots_sum<LPR>(st.s);
        if constexpr (PASS == kSrc) {
#pragma unroll
            for (int c = 0; c < 4; c++) st.a[c] = slots_sum<LPR>(st.a[c]);
        }
    }
}

// where a lane stands in its row's column block
struct Lane {
    int h;              // its head
    int n4;             // floats of its piece (<= 0: the lane idles)
    bool ok, first;     // n4 > 0; the first lane of its head
    size_t colf;        // the column of its piece
};

// what the walked row itself brings
struct Held {
    float el, lse, c;   // forward: el; destination side: all three
    float er;           // source side
    VT own;             // backward: dY[i] | H[j]
};

// Whole wavefronts only (the destination side folds c over the lanes of a head); on: this lane's slot has such a row.
template <int PASS, int LPH>
__device__ __forceinline__ Held load_held(const Args &p, int64_t row, bool on, const Lane &L)
{
    Held r{0.f, 0.f, 0.f, 0.f, (VT)(0.f)};
    const bool ld = on && L.ok && p.hold;
    const size_t sidx = (size_t)(ld ? row : 0) * (size_t)p.heads + (size_t)L.h;
    if constexpr (PASS == kFwd) {
        if (ld) r.el = p.el[sidx];
    } else if constexpr (PASS == kDst) {
        VT y = (VT)(0.f);
        if (ld) {
            r.el = p.el[sidx];
            r.lse = p.lse[sidx];
            r.own = load_piece(p.own + (size_t)row * p.ld_own + L.colf, L.n4);
            y = load_piece(p.Y + (size_t)row * p.ld_y + L.colf, L.n4);
        }
        r.c = head_sum<LPH>((r.own[0] * y[0] + r.own[1] * y[1]) + (r.own[2] * y[2] + r.own[3] * y[3]));
    } else {
        if (ld) {
            r.er = p.er[sidx];
            r.own = load_piece(p.own + (size_t)row * p.ld_own + L.colf, L.n4);
        }
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

// The edges [beg, end) swept by `nl` slots (this one: slot t) in `steps` steps of kEdges edges per slot.  Whole wavefronts only, and
// `steps` is uniform over the wavefront (the backward folds over the lanes of a head in every step); a lane whose row ended earlier,
// or has none, brings no edge.  -> this slot's state.
template <int PASS, int LPH>
__device__ __forceinline__ State sweep(const Args &p, uint32_t beg, uint32_t end, int steps, int t, int nl, const Lane &L, const Held &r)
{
    State st = state_empty<PASS>();
    int next[kEdges];
    load_ids(p, beg, end, t, nl, next);
#pragma unroll 1
    for (int it = 0; it < steps; it++) {
        const uint32_t base = beg + (uint32_t)it * (uint32_t)(nl * kEdges);
        bool live[kEdges];
        VT v[kEdges];
        VT rec[PASS == kSrc ? kEdges : 1];
        float er[kEdges];
#pragma unroll
        for (int k = 0; k < kEdges; k++) {
            const int id = next[k];
            live[k] = id >= 0 && L.ok;
            v[k] = (VT)(0.f);
            er[k] = 0.f;
            if constexpr (PASS == kSrc) rec[k] = (VT)(0.f);
            if (live[k]) {
                v[k] = load_piece(p.gat + (size_t)(uint32_t)id * p.ld_gat + L.colf, L.n4);
                if constexpr (PASS == kSrc) rec[k] = p.pack[(size_t)(uint32_t)id * (size_t)p.heads + (size_t)L.h];
                else er[k] = p.er[(size_t)(uint32_t)id * (size_t)p.heads + (size_t)L.h];
            }
        }
        load_ids(p, base + (uint32_t)(nl * kEdges), end, t, nl, next);
        if constexpr (PASS == kFwd) {
            // the edges of a step enter together: one exp to rescale the state, one per edge
            float z[kEdges];
            float m = st.m;
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                z[k] = live[k] ? leaky(r.el + er[k], p.slope) : -INFINITY;
                m = fmaxf(m, z[k]);
            }
            const float f = st.m == -INFINITY ? 0.f : exp_nonpos(st.m - m);
            st.s *= f;
#pragma unroll
            for (int c = 0; c < 4; c++) st.a[c] *= f;
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                const float e = z[k] == -INFINITY ? 0.f : exp_nonpos(z[k] - m);
                st.s += e;
#pragma unroll
                for (int c = 0; c < 4; c++) st.a[c] += e * v[k][c];
            }
            st.m = m;
        } else {
#pragma unroll
            for (int k = 0; k < kEdges; k++) {
                float z, lse_e, c_e;
                if constexpr (PASS == kSrc) { z = rec[k][0] + r.er; lse_e = rec[k][1]; c_e = rec[k][2]; }
                else { z = r.el + er[k]; lse_e = r.lse; c_e = r.c; }
                const float alpha = live[k] ? __expf(leaky(z, p.slope) - lse_e) : 0.f;
                const float part = (r.own[0] * v[k][0] + r.own[1] * v[k][1]) + (r.own[2] * v[k][2] + r.own[3] * v[k][3]);
                const float dalpha = head_sum<LPH>(part);
                st.s += alpha * (dalpha - c_e) * (z > 0.f ? 1.f : p.slope);
                if constexpr (PASS == kSrc) {
#pragma unroll
                    for (int c = 0; c < 4; c++) st.a[c] += alpha * v[k][c];
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
        const bool any = st.m != -INFINITY;             // a row without edges: out = lse = 0
        VT o;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            o[c] = any ? st.a[c] / st.s : 0.f;
            if (p.relu) o[c] = o[c] < 0.f ? 0.f : o[c];      // (NaN stays NaN, as torch.relu)
        }
        store_piece(p.out + (size_t)row * p.ld_out + L.colf, o, L.n4);
        if (L.first) p.sc[sidx] = any ? st.m + logf(st.s) : 0.f;
    } else if constexpr (PASS == kDst) {
        if (L.first) {
            if (p.sc) p.sc[sidx] = st.s;
            if (p.pack) {
                VT v;
                v[0] = r.el; v[1] = r.lse; v[2] = r.c; v[3] = 0.f;
                p.pack[sidx] = v;
            }
        }
    } else {
        if (p.out) store_piece(p.out + (size_t)row * p.ld_out + L.colf, st.a, L.n4);
        if (L.first && p.sc) p.sc[sidx] = st.s;
    }
}

template <int PASS, int LOG_LPH, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
gat_rows_kernel(const Args p)
{
    constexpr int LPH = 1 << LOG_LPH, LPR = 1 << LOG_LPR, HB = LPR / LPH, R = kWave / LPR, RB = R * kWavesPerBlock;
    constexpr uint32_t kLong = (uint32_t)(R * kEdges * kLongSteps);
    constexpr int kPlanes = PASS == kFwd ? 6 : PASS == kSrc ? 5 : 1;    // floats of a state that the wavefronts exchange
    __shared__ int s_long[RB];
    __shared__ int s_nlong;
    __shared__ float s_red[kPlanes][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH, fl = (cl & (LPH - 1)) * 4;
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
        L.colf = (size_t)L.h * (size_t)p.dim + (size_t)(L.ok ? fl : 0);
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
                const State st = sweep<PASS, LPH>(p, sb, se, steps, 0, 1, L, r);
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
                State st = sweep<PASS, LPH>(p, lb, le, steps, sub, R, L, r);
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
            State st = sweep<PASS, LPH>(p, lb, le, steps, wib * R + sub, RB, L, r);
            slots_meet<PASS, LPR>(st);
            // the wavefronts meet through LDS, in the order of the wavefronts
            __syncthreads();
            if (sub == 0) {
                if constexpr (PASS == kFwd) s_red[5][wib][cl] = st.m;
                s_red[0][wib][cl] = st.s;
                if constexpr (PASS != kDst) {
#pragma unroll
                    for (int c = 0; c < 4; c++) s_red[1 + c][wib][cl] = st.a[c];
                }
            }
            __syncthreads();
            st = state_empty<PASS>();
#pragma unroll 1
            for (int w = 0; w < kWavesPerBlock; w++) {
                State o = state_empty<PASS>();
                if constexpr (PASS == kFwd) o.m = s_red[5][w][cl];
                o.s = s_red[0][w][cl];
                if constexpr (PASS != kDst) {
#pragma unroll
                    for (int c = 0; c < 4; c++) o.a[c] = s_red[1 + c][w][cl];
                }
                state_merge<PASS>(st, o);
            }
            if (wib == 0 && sub == 0) write_row<PASS>(p, rr, L, r, st);
        }
    }
}

template <int PASS>
int launch(const Args &a, hipStream_t stream, const char *noun)
{
    const AttnLayout layout = attn_layout(a.heads, a.dim);                  // (dim <= kMaxDim: log_lph is never capped)
    const dim3 grid = own::rows_grid(a.rows, layout);
    dispatch_layout(layout, [&](auto H, auto L) {
        hipLaunchKernelGGL((gat_rows_kernel<PASS, decltype(H)::value, decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("%s launch", noun);
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_gat_forward_rows_f32(const float *H, int64_t ld_h, int64_t num_in_rows, const float *el, const float *er,
                              const int32_t *row_pointers, const int32_t *column_index, float negative_slope, float *out,
                              int64_t ld_out, float *lse, int64_t num_out_rows, int heads, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_gat_forward_rows_f32";
    const int rc = own::check_rows_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU);
    if (rc != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;                    // nothing to write
    const int64_t W = (int64_t)heads * dim;
    const bool no_in = num_in_rows == 0;                      // every id is out of range: out = 0, lse = 0, nothing else is read
    if ((!no_in && bad_ld(ld_h, W)) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_h=%lld ld_out=%lld)",
                    what, (long long)ld_h, (long long)ld_out);
    if ((!no_in && (!H || !el || !er || !row_pointers)) || !out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (out == H || out == el || out == er || out == lse || lse == el || lse == er || lse == H)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input or the other output", what);
    Args a{};
    a.gat = H; a.ld_gat = (size_t)ld_h; a.el = el; a.er = er; a.rp = row_pointers; a.col = column_index;
    a.out = out; a.ld_out = (size_t)ld_out; a.sc = lse; a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows;
    a.heads = heads; a.dim = dim; a.slope = negative_slope; a.relu = (flags & GNNA_EPILOGUE_RELU) != 0;
    a.walk = a.hold = !no_in && column_index != nullptr;
    return launch<kFwd>(a, static_cast<hipStream_t>(stream_v), "GAT attention (rows)");
}

int gnna_gat_backward_rows_f32(const float *H, int64_t ld_h, int64_t num_in_rows, const float *el, const float *er, const float *lse,
                               const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                               const int32_t *column_index, const int32_t *t_row_pointers, const int32_t *t_column_index,
                               float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_out_rows,
                               int heads, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_gat_backward_rows_f32";
    int rc = own::check_rows_sizes(what, num_out_rows, num_in_rows, heads, dim, flags, GNNA_ACCUMULATE);
    if (rc != GNNA_OK) return rc;
    const int64_t W = (int64_t)heads * dim;
    const bool want_dh = dH && num_in_rows > 0, want_der = d_er && num_in_rows > 0, want_del = d_el && num_out_rows > 0;
    const bool want_src = want_dh || want_der;
    if (!want_src && !want_del) return GNNA_OK;
    const bool one_side = num_out_rows == 0 || num_in_rows == 0;      // no edge can exist: the outputs that have rows are 0
    if (bad_ld_of(dH, ld_dh, W) || (!one_side && (bad_ld(ld_h, W) || bad_ld(ld_y, W) || bad_ld(ld_dy, W))))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_h=%lld ld_y=%lld "
                    "ld_dy=%lld ld_dh=%lld)", what, (long long)ld_h, (long long)ld_y, (long long)ld_dy, (long long)ld_dh);
    if (!one_side) {
        if (!H || !el || !er || !lse || !Y || !dY) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        if ((want_del && !row_pointers) || (want_src && !t_row_pointers))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer (the structure for d_el, the transposed structure for dH "
                        "and d_er)", what);
        const void *const ins[] = {H, el, er, lse, Y, dY}, *const outs[] = {dH, d_el, d_er};
        if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    VT *pack = nullptr;
    if (!one_side && want_src) {
        void *ws = nullptr;
        if ((rc = own::record_scratch(stream, kSlotGatRowsPack, (size_t)num_out_rows * heads * sizeof(VT), &ws)) != GNNA_OK) return rc;
        pack = static_cast<VT *>(ws);
    }
    if (want_del || pack) {
        // destination side: row i holds dY[i], (el, lse, c)[i] and pulls H[j], er[j] -> d_el, and the records of the source side
        Args a{};
        a.gat = H; a.ld_gat = (size_t)ld_h; a.own = dY; a.ld_own = (size_t)ld_dy; a.Y = Y; a.ld_y = (size_t)ld_y;
        a.el = el; a.lse = lse; a.er = er; a.pack = pack; a.rp = row_pointers; a.col = column_index; a.sc = d_el;
        a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim; a.slope = negative_slope;
        a.hold = !one_side; a.walk = !one_side && want_del && column_index != nullptr;
        if ((rc = launch<kDst>(a, stream, "GAT attention (rows) backward: destination side")) != GNNA_OK) return rc;
    }
    if (want_src) {
        // source side: row j of A^T holds H[j], er[j] and pulls dY[i], (el, lse, c)[i] -> dH, d_er
        Args a{};
        a.gat = dY; a.ld_gat = (size_t)ld_dy; a.own = H; a.ld_own = (size_t)ld_h; a.er = er; a.pack = pack;
        a.rp = t_row_pointers; a.col = t_column_index; a.out = dH; a.ld_out = (size_t)ld_dh; a.sc = d_er;
        a.rows = num_in_rows; a.limit = (uint32_t)num_out_rows; a.heads = heads; a.dim = dim; a.slope = negative_slope;
        a.walk = a.hold = !one_side && t_column_index != nullptr;
        if ((rc = launch<kSrc>(a, stream, "GAT attention (rows) backward: source side")) != GNNA_OK) return rc;
    }
    return GNNA_OK;
}

}  // extern "C"

// gnna_gat.hip -- fused multi-head GAT attention, forward and backward (gnna_gat_forward_f32 / gnna_gat_backward_f32 and their
// rectangular forms gnna_gat_forward_rect_f32 / gnna_gat_backward_rect_f32, which the square entries call; with attention dropout
// gnna_gat_forward_drop_f32 / gnna_gat_backward_drop_f32 of gnna_ext.h, the rectangular entries with a mask; with a per-edge score
// term gnna_gat_edge_forward_f32 / gnna_gat_edge_backward_f32 / gnna_gat_alpha_f32 of gnna_gat_edge.h: instances of their own).
// CDNA4 / gfx950 only.  No counterpart in the reference (it has no attention layer).
//
// With lse[i, h] = logsumexp over the edges of row i of s = leaky_relu(el[i, h] + er[j, h]) known, the attention coefficient of
// an edge i <- j is a function of node-sized values only,
//     alpha(i, j, h) = exp(leaky_relu(el[i, h] + er[j, h]) - lse[i, h]),
// so every pass computes it where it gathers the row and no buffer of the size of the edge list exists anywhere.
//
//   forward   (a) gat_lse_kernel: rows of the CSR, a SEG-lane segment of a wavefront per row (the whole block for long rows, after
//                 the short ones), online (max, sum) per head; reads the column ids once and gathers er[j, 0:heads).  One writer
//                 per row, fixed order, plain stores: the same bits on every run.
//             (b) gat_pull_kernel<SIDE_FWD>: out[i] = sum_e alpha * H[col(e)].
//   backward  gat_pack_kernel: c[i, h] = <dY[i, h, :], Y[i, h, :]> (= sum_e alpha * dalpha of the row), packed with el and lse
//                 into 16 bytes per (node, head) of library scratch;
//             gat_pull_kernel<SIDE_BWD_DST>: row i pulls H[j], er[j]:              d_el[i, h] = sum_e dz
//             gat_pull_kernel<SIDE_BWD_SRC>: row j pulls dY[i], (el, lse, c)[i]:   d_er[j, h] = sum_e dz, dH[j] = sum_e alpha * dY[i]
//                 (the edges of row j stand for the edges j -> i: the structure must be symmetric)
//             with dalpha = <dY[i, h, :], H[j, h, :]>, dz = alpha * (dalpha - c[i, h]) * (z > 0 ? 1 : negative_slope).
//
// gat_pull_kernel is the gather of gnna_x16.hip with another lane layout: a wavefront takes G consecutive neighbor-groups, merges
// the groups of one destination row into a run of edges and walks the run 64 edges at a time -- one coalesced load of 64 ids,
// then LPR wave-wide loads of 16 bytes per lane that bring 64 / LPR whole rows each.  A head of `dim` floats is covered by
// LPH = next_pow2(ceil(dim / 4)) lanes and a row by LPR = LPH * (heads of a column block) <= 64 lanes, so a lane's head is fixed:
// it needs one er value (or one 16-byte (el, lse, c) record) per gathered row, and the per-head dot product of the backward is
// a sum over the LPH lanes of the head (DPP).  Rows wider than one wave-wide load are taken in column blocks of whole heads inside
// the call.  dim % 4 != 0: the last lane of a head loads its 1..3 floats one by one; nothing is staged.  At the end of a run the
// 64 / LPR partial rows meet by a butterfly and are ADDED with float atomics (correct for every partition gnna_agg_ld_f32
// accepts, no validation pass), so the outputs are zero-filled first and there is no deterministic schedule for these passes.
//
// Attention dropout (the DROP instances of gat_pull_kernel): alpha' = alpha * k after the softmax, k = 0 or 1 / (1 - attn_drop)
// decided by a splitmix64 key of (rng_seed, i, j, h) that every pass computes beside alpha (gnna_ext.h has the rule; the key is
// key_of_position(rng_seed, u) of gnna_device.h, packed and compared by drop_factor of gnna_gat_common.h).  lse and
// the pack pass do not change: Y = sum alpha' H, so c = <dY, Y> = sum_e alpha' dalpha is still the row's constant, and
// dz = alpha * (k * dalpha - c) * (z > 0 ? 1 : negative_slope), dH[j] = sum alpha * k * dY[i].
//
// Rectangular structures (sampled blocks): num_out_rows destination rows gather from num_in_rows source rows, so every pass has
// two bounds -- one for the rows it walks (what part2Node names), one for the ids it gathers:
//     pass                         rows < (indexed by row)                      ids < (indexed by id)
//     gat_lse_kernel               num_out_rows (el, lse)                       num_in_rows (er)
//     gat_pull_kernel<FWD>         num_out_rows (el, lse, out)                  num_in_rows (H, er)
//     gat_pull_kernel<BWD_DST>     num_out_rows (pack, dY, d_el)                num_in_rows (H, er)
//     gat_pull_kernel<BWD_SRC>     num_in_rows  (er, H, dH, d_er)               num_out_rows (dY, pack)     [transposed structure]
#include <hip/hip_runtime.h>

#include "gnna_ext.h"
#include "gnna_gat_common.h"
#include "gnna_gat_edge.h"

namespace gnna {
namespace {

using namespace gat;      // the folds, the online (max, sum), the dropout factor, the pull launcher, the checks: gnna_gat_common.h

constexpr int kSlotGatPack = 6;   // library scratch: (el, lse, c, 0) per (node, head) of a backward call

enum { SIDE_FWD = 0, SIDE_BWD_DST = 1, SIDE_BWD_SRC = 2 };
// ---- (a) lse[i, h] ------------------------------------------------------------------------------------------------------
// One row [beg, end) swept by `nl` lanes (this one: index t), four edges per lane and step, HB heads from hb0 on.
// EDGE: the score has the per-edge term et[position, h] (gnna_gat_edge.h); a position >= E is skipped like an id >= M.
template <int HB, bool EDGE>
__device__ __forceinline__ void lse_row(const float *__restrict__ el_row, const float *__restrict__ er, const float *__restrict__ et,
                                        int64_t E, const int32_t *__restrict__ col, int64_t beg, int64_t end, int t, int nl, uint32_t M,
                                        int heads, int hb0, float slope, MaxSum acc[HB])
{
    float eli[HB];
#pragma unroll
    for (int hh = 0; hh < HB; hh++) {
        eli[hh] = hb0 + hh < heads ? el_row[hb0 + hh] : 0.f;
        acc[hh] = MaxSum{-INFINITY, 0.f};
    }
    for (int64_t e = beg + t; e < end; e += (int64_t)nl * 4) {
        int id[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t ee = e + (int64_t)k * nl;
            id[k] = ee < end ? col[ee] : -1;
            if ((uint32_t)id[k] >= M) id[k] = -1;                  // an id outside the source rows is skipped, in every pass alike
            if constexpr (EDGE) { if (ee >= E) id[k] = -1; }
        }
#pragma unroll
        for (int hh = 0; hh < HB; hh++) {
            if (hb0 + hh < heads) {
                float x[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if constexpr (EDGE)
                        x[k] = id[k] >= 0 ? leaky(eli[hh] + er[(size_t)(uint32_t)id[k] * heads + hb0 + hh] +
                                                  et[(size_t)(e + (int64_t)k * nl) * heads + hb0 + hh], slope) : -INFINITY;
                    else
                        x[k] = id[k] >= 0 ? leaky(eli[hh] + er[(size_t)(uint32_t)id[k] * heads + hb0 + hh], slope) : -INFINITY;
                }
                acc[hh] = ms_add4(acc[hh], x);
            }
        }
    }
}

// blockIdx.y: block of HB heads.  seg: lanes per row (4 .. 64, a power of two).  N rows (el, lse), ids < M (er).
template <int HB, bool EDGE>
__device__ __forceinline__ void lse_rows(const float *__restrict__ el, const float *__restrict__ er, const float *__restrict__ et,
                                         int64_t E, const int32_t *__restrict__ rp, const int32_t *__restrict__ col, int64_t N,
                                         int64_t M, int heads, float slope, float *__restrict__ lse, int seg)
{
    constexpr int kMaxTile = kWavesPerBlock * (kWave / 4);
    __shared__ int s_long[kMaxTile];
    __shared__ int s_nlong;
    __shared__ float s_red[2][kWavesPerBlock];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int rpw = kWave / seg;                      // rows per wavefront
    const int tile = kWavesPerBlock * rpw;
    const int long_edges = seg * 4 * kLongIters;
    const int hb0 = (int)blockIdx.y * HB;
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * tile;
    const int local = wib * rpw + lane / seg;
    const int64_t row = r0 + local;
    const int t = lane % seg;
    int64_t beg = 0, end = 0;
    if (row < N) { beg = rp[row]; end = rp[row + 1]; }
    const bool is_long = end - beg > long_edges;
    if (is_long && t == 0) s_long[atomicAdd(&s_nlong, 1)] = local;
    // short rows (and rows without edges: lse = 0): the segment -- every lane of a segment takes the same branch
    if (row < N && !is_long) {
        MaxSum acc[HB];
        lse_row<HB, EDGE>(el + (size_t)row * heads, er, et, E, col, beg, end, t, seg, (uint32_t)M, heads, hb0, slope, acc);
#pragma unroll
        for (int hh = 0; hh < HB; hh++) {
            const MaxSum v = seg_reduce(acc[hh], seg);
            if (t == 0 && hb0 + hh < heads) lse[(size_t)row * heads + hb0 + hh] = lse_of(v);
        }
    }
    __syncthreads();
    // long rows: the whole block, one after the other (the list's order may vary; a row's result does not depend on it)
    const int nlong = s_nlong;
    for (int q = 0; q < nlong; q++) {
        const int64_t rr = r0 + s_long[q];
        MaxSum acc[HB];
        lse_row<HB, EDGE>(el + (size_t)rr * heads, er, et, E, col, rp[rr], rp[rr + 1], tid, kBlock, (uint32_t)M, heads, hb0, slope, acc);
#pragma unroll
        for (int hh = 0; hh < HB; hh++) {
            const MaxSum v = seg_reduce(acc[hh], kWave);
            __syncthreads();
            if (lane == 0) { s_red[0][wib] = v.m; s_red[1][wib] = v.l; }
            __syncthreads();
            MaxSum r{s_red[0][0], s_red[1][0]};
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; w++) r = ms_merge(r, MaxSum{s_red[0][w], s_red[1][w]});
            if (tid == 0 && hb0 + hh < heads) lse[(size_t)rr * heads + hb0 + hh] = lse_of(r);
        }
    }
}

template <int HB>
__global__ void __launch_bounds__(kBlock)
gat_lse_kernel(const float *__restrict__ el, const float *__restrict__ er, const int32_t *__restrict__ rp,
               const int32_t *__restrict__ col, int64_t N, int64_t M, int heads, float slope, float *__restrict__ lse, int seg)
{
    lse_rows<HB, false>(el, er, nullptr, 0, rp, col, N, M, heads, slope, lse, seg);
}

// et [E, heads]: the per-edge score term
template <int HB>
__global__ void __launch_bounds__(kBlock)
gat_lse_edge_kernel(const float *__restrict__ el, const float *__restrict__ er, const float *__restrict__ et, int64_t E,
                    const int32_t *__restrict__ rp, const int32_t *__restrict__ col, int64_t N, int64_t M, int heads, float slope,
                    float *__restrict__ lse, int seg)
{
    lse_rows<HB, true>(el, er, et, E, rp, col, N, M, heads, slope, lse, seg);
}

// ---- c[i, h] = <dY[i, h, :], Y[i, h, :]>, packed with el and lse ------------------------------------------------------------

__global__ void __launch_bounds__(kBlock)
gat_pack_kernel(const float *__restrict__ G, size_t ldg, const float *__restrict__ Y, size_t ldy, const float *__restrict__ el,
                const float *__restrict__ lse, VT *__restrict__ pack, size_t N, int heads, int dim)
{
    const size_t n = N * (size_t)heads;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (unsigned)heads, h = i - r * (unsigned)heads;
        const float *g = G + r * ldg + h * (size_t)dim, *y = Y + r * ldy + h * (size_t)dim;
        float c = 0.f;
        for (int f = 0; f < dim; f++) c = __builtin_fmaf(g[f], y[f], c);
        VT v;
        v[0] = el[i]; v[1] = lse[i]; v[2] = c; v[3] = 0.f;
        pack[i] = v;
    }
}

// ---- the gather ----------------------------------------------------------------------------------------------------------

struct GatArgs {
    const float *own; size_t ld_own;      // the row's own features: dY (SIDE_BWD_DST), H (SIDE_BWD_SRC); unused forward
    const float *gat; size_t ld_gat;      // the gathered rows: H (SIDE_FWD, SIDE_BWD_DST), dY (SIDE_BWD_SRC)
    const float *el, *er, *lse;           // [rows, heads]; el and lse: forward only.  er: by id (SIDE_BWD_SRC: by row)
    const VT *pack;                       // backward: (el, lse, c, 0) per (destination row, head)
    const int32_t *col, *pp, *p2n;
    float *out; size_t ld_out;            // out (SIDE_FWD), dH (SIDE_BWD_SRC): zero-filled, added to
    float *dsc;                           // d_el (SIDE_BWD_DST), d_er (SIDE_BWD_SRC): [rows, heads], zero-filled, added to
    float slope;
    int64_t P;
    uint32_t N, M;                        // rows of the structure walked (part2Node < N), rows gathered from (ids < M)
    int heads, dim, G, xcd_remap;
    // attention dropout (gnna_ext.h: the mask rule), read by the DROP instances only
    uint64_t rng_seed;
    uint32_t drop_thr;                    // an edge is kept when the upper 32 bits of its key are >= drop_thr
    float keep_scale;                     // 1 / (1 - attn_drop)
};

// The calls with a per-edge score term (gnna_gat_edge.h): z = el[i] + er[j] + et[position].  A struct of its own, so that the
// kernels without the term keep their arguments.
struct GatEdgeArgs : GatArgs {
    const float *et;                      // [E, heads], by the position in the forward structure's column_index
    float *d_et;                          // SIDE_BWD_DST: [E, heads], zero-filled; dz of every edge walked, one writer per element
    const int32_t *tpos;                  // SIDE_BWD_SRC: [E], position of the transposed structure -> forward position
    uint32_t E;                           // a position >= E is skipped, never read through
};

// k(i, j, h) of the mask rule: keep_scale for a kept edge i <- j of head h, 0 for a dropped one.  A function of the two row
// numbers and the head alone, so the three passes agree without an edge position, a perm array or a reverse-edge map.
__device__ __forceinline__ float drop_factor(const GatArgs &p, uint32_t i, uint32_t j, int h)
{
    return gat::drop_factor(p.rng_seed, p.drop_thr, p.keep_scale, i, j, h);
}

// v, which the compiler may no longer take for uniform when ON.  With one head per column block the head of a lane is the same
// in every lane, and what derives from it is kept in scalar registers: the source-side instances with the mask and the edge term
// then need more than the 102 there are.  As a vector value it costs one register per lane and nothing else.
template <bool ON>
__device__ __forceinline__ int in_vgpr(int v)
{
    if constexpr (ON) asm volatile("" : "+v"(v));
    return v;
}

// DROP: attention dropout after the softmax -- every edge's alpha is scaled by k = drop_factor where it is accumulated, and
// dalpha where it meets c (a dropped edge still contributes -alpha * c to dz).  The DROP = false instances are the code they
// were before the mask existed.
// Args = GatEdgeArgs: the per-edge term, read at the edge's forward position -- e0 + (u0 + k) * R + sub in the structure walked
// (SIDE_FWD, SIDE_BWD_DST), tpos of that position in the transposed one (SIDE_BWD_SRC).  Args = GatArgs is the code without it.
template <int SIDE, int LOG_LPH, int LOG_LPR, bool DROP, class Args>
__global__ void __launch_bounds__(kBlock)
gat_pull_kernel(const Args p)
{
    constexpr bool EDGE = std::is_same<Args, GatEdgeArgs>::value;
    constexpr int LPH = 1 << LOG_LPH;             // lanes per head
    constexpr int LPR = 1 << LOG_LPR;             // lanes per row (of a column block)
    constexpr int HB = LPR / LPH;                 // heads per column block
    constexpr int R = kWave / LPR;                // rows per wave-wide load
    constexpr int U = LPR < 8 ? LPR : 8;          // row loads in flight per lane
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = in_vgpr<EDGE && DROP && SIDE == SIDE_BWD_SRC && HB == 1>(cl >> LOG_LPH), fl = (cl & (LPH - 1)) * 4;
    const int64_t g0 = pull_chunk(p.xcd_remap) * p.G;
    if (g0 >= p.P) return;
    const int cnt = (int)(p.P - g0 < (int64_t)p.G ? p.P - g0 : (int64_t)p.G);
    const PullGroups g = pull_groups(p, g0, cnt, lane);
    unsigned long long starts = g.starts;
    const int heads = p.heads;

    while (starts) {
        const int a = __builtin_ctzll(starts);
        starts &= starts - 1ull;
        const int b = starts ? __builtin_ctzll(starts) : cnt;
        if (__builtin_amdgcn_readlane(g.bad, a)) continue;
        const int rs = __builtin_amdgcn_readlane(g.s, a);
        const int re = __builtin_amdgcn_readlane(g.e, b - 1);
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(g.r, a);
        if (re <= rs) continue;
        for (int hb0 = 0; hb0 < heads; hb0 += HB) {
            const int h = hb0 + hl;
            const int n4 = h < heads ? p.dim - fl : 0;        // floats of this lane's piece (<= 0: the lane idles)
            const bool ok = n4 > 0;
            const size_t colf = (size_t)(ok ? h : 0) * p.dim + (ok ? fl : 0);
            const size_t sidx = (size_t)row * heads + (ok ? h : 0);
            // what the row itself brings
            float el_i = 0.f, lse_i = 0.f, c_i = 0.f, er_j = 0.f;
            VT ownv = (VT)(0.f);
            if (ok) {
                if constexpr (SIDE == SIDE_FWD) { el_i = p.el[sidx]; lse_i = p.lse[sidx]; }
                if constexpr (SIDE == SIDE_BWD_DST) { const VT o = p.pack[sidx]; el_i = o[0]; lse_i = o[1]; c_i = o[2]; }
                if constexpr (SIDE == SIDE_BWD_SRC) er_j = p.er[sidx];
                if constexpr (SIDE != SIDE_FWD) ownv = load_piece(p.own + (size_t)row * p.ld_own + colf, n4);
            }
            VT acc = (VT)(0.f);
            float dzs = 0.f;
            for (int e0 = rs; e0 < re; e0 += kWave) {
                const int nb = re - e0 < kWave ? re - e0 : kWave;
                int id = -1;
                if (lane < nb) {
                    id = p.col[(int64_t)e0 + lane];
                    if ((uint32_t)id >= p.M) id = -1;           // (an id outside the gathered side is skipped, never read)
                }
                int pos = -1;                                   // EDGE: the forward position of this lane's edge
                if constexpr (EDGE) {
                    if (lane < nb) pos = e0 + lane;
                    if constexpr (SIDE == SIDE_BWD_SRC) { if ((uint32_t)pos < p.E) pos = p.tpos[pos]; }      // (tpos has E entries)
                    if ((uint32_t)pos >= p.E) id = -1;
                }
#pragma unroll
                for (int u0 = 0; u0 < LPR; u0 += U) {
                    if (u0 * R >= nb) break;
                    VT v[U];
                    VT rec[SIDE == SIDE_BWD_SRC ? U : 1];
                    float sc[U];
                    float kf[DROP ? U : 1];
                    float et[EDGE ? U : 1];
                    bool live[U];
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const int idj = __shfl(id, (u0 + k) * R + sub);
                        live[k] = idj >= 0 && ok;
                        v[k] = (VT)(0.f);
                        sc[k] = 0.f;
                        if constexpr (SIDE == SIDE_BWD_SRC) rec[k] = (VT)(0.f);
                        [[maybe_unused]] int posj = 0;          // EDGE: the forward position of the edge of this slot
                        if constexpr (EDGE) {
                            posj = SIDE == SIDE_BWD_SRC ? __shfl(pos, (u0 + k) * R + sub) : e0 + (u0 + k) * R + sub;
                            et[k] = 0.f;
                        }
                        if (live[k]) {
                            v[k] = load_piece(p.gat + (size_t)(uint32_t)idj * p.ld_gat + colf, n4);
                            if constexpr (SIDE == SIDE_BWD_SRC) rec[k] = p.pack[(size_t)(uint32_t)idj * heads + h];
                            else sc[k] = p.er[(size_t)(uint32_t)idj * heads + h];
                            if constexpr (EDGE) et[k] = p.et[(size_t)(uint32_t)posj * heads + h];
                        }
                        // (the LPH lanes of a head compute the same key, as they compute the same alpha; an idle lane's is unused)
                        if constexpr (DROP)
                            kf[k] = SIDE == SIDE_BWD_SRC ? drop_factor(p, (uint32_t)idj, row, h) : drop_factor(p, row, (uint32_t)idj, h);
                    }
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        float z, lse_e, c_e;
                        if constexpr (SIDE == SIDE_BWD_SRC) { z = rec[k][0] + er_j; lse_e = rec[k][1]; c_e = rec[k][2]; }
                        else { z = el_i + sc[k]; lse_e = lse_i; c_e = c_i; }
                        if constexpr (EDGE) z += et[k];
                        float alpha = __expf(leaky(z, p.slope) - lse_e);
                        alpha = live[k] ? alpha : 0.f;
                        if constexpr (SIDE != SIDE_FWD) {
                            const float part = (ownv[0] * v[k][0] + ownv[1] * v[k][1]) + (ownv[2] * v[k][2] + ownv[3] * v[k][3]);
                            const float dalpha = head_sum<LPH>(part);
                            if constexpr (EDGE) {
                                float kd = dalpha;
                                if constexpr (DROP) kd = kf[k] * dalpha;
                                const float dz = alpha * (kd - c_e) * (z > 0.f ? 1.f : p.slope);
                                dzs += dz;
                                if constexpr (SIDE == SIDE_BWD_DST) {
                                    if (live[k] && fl == 0) p.d_et[(size_t)(e0 + (u0 + k) * R + sub) * heads + h] = dz;
                                }
                            } else if constexpr (DROP) dzs += alpha * (kf[k] * dalpha - c_e) * (z > 0.f ? 1.f : p.slope);
                            else dzs += alpha * (dalpha - c_e) * (z > 0.f ? 1.f : p.slope);
                        }
                        if constexpr (SIDE != SIDE_BWD_DST) {
                            if constexpr (DROP) alpha *= kf[k];
#pragma unroll
                            for (int q = 0; q < 4; q++) acc[q] = __builtin_fmaf(alpha, v[k][q], acc[q]);
                        }
                    }
                }
            }
            // ---- the R partial rows of the wavefront meet; the first slot adds them to the output ------------------------
            if constexpr (SIDE != SIDE_BWD_DST) {
                VT t;
#pragma unroll
                for (int q = 0; q < 4; q++) t[q] = slots_sum<LPR>(acc[q]);
                if (sub == 0 && ok) {
                    float *dst = p.out + (size_t)row * p.ld_out + colf;
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (q < n4) atomicAdd(dst + q, t[q]);
                }
            }
            if constexpr (SIDE != SIDE_FWD) {
                const float t = slots_sum<LPR>(dzs);
                if (sub == 0 && ok && fl == 0) atomicAdd(p.dsc + sidx, t);
            }
        }
    }
}

// Args: GatArgs, or GatEdgeArgs for the instances with the edge term
template <int SIDE, class Args>
int launch_pull(DeviceState *ds, hipStream_t stream, const Args &a, int partSize)
{
    return gat::launch_pull("GAT attention", ds, stream, a, partSize, [](auto H, auto L, auto D) {
        return gat_pull_kernel<SIDE, decltype(H)::value, decltype(L)::value, decltype(D)::value, Args>;
    });
}

// et: the per-edge term [E, heads] of the edge entries, or null
int launch_lse(hipStream_t stream, const float *el, const float *er, const float *et, int64_t E, const int32_t *rp, const int32_t *col,
               int64_t N, int64_t M, int64_t avg, int heads, float slope, float *lse)
{
    // lanes per row: about a quarter of the average degree (every lane reads 4 edges per step), 4 .. 64
    int seg = 4;
    while (seg < kWave && (int64_t)seg * 4 < avg) seg <<= 1;
    const int64_t tile = (int64_t)kWavesPerBlock * (kWave / seg);
    const int64_t blocks = (N + tile - 1) / tile;
    int hb = 1;
    while (hb < 8 && hb < heads) hb <<= 1;
    const dim3 grid((unsigned)blocks, (unsigned)((heads + hb - 1) / hb));
    if (et) {
        switch (hb) {
        case 1: hipLaunchKernelGGL(gat_lse_edge_kernel<1>, grid, dim3(kBlock), 0, stream, el, er, et, E, rp, col, N, M, heads, slope, lse, seg); break;
        case 2: hipLaunchKernelGGL(gat_lse_edge_kernel<2>, grid, dim3(kBlock), 0, stream, el, er, et, E, rp, col, N, M, heads, slope, lse, seg); break;
        case 4: hipLaunchKernelGGL(gat_lse_edge_kernel<4>, grid, dim3(kBlock), 0, stream, el, er, et, E, rp, col, N, M, heads, slope, lse, seg); break;
        default: hipLaunchKernelGGL(gat_lse_edge_kernel<8>, grid, dim3(kBlock), 0, stream, el, er, et, E, rp, col, N, M, heads, slope, lse, seg); break;
        }
        return launch_ok("GAT lse launch");
    }
    switch (hb) {
    case 1: hipLaunchKernelGGL(gat_lse_kernel<1>, grid, dim3(kBlock), 0, stream, el, er, rp, col, N, M, heads, slope, lse, seg); break;
    case 2: hipLaunchKernelGGL(gat_lse_kernel<2>, grid, dim3(kBlock), 0, stream, el, er, rp, col, N, M, heads, slope, lse, seg); break;
    case 4: hipLaunchKernelGGL(gat_lse_kernel<4>, grid, dim3(kBlock), 0, stream, el, er, rp, col, N, M, heads, slope, lse, seg); break;
    default: hipLaunchKernelGGL(gat_lse_kernel<8>, grid, dim3(kBlock), 0, stream, el, er, rp, col, N, M, heads, slope, lse, seg); break;
    }
    return launch_ok("GAT lse launch");
}

// What the edge entries (gnna_gat_edge.h) add to a call; the others pass none.
struct EdgeTerm {
    const float *ee;                // [num_edges, heads]
    float *d_ee;                    // backward: [num_edges, heads]
    const int32_t *t_edge_pos;      // backward: [num_edges]
    int64_t num_edges;
};

// num_edges, and the arrays it sizes (d_ee and t_edge_pos: the backward)
int check_edge(const char *what, const EdgeTerm &t, bool backward)
{
    if (t.num_edges < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (num_edges=%lld)", what, (long long)t.num_edges);
    if (t.num_edges >= ((int64_t)1 << 31))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld edges in one call (at most 2147483647)", what, (long long)t.num_edges);
    if (t.num_edges > 0 && (!t.ee || (backward && (!t.d_ee || !t.t_edge_pos))))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null edge pointer (%s with num_edges > 0)", what,
                    backward ? "ee, d_ee, t_edge_pos" : "ee");
    return GNNA_OK;
}

// The forward of all entries: num_out_rows rows (el, lse, out) gather from num_in_rows rows (H, er).
int gat_forward_impl(const char *what, bool rect, const EdgeTerm *edge, const float *H, int64_t ld_h, const float *el, const float *er,
                     const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers,
                     const int32_t *part2Node, float negative_slope, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out,
                     float *lse, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize,
                     unsigned flags, void *stream_v)
{
    int rc = check_common(what, rect, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags,
                          GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU);
    if (rc == GNNA_OK) rc = check_drop(what, attn_drop);
    if (rc == GNNA_OK && edge) rc = check_edge(what, *edge, false);
    if (rc != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;                    // nothing to write
    const int64_t W = (int64_t)heads * dim;
    const bool no_in = num_in_rows == 0;                      // every id is out of range: out = 0, lse = 0, H / el / er not read
    if ((!no_in && bad_ld(ld_h, W)) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_h=%lld ld_out=%lld)",
                    what, (long long)ld_h, (long long)ld_out);
    if ((!no_in && (!H || !el || !er || !row_pointers)) || !out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (!no_in && num_parts > 0 && (!column_index || !part_pointers || !part2Node))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (out == H || out == el || out == er || out == lse || lse == el || lse == er || lse == H ||
        (edge && edge->ee && ((const float *)out == edge->ee || (const float *)lse == edge->ee)))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input or the other output", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, out, num_out_rows, (int)W, ld_out);
    if (rc != GNNA_OK) return rc;
    if (num_parts == 0 || no_in || (edge && edge->num_edges == 0)) return launch_zero_fill(ds, stream, lse, num_out_rows, heads, heads);
    const gnna_tuning tune = hinted_tuning(column_index, (int)W);
    // edges per row, for the segment width of the lse pass only: the graph's hint, else what the groups can hold at most
    const int64_t avg = tune.avg_degree > 0 ? tune.avg_degree : (num_parts * (int64_t)partSize + num_out_rows - 1) / num_out_rows;
    rc = launch_lse(stream, el, er, edge ? edge->ee : nullptr, edge ? edge->num_edges : 0, row_pointers, column_index, num_out_rows,
                    num_in_rows, avg, heads, negative_slope, lse);
    if (rc != GNNA_OK) return rc;
    GatEdgeArgs a{};
    if (edge) { a.et = edge->ee; a.E = (uint32_t)edge->num_edges; }
    a.gat = H; a.ld_gat = (size_t)ld_h; a.el = el; a.er = er; a.lse = lse;
    a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.out = out; a.ld_out = (size_t)ld_out;
    a.slope = negative_slope; a.P = num_parts; a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim;
    a.xcd_remap = tune.xcd_remap != 0 ? 1 : 0;
    set_drop(&a, attn_drop, rng_seed);
    rc = edge ? launch_pull<SIDE_FWD>(ds, stream, a, partSize) : launch_pull<SIDE_FWD>(ds, stream, static_cast<const GatArgs &>(a), partSize);
    if (rc != GNNA_OK) return rc;
    return relu_epilogue(what, ds, stream, flags, out, num_out_rows, (int)W, ld_out);
}

// The backward of all entries: the destination-side pass walks the structure (num_out_rows rows, ids < num_in_rows), the
// source-side pass the transposed one (num_in_rows rows, ids < num_out_rows).
int gat_backward_impl(const char *what, bool rect, const EdgeTerm *edge, const float *H, int64_t ld_h, const float *el, const float *er, const float *lse,
                      const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *column_index,
                      const int32_t *part_pointers, const int32_t *part2Node, int64_t num_parts, const int32_t *t_column_index,
                      const int32_t *t_part_pointers, const int32_t *t_part2Node, int64_t t_num_parts, float negative_slope,
                      float attn_drop, uint64_t rng_seed, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_out_rows, int64_t num_in_rows, int heads,
                      int dim, int partSize, unsigned flags, void *stream_v)
{
    int rc = check_common(what, rect, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags, GNNA_ACCUMULATE);
    if (rc == GNNA_OK) rc = check_drop(what, attn_drop);
    if (rc == GNNA_OK && edge) rc = check_edge(what, *edge, true);
    if (rc != GNNA_OK) return rc;
    if (t_num_parts < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (t_num_parts=%lld)", what, (long long)t_num_parts);
    if (num_out_rows == 0 && num_in_rows == 0 && !(edge && edge->num_edges > 0)) return GNNA_OK;
    const int64_t W = (int64_t)heads * dim;
    const bool one_side = num_out_rows == 0 || num_in_rows == 0;      // no edge can exist: the outputs that have rows are 0
    if (one_side) {
        if (num_in_rows > 0 && (bad_ld(ld_dh, W) || !dH || !d_er))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dH / d_er: null pointer or a row stride outside [heads * dim, 2^29)", what);
        if (num_out_rows > 0 && !d_el) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    } else {
        if (bad_ld(ld_h, W) || bad_ld(ld_y, W) || bad_ld(ld_dy, W) || bad_ld(ld_dh, W))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_h=%lld ld_y=%lld "
                        "ld_dy=%lld ld_dh=%lld)", what, (long long)ld_h, (long long)ld_y, (long long)ld_dy, (long long)ld_dh);
        if (!H || !el || !er || !lse || !Y || !dY || !dH || !d_el || !d_er) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        if ((num_parts > 0 && (!column_index || !part_pointers || !part2Node)) ||
            (t_num_parts > 0 && (!t_column_index || !t_part_pointers || !t_part2Node)))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
        const void *const ins[] = {H, el, er, lse, Y, dY, edge ? edge->ee : nullptr, edge ? edge->t_edge_pos : nullptr},
                   *const outs[] = {dH, d_el, d_er, edge ? edge->d_ee : nullptr};
        rc = check_alias(what, ins, outs);
        if (rc != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, dH, num_in_rows, (int)W, ld_dh);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, d_el, num_out_rows, heads, heads);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, d_er, num_in_rows, heads, heads);
    if (rc == GNNA_OK && edge) rc = launch_zero_fill(ds, stream, edge->d_ee, edge->num_edges, heads, heads);      // (a skipped edge's stays 0)
    if (rc == GNNA_OK && edge && edge->num_edges == 0) return rc;                                                // no edge is walked
    if (rc != GNNA_OK || one_side || (num_parts == 0 && t_num_parts == 0)) return rc;
    void *ws = nullptr;
    rc = get_workspace(ds, stream, kSlotGatPack, ((size_t)num_out_rows * heads * sizeof(VT) + 255) & ~(size_t)255, &ws);
    if (rc != GNNA_OK) return rc;
    VT *pack = static_cast<VT *>(ws);
    hipLaunchKernelGGL(gat_pack_kernel, dim3(elementwise_grid(num_out_rows * heads, ds->num_cus, 8)), dim3(kBlock), 0, stream, dY,
                       (size_t)ld_dy, Y, (size_t)ld_y, el, lse, pack, (size_t)num_out_rows, heads, dim);
    rc = launch_ok("%s: pack launch", what);
    if (rc != GNNA_OK) return rc;
    GatEdgeArgs a{};
    if (edge) { a.et = edge->ee; a.d_et = edge->d_ee; a.tpos = edge->t_edge_pos; a.E = (uint32_t)edge->num_edges; }
    const GatArgs &plain = a;
    a.er = er; a.pack = pack; a.col = column_index; a.pp = part_pointers; a.p2n = part2Node;
    a.slope = negative_slope; a.P = num_parts; a.heads = heads; a.dim = dim;
    a.xcd_remap = xcd_remap_on();
    set_drop(&a, attn_drop, rng_seed);
    // destination side: row i pulls H[j], er[j] -> d_el
    a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows;
    a.own = dY; a.ld_own = (size_t)ld_dy; a.gat = H; a.ld_gat = (size_t)ld_h; a.dsc = d_el;
    rc = edge ? launch_pull<SIDE_BWD_DST>(ds, stream, a, partSize) : launch_pull<SIDE_BWD_DST>(ds, stream, plain, partSize);
    if (rc != GNNA_OK) return rc;
    // source side: row j pulls dY[i], (el, lse, c)[i] -> d_er, dH -- over the edges j -> i, the rows of the transposed structure
    a.N = (uint32_t)num_in_rows; a.M = (uint32_t)num_out_rows;
    a.col = t_column_index; a.pp = t_part_pointers; a.p2n = t_part2Node; a.P = t_num_parts;
    a.own = H; a.ld_own = (size_t)ld_h; a.gat = dY; a.ld_gat = (size_t)ld_dy; a.dsc = d_er; a.out = dH; a.ld_out = (size_t)ld_dh;
    return edge ? launch_pull<SIDE_BWD_SRC>(ds, stream, a, partSize) : launch_pull<SIDE_BWD_SRC>(ds, stream, plain, partSize);
}

// ---- alpha[e, h], edge for edge (gnna_gat_alpha_f32) ----------------------------------------------------------------------
// One thread per (position, head); the row of a position by bisection of the row pointers (the last row that begins at or
// before it).  A position outside [rp[0], rp[N]) or with an id >= M: 0.  et may be null.
__global__ void __launch_bounds__(kBlock)
gat_alpha_kernel(const float *__restrict__ el, const float *__restrict__ er, const float *__restrict__ et,
                 const float *__restrict__ lse, const int32_t *__restrict__ rp, const int32_t *__restrict__ col, int64_t N,
                 uint32_t M, int64_t E, int heads, float slope, float *__restrict__ alpha)
{
    const size_t n = (size_t)E * (size_t)heads;
    const int64_t first = rp[0], last = rp[N];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int64_t e = (int64_t)(i / (unsigned)heads);
        const int h = (int)(i - (size_t)e * (unsigned)heads);
        float a = 0.f;
        if (e >= first && e < last) {
            int64_t lo = 0, hi = N;                              // rp[lo] <= e < rp[hi]
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (rp[mid] <= e) lo = mid; else hi = mid;
            }
            const uint32_t j = (uint32_t)col[e];
            if (j < M) {
                float z = el[(size_t)lo * heads + h] + er[(size_t)j * heads + h];
                if (et) z += et[i];
                a = __expf(leaky(z, slope) - lse[(size_t)lo * heads + h]);
            }
        }
        alpha[i] = a;
    }
}

int gat_alpha_impl(const char *what, const float *el, const float *er, const float *ee, const float *lse, const int32_t *row_pointers,
                   const int32_t *column_index, float negative_slope, float *alpha, int64_t num_out_rows, int64_t num_in_rows,
                   int64_t num_edges, int heads, void *stream_v)
{
    if (num_out_rows < 0 || num_in_rows < 0 || num_edges < 0 || heads < 1)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (num_out_rows=%lld num_in_rows=%lld num_edges=%lld heads=%d)", what,
                    (long long)num_out_rows, (long long)num_in_rows, (long long)num_edges, heads);
    if (std::max(num_out_rows, num_in_rows) >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 536870911): shard the rows", what,
                    (long long)std::max(num_out_rows, num_in_rows));
    if (num_edges >= ((int64_t)1 << 31))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld edges in one call (at most 2147483647)", what, (long long)num_edges);
    if (heads > 64) return fail(GNNA_ERR_UNSUPPORTED, "%s: at most 64 heads (got %d)", what, heads);
    if (num_edges == 0) return GNNA_OK;                       // nothing to write
    if (!alpha) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    const bool none = num_out_rows == 0 || num_in_rows == 0;  // no edge can exist: alpha = 0, nothing is read
    if (!none && (!el || !er || !lse || !row_pointers || !column_index)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (alpha == el || alpha == er || alpha == ee || alpha == lse)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    int rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    if (none) return launch_zero_fill(ds, stream, alpha, num_edges, heads, heads);
    hipLaunchKernelGGL(gat_alpha_kernel, dim3(elementwise_grid(num_edges * heads, ds->num_cus, 8)), dim3(kBlock), 0, stream, el, er, ee,
                       lse, row_pointers, column_index, num_out_rows, (uint32_t)num_in_rows, num_edges, heads, negative_slope, alpha);
    return launch_ok("%s launch", what);
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_gat_forward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const int32_t *row_pointers,
                         const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                         float negative_slope, float *out, int64_t ld_out, float *lse, int64_t num_nodes, int heads, int dim,
                         int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    return gat_forward_impl("gnna_gat_forward_f32", false, nullptr, H, ld_h, el, er, row_pointers, column_index, part_pointers, part2Node,
                            negative_slope, 0.f, 0, out, ld_out, lse, num_nodes, num_nodes, heads, dim, num_parts, partSize, flags, stream_v);
}

int gnna_gat_forward_rect_f32(const float *H, int64_t ld_h, const float *el, const float *er, const int32_t *row_pointers,
                              const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                              float negative_slope, float *out, int64_t ld_out, float *lse, int64_t num_out_rows,
                              int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize, unsigned flags,
                              void *stream_v)
{
    return gat_forward_impl("gnna_gat_forward_rect_f32", true, nullptr, H, ld_h, el, er, row_pointers, column_index, part_pointers, part2Node,
                            negative_slope, 0.f, 0, out, ld_out, lse, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags,
                            stream_v);
}

int gnna_gat_backward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse, const float *Y,
                          int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                          const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                          float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_nodes,
                          int heads, int dim, int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    (void)row_pointers;     // both passes walk the neighbor-groups
    // a symmetric structure is its own transpose
    return gat_backward_impl("gnna_gat_backward_f32", false, nullptr, H, ld_h, el, er, lse, Y, ld_y, dY, ld_dy, column_index, part_pointers,
                             part2Node, num_parts, column_index, part_pointers, part2Node, num_parts, negative_slope, 0.f, 0, dH, ld_dh,
                             d_el, d_er, num_nodes, num_nodes, heads, dim, partSize, flags, stream_v);
}

int gnna_gat_backward_dir_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse, const float *Y,
                              int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                              const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                              int64_t num_parts, const int32_t *t_row_pointers, const int32_t *t_column_index,
                              const int32_t *t_part_pointers, const int32_t *t_part2Node, int64_t t_num_parts,
                              float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_nodes,
                              int heads, int dim, int partSize, unsigned flags, void *stream_v)
{
    (void)row_pointers;
    (void)t_row_pointers;
    return gat_backward_impl("gnna_gat_backward_f32", false, nullptr, H, ld_h, el, er, lse, Y, ld_y, dY, ld_dy, column_index, part_pointers,
                             part2Node, num_parts, t_column_index, t_part_pointers, t_part2Node, t_num_parts, negative_slope, 0.f, 0,
                             dH, ld_dh, d_el, d_er, num_nodes, num_nodes, heads, dim, partSize, flags, stream_v);
}

int gnna_gat_backward_rect_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse, const float *Y,
                               int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                               const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                               int64_t num_parts, const int32_t *t_row_pointers, const int32_t *t_column_index,
                               const int32_t *t_part_pointers, const int32_t *t_part2Node, int64_t t_num_parts,
                               float negative_slope, float *dH, int64_t ld_dh, float *d_el, float *d_er, int64_t num_out_rows,
                               int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags, void *stream_v)
{
    (void)row_pointers;
    (void)t_row_pointers;
    return gat_backward_impl("gnna_gat_backward_rect_f32", true, nullptr, H, ld_h, el, er, lse, Y, ld_y, dY, ld_dy, column_index,
                             part_pointers, part2Node, num_parts, t_column_index, t_part_pointers, t_part2Node, t_num_parts,
                             negative_slope, 0.f, 0, dH, ld_dh, d_el, d_er, num_out_rows, num_in_rows, heads, dim, partSize, flags,
                             stream_v);
}

int gnna_gat_forward_drop_f32(const float *H, int64_t ld_h, const float *el, const float *er, const int32_t *row_pointers,
                              const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                              float negative_slope, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out, float *lse,
                              int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts, int partSize,
                              unsigned flags, void *stream_v)
{
    return gat_forward_impl("gnna_gat_forward_drop_f32", true, nullptr, H, ld_h, el, er, row_pointers, column_index, part_pointers, part2Node,
                            negative_slope, attn_drop, rng_seed, out, ld_out, lse, num_out_rows, num_in_rows, heads, dim, num_parts,
                            partSize, flags, stream_v);
}

int gnna_gat_backward_drop_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *lse, const float *Y,
                               int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                               const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                               int64_t num_parts, const int32_t *t_row_pointers, const int32_t *t_column_index,
                               const int32_t *t_part_pointers, const int32_t *t_part2Node, int64_t t_num_parts,
                               float negative_slope, float attn_drop, uint64_t rng_seed, float *dH, int64_t ld_dh, float *d_el,
                               float *d_er, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize,
                               unsigned flags, void *stream_v)
{
    (void)row_pointers;
    (void)t_row_pointers;
    return gat_backward_impl("gnna_gat_backward_drop_f32", true, nullptr, H, ld_h, el, er, lse, Y, ld_y, dY, ld_dy, column_index,
                             part_pointers, part2Node, num_parts, t_column_index, t_part_pointers, t_part2Node, t_num_parts,
                             negative_slope, attn_drop, rng_seed, dH, ld_dh, d_el, d_er, num_out_rows, num_in_rows, heads, dim,
                             partSize, flags, stream_v);
}

// ---- with a per-edge score term (gnna_gat_edge.h) ---------------------------------------------------------------------------

int gnna_gat_edge_forward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *ee,
                              const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers,
                              const int32_t *part2Node, float negative_slope, float attn_drop, uint64_t rng_seed, float *out,
                              int64_t ld_out, float *lse, int64_t num_out_rows, int64_t num_in_rows, int64_t num_edges, int heads,
                              int dim, int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    const EdgeTerm edge{ee, nullptr, nullptr, num_edges};
    return gat_forward_impl("gnna_gat_edge_forward_f32", true, &edge, H, ld_h, el, er, row_pointers, column_index, part_pointers,
                            part2Node, negative_slope, attn_drop, rng_seed, out, ld_out, lse, num_out_rows, num_in_rows, heads, dim,
                            num_parts, partSize, flags, stream_v);
}

int gnna_gat_edge_backward_f32(const float *H, int64_t ld_h, const float *el, const float *er, const float *ee, const float *lse,
                               const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                               const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node,
                               int64_t num_parts, const int32_t *t_row_pointers, const int32_t *t_column_index,
                               const int32_t *t_part_pointers, const int32_t *t_part2Node, int64_t t_num_parts,
                               const int32_t *t_edge_pos, float negative_slope, float attn_drop, uint64_t rng_seed, float *dH,
                               int64_t ld_dh, float *d_el, float *d_er, float *d_ee, int64_t num_out_rows, int64_t num_in_rows,
                               int64_t num_edges, int heads, int dim, int partSize, unsigned flags, void *stream_v)
{
    (void)row_pointers;
    (void)t_row_pointers;
    const EdgeTerm edge{ee, d_ee, t_edge_pos, num_edges};
    return gat_backward_impl("gnna_gat_edge_backward_f32", true, &edge, H, ld_h, el, er, lse, Y, ld_y, dY, ld_dy, column_index,
                             part_pointers, part2Node, num_parts, t_column_index, t_part_pointers, t_part2Node, t_num_parts,
                             negative_slope, attn_drop, rng_seed, dH, ld_dh, d_el, d_er, num_out_rows, num_in_rows, heads, dim,
                             partSize, flags, stream_v);
}

int gnna_gat_alpha_f32(const float *el, const float *er, const float *ee, const float *lse, const int32_t *row_pointers,
                       const int32_t *column_index, float negative_slope, float *alpha, int64_t num_out_rows, int64_t num_in_rows,
                       int64_t num_edges, int heads, void *stream_v)
{
    return gat_alpha_impl("gnna_gat_alpha_f32", el, er, ee, lse, row_pointers, column_index, negative_slope, alpha, num_out_rows,
                          num_in_rows, num_edges, heads, stream_v);
}

#pragma GCC visibility pop
}  // extern "C"

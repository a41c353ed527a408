// gnna_gatv2.hip -- fused multi-head GATv2 ("dynamic") attention, forward and backward (gnna_gatv2_forward_f32 /
// gnna_gatv2_backward_f32 of gnna_gatv2.h: the rectangular form with the dropout mask of gnna_ext.h).  CDNA4 / gfx950 only.
// No counterpart in the reference (it has no attention layer).
//
// The score of an edge i <- j is z = sum_d att[h, d] * lrelu(Hs[j, h, d] + Hd[i, h, d]): the non-linearity sits inside the dot
// product, so unlike gnna_gat.hip there is no pair of node-sized scalars to make it from.  But the lane layout of the gather gives
// every head LPH consecutive lanes that hold the gathered row's piece of that head in registers, so z is one head_sum<LPH> (DPP)
// over a product each lane makes from what it has loaded anyway plus the walked row's own Hd and att pieces (loaded once per
// run and column block).  With lse[i, h] known, alpha = exp(z - lse[i, h]) is recomputed wherever a row is gathered and no buffer
// of the size of the edge list exists anywhere.
//
//   forward   (a) gat::lse_kernel<LseArgs> (gnna_gat_common.h: the lse pass shared with gnna_dotattn.hip; LseArgs below says what
//                 the score is): rows of the CSR, one wavefront per row (the whole block for long rows, after the short
//                 ones); 64 / LPR edges per wave-wide load, four loads per step, online (max, sum) per head and slot.  The slots,
//                 then the waves, meet in a fixed order; one writer per (row, head), plain stores: the same bits on every run.
//             (b) gatv2_pull_kernel<SIDE_FWD>: out[i] = sum_e alpha * k * Hs[col(e)] over the neighbor-groups.
//             Two full gathers of Hs.  A one-pass online softmax would keep (max, sum, row accumulator) per run and need a merge
//             across the waves (and workgroups) that share a destination row: out of scope here, see DESIGN 7k.
//   backward  gat::lse_c_pack_kernel (gnna_gat_common.h, shared with gnna_dotattn.hip): (lse, c = <dY[i, h, :], Y[i, h, :]>) per (row, head), 8 bytes, in library scratch;
//             gatv2_pull_kernel<SIDE_BWD_DST>: row i pulls Hs[j]:                     dHd[i] = sum_e g, d_att += sum_e dz * lrelu(t)
//             gatv2_pull_kernel<SIDE_BWD_SRC>: row j pulls dY[i], Hd[i], pack[i]:      dHs[j] = sum_e (alpha * k * dY[i] + g)
//                 (over the transposed structure; a symmetric graph passes its own)
//             with t = Hs[j] + Hd[i], dalpha = <dY[i, h, :], Hs[j, h, :]>, dz = alpha * (k * dalpha - c), g = dz * att * (t > 0 ? 1 : slope).
//
// gatv2_pull_kernel has the layout of gat_pull_kernel (gnna_gat.hip): G consecutive neighbor-groups per wavefront, the groups of
// one row merged into a run, 64 ids per coalesced load, LPR-lane rows, column blocks of whole heads, the 64 / LPR partial rows
// met by a butterfly and ADDED with float atomics (outputs zero-filled first; no deterministic schedule).  On the destination
// side of the backward the loop over the column blocks is the outer one, so that a lane's piece of d_att stays in registers
// across every run its wavefront walks (the other two sides keep gat_pull_kernel's order: runs outside, column blocks inside);
// it then meets over the slots of the wavefront (DPP) and the waves of the workgroup (LDS) and goes out with one float atomic
// per element and workgroup.  The backward passes keep 4 edges in flight per lane (the source side holds two gathered rows per
// edge, the destination side a vector gradient and its share of d_att), the forward 8.  The bounds of the passes are those of
// the table in gnna_gat.hip (rows of the side walked, ids of the side gathered).
#include <hip/hip_runtime.h>

#include "gnna_gatv2.h"
#include "gnna_gat_common.h"

namespace gnna {
namespace {

using namespace gat;

constexpr int kSlotGatv2Pack = 9;     // library scratch: (lse, c) per (destination row, head) of a backward call

enum { SIDE_FWD = 0, SIDE_BWD_DST = 1, SIDE_BWD_SRC = 2 };

// this lane's share of z: sum over its (<= 4) floats of att * lrelu(hs + hd); att is 0 beyond the head's floats
__device__ __forceinline__ float score_part(const VT hs, const VT hd, const VT at, float slope)
{
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) s = __builtin_fmaf(at[q], leaky(hs[q] + hd[q], slope), s);
    return s;
}

// ---- (a) lse[i, h] ------------------------------------------------------------------------------------------------------

// (the score of gat::lse_kernel, gnna_gat_common.h)
struct LseArgs {
    const float *hs; size_t ld_hs;        // by id (< M)
    const float *hd; size_t ld_hd;        // by row (< N)
    const float *att;
    const int32_t *rp, *col;
    float *lse;
    int64_t N;
    uint32_t M;
    int heads, dim;
    float slope;

    struct Own { VT hd, at; };
    __device__ __forceinline__ Own own(int64_t row, size_t colf, int n4) const
    {
        return Own{load_piece(hd + (size_t)row * ld_hd + colf, n4), load_piece(att + colf, n4)};
    }
    __device__ __forceinline__ const float *gathered(uint32_t id) const { return hs + (size_t)id * ld_hs; }
    __device__ __forceinline__ float part(const Own &o, const VT v) const { return score_part(v, o.hd, o.at, slope); }
    __device__ __forceinline__ float scaled(float s) const { return s; }
};

// ---- the gather ----------------------------------------------------------------------------------------------------------

struct PullArgs {
    const float *own; size_t ld_own;      // the walked row's side of t: Hd (SIDE_FWD, SIDE_BWD_DST), Hs (SIDE_BWD_SRC)
    const float *gat; size_t ld_gat;      // the gathered rows: Hs (SIDE_FWD, SIDE_BWD_DST), dY (SIDE_BWD_SRC)
    const float *gat2; size_t ld_gat2;    // SIDE_BWD_SRC: Hd, the second row gathered per edge
    const float *dy; size_t ld_dy;        // SIDE_BWD_DST: dY, by the walked row
    const float *att;                     // [heads * dim]
    const float *lse;                     // SIDE_FWD: [rows, heads]
    const float2 *pack;                   // backward: (lse, c) per (destination row, head)
    const int32_t *col, *pp, *p2n;
    float *out; size_t ld_out;            // out (SIDE_FWD), dHd (SIDE_BWD_DST), dHs (SIDE_BWD_SRC): zero-filled, added to
    float *d_att;                         // SIDE_BWD_DST: [heads * dim], zero-filled, added to
    float slope;
    int64_t P;
    uint32_t N, M;                        // rows of the structure walked (part2Node < N), rows gathered from (ids < M)
    int heads, dim, G, xcd_remap;
    uint64_t rng_seed;                    // attention dropout (gnna_ext.h: the mask rule), read by the DROP instances only
    uint32_t drop_thr;
    float keep_scale;
};

template <int SIDE, int LOG_LPH, int LOG_LPR, bool DROP>
__global__ void __launch_bounds__(kBlock)
gatv2_pull_kernel(const PullArgs p)
{
    constexpr int LPH = 1 << LOG_LPH;             // lanes per head
    constexpr int LPR = 1 << LOG_LPR;             // lanes per row (of a column block)
    constexpr int HB = LPR / LPH;                 // heads per column block
    constexpr int R = kWave / LPR;                // rows per wave-wide load
    constexpr int UMAX = SIDE == SIDE_FWD ? 8 : 4;           // (backward: a vector gradient per edge, two gathered rows on the source side)
    constexpr int U = LPR < UMAX ? LPR : UMAX;    // edges in flight per lane
    __shared__ float s_datt[SIDE == SIDE_BWD_DST ? kWavesPerBlock * kWave * 4 : 1];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH, fl = (cl & (LPH - 1)) * 4;
    const int64_t g0 = pull_chunk(p.xcd_remap) * p.G;
    // (a wavefront without groups walks nothing but stays for the workgroup's barriers of SIDE_BWD_DST)
    const int cnt = g0 >= p.P ? 0 : (int)(p.P - g0 < (int64_t)p.G ? p.P - g0 : (int64_t)p.G);
    if constexpr (SIDE != SIDE_BWD_DST)
        if (cnt == 0) return;
    const PullGroups g = pull_groups(p, g0, cnt, lane);
    const int heads = p.heads;

    // One run -- the edges [rs, re) of `row` -- for the column block at hb0: the row's own pieces, the gather, the butterfly, the
    // atomics.  da: SIDE_BWD_DST's share of d_att for this lane's piece of the block, carried by the caller.
    auto run_block = [&](int hb0, int rs, int re, uint32_t row, VT &da) {
        const int h = hb0 + hl;
        const int n4 = h < heads ? p.dim - fl : 0;            // floats of this lane's piece (<= 0: the lane idles)
        const bool ok = n4 > 0;
        const size_t colf = (size_t)(ok ? h : 0) * p.dim + (ok ? fl : 0);
        const size_t sidx = (size_t)row * heads + (ok ? h : 0);
        // what the row itself brings
        float lse_i = 0.f, c_i = 0.f;
        VT at = (VT)(0.f), ownv = (VT)(0.f), dyv = (VT)(0.f);
        if (ok) {
            at = load_piece(p.att + colf, n4);
            ownv = load_piece(p.own + (size_t)row * p.ld_own + colf, n4);
            if constexpr (SIDE == SIDE_FWD) lse_i = p.lse[sidx];
            if constexpr (SIDE == SIDE_BWD_DST) {
                const float2 o = p.pack[sidx];
                lse_i = o.x; c_i = o.y;
                dyv = load_piece(p.dy + (size_t)row * p.ld_dy + colf, n4);
            }
        }
        VT acc = (VT)(0.f);
        for (int e0 = rs; e0 < re; e0 += kWave) {
            const int nb = re - e0 < kWave ? re - e0 : kWave;
            int id = -1;
            if (lane < nb) {
                id = p.col[(int64_t)e0 + lane];
                if ((uint32_t)id >= p.M) id = -1;           // (an id outside the gathered side is skipped, never read)
            }
            for (int u0 = 0; u0 < LPR; u0 += U) {
                if (u0 * R >= nb) break;
                VT v[U];
                VT w[SIDE == SIDE_BWD_SRC ? U : 1];
                float2 rec[SIDE == SIDE_BWD_SRC ? U : 1];
                float kf[DROP ? U : 1];
                bool live[U];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const int idj = __shfl(id, (u0 + k) * R + sub);
                    live[k] = idj >= 0 && ok;
                    v[k] = (VT)(0.f);
                    if constexpr (SIDE == SIDE_BWD_SRC) { w[k] = (VT)(0.f); rec[k] = make_float2(0.f, 0.f); }
                    if (live[k]) {
                        v[k] = load_piece(p.gat + (size_t)(uint32_t)idj * p.ld_gat + colf, n4);
                        if constexpr (SIDE == SIDE_BWD_SRC) {
                            w[k] = load_piece(p.gat2 + (size_t)(uint32_t)idj * p.ld_gat2 + colf, n4);
                            rec[k] = p.pack[(size_t)(uint32_t)idj * heads + h];
                        }
                    }
                    // (the LPH lanes of a head compute the same key, as they compute the same alpha; an idle lane's is unused)
                    if constexpr (DROP)
                        kf[k] = SIDE == SIDE_BWD_SRC ? drop_factor(p.rng_seed, p.drop_thr, p.keep_scale, (uint32_t)idj, row, h)
                                                     : drop_factor(p.rng_seed, p.drop_thr, p.keep_scale, row, (uint32_t)idj, h);
                }
#pragma unroll
                for (int k = 0; k < U; k++) {
                    // t = Hs[j] + Hd[i]: the gathered row is Hs[j] (forward, destination side) or Hd[i] (source side)
                    VT hsv, hdv, dyk;
                    float lse_e, c_e;
                    if constexpr (SIDE == SIDE_BWD_SRC) { hsv = ownv; hdv = w[k]; dyk = v[k]; lse_e = rec[k].x; c_e = rec[k].y; }
                    else { hsv = v[k]; hdv = ownv; dyk = dyv; lse_e = lse_i; c_e = c_i; }
                    const float z = head_sum<LPH>(score_part(hsv, hdv, at, p.slope));
                    float alpha = __expf(z - lse_e);
                    alpha = live[k] ? alpha : 0.f;
                    if constexpr (SIDE == SIDE_FWD) {
                        if constexpr (DROP) alpha *= kf[k];
#pragma unroll
                        for (int q = 0; q < 4; q++) acc[q] = __builtin_fmaf(alpha, v[k][q], acc[q]);
                    } else {
                        const float part = (dyk[0] * hsv[0] + dyk[1] * hsv[1]) + (dyk[2] * hsv[2] + dyk[3] * hsv[3]);
                        float dalpha = head_sum<LPH>(part);
                        if constexpr (DROP) dalpha *= kf[k];
                        const float dz = alpha * (dalpha - c_e);      // (a dropped edge still contributes -alpha * c)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float tq = hsv[q] + hdv[q];
                            const float g = dz * at[q] * (tq > 0.f ? 1.f : p.slope);
                            if constexpr (SIDE == SIDE_BWD_DST) {
                                acc[q] += g;
                                da[q] = __builtin_fmaf(dz, leaky(tq, p.slope), da[q]);
                            } else {
                                const float ak = DROP ? alpha * kf[k] : alpha;
                                acc[q] = __builtin_fmaf(ak, dyk[q], acc[q]) + g;
                            }
                        }
                    }
                }
            }
        }
        // ---- the R partial rows of the wavefront meet; the first slot adds them to the output ----------------------------
        VT t;
#pragma unroll
        for (int q = 0; q < 4; q++) t[q] = slots_sum<LPR>(acc[q]);
        if (sub == 0 && ok) {
            float *dst = p.out + (size_t)row * p.ld_out + colf;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q < n4) atomicAdd(dst + q, t[q]);
        }
    };
    // the next run of the wavefront's groups: false for one that contributes nothing
    auto next_run = [&](unsigned long long &starts, int &rs, int &re, uint32_t &row) {
        const int a = __builtin_ctzll(starts);
        starts &= starts - 1ull;
        const int b = starts ? __builtin_ctzll(starts) : cnt;
        if (__builtin_amdgcn_readlane(g.bad, a)) return false;
        rs = __builtin_amdgcn_readlane(g.s, a);
        re = __builtin_amdgcn_readlane(g.e, b - 1);
        row = (uint32_t)__builtin_amdgcn_readlane(g.r, a);
        return re > rs;
    };
    int rs = 0, re = 0;
    uint32_t row = 0;
    if constexpr (SIDE != SIDE_BWD_DST) {
        // runs outside, column blocks inside, as gat_pull_kernel: a run is decoded once
        VT unused = (VT)(0.f);
        unsigned long long starts = g.starts;
        while (starts) {
            if (!next_run(starts, rs, re, row)) continue;
            for (int hb0 = 0; hb0 < heads; hb0 += HB) run_block(hb0, rs, re, row, unused);
        }
    } else {
        // column blocks outside: a lane's share of d_att stays in registers across every run of the wavefront, then meets over
        // the slots of the wavefront and the waves of the workgroup and goes out with one atomic per element
        for (int hb0 = 0; hb0 < heads; hb0 += HB) {
            VT da = (VT)(0.f);
            unsigned long long starts = g.starts;
            while (starts)
                if (next_run(starts, rs, re, row)) run_block(hb0, rs, re, row, da);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float t = slots_sum<LPR>(da[q]);
                if (sub == 0) s_datt[(wib * kWave + cl) * 4 + q] = t;
            }
            __syncthreads();
            const int h = hb0 + hl;
            const int n4 = h < heads ? p.dim - fl : 0;
            if (wib == 0 && sub == 0 && n4 > 0) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float t = 0.f;
#pragma unroll
                    for (int w = 0; w < kWavesPerBlock; w++) t += s_datt[(w * kWave + cl) * 4 + q];
                    if (q < n4 && t != 0.f) atomicAdd(p.d_att + (size_t)h * p.dim + fl + q, t);
                }
            }
            __syncthreads();
        }
    }
}

template <int SIDE>
int launch_pull(DeviceState *ds, hipStream_t stream, const PullArgs &a, int partSize)
{
    return gat::launch_pull("GATv2 attention", ds, stream, a, partSize, [](auto H, auto L, auto D) {
        return gatv2_pull_kernel<SIDE, decltype(H)::value, decltype(L)::value, decltype(D)::value>;
    });
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

// num_out_rows rows (Hd, lse, out) gather from num_in_rows rows (Hs).
int gnna_gatv2_forward_f32(const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att,
                           const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers,
                           const int32_t *part2Node, float negative_slope, float attn_drop, uint64_t rng_seed, float *out,
                           int64_t ld_out, float *lse, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim,
                           int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    const char *what = "gnna_gatv2_forward_f32";
    int rc = check_common(what, true, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags,
                          GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU);
    if (rc == GNNA_OK) rc = check_drop(what, attn_drop);
    if (rc != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;                    // nothing to write
    const int64_t W = (int64_t)heads * dim;
    const bool no_in = num_in_rows == 0;                      // every id is out of range: out = 0, lse = 0, Hs / Hd / att not read
    if ((!no_in && (bad_ld(ld_hs, W) || bad_ld(ld_hd, W))) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_hs=%lld ld_hd=%lld "
                    "ld_out=%lld)", what, (long long)ld_hs, (long long)ld_hd, (long long)ld_out);
    if ((!no_in && (!Hs || !Hd || !att || !row_pointers)) || !out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (!no_in && num_parts > 0 && (!column_index || !part_pointers || !part2Node))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (out == Hs || out == Hd || out == att || out == lse || lse == Hs || lse == Hd || lse == att)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input or the other output", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, out, num_out_rows, (int)W, ld_out);
    if (rc != GNNA_OK) return rc;
    if (num_parts == 0 || no_in) return launch_zero_fill(ds, stream, lse, num_out_rows, heads, heads);
    const gnna_tuning tune = hinted_tuning(column_index, (int)W);
    LseArgs l{};
    l.hs = Hs; l.ld_hs = (size_t)ld_hs; l.hd = Hd; l.ld_hd = (size_t)ld_hd; l.att = att; l.rp = row_pointers; l.col = column_index;
    l.lse = lse; l.N = num_out_rows; l.M = (uint32_t)num_in_rows; l.heads = heads; l.dim = dim; l.slope = negative_slope;
    rc = launch_lse("GATv2 lse", stream, l);
    if (rc != GNNA_OK) return rc;
    PullArgs a{};
    a.own = Hd; a.ld_own = (size_t)ld_hd; a.gat = Hs; a.ld_gat = (size_t)ld_hs; a.att = att; a.lse = lse;
    a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.out = out; a.ld_out = (size_t)ld_out;
    a.slope = negative_slope; a.P = num_parts; a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim;
    a.xcd_remap = tune.xcd_remap != 0 ? 1 : 0;
    set_drop(&a, attn_drop, rng_seed);
    rc = launch_pull<SIDE_FWD>(ds, stream, a, partSize);
    if (rc != GNNA_OK) return rc;
    return relu_epilogue(what, ds, stream, flags, out, num_out_rows, (int)W, ld_out);
}

// The destination-side pass walks the structure (num_out_rows rows, ids < num_in_rows), the source-side pass the transposed one
// (num_in_rows rows, ids < num_out_rows).
int gnna_gatv2_backward_f32(const float *Hs, int64_t ld_hs, const float *Hd, int64_t ld_hd, const float *att, const float *lse,
                            const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                            const int32_t *column_index, const int32_t *part_pointers, const int32_t *part2Node, int64_t num_parts,
                            const int32_t *t_row_pointers, const int32_t *t_column_index, const int32_t *t_part_pointers,
                            const int32_t *t_part2Node, int64_t t_num_parts, float negative_slope, float attn_drop,
                            uint64_t rng_seed, float *dHs, int64_t ld_dhs, float *dHd, int64_t ld_dhd, float *d_att,
                            int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int partSize, unsigned flags,
                            void *stream_v)
{
    (void)row_pointers;     // both passes walk the neighbor-groups
    (void)t_row_pointers;
    const char *what = "gnna_gatv2_backward_f32";
    int rc = check_common(what, true, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags, GNNA_ACCUMULATE);
    if (rc == GNNA_OK) rc = check_drop(what, attn_drop);
    if (rc != GNNA_OK) return rc;
    if (t_num_parts < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (t_num_parts=%lld)", what, (long long)t_num_parts);
    const int64_t W = (int64_t)heads * dim;
    const bool one_side = num_out_rows == 0 || num_in_rows == 0;      // no edge can exist: every output is 0
    if (!d_att) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (one_side) {
        if (num_in_rows > 0 && (bad_ld(ld_dhs, W) || !dHs))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dHs: null pointer or a row stride outside [heads * dim, 2^29)", what);
        if (num_out_rows > 0 && (bad_ld(ld_dhd, W) || !dHd))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dHd: null pointer or a row stride outside [heads * dim, 2^29)", what);
    } else {
        if (bad_ld(ld_hs, W) || bad_ld(ld_hd, W) || bad_ld(ld_y, W) || bad_ld(ld_dy, W) || bad_ld(ld_dhs, W) || bad_ld(ld_dhd, W))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_hs=%lld ld_hd=%lld "
                        "ld_y=%lld ld_dy=%lld ld_dhs=%lld ld_dhd=%lld)", what, (long long)ld_hs, (long long)ld_hd, (long long)ld_y,
                        (long long)ld_dy, (long long)ld_dhs, (long long)ld_dhd);
        if (!Hs || !Hd || !att || !lse || !Y || !dY || !dHs || !dHd) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        if ((num_parts > 0 && (!column_index || !part_pointers || !part2Node)) ||
            (t_num_parts > 0 && (!t_column_index || !t_part_pointers || !t_part2Node)))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
        const void *const ins[] = {Hs, Hd, att, lse, Y, dY}, *const outs[] = {dHs, dHd, d_att};
        rc = check_alias(what, ins, outs);
        if (rc != GNNA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, d_att, 1, (int)W, W);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, dHs, num_in_rows, (int)W, ld_dhs);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, dHd, num_out_rows, (int)W, ld_dhd);
    if (rc != GNNA_OK || one_side || (num_parts == 0 && t_num_parts == 0)) return rc;
    PullArgs a{};
    rc = launch_lse_c_pack<kSlotGatv2Pack>(what, ds, stream, dY, ld_dy, Y, ld_y, lse, num_out_rows, heads, dim, &a.pack);
    if (rc != GNNA_OK) return rc;
    a.att = att; a.slope = negative_slope; a.heads = heads; a.dim = dim;
    a.xcd_remap = xcd_remap_on();
    set_drop(&a, attn_drop, rng_seed);
    // destination side: row i pulls Hs[j] -> dHd, d_att
    a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows;
    a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.P = num_parts;
    a.own = Hd; a.ld_own = (size_t)ld_hd; a.gat = Hs; a.ld_gat = (size_t)ld_hs; a.dy = dY; a.ld_dy = (size_t)ld_dy;
    a.out = dHd; a.ld_out = (size_t)ld_dhd; a.d_att = d_att;
    rc = launch_pull<SIDE_BWD_DST>(ds, stream, a, partSize);
    if (rc != GNNA_OK) return rc;
    // source side: row j pulls dY[i], Hd[i], (lse, c)[i] -> dHs -- over the edges j -> i, the rows of the transposed structure
    a.N = (uint32_t)num_in_rows; a.M = (uint32_t)num_out_rows;
    a.col = t_column_index; a.pp = t_part_pointers; a.p2n = t_part2Node; a.P = t_num_parts;
    a.own = Hs; a.ld_own = (size_t)ld_hs; a.gat = dY; a.ld_gat = (size_t)ld_dy; a.gat2 = Hd; a.ld_gat2 = (size_t)ld_hd;
    a.dy = nullptr; a.ld_dy = 0; a.out = dHs; a.ld_out = (size_t)ld_dhs; a.d_att = nullptr;
    return launch_pull<SIDE_BWD_SRC>(ds, stream, a, partSize);
}

#pragma GCC visibility pop
}  // extern "C"

// gnna_dotattn.hip -- fused multi-head scaled dot-product graph attention, forward and backward (gnna_dot_attn_forward_f32 /
// gnna_dot_attn_backward_f32 of gnna_dotattn.h: the rectangular form with the dropout mask of gnna_ext.h).  CDNA4 / gfx950 only.
// No counterpart in the reference (it has no attention layer).
//
// The score of an edge i <- j is z = scale * <Q[i, h, :], K[j, h, :]> and the message is a second matrix, V[j].  The lane layout
// is that of gnna_gat.hip / gnna_gatv2.hip: every head has LPH consecutive lanes that hold the gathered row's piece of that head in
// registers, so z is one head_sum<LPH> (DPP) over a product each lane makes from the K piece it has loaded and the walked row's own
// Q piece (loaded once per run and column block).  With lse[i, h] known, alpha = exp(z - lse[i, h]) is recomputed wherever a row
// is gathered and no buffer of the size of the edge list exists anywhere.
//
//   forward   (a) gat::lse_kernel<LseArgs> (gnna_gat_common.h: the lse pass shared with gnna_gatv2.hip; LseArgs below says what
//                 the score is): rows of the CSR, one wavefront per row (the whole block for long rows, after the short ones);
//                 64 / LPR edges per wave-wide load, four loads per step, online (max, sum) per head and slot.  The slots, then
//                 the waves, meet in a fixed order; one writer per (row, head), plain stores: the same bits on every run.
//             (b) dot_pull_kernel<SIDE_FWD>: out[i] = sum_e alpha * k * V[col(e)] over the neighbor-groups; gathers K[j] and V[j].
//             A one-pass online softmax is out of scope here, see DESIGN 7l.
//   backward  gat::lse_c_pack_kernel (gnna_gat_common.h, shared with gnna_gatv2.hip): (lse, c = <dY[i, h, :], Y[i, h, :]>) per (row, head), 8 bytes, in library scratch;
//             dot_pull_kernel<SIDE_BWD_DST>: row i owns Q[i], dY[i], pack[i], pulls K[j], V[j]:   dQ[i] = scale * sum_e dz * K[j]
//             dot_pull_kernel<SIDE_BWD_SRC>: row j owns K[j], V[j], pulls Q[i], dY[i], pack[i]:   dK[j] = scale * sum_e dz * Q[i],
//                 dV[j] = sum_e alpha * k * dY[i]   (over the transposed structure; a symmetric graph passes its own)
//             with dalpha = <dY[i, h, :], V[j, h, :]>, dz = alpha * (k * dalpha - c).
//
// dot_pull_kernel has the layout of gatv2_pull_kernel: G consecutive neighbor-groups per wavefront, the groups of one row merged
// into a run, 64 ids per coalesced load, LPR-lane rows, column blocks of whole heads, the 64 / LPR partial rows met by a butterfly
// and ADDED with float atomics (outputs zero-filled first; no deterministic schedule).  Every side gathers two rows per edge; the
// source side of the backward also carries two accumulators, which meet through two butterflies.  The bounds of the passes are
// those of the table in gnna_gat.hip (rows of the side walked, ids of the side gathered).
#include <hip/hip_runtime.h>

#include "gnna_dotattn.h"
#include "gnna_gat_common.h"

namespace gnna {
namespace {

using namespace gat;

constexpr int kSlotDotPack = 10;      // library scratch: (lse, c) per (destination row, head) of a backward call

enum { SIDE_FWD = 0, SIDE_BWD_DST = 1, SIDE_BWD_SRC = 2 };

// this lane's share of <a, b> over its (<= 4) floats; both are 0 beyond the head's floats
__device__ __forceinline__ float dot_part(const VT a, const VT b)
{
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) s = __builtin_fmaf(a[q], b[q], s);
    return s;
}

// ---- (a) lse[i, h] ------------------------------------------------------------------------------------------------------

// (the score of gat::lse_kernel, gnna_gat_common.h)
struct LseArgs {
    const float *q; size_t ld_q;          // by row (< N)
    const float *k; size_t ld_k;          // by id (< M)
    const int32_t *rp, *col;
    float *lse;
    int64_t N;
    uint32_t M;
    int heads, dim;
    float scale;

    typedef VT Own;
    __device__ __forceinline__ Own own(int64_t row, size_t colf, int n4) const { return load_piece(q + (size_t)row * ld_q + colf, n4); }
    __device__ __forceinline__ const float *gathered(uint32_t id) const { return k + (size_t)id * ld_k; }
    __device__ __forceinline__ float part(const Own qv, const VT v) const { return dot_part(qv, v); }
    __device__ __forceinline__ float scaled(float s) const { return scale * s; }
};

// ---- the gather ----------------------------------------------------------------------------------------------------------

// (the row strides are 32-bit here: the entries refuse a stride of 2^29 floats or more, and six 64-bit strides cost the source
// side of the backward with the mask its last SGPRs)
struct PullArgs {
    const float *own; uint32_t ld_own;      // the walked row's side of z: Q (SIDE_FWD, SIDE_BWD_DST), K (SIDE_BWD_SRC)
    const float *own2; uint32_t ld_own2;    // the walked row's second piece: dY (SIDE_BWD_DST), V (SIDE_BWD_SRC)
    const float *gat; uint32_t ld_gat;      // the gathered side of z: K (SIDE_FWD, SIDE_BWD_DST), Q (SIDE_BWD_SRC)
    const float *gat2; uint32_t ld_gat2;    // the second row gathered per edge: V (SIDE_FWD, SIDE_BWD_DST), dY (SIDE_BWD_SRC)
    const float *lse;                     // SIDE_FWD: [rows, heads]
    const float2 *pack;                   // backward: (lse, c) per (destination row, head)
    const int32_t *col, *pp, *p2n;
    float *out; uint32_t ld_out;            // out (SIDE_FWD), dQ (SIDE_BWD_DST), dK (SIDE_BWD_SRC): zero-filled, added to
    float *out2; uint32_t ld_out2;          // SIDE_BWD_SRC: dV, zero-filled, added to
    float scale;
    int64_t P;
    uint32_t N, M;                        // rows of the structure walked (part2Node < N), rows gathered from (ids < M)
    int heads, dim, G, xcd_remap;
    uint64_t rng_seed;                    // attention dropout (gnna_ext.h: the mask rule), read by the DROP instances only
    uint32_t drop_thr;
    float keep_scale;
};

template <int SIDE, int LOG_LPH, int LOG_LPR, bool DROP>
__global__ void __launch_bounds__(kBlock)
dot_pull_kernel(const PullArgs p)
{
    constexpr int LPH = 1 << LOG_LPH;             // lanes per head
    constexpr int LPR = 1 << LOG_LPR;             // lanes per row (of a column block)
    constexpr int HB = LPR / LPH;                 // heads per column block
    constexpr int R = kWave / LPR;                // rows per wave-wide load
    constexpr int UMAX = SIDE == SIDE_FWD ? 8 : 4;           // (two gathered rows per edge on every side; two accumulators on the source side)
    constexpr int U = LPR < UMAX ? LPR : UMAX;    // edges in flight per lane
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH, fl = (cl & (LPH - 1)) * 4;
    const int64_t g0 = pull_chunk(p.xcd_remap) * p.G;
    if (g0 >= p.P) return;
    const int cnt = (int)(p.P - g0 < (int64_t)p.G ? p.P - g0 : (int64_t)p.G);
    const PullGroups g = pull_groups(p, g0, cnt, lane);
    unsigned long long starts = g.starts;
    const int heads = p.heads;

    // One run -- the edges [rs, re) of `row` -- for the column block at hb0: the row's own pieces, the gather, the butterflies,
    // the atomics.
    auto run_block = [&](int hb0, int rs, int re, uint32_t row) {
        const int h = hb0 + hl;
        const int n4 = h < heads ? p.dim - fl : 0;            // floats of this lane's piece (<= 0: the lane idles)
        const bool ok = n4 > 0;
        const size_t colf = (size_t)(ok ? h : 0) * p.dim + (ok ? fl : 0);
        const size_t sidx = (size_t)row * heads + (ok ? h : 0);
        // what the row itself brings
        float lse_i = 0.f, c_i = 0.f;
        VT ownv = (VT)(0.f), own2v = (VT)(0.f);
        if (ok) {
            ownv = load_piece(p.own + (size_t)row * p.ld_own + colf, n4);
            if constexpr (SIDE == SIDE_FWD) lse_i = p.lse[sidx];
            else own2v = load_piece(p.own2 + (size_t)row * p.ld_own2 + colf, n4);
            if constexpr (SIDE == SIDE_BWD_DST) {
                const float2 o = p.pack[sidx];
                lse_i = o.x; c_i = o.y;
            }
        }
        VT acc = (VT)(0.f), acc2 = (VT)(0.f);
        for (int e0 = rs; e0 < re; e0 += kWave) {
            const int nb = re - e0 < kWave ? re - e0 : kWave;
            int id = -1;
            if (lane < nb) {
                id = p.col[(int64_t)e0 + lane];
                if ((uint32_t)id >= p.M) id = -1;           // (an id outside the gathered side is skipped, never read)
            }
            for (int u0 = 0; u0 < LPR; u0 += U) {
                if (u0 * R >= nb) break;
                VT v[U], w[U];
                float2 rec[SIDE == SIDE_BWD_SRC ? U : 1];
                float kf[DROP ? U : 1];
                bool live[U];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const int idj = __shfl(id, (u0 + k) * R + sub);
                    live[k] = idj >= 0 && ok;
                    v[k] = (VT)(0.f);
                    w[k] = (VT)(0.f);
                    if constexpr (SIDE == SIDE_BWD_SRC) rec[k] = make_float2(0.f, 0.f);
                    if (live[k]) {
                        v[k] = load_piece(p.gat + (size_t)(uint32_t)idj * p.ld_gat + colf, n4);
                        w[k] = load_piece(p.gat2 + (size_t)(uint32_t)idj * p.ld_gat2 + colf, n4);
                        if constexpr (SIDE == SIDE_BWD_SRC) rec[k] = p.pack[(size_t)(uint32_t)idj * heads + h];
                    }
                    // (the LPH lanes of a head compute the same key, as they compute the same alpha; an idle lane's is unused)
                    if constexpr (DROP)
                        kf[k] = SIDE == SIDE_BWD_SRC ? drop_factor(p.rng_seed, p.drop_thr, p.keep_scale, (uint32_t)idj, row, h)
                                                     : drop_factor(p.rng_seed, p.drop_thr, p.keep_scale, row, (uint32_t)idj, h);
                }
#pragma unroll
                for (int k = 0; k < U; k++) {
                    // z = scale * <Q[i], K[j]>: one of the two is the walked row's, the other the gathered row
                    const float z = p.scale * head_sum<LPH>(dot_part(ownv, v[k]));
                    float lse_e = lse_i, c_e = c_i;
                    if constexpr (SIDE == SIDE_BWD_SRC) { lse_e = rec[k].x; c_e = rec[k].y; }
                    float alpha = __expf(z - lse_e);
                    alpha = live[k] ? alpha : 0.f;
                    if constexpr (SIDE == SIDE_FWD) {
                        if constexpr (DROP) alpha *= kf[k];
#pragma unroll
                        for (int q = 0; q < 4; q++) acc[q] = __builtin_fmaf(alpha, w[k][q], acc[q]);
                    } else {
                        // dalpha = <dY[i], V[j]>: (own2, gathered V) on the destination side, (gathered dY, own V) on the source side
                        float dalpha = head_sum<LPH>(dot_part(own2v, w[k]));
                        if constexpr (DROP) dalpha *= kf[k];
                        const float dz = alpha * (dalpha - c_e);      // (a dropped edge still contributes -alpha * c)
#pragma unroll
                        for (int q = 0; q < 4; q++) acc[q] = __builtin_fmaf(dz, v[k][q], acc[q]);
                        if constexpr (SIDE == SIDE_BWD_SRC) {
                            const float ak = DROP ? alpha * kf[k] : alpha;
#pragma unroll
                            for (int q = 0; q < 4; q++) acc2[q] = __builtin_fmaf(ak, w[k][q], acc2[q]);
                        }
                    }
                }
            }
        }
        // ---- the R partial rows of the wavefront meet; the first slot adds them to the output ----------------------------
        VT t, t2 = (VT)(0.f);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            t[q] = slots_sum<LPR>(acc[q]);
            if constexpr (SIDE != SIDE_FWD) t[q] *= p.scale;
            if constexpr (SIDE == SIDE_BWD_SRC) t2[q] = slots_sum<LPR>(acc2[q]);
        }
        if (sub == 0 && ok) {
            float *dst = p.out + (size_t)row * p.ld_out + colf;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q < n4) atomicAdd(dst + q, t[q]);
            if constexpr (SIDE == SIDE_BWD_SRC) {
                float *dst2 = p.out2 + (size_t)row * p.ld_out2 + colf;
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (q < n4) atomicAdd(dst2 + q, t2[q]);
            }
        }
    };
    // runs outside, column blocks inside, as gat_pull_kernel: a run is decoded once
    while (starts) {
        const int a = __builtin_ctzll(starts);
        starts &= starts - 1ull;
        const int b = starts ? __builtin_ctzll(starts) : cnt;
        if (__builtin_amdgcn_readlane(g.bad, a)) continue;      // a run that contributes nothing
        const int rs = __builtin_amdgcn_readlane(g.s, a);
        const int re = __builtin_amdgcn_readlane(g.e, b - 1);
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(g.r, a);
        if (re <= rs) continue;
        for (int hb0 = 0; hb0 < heads; hb0 += HB) run_block(hb0, rs, re, row);
    }
}

template <int SIDE>
int launch_pull(DeviceState *ds, hipStream_t stream, const PullArgs &a, int partSize)
{
    return gat::launch_pull("dot-product attention", ds, stream, a, partSize, [](auto H, auto L, auto D) {
        return dot_pull_kernel<SIDE, decltype(H)::value, decltype(L)::value, decltype(D)::value>;
    });
}

// scale of the dot entries: finite, refused before any device work (0 is uniform attention, a negative one is allowed)
int check_scale(const char *what, float scale)
{
    if (!std::isfinite(scale)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: scale must be finite (got %g)", what, (double)scale);
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

// num_out_rows rows (Q, lse, out) gather from num_in_rows rows (K, V).
int gnna_dot_attn_forward_f32(const float *Q, int64_t ld_q, const float *K, int64_t ld_k, const float *V, int64_t ld_v,
                              const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers,
                              const int32_t *part2Node, float scale, float attn_drop, uint64_t rng_seed, float *out, int64_t ld_out,
                              float *lse, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts,
                              int partSize, unsigned flags, void *stream_v)
{
    const char *what = "gnna_dot_attn_forward_f32";
    int rc = check_common(what, true, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags,
                          GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU);
    if (rc == GNNA_OK) rc = check_drop(what, attn_drop);
    if (rc == GNNA_OK) rc = check_scale(what, scale);
    if (rc != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;                    // nothing to write
    const int64_t W = (int64_t)heads * dim;
    const bool no_in = num_in_rows == 0;                      // every id is out of range: out = 0, lse = 0, Q / K / V not read
    if ((!no_in && (bad_ld(ld_q, W) || bad_ld(ld_k, W) || bad_ld(ld_v, W))) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_q=%lld ld_k=%lld "
                    "ld_v=%lld ld_out=%lld)", what, (long long)ld_q, (long long)ld_k, (long long)ld_v, (long long)ld_out);
    if ((!no_in && (!Q || !K || !V || !row_pointers)) || !out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (!no_in && num_parts > 0 && (!column_index || !part_pointers || !part2Node))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (out == Q || out == K || out == V || out == lse || lse == Q || lse == K || lse == V)
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
    l.q = Q; l.ld_q = (size_t)ld_q; l.k = K; l.ld_k = (size_t)ld_k; l.rp = row_pointers; l.col = column_index;
    l.lse = lse; l.N = num_out_rows; l.M = (uint32_t)num_in_rows; l.heads = heads; l.dim = dim; l.scale = scale;
    rc = launch_lse("dot-product attention lse", stream, l);
    if (rc != GNNA_OK) return rc;
    PullArgs a{};
    a.own = Q; a.ld_own = (uint32_t)ld_q; a.gat = K; a.ld_gat = (uint32_t)ld_k; a.gat2 = V; a.ld_gat2 = (uint32_t)ld_v; a.lse = lse;
    a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.out = out; a.ld_out = (uint32_t)ld_out;
    a.scale = scale; a.P = num_parts; a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim;
    a.xcd_remap = tune.xcd_remap != 0 ? 1 : 0;
    set_drop(&a, attn_drop, rng_seed);
    rc = launch_pull<SIDE_FWD>(ds, stream, a, partSize);
    if (rc != GNNA_OK) return rc;
    return relu_epilogue(what, ds, stream, flags, out, num_out_rows, (int)W, ld_out);
}

// The destination-side pass walks the structure (num_out_rows rows, ids < num_in_rows), the source-side pass the transposed one
// (num_in_rows rows, ids < num_out_rows).
int gnna_dot_attn_backward_f32(const float *Q, int64_t ld_q, const float *K, int64_t ld_k, const float *V, int64_t ld_v,
                               const float *lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
                               const int32_t *row_pointers, const int32_t *column_index, const int32_t *part_pointers,
                               const int32_t *part2Node, int64_t num_parts, const int32_t *t_row_pointers,
                               const int32_t *t_column_index, const int32_t *t_part_pointers, const int32_t *t_part2Node,
                               int64_t t_num_parts, float scale, float attn_drop, uint64_t rng_seed, float *dQ, int64_t ld_dq,
                               float *dK, int64_t ld_dk, float *dV, int64_t ld_dv, int64_t num_out_rows, int64_t num_in_rows,
                               int heads, int dim, int partSize, unsigned flags, void *stream_v)
{
    (void)row_pointers;     // both passes walk the neighbor-groups
    (void)t_row_pointers;
    const char *what = "gnna_dot_attn_backward_f32";
    int rc = check_common(what, true, num_out_rows, num_in_rows, heads, dim, num_parts, partSize, flags, GNNA_ACCUMULATE);
    if (rc == GNNA_OK) rc = check_drop(what, attn_drop);
    if (rc == GNNA_OK) rc = check_scale(what, scale);
    if (rc != GNNA_OK) return rc;
    if (t_num_parts < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (t_num_parts=%lld)", what, (long long)t_num_parts);
    const int64_t W = (int64_t)heads * dim;
    const bool one_side = num_out_rows == 0 || num_in_rows == 0;      // no edge can exist: every output is 0
    if (one_side) {
        if (num_in_rows > 0 && (bad_ld(ld_dk, W) || bad_ld(ld_dv, W) || !dK || !dV))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dK / dV: null pointer or a row stride outside [heads * dim, 2^29)", what);
        if (num_out_rows > 0 && (bad_ld(ld_dq, W) || !dQ))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dQ: null pointer or a row stride outside [heads * dim, 2^29)", what);
    } else {
        if (bad_ld(ld_q, W) || bad_ld(ld_k, W) || bad_ld(ld_v, W) || bad_ld(ld_y, W) || bad_ld(ld_dy, W) || bad_ld(ld_dq, W) ||
            bad_ld(ld_dk, W) || bad_ld(ld_dv, W))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= heads * dim and < 2^29 floats (ld_q=%lld ld_k=%lld "
                        "ld_v=%lld ld_y=%lld ld_dy=%lld ld_dq=%lld ld_dk=%lld ld_dv=%lld)", what, (long long)ld_q, (long long)ld_k,
                        (long long)ld_v, (long long)ld_y, (long long)ld_dy, (long long)ld_dq, (long long)ld_dk, (long long)ld_dv);
        if (!Q || !K || !V || !lse || !Y || !dY || !dQ || !dK || !dV) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        if ((num_parts > 0 && (!column_index || !part_pointers || !part2Node)) ||
            (t_num_parts > 0 && (!t_column_index || !t_part_pointers || !t_part2Node)))
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    }
    // (with no row on one side the inputs are not read, but an output that is an input is still refused)
    const void *const ins[] = {Q, K, V, lse, Y, dY}, *const outs[] = {dQ, dK, dV};
    rc = check_alias(what, ins, outs);
    if (rc != GNNA_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, dQ, num_out_rows, (int)W, ld_dq);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, dK, num_in_rows, (int)W, ld_dk);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, dV, num_in_rows, (int)W, ld_dv);
    if (rc != GNNA_OK || one_side || (num_parts == 0 && t_num_parts == 0)) return rc;
    PullArgs a{};
    rc = launch_lse_c_pack<kSlotDotPack>(what, ds, stream, dY, ld_dy, Y, ld_y, lse, num_out_rows, heads, dim, &a.pack);
    if (rc != GNNA_OK) return rc;
    a.scale = scale; a.heads = heads; a.dim = dim;
    a.xcd_remap = xcd_remap_on();
    set_drop(&a, attn_drop, rng_seed);
    // destination side: row i (Q[i], dY[i], pack[i]) pulls K[j], V[j] -> dQ
    a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows;
    a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.P = num_parts;
    a.own = Q; a.ld_own = (uint32_t)ld_q; a.own2 = dY; a.ld_own2 = (uint32_t)ld_dy;
    a.gat = K; a.ld_gat = (uint32_t)ld_k; a.gat2 = V; a.ld_gat2 = (uint32_t)ld_v;
    a.out = dQ; a.ld_out = (uint32_t)ld_dq;
    rc = launch_pull<SIDE_BWD_DST>(ds, stream, a, partSize);
    if (rc != GNNA_OK) return rc;
    // source side: row j (K[j], V[j]) pulls Q[i], dY[i], (lse, c)[i] -> dK, dV -- over the edges j -> i, the rows of the
    // transposed structure
    a.N = (uint32_t)num_in_rows; a.M = (uint32_t)num_out_rows;
    a.col = t_column_index; a.pp = t_part_pointers; a.p2n = t_part2Node; a.P = t_num_parts;
    a.own = K; a.ld_own = (uint32_t)ld_k; a.own2 = V; a.ld_own2 = (uint32_t)ld_v;
    a.gat = Q; a.ld_gat = (uint32_t)ld_q; a.gat2 = dY; a.ld_gat2 = (uint32_t)ld_dy;
    a.out = dK; a.ld_out = (uint32_t)ld_dk; a.out2 = dV; a.ld_out2 = (uint32_t)ld_dv;
    return launch_pull<SIDE_BWD_SRC>(ds, stream, a, partSize);
}

#pragma GCC visibility pop
}  // extern "C"

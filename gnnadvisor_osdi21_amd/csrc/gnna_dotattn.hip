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
//   forward   (a) dot_lse_kernel: rows of the CSR, one wavefront per row (the whole block for long rows, after the short ones);
//                 64 / LPR edges per wave-wide load, four loads per step, online (max, sum) per head and slot.  The slots, then
//                 the waves, meet in a fixed order; one writer per (row, head), plain stores: the same bits on every run.
//             (b) dot_pull_kernel<SIDE_FWD>: out[i] = sum_e alpha * k * V[col(e)] over the neighbor-groups; gathers K[j] and V[j].
//             A one-pass online softmax is out of scope here, see DESIGN 7l.
//   backward  dot_pack_kernel: (lse, c = <dY[i, h, :], Y[i, h, :]>) per (row, head), 8 bytes, in library scratch;
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

struct LseArgs {
    const float *q; size_t ld_q;          // by row (< N)
    const float *k; size_t ld_k;          // by id (< M)
    const int32_t *rp, *col;
    float *lse;
    int64_t N;
    uint32_t M;
    int heads, dim;
    float scale;
};

// The edges [beg, end) of `row` swept by `nl` slots of LPR lanes (this one: slot t), four edges per slot and step, for the heads
// of the column block at hb0.  Every lane of a wavefront makes the same number of steps (the folds are wave-wide).
template <int LOG_LPH, int LOG_LPR>
__device__ __forceinline__ MaxSum lse_sweep(const LseArgs &p, int64_t row, int64_t beg, int64_t end, int t, int nl, int hb0, int cl)
{
    constexpr int LPH = 1 << LOG_LPH;
    const int h = hb0 + (cl >> LOG_LPH), fl = (cl & (LPH - 1)) * 4;
    const int n4 = h < p.heads ? p.dim - fl : 0;
    const bool ok = n4 > 0;
    const size_t colf = (size_t)(ok ? h : 0) * p.dim + (ok ? fl : 0);
    VT qv = (VT)(0.f);
    if (ok) qv = load_piece(p.q + (size_t)row * p.ld_q + colf, n4);
    MaxSum acc{-INFINITY, 0.f};
    for (int64_t base = beg; base < end; base += (int64_t)nl * 4) {
        int id[4];
        VT v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t ee = base + t + (int64_t)k * nl;
            id[k] = ee < end ? p.col[ee] : -1;
            if ((uint32_t)id[k] >= p.M) id[k] = -1;                // an id outside the source rows is skipped, in every pass alike
            v[k] = (VT)(0.f);
            if (id[k] >= 0 && ok) v[k] = load_piece(p.k + (size_t)(uint32_t)id[k] * p.ld_k + colf, n4);
        }
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float z = p.scale * head_sum<LPH>(dot_part(qv, v[k]));
            x[k] = id[k] >= 0 ? z : -INFINITY;
        }
        acc = ms_add4(acc, x);
    }
    // the 64 / LPR slots of the wavefront meet (lanes that share lane % LPR), in a fixed order
#pragma unroll
    for (int d = kWave >> 1; d >= (1 << LOG_LPR); d >>= 1) acc = ms_merge(acc, MaxSum{__shfl_xor(acc.m, d), __shfl_xor(acc.l, d)});
    return acc;
}

// One wavefront per row; N rows (Q, lse), ids < M (K).
template <int LOG_LPH, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
dot_lse_kernel(const LseArgs p)
{
    constexpr int LPH = 1 << LOG_LPH, LPR = 1 << LOG_LPR, HB = LPR / LPH, R = kWave / LPR;
    __shared__ int s_long[kWavesPerBlock];
    __shared__ int s_nlong;
    __shared__ float s_red[2][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH;
    const bool writer = sub == 0 && (cl & (LPH - 1)) == 0;          // the first lane of a head in the first slot
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * kWavesPerBlock;
    const int64_t row = r0 + wib;
    int64_t beg = 0, end = 0;
    if (row < p.N) { beg = p.rp[row]; end = p.rp[row + 1]; }
    const bool is_long = end - beg > R * 4 * kLongIters;
    if (is_long && lane == 0) s_long[atomicAdd(&s_nlong, 1)] = wib;
    // short rows (and rows without edges: lse = 0): the wavefront
    if (row < p.N && !is_long) {
        for (int hb0 = 0; hb0 < p.heads; hb0 += HB) {
            const MaxSum v = lse_sweep<LOG_LPH, LOG_LPR>(p, row, beg, end, sub, R, hb0, cl);
            if (writer && hb0 + hl < p.heads) p.lse[(size_t)row * p.heads + hb0 + hl] = lse_of(v);
        }
    }
    __syncthreads();
    // long rows: the whole block, one after the other (the list's order may vary; a row's result does not depend on it)
    const int nlong = s_nlong;
    for (int q = 0; q < nlong; q++) {
        const int64_t rr = r0 + s_long[q];
        const int64_t lb = p.rp[rr], le = p.rp[rr + 1];
        for (int hb0 = 0; hb0 < p.heads; hb0 += HB) {
            const MaxSum v = lse_sweep<LOG_LPH, LOG_LPR>(p, rr, lb, le, wib * R + sub, kWavesPerBlock * R, hb0, cl);
            __syncthreads();
            if (sub == 0) { s_red[0][wib][cl] = v.m; s_red[1][wib][cl] = v.l; }
            __syncthreads();
            MaxSum r{s_red[0][0][cl], s_red[1][0][cl]};
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; w++) r = ms_merge(r, MaxSum{s_red[0][w][cl], s_red[1][w][cl]});
            if (wib == 0 && writer && hb0 + hl < p.heads) p.lse[(size_t)rr * p.heads + hb0 + hl] = lse_of(r);
        }
    }
}

// ---- c[i, h] = <dY[i, h, :], Y[i, h, :]>, packed with lse -----------------------------------------------------------------

__global__ void __launch_bounds__(kBlock)
dot_pack_kernel(const float *__restrict__ G, size_t ldg, const float *__restrict__ Y, size_t ldy, const float *__restrict__ lse,
                float2 *__restrict__ pack, size_t N, int heads, int dim)
{
    const size_t n = N * (size_t)heads;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (unsigned)heads, h = i - r * (unsigned)heads;
        const float *g = G + r * ldg + h * (size_t)dim, *y = Y + r * ldy + h * (size_t)dim;
        float c = 0.f;
        for (int f = 0; f < dim; f++) c = __builtin_fmaf(g[f], y[f], c);
        pack[i] = make_float2(lse[i], c);
    }
}

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
    const int wib = threadIdx.x >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    const int hl = cl >> LOG_LPH, fl = (cl & (LPH - 1)) * 4;
    // consecutive chunks on one XCD (workgroups go round the 8 XCDs): neighbouring rows share source rows in that L2
    uint32_t vb = blockIdx.x;
    if (p.xcd_remap) {
        const uint32_t nb = gridDim.x, q = nb / kXcds, rem = nb % kXcds, x = vb % kXcds, i = vb / kXcds;
        vb = x < rem ? x * (q + 1) + i : rem * (q + 1) + (x - rem) * q + i;
    }
    const int64_t chunk = (int64_t)vb * kWavesPerBlock + wib;
    const int64_t g0 = chunk * p.G;
    if (g0 >= p.P) return;
    const int cnt = (int)(p.P - g0 < (int64_t)p.G ? p.P - g0 : (int64_t)p.G);
    int s = 0, e = 0, r = -1;
    if (lane < cnt) {
        s = p.pp[g0 + lane];
        e = p.pp[g0 + lane + 1];
        r = p.p2n[g0 + lane];
    }
    // a group without edges, with a negative range or with a row outside its side's rows contributes nothing and ends the run
    const bool bad = lane >= cnt || e <= s || s < 0 || (uint32_t)r >= p.N;
    const int prev_r = __shfl_up(r, 1);
    const int prev_bad = __shfl_up((int)bad, 1);
    const bool first = lane == 0 || bad || prev_bad != 0 || r != prev_r;
    unsigned long long starts = __ballot(first);
    if (cnt < kWave) starts &= (1ull << cnt) - 1ull;
    const int bad_i = bad ? 1 : 0;
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
        if (__builtin_amdgcn_readlane(bad_i, a)) continue;      // a run that contributes nothing
        const int rs = __builtin_amdgcn_readlane(s, a);
        const int re = __builtin_amdgcn_readlane(e, b - 1);
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(r, a);
        if (re <= rs) continue;
        for (int hb0 = 0; hb0 < heads; hb0 += HB) run_block(hb0, rs, re, row);
    }
}

template <int SIDE, bool DROP>
int launch_pull_drop(DeviceState *ds, hipStream_t stream, PullArgs a, int partSize)
{
    if (a.P <= 0) return GNNA_OK;
    const int log_lph = log2_lanes(a.dim, 4);                  // (dim <= kMaxDim: never capped)
    int log_lpr = log_lph;
    while (log_lpr < 6 && (1 << (log_lpr - log_lph)) < a.heads) log_lpr++;
    const ChunkGrid cg = chunk_grid(a.P, partSize, ds->num_cus);
    a.G = cg.G;
    if (cg.blocks > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "dot-product attention: %lld neighbor-groups in one call", (long long)a.P);
    const dim3 grid((unsigned)cg.blocks);
    dispatch_lpr(log_lph, [&](auto H) {
        dispatch_lpr(log_lpr, [&](auto L) {
            constexpr int LOG_LPH = decltype(H)::value, LOG_LPR = decltype(L)::value;
            if constexpr (LOG_LPR >= LOG_LPH)      // (a row has at least the lanes of one head)
                hipLaunchKernelGGL((dot_pull_kernel<SIDE, LOG_LPH, LOG_LPR, DROP>), grid, dim3(kBlock), 0, stream, a);
        });
    });
    return launch_ok("dot-product attention launch");
}

// attn_drop = 0 keeps every edge with k = 1: the call runs the instances without the mask
template <int SIDE>
int launch_pull(DeviceState *ds, hipStream_t stream, const PullArgs &a, int partSize)
{
    return a.drop_thr ? launch_pull_drop<SIDE, true>(ds, stream, a, partSize) : launch_pull_drop<SIDE, false>(ds, stream, a, partSize);
}

int launch_lse(hipStream_t stream, const LseArgs &a)
{
    const int log_lph = log2_lanes(a.dim, 4);
    int log_lpr = log_lph;
    while (log_lpr < 6 && (1 << (log_lpr - log_lph)) < a.heads) log_lpr++;
    const dim3 grid((unsigned)((a.N + kWavesPerBlock - 1) / kWavesPerBlock));      // (N < 2^29)
    dispatch_lpr(log_lph, [&](auto H) {
        dispatch_lpr(log_lpr, [&](auto L) {
            constexpr int LOG_LPH = decltype(H)::value, LOG_LPR = decltype(L)::value;
            if constexpr (LOG_LPR >= LOG_LPH)
                hipLaunchKernelGGL((dot_lse_kernel<LOG_LPH, LOG_LPR>), grid, dim3(kBlock), 0, stream, a);
        });
    });
    return launch_ok("dot-product attention lse launch");
}

void set_drop(PullArgs *a, float attn_drop, uint64_t rng_seed)
{
    a->rng_seed = rng_seed;
    a->drop_thr = drop_threshold(attn_drop);
    a->keep_scale = drop_keep_scale(attn_drop);
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
    gnna_tuning tune;
    gnna_get_tuning(&tune);
    apply_graph_hints(column_index, (int)W, &tune);
    LseArgs l{};
    l.q = Q; l.ld_q = (size_t)ld_q; l.k = K; l.ld_k = (size_t)ld_k; l.rp = row_pointers; l.col = column_index;
    l.lse = lse; l.N = num_out_rows; l.M = (uint32_t)num_in_rows; l.heads = heads; l.dim = dim; l.scale = scale;
    rc = launch_lse(stream, l);
    if (rc != GNNA_OK) return rc;
    PullArgs a{};
    a.own = Q; a.ld_own = (uint32_t)ld_q; a.gat = K; a.ld_gat = (uint32_t)ld_k; a.gat2 = V; a.ld_gat2 = (uint32_t)ld_v; a.lse = lse;
    a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.out = out; a.ld_out = (uint32_t)ld_out;
    a.scale = scale; a.P = num_parts; a.N = (uint32_t)num_out_rows; a.M = (uint32_t)num_in_rows; a.heads = heads; a.dim = dim;
    a.xcd_remap = tune.xcd_remap != 0 ? 1 : 0;                // (this tune went through apply_graph_hints: not xcd_remap_on())
    set_drop(&a, attn_drop, rng_seed);
    rc = launch_pull<SIDE_FWD>(ds, stream, a, partSize);
    if (rc != GNNA_OK) return rc;
    if (flags & GNNA_EPILOGUE_RELU) {
        launch_relu_rows(ds, stream, out, num_out_rows, (int)W, ld_out);
        return launch_ok("%s: epilogue launch", what);
    }
    return GNNA_OK;
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
    const void *ins[] = {Q, K, V, lse, Y, dY};
    const void *outs[] = {dQ, dK, dV};
    for (const void *o : outs)
        for (const void *i : ins)
            if (o && o == i) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input", what);
    if ((dQ && (dQ == dK || dQ == dV)) || (dK && dK == dV))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: the outputs must not alias each other", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, dQ, num_out_rows, (int)W, ld_dq);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, dK, num_in_rows, (int)W, ld_dk);
    if (rc == GNNA_OK) rc = launch_zero_fill(ds, stream, dV, num_in_rows, (int)W, ld_dv);
    if (rc != GNNA_OK || one_side || (num_parts == 0 && t_num_parts == 0)) return rc;
    void *ws = nullptr;
    rc = get_workspace(ds, stream, kSlotDotPack, ((size_t)num_out_rows * heads * sizeof(float2) + 255) & ~(size_t)255, &ws);
    if (rc != GNNA_OK) return rc;
    float2 *pack = static_cast<float2 *>(ws);
    hipLaunchKernelGGL(dot_pack_kernel, dim3(elementwise_grid(num_out_rows * heads, ds->num_cus, 8)), dim3(kBlock), 0, stream, dY,
                       (size_t)ld_dy, Y, (size_t)ld_y, lse, pack, (size_t)num_out_rows, heads, dim);
    rc = launch_ok("%s: pack launch", what);
    if (rc != GNNA_OK) return rc;
    PullArgs a{};
    a.pack = pack; a.scale = scale; a.heads = heads; a.dim = dim;
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

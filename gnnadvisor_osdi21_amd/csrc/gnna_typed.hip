// gnna_typed.hip -- relation-typed aggregation for R-GCN in basis form (gnna_agg_typed_expand_ld_f32,
// gnna_agg_typed_contract_ld_f32, gnna_typed_coef_grad_ld_f32).  CDNA4 / gfx950 only.  No counterpart in the reference (it has
// no relational layer).
//
// Every edge position e (indexed like column_index) carries a type t[e] in [0, R) and an optional factor n[e]; C is a small
// coefficient table [R, B].  The weight of an edge for basis b, n[e] * C[t[e], b], is made where the edge's row is gathered, so
// no buffer of the size of the edge list exists anywhere:
//
//   expand     T[i, b dim + f]  = sum_{e in row i} n[e] C[t[e], b] X[col(e), f]             one gather of X[col(e)] feeds B accumulators
//   contract   out[i, f]        = sum_{e in row i} n[e] sum_b C[t[e], b] G[col(e), b dim + f]   (the backward of expand, over A^T)
//   coef grad  dC[r, b]         = sum_{e: t[e] = r} n[e] <X[col(e), :], G[row(e), b dim : (b + 1) dim]>
//
// All three walk the neighbor-groups the way gat_pull_kernel does: a wavefront takes G consecutive groups, merges the groups of one
// destination row into a run of edges and walks the run 64 edges at a time -- one coalesced load of 64 ids, 64 types and 64
// factors, then wave-wide loads of 16 bytes per lane that bring 64 / LPR whole rows each (LPR = next_pow2(ceil(dim / 4)) <= 64
// lanes per row; rows wider than 256 floats are taken in column blocks inside the call; dim % 4 != 0: the last lane of a row
// loads its 1..3 floats one by one).  The type of an edge is the same in the LPR lanes that work on it, and so is its row of C.
// At the end of a run the 64 / LPR partial rows meet by a butterfly and are ADDED with float atomics (correct for every partition
// gnna_agg_ld_f32 accepts, no validation pass), so the outputs are zero-filled first and there is no deterministic schedule.
//
// The table: C (expand, contract) or the partial sums of dC (coef grad) live in LDS, rows padded to the kernel's stride BS (the
// bases rounded up to 1, 2, 4, 8, 16 where they index registers; to a multiple of 4 in the contract kernel), while
// num_types * BS <= kTypedLdsCells = 4096 cells (16 KiB).  Beyond that C is read from global memory (it stays in L2) and the
// partial sums of dC go straight to dcoef with global float atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gnna.h"
#include "gnna_device.h"
#include "gnna_internal.h"

namespace gnna {
namespace {

typedef VecOf<4>::T VT;
typedef VecOf<4>::M MT;

constexpr int kTypedLdsCells = 4096;   // floats of the per-block LDS table (_lib.TYPED_LDS_CELLS mirrors it)
constexpr int kMaxBases = 16;

struct TypedArgs {
    const float *src; size_t ld_src;      // the gathered rows: X (expand, coef grad), G (contract)
    const float *own; size_t ld_own;      // coef grad: G, the B blocks of the destination row itself
    const int32_t *col, *ety;             // per edge: source row, type
    const float *enorm;                   // per edge: factor, or null (1)
    const float *coef;                    // [R, B]
    const int32_t *pp, *p2n;
    float *out; size_t ld_out;            // T (expand), out (contract): zero-filled, added to; dcoef [R, B] (coef grad)
    int64_t P;
    uint32_t n_in, n_out;                 // rows gathered from, rows of the structure
    int R, B, BS, dim, G, xcd_remap, lds; // BS: row stride of the LDS table; lds: the table is in LDS
};

// the first n4 (<= 4) floats at p, the others 0
__device__ __forceinline__ VT load_piece(const float *__restrict__ p, int n4)
{
    if (n4 >= 4) return *reinterpret_cast<const MT *>(p);
    VT v = (VT)(0.f);
    if (n4 > 0) v[0] = p[0];
    if (n4 > 1) v[1] = p[1];
    if (n4 > 2) v[2] = p[2];
    return v;
}

// sum over the LPR consecutive lanes of a row; result in every lane of the row
template <int LPR>
__device__ __forceinline__ float row_sum(float v)
{
    if constexpr (LPR == 1) return v;
    else if constexpr (LPR == 2) return v + dpp_move<0xB1>(v);      // quad_perm [1,0,3,2]
    else return lane_group_sum<LPR>(v);
}

// sum over the 64 / LPR lanes that share lane % LPR (the partial rows of a wavefront); result in every lane
template <int LPR>
__device__ __forceinline__ float slots_sum(float v)
{
    v = slot_reduce<LPR>(v);                                        // strides 32 .. 4
    if constexpr (LPR <= 2) v += dpp_move<0x4E>(v);                 // quad_perm [2,3,0,1]: stride 2
    if constexpr (LPR <= 1) v += dpp_move<0xB1>(v);                 // quad_perm [1,0,3,2]: stride 1
    return v;
}

// this wavefront's chunk of G neighbor-groups; consecutive chunks on one XCD (workgroups go round the 8 XCDs): neighbouring
// rows share source rows in that L2
__device__ __forceinline__ int64_t chunk_of(const TypedArgs &p)
{
    uint32_t vb = blockIdx.x;
    if (p.xcd_remap) {
        const uint32_t nb = gridDim.x, q = nb / kXcds, rem = nb % kXcds, x = vb % kXcds, i = vb / kXcds;
        vb = x < rem ? x * (q + 1) + i : rem * (q + 1) + (x - rem) * q + i;
    }
    return (int64_t)vb * kWavesPerBlock + (threadIdx.x >> 6);
}

// body(first edge, end edge, row) for every run of the chunk: the groups of one destination row that follow each other
template <class F>
__device__ __forceinline__ void for_each_run(const TypedArgs &p, int64_t chunk, int lane, F &&body)
{
    const int64_t g0 = chunk * p.G;
    if (g0 >= p.P) return;
    const int cnt = (int)(p.P - g0 < (int64_t)p.G ? p.P - g0 : (int64_t)p.G);
    int s = 0, e = 0, r = -1;
    if (lane < cnt) {
        s = p.pp[g0 + lane];
        e = p.pp[g0 + lane + 1];
        r = p.p2n[g0 + lane];
    }
    // a group without edges, with a negative range or with a row outside the output contributes nothing and ends the run
    const bool bad = lane >= cnt || e <= s || s < 0 || (uint32_t)r >= p.n_out;
    const int prev_r = __shfl_up(r, 1);
    const int prev_bad = __shfl_up((int)bad, 1);
    const bool first = lane == 0 || bad || prev_bad != 0 || r != prev_r;
    unsigned long long starts = __ballot(first);
    if (cnt < kWave) starts &= (1ull << cnt) - 1ull;
    const int bad_i = bad ? 1 : 0;
    while (starts) {
        const int a = __builtin_ctzll(starts);
        starts &= starts - 1ull;
        const int b = starts ? __builtin_ctzll(starts) : cnt;
        if (__builtin_amdgcn_readlane(bad_i, a)) continue;
        const int rs = __builtin_amdgcn_readlane(s, a);
        const int re = __builtin_amdgcn_readlane(e, b - 1);
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(r, a);
        if (re <= rs) continue;
        body(rs, re, row);
    }
}

// 64 edges of a run from e0 on: source row (-1: the edge counts for nothing), type, factor -- one coalesced load each.
// An id outside [0, n_in) or a type outside [0, R) skips the edge, in all three kernels alike.
__device__ __forceinline__ void load_edges(const TypedArgs &p, int e0, int nb, int lane, int &id, int &ty, float &nr)
{
    id = -1; ty = 0; nr = 0.f;
    if (lane < nb) {
        const int64_t e = (int64_t)e0 + lane;
        id = p.col[e];
        ty = p.ety[e];
        nr = p.enorm ? p.enorm[e] : 1.f;
        if ((uint32_t)id >= p.n_in || (uint32_t)ty >= (uint32_t)p.R) { id = -1; ty = 0; nr = 0.f; }
    }
}

// C into the block's LDS table, rows padded with zeros to BS
__device__ __forceinline__ void stage_coef(const TypedArgs &p, float *tab)
{
    const int n = p.R * p.BS;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const int r = i / p.BS, b = i - r * p.BS;
        tab[i] = b < p.B ? p.coef[(size_t)r * p.B + b] : 0.f;
    }
}

// ---- expand ---------------------------------------------------------------------------------------------------------------
// BT: accumulators per lane (bases rounded up); the table's stride is BT.
template <int BT, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
typed_expand_kernel(const TypedArgs p)
{
    extern __shared__ float s_tab[];
    constexpr int LPR = 1 << LOG_LPR;             // lanes per row (of a column block)
    constexpr int R = kWave / LPR;                // rows per wave-wide load
    constexpr int UMAX = BT >= 16 ? 4 : 8;
    constexpr int U = LPR < UMAX ? LPR : UMAX;    // row loads in flight per lane
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (p.lds) {
        stage_coef(p, s_tab);
        __syncthreads();
    }
    for_each_run(p, chunk_of(p), lane, [&](int rs, int re, uint32_t row) {
        for (int cb0 = 0; cb0 < p.dim; cb0 += LPR * 4) {
            const int fl = cb0 + cl * 4;
            const int n4 = p.dim - fl;                // floats of this lane's piece (<= 0: the lane idles)
            const bool ok = n4 > 0;
            const size_t colf = ok ? (size_t)fl : 0;
            VT acc[BT];
#pragma unroll
            for (int b = 0; b < BT; b++) acc[b] = (VT)(0.f);
            for (int e0 = rs; e0 < re; e0 += kWave) {
                const int nb = re - e0 < kWave ? re - e0 : kWave;
                int id, ty;
                float nr;
                load_edges(p, e0, nb, lane, id, ty, nr);
                for (int u0 = 0; u0 < LPR; u0 += U) {
                    if (u0 * R >= nb) break;
                    VT v[U];
                    int tj[U];
                    float w[U];
                    bool live[U];
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const int from = (u0 + k) * R + sub;
                        const int idj = __shfl(id, from);
                        tj[k] = __shfl(ty, from);
                        w[k] = __shfl(nr, from);
                        live[k] = idj >= 0 && ok;
                        v[k] = (VT)(0.f);
                        if (live[k]) v[k] = load_piece(p.src + (size_t)(uint32_t)idj * p.ld_src + colf, n4);
                        else w[k] = 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        // (a slot without an edge takes c = 0, not row 0 of C: whatever that row holds, it adds nothing)
                        float c[BT];
                        if (p.lds) {
#pragma unroll
                            for (int b = 0; b < BT; b++) c[b] = live[k] ? s_tab[tj[k] * BT + b] : 0.f;
                        } else {
#pragma unroll
                            for (int b = 0; b < BT; b++) c[b] = live[k] && b < p.B ? p.coef[(size_t)tj[k] * p.B + b] : 0.f;
                        }
                        const VT wv = v[k] * w[k];
#pragma unroll
                        for (int b = 0; b < BT; b++) {
#pragma unroll
                            for (int q = 0; q < 4; q++) acc[b][q] = __builtin_fmaf(c[b], wv[q], acc[b][q]);
                        }
                    }
                }
            }
            // the R partial rows of the wavefront meet; the first slot adds them to the output
#pragma unroll
            for (int b = 0; b < BT; b++) {
                if (b < p.B) {
                    VT t;
#pragma unroll
                    for (int q = 0; q < 4; q++) t[q] = slots_sum<LPR>(acc[b][q]);
                    if (sub == 0 && ok) {
                        float *dst = p.out + (size_t)row * p.ld_out + (size_t)b * p.dim + colf;
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if (q < n4) atomicAdd(dst + q, t[q]);
                    }
                }
            }
        }
    });
}

// ---- contract -------------------------------------------------------------------------------------------------------------
// The gathered row is B * dim wide: a lane loads its piece of four blocks of U rows before the first add.
template <int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
typed_contract_kernel(const TypedArgs p)
{
    extern __shared__ float s_tab[];
    constexpr int LPR = 1 << LOG_LPR;
    constexpr int R = kWave / LPR;
    constexpr int U = LPR < 4 ? LPR : 4;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (p.lds) {
        stage_coef(p, s_tab);
        __syncthreads();
    }
    for_each_run(p, chunk_of(p), lane, [&](int rs, int re, uint32_t row) {
        for (int cb0 = 0; cb0 < p.dim; cb0 += LPR * 4) {
            const int fl = cb0 + cl * 4;
            const int n4 = p.dim - fl;
            const bool ok = n4 > 0;
            const size_t colf = ok ? (size_t)fl : 0;
            VT acc = (VT)(0.f);
            for (int e0 = rs; e0 < re; e0 += kWave) {
                const int nb = re - e0 < kWave ? re - e0 : kWave;
                int id, ty;
                float nr;
                load_edges(p, e0, nb, lane, id, ty, nr);
                for (int u0 = 0; u0 < LPR; u0 += U) {
                    if (u0 * R >= nb) break;
                    int idj[U], tj[U];
                    float w[U];
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const int from = (u0 + k) * R + sub;
                        idj[k] = __shfl(id, from);
                        tj[k] = __shfl(ty, from);
                        w[k] = __shfl(nr, from);
                        if (!ok) idj[k] = -1;
                        if (idj[k] < 0) w[k] = 0.f;
                    }
                    for (int b0 = 0; b0 < p.B; b0 += 4) {
                        VT v[U][4];
#pragma unroll
                        for (int k = 0; k < U; k++) {
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                v[k][j] = (VT)(0.f);
                                if (idj[k] >= 0 && b0 + j < p.B)
                                    v[k][j] = load_piece(p.src + (size_t)(uint32_t)idj[k] * p.ld_src + (size_t)(b0 + j) * p.dim + colf, n4);
                            }
                        }
#pragma unroll
                        for (int k = 0; k < U; k++) {
                            float c[4];
                            if (p.lds) {
#pragma unroll
                                for (int j = 0; j < 4; j++) c[j] = idj[k] >= 0 ? s_tab[tj[k] * p.BS + b0 + j] : 0.f;   // (BS: a multiple of 4)
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; j++)
                                    c[j] = idj[k] >= 0 && b0 + j < p.B ? p.coef[(size_t)tj[k] * p.B + b0 + j] : 0.f;
                            }
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const float cw = c[j] * w[k];
#pragma unroll
                                for (int q = 0; q < 4; q++) acc[q] = __builtin_fmaf(cw, v[k][j][q], acc[q]);
                            }
                        }
                    }
                }
            }
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
    });
}

// ---- coef grad ------------------------------------------------------------------------------------------------------------
// Within a run the B blocks of G[row] stay in registers (BT pieces per lane); every gathered X row gives B dot products, summed
// over the LPR lanes of the row (DPP) and added by the row's first lane to cell (type, b) of the block's LDS table -- or, when
// the table does not fit, to dcoef itself.  The block adds every non-zero cell of its table to dcoef once.
template <int BT, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
typed_coef_grad_kernel(const TypedArgs p)
{
    extern __shared__ float s_tab[];
    constexpr int LPR = 1 << LOG_LPR;
    constexpr int R = kWave / LPR;
    constexpr int UMAX = BT >= 16 ? 4 : 8;
    constexpr int U = LPR < UMAX ? LPR : UMAX;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (p.lds) {
        for (int i = threadIdx.x; i < p.R * BT; i += kBlock) s_tab[i] = 0.f;
        __syncthreads();
    }
    for_each_run(p, chunk_of(p), lane, [&](int rs, int re, uint32_t row) {
        for (int cb0 = 0; cb0 < p.dim; cb0 += LPR * 4) {
            const int fl = cb0 + cl * 4;
            const int n4 = p.dim - fl;
            const bool ok = n4 > 0;
            const size_t colf = ok ? (size_t)fl : 0;
            VT g[BT];
#pragma unroll
            for (int b = 0; b < BT; b++) {
                g[b] = (VT)(0.f);
                if (ok && b < p.B) g[b] = load_piece(p.own + (size_t)row * p.ld_own + (size_t)b * p.dim + colf, n4);
            }
            for (int e0 = rs; e0 < re; e0 += kWave) {
                const int nb = re - e0 < kWave ? re - e0 : kWave;
                int id, ty;
                float nr;
                load_edges(p, e0, nb, lane, id, ty, nr);
                for (int u0 = 0; u0 < LPR; u0 += U) {
                    if (u0 * R >= nb) break;
                    VT v[U];
                    int tj[U];
                    float w[U];
                    bool live[U];
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const int from = (u0 + k) * R + sub;
                        const int idj = __shfl(id, from);
                        tj[k] = __shfl(ty, from);
                        w[k] = __shfl(nr, from);
                        live[k] = idj >= 0;
                        v[k] = (VT)(0.f);
                        if (live[k] && ok) v[k] = load_piece(p.src + (size_t)(uint32_t)idj * p.ld_src + colf, n4);
                    }
#pragma unroll
                    for (int k = 0; k < U; k++) {
#pragma unroll
                        for (int b = 0; b < BT; b++) {
                            if (b < p.B) {
                                const float part = (v[k][0] * g[b][0] + v[k][1] * g[b][1]) + (v[k][2] * g[b][2] + v[k][3] * g[b][3]);
                                const float d = row_sum<LPR>(part) * w[k];
                                if (cl == 0 && live[k]) {
                                    if (p.lds) atomicAdd(&s_tab[tj[k] * BT + b], d);
                                    else atomicAdd(p.out + (size_t)tj[k] * p.B + b, d);
                                }
                            }
                        }
                    }
                }
            }
        }
    });
    if (p.lds) {
        __syncthreads();
        const int n = p.R * p.B;
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int r = i / p.B, b = i - r * p.B;
            const float t = s_tab[r * BT + b];
            if (t != 0.f) atomicAdd(p.out + i, t);
        }
    }
}

// ---- launch ---------------------------------------------------------------------------------------------------------------

enum { KIND_EXPAND = 0, KIND_CONTRACT = 1, KIND_COEF_GRAD = 2 };

template <int KIND, int BT>
void launch_lpr(int log_lpr, dim3 grid, size_t lds_bytes, hipStream_t stream, const TypedArgs &a)
{
    dispatch_lpr(log_lpr, [&](auto LL) {
        constexpr int L = decltype(LL)::value;
        const dim3 block(kBlock);
        if constexpr (KIND == KIND_EXPAND) hipLaunchKernelGGL((typed_expand_kernel<BT, L>), grid, block, lds_bytes, stream, a);
        else if constexpr (KIND == KIND_CONTRACT) hipLaunchKernelGGL((typed_contract_kernel<L>), grid, block, lds_bytes, stream, a);
        else hipLaunchKernelGGL((typed_coef_grad_kernel<BT, L>), grid, block, lds_bytes, stream, a);
    });
}

template <int KIND>
int launch_typed(DeviceState *ds, hipStream_t stream, TypedArgs a, int partSize, const char *what)
{
    if (a.P <= 0) return GNNA_OK;
    const int log_lpr = log2_lanes(a.dim, 4);
    int bt = 1;
    while (bt < a.B) bt <<= 1;
    a.BS = KIND == KIND_CONTRACT ? (a.B + 3) & ~3 : bt;
    a.lds = (int64_t)a.R * a.BS <= kTypedLdsCells ? 1 : 0;
    const size_t lds_bytes = a.lds ? (size_t)a.R * a.BS * sizeof(float) : 0;
    const ChunkGrid cg = chunk_grid(a.P, partSize, ds->num_cus);
    a.G = cg.G;
    if (cg.blocks > 0x7fffffffll) return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld neighbor-groups in one call", what, (long long)a.P);
    const dim3 grid((unsigned)cg.blocks);
    if constexpr (KIND == KIND_CONTRACT) {
        launch_lpr<KIND, 1>(log_lpr, grid, lds_bytes, stream, a);
    } else {
        switch (bt) {
        case 1: launch_lpr<KIND, 1>(log_lpr, grid, lds_bytes, stream, a); break;
        case 2: launch_lpr<KIND, 2>(log_lpr, grid, lds_bytes, stream, a); break;
        case 4: launch_lpr<KIND, 4>(log_lpr, grid, lds_bytes, stream, a); break;
        case 8: launch_lpr<KIND, 8>(log_lpr, grid, lds_bytes, stream, a); break;
        default: launch_lpr<KIND, 16>(log_lpr, grid, lds_bytes, stream, a); break;
        }
    }
    return launch_ok("%s launch", what);
}

// what the three entry points check alike, before any device work
int check_typed(const char *what, int64_t num_in_rows, int64_t num_out_rows, int num_types, int num_bases, int dim,
                int64_t num_parts, int partSize, unsigned flags, bool may_accumulate)
{
    if ((flags & GNNA_ACCUMULATE) && !may_accumulate) return fail(GNNA_ERR_UNSUPPORTED, "%s: GNNA_ACCUMULATE is not supported", what);
    if (flags & ~GNNA_ACCUMULATE)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: flag bits 0x%x are not accepted (GNNA_EPILOGUE_RELU among them)", what, flags);
    if (num_in_rows < 0 || num_out_rows < 0 || num_parts < 0 || num_types < 1 || num_bases < 1 || dim < 1)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (num_in_rows=%lld num_out_rows=%lld num_types=%d num_bases=%d dim=%d "
                    "num_parts=%lld)", what, (long long)num_in_rows, (long long)num_out_rows, num_types, num_bases, dim,
                    (long long)num_parts);
    if (partSize <= 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must be positive (got %d)", what, partSize);
    if (num_bases > kMaxBases) return fail(GNNA_ERR_UNSUPPORTED, "%s: at most %d bases (got %d)", what, kMaxBases, num_bases);
    if (num_in_rows >= ((int64_t)1 << 29) || num_out_rows >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld x %lld rows in one call (at most 536870911 each): shard the rows", what,
                    (long long)num_out_rows, (long long)num_in_rows);
    if ((int64_t)num_bases * dim >= ((int64_t)1 << 29) || (int64_t)num_types * kMaxBases >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: num_bases * dim and num_types * 16 must stay below 2^29 (num_types=%d num_bases=%d "
                    "dim=%d)", what, num_types, num_bases, dim);
    // the gathered rows are added with float atomics: the order of the additions is not fixed
    return deterministic_refused(what, "its sums are added with float atomics");
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_agg_typed_expand_ld_f32(const float *X, int64_t ld_x, int64_t num_in_rows, const int32_t *column_index,
                                 const int32_t *edge_type, const float *edge_norm, const float *coef, int num_types, int num_bases,
                                 const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out,
                                 int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    const char *what = "gnna_agg_typed_expand_ld_f32";
    int rc = check_typed(what, num_in_rows, num_out_rows, num_types, num_bases, dim, num_parts, partSize, flags, false);
    if (rc != GNNA_OK) return rc;
    const int64_t W = (int64_t)num_bases * dim;
    if (bad_ld(ld_x, dim) || bad_ld(ld_out, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim (X) and >= num_bases * dim (out) and < 2^29 floats "
                    "(ld_x=%lld ld_out=%lld)", what, (long long)ld_x, (long long)ld_out);
    if (!X || !coef || !out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (num_parts > 0 && (!column_index || !edge_type || !part_pointers || !part2Node))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (out == X || out == coef || (const void *)out == (const void *)edge_norm)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: the output must not alias an input", what);
    if (num_out_rows == 0) return GNNA_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, out, num_out_rows, (int)W, ld_out);
    if (rc != GNNA_OK || num_parts == 0 || num_in_rows == 0) return rc;
    TypedArgs a{};
    a.src = X; a.ld_src = (size_t)ld_x; a.col = column_index; a.ety = edge_type; a.enorm = edge_norm; a.coef = coef;
    a.pp = part_pointers; a.p2n = part2Node; a.out = out; a.ld_out = (size_t)ld_out; a.P = num_parts;
    a.n_in = (uint32_t)num_in_rows; a.n_out = (uint32_t)num_out_rows; a.R = num_types; a.B = num_bases; a.dim = dim;
    a.xcd_remap = xcd_remap_on();
    return launch_typed<KIND_EXPAND>(ds, stream, a, partSize, what);
}

int gnna_agg_typed_contract_ld_f32(const float *G, int64_t ld_g, int64_t num_in_rows, const int32_t *column_index,
                                   const int32_t *edge_type, const float *edge_norm, const float *coef, int num_types, int num_bases,
                                   const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out,
                                   int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    const char *what = "gnna_agg_typed_contract_ld_f32";
    int rc = check_typed(what, num_in_rows, num_out_rows, num_types, num_bases, dim, num_parts, partSize, flags, false);
    if (rc != GNNA_OK) return rc;
    const int64_t W = (int64_t)num_bases * dim;
    if (bad_ld(ld_g, W) || bad_ld(ld_out, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= num_bases * dim (G) and >= dim (out) and < 2^29 floats "
                    "(ld_g=%lld ld_out=%lld)", what, (long long)ld_g, (long long)ld_out);
    if (!G || !coef || !out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (num_parts > 0 && (!column_index || !edge_type || !part_pointers || !part2Node))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (out == G || out == coef || (const void *)out == (const void *)edge_norm)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: the output must not alias an input", what);
    if (num_out_rows == 0) return GNNA_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    rc = launch_zero_fill(ds, stream, out, num_out_rows, dim, ld_out);
    if (rc != GNNA_OK || num_parts == 0 || num_in_rows == 0) return rc;
    TypedArgs a{};
    a.src = G; a.ld_src = (size_t)ld_g; a.col = column_index; a.ety = edge_type; a.enorm = edge_norm; a.coef = coef;
    a.pp = part_pointers; a.p2n = part2Node; a.out = out; a.ld_out = (size_t)ld_out; a.P = num_parts;
    a.n_in = (uint32_t)num_in_rows; a.n_out = (uint32_t)num_out_rows; a.R = num_types; a.B = num_bases; a.dim = dim;
    a.xcd_remap = xcd_remap_on();
    return launch_typed<KIND_CONTRACT>(ds, stream, a, partSize, what);
}

int gnna_typed_coef_grad_ld_f32(const float *X, int64_t ld_x, int64_t num_in_rows, const float *G, int64_t ld_g,
                                int64_t num_out_rows, const int32_t *column_index, const int32_t *edge_type, const float *edge_norm,
                                const int32_t *part_pointers, const int32_t *part2Node, float *dcoef, int num_types, int num_bases,
                                int dim, int64_t num_parts, int partSize, unsigned flags, void *stream_v)
{
    const char *what = "gnna_typed_coef_grad_ld_f32";
    int rc = check_typed(what, num_in_rows, num_out_rows, num_types, num_bases, dim, num_parts, partSize, flags, true);
    if (rc != GNNA_OK) return rc;
    const int64_t W = (int64_t)num_bases * dim;
    if (bad_ld(ld_x, dim) || bad_ld(ld_g, W))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim (X) and >= num_bases * dim (G) and < 2^29 floats "
                    "(ld_x=%lld ld_g=%lld)", what, (long long)ld_x, (long long)ld_g);
    if (!X || !G || !dcoef) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (num_parts > 0 && (!column_index || !edge_type || !part_pointers || !part2Node))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (dcoef == X || dcoef == G || (const void *)dcoef == (const void *)edge_norm)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: the output must not alias an input", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    const int cells = num_types * num_bases;
    if (!(flags & GNNA_ACCUMULATE)) {
        rc = launch_zero_fill(ds, stream, dcoef, 1, cells, cells);
        if (rc != GNNA_OK) return rc;
    }
    if (num_parts == 0 || num_in_rows == 0 || num_out_rows == 0) return GNNA_OK;
    TypedArgs a{};
    a.src = X; a.ld_src = (size_t)ld_x; a.own = G; a.ld_own = (size_t)ld_g; a.col = column_index; a.ety = edge_type;
    a.enorm = edge_norm; a.pp = part_pointers; a.p2n = part2Node; a.out = dcoef; a.P = num_parts;
    a.n_in = (uint32_t)num_in_rows; a.n_out = (uint32_t)num_out_rows; a.R = num_types; a.B = num_bases; a.dim = dim;
    a.xcd_remap = xcd_remap_on();
    return launch_typed<KIND_COEF_GRAD>(ds, stream, a, partSize, what);
}

#pragma GCC visibility pop
}  // extern "C"

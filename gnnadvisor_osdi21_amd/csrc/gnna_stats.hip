// gnna_stats.hip -- sum, sum of squares, max and min over a node's neighbours, with the positions of the winning edges, from one
// walk over the ids and one load of every source row (gnna_agg_stats_ld_f32, include/gnna_stats.h).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its kernels only sum, GNNAdvisor_kernel.cu:186-259); the partition arguments are those of
// gnna_agg_ld_f32.
//
// The gather is that of reduce_kernel (gnna_reduce.hip), which is gnna_x16.hip's: a wavefront takes G consecutive
// neighbor-groups, merges the groups that follow each other in the same destination row into one run of edges and walks the run
// 64 edges at a time -- one coalesced load of 64 column ids, then LPR wave-wide row loads of 16 bytes per lane, up to 8 in
// flight, LPR = next_pow2(ceil(D / 4)) lanes per row, column blocks of 256 floats for wider rows, element-wise loads for a
// partial last vector.  What differs is what a loaded value feeds: per lane and element a running sum, a running sum of squares,
// a max key and a min key (gnna_keys.h) -- 24 registers -- so the four statistics cost one read of column_index and of X.
//   * at the end of a run the 64 / LPR partial rows of the wavefront meet across the lanes: the sums by the DPP / permlane folds
//     of the sum kernels, the keys by the butterfly of key maxima.  The lanes of the first partial row then send the row out:
//     one float atomic add per element into `sum` / `sumsq` (the caller's matrices, zero-filled by a kernel beforehand) and one
//     64-bit atomic max per element and key array (library scratch, zero-filled likewise).  Atomics for every run make the kernel
//     correct for any partition, as in the reduce kernel.
//   * stats_finish_kernel reads every key once and writes the values (0 for the key 0) and positions (-1).
// The keys are those of gnna_agg_reduce_ld_f32 and an unsigned maximum never rounds: max / argmax / min / argmin are that
// entry's bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gnna_stats.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::slots_sum
#include "gnna_internal.h"
#include "gnna_keys.h"

namespace gnna {
namespace {

struct StatsArgs {
    const float *X;             // source rows
    size_t ldx;                 // floats
    const int32_t *col, *pp, *p2n;
    float *S, *Q;               // sum / sum of squares (either may be null), zero when the kernel starts
    size_t lds, ldq;
    u64 *Kmax, *Kmin;           // [num_out_rows][D] keys (either may be null), zero when the kernel starts
    int64_t P;
    uint32_t num_in_rows, num_out_rows;
    int D, G, xcd_remap;
};

template <bool MOM, bool EXT, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
stats_kernel(const StatsArgs p)
{
    constexpr int LPR = 1 << LOG_LPR;             // lanes per row
    constexpr int R = kWave / LPR;                // rows per wave-wide load
    constexpr int U = LPR < 8 ? LPR : 8;          // row loads in flight per lane
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    // consecutive chunks on one XCD (workgroups go round the 8 XCDs): neighbouring rows share source rows in that L2
    uint32_t vb = blockIdx.x;
    if (p.xcd_remap) {
        const uint32_t nb = gridDim.x, q = nb / kXcds, rem = nb % kXcds, x = vb % kXcds, i = vb / kXcds;
        vb = x < rem ? x * (q + 1) + i : rem * (q + 1) + (x - rem) * q + i;
    }
    const int64_t chunk = (int64_t)vb * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t g0 = chunk * p.G;
    if (g0 >= p.P) return;
    const int cnt = (int)(p.P - g0 < (int64_t)p.G ? p.P - g0 : (int64_t)p.G);
    int s = 0, e = 0, r = -1;
    if (lane < cnt) {
        s = p.pp[g0 + lane];
        e = p.pp[g0 + lane + 1];
        r = p.p2n[g0 + lane];
    }
    // a group without edges, with a negative range or with a row outside the outputs contributes nothing and ends the run
    const bool bad = lane >= cnt || e <= s || s < 0 || (uint32_t)r >= p.num_out_rows;
    const int prev_r = __shfl_up(r, 1);
    const int prev_e = __shfl_up(e, 1);
    const int prev_bad = __shfl_up((int)bad, 1);
    // (a run must be one range of positions: a group that does not start where its predecessor ended starts a new one)
    const bool head = lane == 0 || bad || prev_bad != 0 || r != prev_r || s != prev_e;
    unsigned long long heads = __ballot(head);
    if (cnt < kWave) heads &= (1ull << cnt) - 1ull;
    const int bad_i = bad ? 1 : 0;

    while (heads) {
        const int a = __builtin_ctzll(heads);
        heads &= heads - 1ull;
        const int b = heads ? __builtin_ctzll(heads) : cnt;
        if (__builtin_amdgcn_readlane(bad_i, a)) continue;
        const int rs = __builtin_amdgcn_readlane(s, a);
        const int re = __builtin_amdgcn_readlane(e, b - 1);
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(r, a);
        if (re <= rs) continue;
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4;
            const bool col_ok = mycol < p.D;
            const bool whole = mycol + 4 <= p.D;
            float sum[4], sq[4];
            u64 hi[4], lo[4];                     // the running max key and min key
#pragma unroll
            for (int q = 0; q < 4; q++) {
                sum[q] = 0.f; sq[q] = 0.f;
                hi[q] = 0ull; lo[q] = 0ull;
            }
            for (int e0 = rs; e0 < re; e0 += kWave) {
                const int nb = re - e0 < kWave ? re - e0 : kWave;
                int id = -1;
                if (lane < nb) {
                    id = p.col[(int64_t)e0 + lane];
                    if ((uint32_t)id >= p.num_in_rows) id = -1;           // (an id outside the source matrix is skipped, never read)
                }
#pragma unroll
                for (int u0 = 0; u0 < LPR; u0 += U) {
                    if (u0 * R >= nb) break;
                    float v[U][4];
                    bool ok[U];
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const int j = (u0 + k) * R + sub;
                        const int idj = __shfl(id, j);
                        ok[k] = idj >= 0 && col_ok;
#pragma unroll
                        for (int q = 0; q < 4; q++) v[k][q] = 0.f;
                        if (ok[k]) {
                            const float *src = p.X + (size_t)(uint32_t)idj * p.ldx + (size_t)mycol;
                            if (whole) {
                                const f32x4u t = *reinterpret_cast<const f32x4u *>(src);
#pragma unroll
                                for (int q = 0; q < 4; q++) v[k][q] = t[q];
                            } else {
#pragma unroll
                                for (int q = 0; q < 3; q++)
                                    if (mycol + q < p.D) v[k][q] = src[q];
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        // (positions rise with k, u0 and e0: the low word falls, so among equal values the first one stays)
                        const uint32_t npos = 0xFFFFFFFFu - (uint32_t)(e0 + (u0 + k) * R + sub);
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            if constexpr (MOM) {                      // (a skipped edge holds 0 here)
                                sum[q] += v[k][q];
                                sq[q] += v[k][q] * v[k][q];
                            }
                            if constexpr (EXT) {
                                hi[q] = umax64(hi[q], ok[k] ? pack(order_of<GNNA_REDUCE_MAX>(v[k][q]), npos) : 0ull);
                                lo[q] = umax64(lo[q], ok[k] ? pack(order_of<GNNA_REDUCE_MIN>(v[k][q]), npos) : 0ull);
                            }
                        }
                    }
                }
            }
            // ---- the R partial rows of the wavefront -> one row, in every lane ---------------------------------------------
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if constexpr (MOM) {
                    sum[q] = gat::slots_sum<LPR>(sum[q]);
                    sq[q] = gat::slots_sum<LPR>(sq[q]);
                }
                if constexpr (EXT) {
                    hi[q] = partial_rows_max<R>(hi[q]);
                    lo[q] = partial_rows_max<R>(lo[q]);
                }
            }
            if (sub == 0 && col_ok) {
                const size_t at = (size_t)row * (size_t)p.D + (size_t)mycol;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool in_row = mycol + q < p.D;
                    if constexpr (MOM) {
                        if (in_row && p.S) atomicAdd(p.S + (size_t)row * p.lds + (size_t)(mycol + q), sum[q]);
                        if (in_row && p.Q) atomicAdd(p.Q + (size_t)row * p.ldq + (size_t)(mycol + q), sq[q]);
                    }
                    if constexpr (EXT) {
                        if (in_row && p.Kmax && hi[q] != 0ull) atomicMax(p.Kmax + at + q, hi[q]);
                        if (in_row && p.Kmin && lo[q] != 0ull) atomicMax(p.Kmin + at + q, lo[q]);
                    }
                }
            }
        }
    }
}

// (max_out, argmax) from Kmax and (min_out, argmin) from Kmin: the value of a key (0 when no edge reached it) and its edge position
// (-1).  A null key array stands for keys that are all 0 (a call without edges); a null output is not written.  Every element of
// the D columns of every row is written.
__global__ void __launch_bounds__(kBlock)
stats_finish_kernel(const u64 *__restrict__ Kmax, const u64 *__restrict__ Kmin, float *__restrict__ mx, size_t ld_mx,
                    int32_t *__restrict__ amx, size_t ld_amx, float *__restrict__ mn, size_t ld_mn, int32_t *__restrict__ amn,
                    size_t ld_amn, size_t rows, int D)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t n = rows * (size_t)D;
    for (size_t i = tid; i < n; i += nthreads) {
        const size_t r = i / (unsigned)D, c = i - r * (unsigned)D;
        float v;
        int32_t pos;
        if (mx) {
            key_result(Kmax ? Kmax[i] : 0ull, GNNA_REDUCE_MAX, &v, &pos);
            mx[r * ld_mx + c] = v;
            if (amx) amx[r * ld_amx + c] = pos;
        }
        if (mn) {
            key_result(Kmin ? Kmin[i] : 0ull, GNNA_REDUCE_MIN, &v, &pos);
            mn[r * ld_mn + c] = v;
            if (amn) amn[r * ld_amn + c] = pos;
        }
    }
}

template <bool MOM, bool EXT>
void launch_main(int log_lpr, dim3 grid, hipStream_t stream, const StatsArgs &a)
{
    dispatch_lpr(log_lpr, [&](auto L) {
        hipLaunchKernelGGL((stats_kernel<MOM, EXT, decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
}

// Scratch of the stats entry: slot 11 = the keys (the max keys, then the min keys).  Eager calls of a stream share it
// (grow-only), a captured call gets its capture's own.
constexpr int kSlotStatsKeys = 11;

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_agg_stats_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows, const int32_t *column_index,
                          const int32_t *part_pointers, const int32_t *part2Node, float *sum, int64_t ld_sum, float *sumsq,
                          int64_t ld_sumsq, float *max_out, int64_t ld_max, int32_t *argmax, int64_t ld_argmax, float *min_out,
                          int64_t ld_min, int32_t *argmin, int64_t ld_argmin, int64_t num_out_rows, int dim, int64_t num_parts,
                          int partSize, unsigned flags, void *stream_v)
{
    if (flags != 0u)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "gnna_agg_stats_ld_f32 takes no flags (got 0x%x): GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU "
                    "have no meaning for several statistics", flags);
    if (dim < 1) return fail(GNNA_ERR_INVALID_ARGUMENT, "dim must be >= 1 (got %d)", dim);
    if (num_out_rows < 0 || num_parts < 0 || num_in_rows < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "negative size (num_out_rows=%lld num_in_rows=%lld num_parts=%lld)",
                    (long long)num_out_rows, (long long)num_in_rows, (long long)num_parts);
    if (partSize <= 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "partSize must be positive (got %d)", partSize);
    if (num_out_rows >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%lld destination rows in one call (at most 536870911): shard the rows", (long long)num_out_rows);
    if (!sum && !sumsq && !max_out && !min_out)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "no statistic asked for: sum, sumsq, max_out and min_out are all null");
    if ((argmax && !max_out) || (argmin && !min_out))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s without %s: positions come with their values", argmax && !max_out ? "argmax" : "argmin",
                    argmax && !max_out ? "max_out" : "min_out");
    // (a null output leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld_of(sum, ld_sum, dim) || bad_ld_of(sumsq, ld_sumsq, dim) || bad_ld_of(max_out, ld_max, dim) ||
        bad_ld_of(argmax, ld_argmax, dim) || bad_ld_of(min_out, ld_min, dim) || bad_ld_of(argmin, ld_argmin, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_sum=%lld ld_sumsq=%lld "
                    "ld_max=%lld ld_argmax=%lld ld_min=%lld ld_argmin=%lld dim=%d)", (long long)ld_in, (long long)ld_sum,
                    (long long)ld_sumsq, (long long)ld_max, (long long)ld_argmax, (long long)ld_min, (long long)ld_argmin, dim);
    const void *outs[6] = {sum, sumsq, max_out, argmax, min_out, argmin};
    static const char *const names[6] = {"sum", "sumsq", "max_out", "argmax", "min_out", "argmin"};
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(input);
    for (const void *o : outs) low_bits |= reinterpret_cast<uintptr_t>(o);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "feature, statistic and arg pointers must be 4-byte aligned");
    for (int a = 0; a < 6; a++) {
        if (!outs[a]) continue;
        if (outs[a] == input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s must not alias input", names[a]);
        for (int b = a + 1; b < 6; b++)
            if (outs[a] == outs[b]) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s must not alias %s", names[b], names[a]);
    }
    const bool moments = sum || sumsq, extrema = max_out || min_out;
    if (moments) {
        // one float atomic per run and element: the order of the additions into a row is not fixed
        const int rc = deterministic_refused("gnna_agg_stats_ld_f32 with sum or sumsq", "its sums meet through float atomics");
        if (rc != GNNA_OK) return rc;
    }
    if (num_out_rows == 0) return GNNA_OK;
    const bool work = num_parts > 0 && num_in_rows > 0;
    if (work && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "null feature pointer");
    if (work && (!column_index || !part_pointers || !part2Node)) return fail(GNNA_ERR_INVALID_ARGUMENT, "null index pointer");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    int rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    const ChunkGrid cg = chunk_grid(num_parts, partSize, ds->num_cus);
    if (cg.blocks > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "neighbor statistics: %lld neighbor-groups in one call", (long long)num_parts);
    const size_t n = (size_t)num_out_rows * (size_t)dim;
    const unsigned eblocks = elementwise_grid((int64_t)n, ds->num_cus, 8);
    // (kernels, not hipMemsetAsync: a captured call then consists of kernel nodes only)
    if (sum && (rc = launch_zero_fill(ds, stream, sum, num_out_rows, dim, ld_sum)) != GNNA_OK) return rc;
    if (sumsq && (rc = launch_zero_fill(ds, stream, sumsq, num_out_rows, dim, ld_sumsq)) != GNNA_OK) return rc;
    u64 *Kmax = nullptr, *Kmin = nullptr;
    if (work && extrema) {
        const int arrays = (max_out ? 1 : 0) + (min_out ? 1 : 0);
        void *ws = nullptr;
        rc = get_workspace(ds, stream, kSlotStatsKeys, ((size_t)arrays * n * sizeof(u64) + 255) & ~(size_t)255, &ws);
        if (rc != GNNA_OK) return rc;
        u64 *K = static_cast<u64 *>(ws);
        rc = launch_zero_fill(ds, stream, reinterpret_cast<float *>(K), num_out_rows, 2 * arrays * dim, 2 * (int64_t)arrays * dim);
        if (rc != GNNA_OK) return rc;
        if (max_out) { Kmax = K; K += n; }
        if (min_out) Kmin = K;
    }
    if (work) {
        StatsArgs a;
        a.X = input; a.ldx = (size_t)ld_in; a.col = column_index; a.pp = part_pointers; a.p2n = part2Node;
        a.S = sum; a.lds = (size_t)ld_sum; a.Q = sumsq; a.ldq = (size_t)ld_sumsq; a.Kmax = Kmax; a.Kmin = Kmin;
        a.P = num_parts; a.num_in_rows = (uint32_t)std::min<int64_t>(num_in_rows, (int64_t)1 << 31);   // (ids are int32)
        a.num_out_rows = (uint32_t)num_out_rows;
        a.D = dim; a.xcd_remap = xcd_remap_on();
        a.G = cg.G;
        const int log_lpr = log2_lanes(dim, 4);
        const dim3 grid((unsigned)cg.blocks);
        if (moments && extrema) launch_main<true, true>(log_lpr, grid, stream, a);
        else if (moments) launch_main<true, false>(log_lpr, grid, stream, a);
        else launch_main<false, true>(log_lpr, grid, stream, a);
    }
    if (extrema)
        hipLaunchKernelGGL(stats_finish_kernel, dim3(eblocks), dim3(kBlock), 0, stream, Kmax, Kmin, max_out, (size_t)ld_max, argmax,
                           (size_t)ld_argmax, min_out, (size_t)ld_min, argmin, (size_t)ld_argmin, (size_t)num_out_rows, dim);
    return launch_ok("neighbor statistics launch");
}

}  // extern "C"

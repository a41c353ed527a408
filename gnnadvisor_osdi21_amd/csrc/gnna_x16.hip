// gnna_x16.hip -- aggregation over features STORED in bf16 / fp16 and ACCUMULATED in fp32 (gnna_agg_ld_x16).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its kernels are float only, GNNAdvisor_kernel.cu:186-259); the partition arguments and the
// three modes are those of gnna_agg_ld_f32.
//
// Shape of the computation:
//   * a wavefront takes G consecutive neighbor-groups (lane l: group l of the chunk), merges the groups that follow each other
//     in the same destination row into one run of edges, and walks the run 64 edges at a time: one coalesced load of 64 column
//     ids (and, for GCN, of the 64 source-side degrees), then LPR wave-wide row loads of 16 bytes per lane.  A row of D 16-bit
//     elements is covered by LPR = next_pow2(ceil(D / 8)) lanes, so one load instruction brings 64 / LPR whole rows (D = 64:
//     eight 128-byte rows -- one cache line each).  Rows wider than 512 elements are walked in column blocks of 512.
//   * every element is widened in registers (bf16: a shift / a mask, fp16: v_cvt_f32_f16) and added -- multiplied by the fp32
//     source degree for GCN -- into 8 fp32 accumulators per lane.  Nothing is rounded to 16 bits on the way.
//   * at the end of a run the 64 / LPR partial rows of the wavefront meet by a reduce-scatter over the lanes (permlane32_swap,
//     permlane16_swap, DPP row_ror:8 -- gnna_device.h), the row factor (epsilon, or the fp32 destination degree) is applied and
//     the row is ADDED to an fp32 matrix with float atomics: the caller's `out` when it is fp32, library scratch otherwise.
//     Atomics for every row make the kernel correct for any partition -- rows split over chunks, unordered part2Node, groups
//     with part_pointers[p + 1] < part_pointers[p] (taken as empty, as the fp32 kernels do) -- without a validation pass; a run
//     is a whole row of a chunk, so there are about (rows + chunks) x D of them per call, not one per group.
//   * 16-bit output: x16_finish_kernel reads the fp32 sums once, applies the ReLU and rounds every element exactly once
//     (round-to-nearest-even: v_cvt_pk_bf16_f32 for bf16, v_cvt_f16_f32 for fp16 -- not the round-to-zero v_cvt_pkrtz).
//   * source rows that are not 16-byte addressable (row stride not a multiple of 8 elements, width not a multiple of 8, base
//     not 16-byte aligned) are first copied into library scratch with the width padded to a multiple of 8 (zeros in the pad):
//     the gather itself never issues a 16-bit load.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdint>

#include "gnna.h"
#include "gnna_device.h"
#include "gnna_internal.h"

namespace gnna {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// the two 16-bit elements of one 32-bit word, widened (exact in both formats)
template <int TYPE>
__device__ __forceinline__ void widen2(uint32_t w, float &lo, float &hi)
{
    if constexpr (TYPE == GNNA_BF16) {
        lo = __uint_as_float(w << 16);
        hi = __uint_as_float(w & 0xffff0000u);
    } else {
        const f16x2 h = __builtin_bit_cast(f16x2, w);
        lo = (float)h.x;
        hi = (float)h.y;
    }
}

// one fp32 value -> the 16 bits of its round-to-nearest-even bf16 / fp16 (overflow: +-inf, NaN stays NaN)
template <int TYPE>
__device__ __forceinline__ uint16_t narrow1(float v)
{
    if constexpr (TYPE == GNNA_BF16) {
        const __hip_bfloat16 r = __float2bfloat16(v);
        uint16_t u;
        __builtin_memcpy(&u, &r, sizeof(u));
        return u;
    } else {
        return __builtin_bit_cast(uint16_t, (_Float16)v);
    }
}
template <int TYPE>
__device__ __forceinline__ uint32_t narrow2(float a, float b)
{
    if constexpr (TYPE == GNNA_BF16) {
        const __hip_bfloat162 r = __float22bfloat162_rn(make_float2(a, b));     // v_cvt_pk_bf16_f32
        uint32_t u;
        __builtin_memcpy(&u, &r, sizeof(u));
        return u;
    } else {
        f16x2 r;
        r.x = (_Float16)a;                                                       // v_cvt_f16_f32 (round-to-nearest-even)
        r.y = (_Float16)b;
        return __builtin_bit_cast(uint32_t, r);
    }
}

// Reduce-scatter steps over the lane pairs (l, l ^ STRIDE): the lanes whose STRIDE bit is clear get a(l) + a(l ^ STRIDE), the
// others b(l) + b(l ^ STRIDE).
__device__ __forceinline__ float scatter32(float a, float b)
{
    auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(t[0]) + __uint_as_float(t[1]);
}
__device__ __forceinline__ float scatter16(float a, float b)
{
    auto t = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(t[0]) + __uint_as_float(t[1]);
}
__device__ __forceinline__ float scatter8(float a, float b, bool upper)
{
    const float keep = upper ? b : a, send = upper ? a : b;
    return keep + row_ror<8>(send);          // (l + 8) mod 16 == l ^ 8 inside a 16-lane DPP row
}

struct X16Args {
    const char *X;              // 16-bit source rows, 16-byte aligned
    size_t ldx_bytes;           // a multiple of 16
    const int32_t *col, *pp, *p2n;
    float *F;                   // fp32 sums (zero-filled, or the caller's matrix to add to)
    size_t ldf;                 // floats
    const float *row_scale;     // GCN: destination-side degrees, else null
    const float *deg_col;       // GCN: source-side degrees
    float eps;                  // GIN: epsilon, else 1
    int64_t P;
    uint32_t num_in_rows, num_out_rows;
    int D, G, xcd_remap;
};

template <int TYPE, int LOG_LPR, bool WEIGHTED>
__global__ void __launch_bounds__(kBlock)
x16_kernel(const X16Args p)
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
    // a group without edges, with a negative range or with a row outside `out` contributes nothing and ends the run
    const bool bad = lane >= cnt || e <= s || s < 0 || (uint32_t)r >= p.num_out_rows;
    const int prev_r = __shfl_up(r, 1);
    const int prev_bad = __shfl_up((int)bad, 1);
    const bool head = lane == 0 || bad || prev_bad != 0 || r != prev_r;
    unsigned long long heads = __ballot(head);
    if (cnt < kWave) heads &= (1ull << cnt) - 1ull;
    const int bad_i = bad ? 1 : 0;
    // which of the 8 accumulator slots this lane ends up holding after the reduce-scatter, and whether it writes at all
    int kbase = 0;
    if constexpr (R >= 2) kbase += (lane & 32) ? 4 : 0;
    if constexpr (R >= 4) kbase += (lane & 16) ? 2 : 0;
    if constexpr (R >= 8) kbase += (lane & 8) ? 1 : 0;
    constexpr int NREM = R >= 8 ? 1 : (R == 4 ? 2 : (R == 2 ? 4 : 8));
    const bool writer = LPR >= 8 ? true : ((lane & 7 & ~(LPR - 1)) == 0);

    while (heads) {
        const int a = __builtin_ctzll(heads);
        heads &= heads - 1ull;
        const int b = heads ? __builtin_ctzll(heads) : cnt;
        if (__builtin_amdgcn_readlane(bad_i, a)) continue;
        const int rs = __builtin_amdgcn_readlane(s, a);
        const int re = __builtin_amdgcn_readlane(e, b - 1);
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(r, a);
        if (re <= rs) continue;
        for (int c0 = 0; c0 < p.D; c0 += LPR * 8) {
            const int mycol = c0 + cl * 8;
            const bool col_ok = mycol < p.D;
            float acc[8];
#pragma unroll
            for (int k = 0; k < 8; k++) acc[k] = 0.f;
            for (int e0 = rs; e0 < re; e0 += kWave) {
                const int nb = re - e0 < kWave ? re - e0 : kWave;
                int id = -1;
                float w = 0.f;
                if (lane < nb) {
                    id = p.col[(int64_t)e0 + lane];
                    if ((uint32_t)id >= p.num_in_rows) id = -1;           // (an id outside the source matrix is skipped, never read)
                    else if constexpr (WEIGHTED) w = p.deg_col[id];
                }
#pragma unroll
                for (int u0 = 0; u0 < LPR; u0 += U) {
                    if (u0 * R >= nb) break;
                    u32x4 v[U];
                    float ww[U];
#pragma unroll
                    for (int k = 0; k < U; k++) {
                        const int j = (u0 + k) * R + sub;
                        const int idj = __shfl(id, j);
                        if constexpr (WEIGHTED) ww[k] = __shfl(w, j); else ww[k] = 1.f;
                        v[k] = (u32x4)(0u);
                        if (idj >= 0 && col_ok)
                            v[k] = *reinterpret_cast<const u32x4 *>(p.X + (size_t)(uint32_t)idj * p.ldx_bytes + (size_t)mycol * 2);
                    }
#pragma unroll
                    for (int k = 0; k < U; k++) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            float lo, hi;
                            widen2<TYPE>(v[k][q], lo, hi);
                            if constexpr (WEIGHTED) {
                                acc[2 * q] = __builtin_fmaf(ww[k], lo, acc[2 * q]);
                                acc[2 * q + 1] = __builtin_fmaf(ww[k], hi, acc[2 * q + 1]);
                            } else {
                                acc[2 * q] += lo;
                                acc[2 * q + 1] += hi;
                            }
                        }
                    }
                }
            }
            // ---- the R partial rows of the wavefront -> one row, NREM elements per writing lane -------------------------
            float t4[4], t2[2], t1;
            float outv[8];
            if constexpr (R >= 2) {
#pragma unroll
                for (int i = 0; i < 4; i++) t4[i] = scatter32(acc[i], acc[i + 4]);
            }
            if constexpr (R >= 4) {
#pragma unroll
                for (int i = 0; i < 2; i++) t2[i] = scatter16(t4[i], t4[i + 2]);
            }
            if constexpr (R >= 8) {
                t1 = scatter8(t2[0], t2[1], (lane & 8) != 0);
                // narrower rows: the lanes that still hold the same element (lane bits LOG_LPR .. 2) sum up
                if constexpr (LPR <= 4) t1 += __shfl_xor(t1, 4);
                if constexpr (LPR <= 2) t1 += __shfl_xor(t1, 2);
                if constexpr (LPR <= 1) t1 += __shfl_xor(t1, 1);
                outv[0] = t1;
            } else if constexpr (R == 4) {
                outv[0] = t2[0]; outv[1] = t2[1];
            } else if constexpr (R == 2) {
#pragma unroll
                for (int i = 0; i < 4; i++) outv[i] = t4[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) outv[i] = acc[i];
            }
            if (writer && col_ok) {
                const float coef = p.row_scale ? p.row_scale[row] * p.eps : p.eps;
                float *dst = p.F + (size_t)row * p.ldf + (size_t)(mycol + kbase);
#pragma unroll
                for (int i = 0; i < NREM; i++)
                    if (mycol + kbase + i < p.D) atomicAdd(dst + i, outv[i] * coef);
            }
        }
    }
}

// out[r, 0:D] (16-bit, rows ld_out elements apart) = round(relu?(F[r, 0:D])); F rows ldf floats apart.  Every element of the
// D columns is written, whether or not the row had an edge.
template <int TYPE>
__global__ void __launch_bounds__(kBlock)
x16_finish_kernel(const float *__restrict__ F, size_t ldf, uint16_t *__restrict__ out, size_t ld_out, size_t rows, int D, int relu,
                  int vec)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    if (vec) {          // D, ldf, ld_out multiples of 8 and both bases 16-byte aligned: 8 elements per thread
        const size_t d8 = (size_t)D >> 3, n8 = rows * d8;
        for (size_t i = tid; i < n8; i += nthreads) {
            const size_t r = i / d8, c = (i - r * d8) << 3;
            f32x4 a = *reinterpret_cast<const f32x4 *>(F + r * ldf + c);
            f32x4 b = *reinterpret_cast<const f32x4 *>(F + r * ldf + c + 4);
            if (relu) {
#pragma unroll
                for (int k = 0; k < 4; k++) { a[k] = a[k] > 0.f ? a[k] : (a[k] != a[k] ? a[k] : 0.f); b[k] = b[k] > 0.f ? b[k] : (b[k] != b[k] ? b[k] : 0.f); }
            }
            u32x4 o;
            o[0] = narrow2<TYPE>(a[0], a[1]); o[1] = narrow2<TYPE>(a[2], a[3]);
            o[2] = narrow2<TYPE>(b[0], b[1]); o[3] = narrow2<TYPE>(b[2], b[3]);
            *reinterpret_cast<u32x4 *>(out + r * ld_out + c) = o;
        }
    } else {
        const size_t n = rows * (size_t)D;
        for (size_t i = tid; i < n; i += nthreads) {
            const size_t r = i / (unsigned)D, c = i - r * (unsigned)D;
            float v = F[r * ldf + c];
            if (relu) v = v > 0.f ? v : (v != v ? v : 0.f);
            out[r * ld_out + c] = narrow1<TYPE>(v);
        }
    }
}

// staged copy of source rows that cannot be read 16 bytes at a time: Xs[r, 0:Dp] = X[r, 0:D] | zeros, Dp a multiple of 8
__global__ void __launch_bounds__(kBlock)
x16_stage_kernel(const uint16_t *__restrict__ X, size_t ld_in, uint16_t *__restrict__ Xs, size_t rows, int D, int Dp)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t n = rows * (size_t)Dp;
    for (size_t i = tid; i < n; i += nthreads) {
        const size_t r = i / (unsigned)Dp, c = i - r * (unsigned)Dp;
        Xs[i] = c < (size_t)D ? X[r * ld_in + c] : (uint16_t)0;
    }
}

template <int TYPE, bool WEIGHTED>
void launch_main(int log_lpr, dim3 grid, hipStream_t stream, const X16Args &a)
{
    dispatch_lpr(log_lpr, [&](auto L) {
        hipLaunchKernelGGL((x16_kernel<TYPE, decltype(L)::value, WEIGHTED>), grid, dim3(kBlock), 0, stream, a);
    });
}

}  // namespace

// Scratch of the 16-bit path: slot 3 = staged source rows (only layouts that are not 16-byte addressable), slot 4 = fp32 sums of
// a call with 16-bit output.  Eager calls of a stream share them (grow-only), a captured call gets its capture's own.
constexpr int kSlotX16Stage = 3, kSlotX16Sums = 4;

bool x16_needs_staging(const void *input, int64_t ld_in, int dim)
{
    return (reinterpret_cast<uintptr_t>(input) & 15) != 0 || (ld_in & 7) != 0 || (dim & 7) != 0;
}

int reserve_x16(DeviceState *ds, hipStream_t stream, int64_t num_in_rows, int64_t num_out_rows, int dim)
{
    void *ws = nullptr;
    const size_t dp = (size_t)(dim + 7) / 8 * 8;
    int rc = get_workspace(ds, stream, kSlotX16Stage, align256((size_t)num_in_rows * dp * 2), &ws);
    if (rc != GNNA_OK) return rc;
    return get_workspace(ds, stream, kSlotX16Sums, align256((size_t)num_out_rows * (size_t)dim * sizeof(float)), &ws);
}

int launch_x16(DeviceState *ds, hipStream_t stream, const X16Launch &c)
{
    const int elem = 2;
    const bool out16 = c.out_type != GNNA_F32;
    const char *X = static_cast<const char *>(c.input);
    size_t ldx_bytes = (size_t)c.ld_in * elem;
    int rc;
    if (c.num_parts > 0 && c.num_in_rows > 0 && x16_needs_staging(c.input, c.ld_in, c.dim)) {
        const int dp = (c.dim + 7) / 8 * 8;
        void *xs = nullptr;
        rc = get_workspace(ds, stream, kSlotX16Stage, align256((size_t)c.num_in_rows * (size_t)dp * elem), &xs);
        if (rc != GNNA_OK) return rc;
        hipLaunchKernelGGL(x16_stage_kernel, dim3(elementwise_grid(c.num_in_rows * dp, ds->num_cus, 8)), dim3(kBlock), 0, stream,
                           static_cast<const uint16_t *>(c.input), (size_t)c.ld_in, static_cast<uint16_t *>(xs),
                           (size_t)c.num_in_rows, c.dim, dp);
        X = static_cast<const char *>(xs);
        ldx_bytes = (size_t)dp * elem;
    }
    // ---- where the fp32 sums meet ----------------------------------------------------------------------------------------
    float *F = static_cast<float *>(c.out);
    size_t ldf = (size_t)c.ld_out;
    if (out16) {
        void *ws = nullptr;
        const size_t bytes = (size_t)c.num_out_rows * (size_t)c.dim * sizeof(float);
        rc = get_workspace(ds, stream, kSlotX16Sums, align256(bytes), &ws);
        if (rc != GNNA_OK) return rc;
        F = static_cast<float *>(ws);
        ldf = (size_t)c.dim;
        // (a kernel, not hipMemsetAsync: a captured call then consists of kernel nodes only, like the fp32 path)
        rc = launch_zero_fill(ds, stream, F, c.num_out_rows, c.dim, c.dim);
        if (rc != GNNA_OK) return rc;
    } else if (!c.accumulate) {
        rc = launch_zero_fill(ds, stream, F, c.num_out_rows, c.dim, c.ld_out);
        if (rc != GNNA_OK) return rc;
    }
    profile_record(c.prof_call, 1, stream);
    if (c.num_parts > 0 && c.num_in_rows > 0) {
        X16Args a;
        a.X = X; a.ldx_bytes = ldx_bytes; a.col = c.column_index; a.pp = c.part_pointers; a.p2n = c.part2Node;
        a.F = F; a.ldf = ldf;
        a.row_scale = c.mode == MODE_GCN ? c.degrees_out : nullptr;
        a.deg_col = c.mode == MODE_GCN ? c.degrees_in : nullptr;
        a.eps = c.mode == MODE_GIN ? c.epsilon : 1.f;
        a.P = c.num_parts; a.num_in_rows = (uint32_t)std::min<int64_t>(c.num_in_rows, (int64_t)1 << 31);   // (ids are int32)
         a.num_out_rows = (uint32_t)c.num_out_rows;
        a.D = c.dim; a.xcd_remap = c.xcd_remap ? 1 : 0;
        const ChunkGrid cg = chunk_grid(c.num_parts, c.partSize, ds->num_cus);
        a.G = cg.G;
        if (cg.blocks > 0x7fffffffll)
            return fail(GNNA_ERR_UNSUPPORTED, "16-bit aggregation: %lld neighbor-groups in one call", (long long)c.num_parts);
        const int log_lpr = log2_lanes(c.dim, 8);
        const dim3 grid((unsigned)cg.blocks);
        const bool weighted = c.mode == MODE_GCN;
        if (c.in_type == GNNA_BF16) {
            if (weighted) launch_main<GNNA_BF16, true>(log_lpr, grid, stream, a); else launch_main<GNNA_BF16, false>(log_lpr, grid, stream, a);
        } else {
            if (weighted) launch_main<GNNA_F16, true>(log_lpr, grid, stream, a); else launch_main<GNNA_F16, false>(log_lpr, grid, stream, a);
        }
        rc = launch_ok("16-bit aggregation launch");
        if (rc != GNNA_OK) return rc;
    }
    // ---- epilogue: ReLU, and the one rounding of a 16-bit output ------------------------------------------------------------
    if (out16) {
        const int vec = (c.dim & 7) == 0 && (c.ld_out & 7) == 0 && (reinterpret_cast<uintptr_t>(c.out) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(F) & 15) == 0;
        const unsigned blocks = elementwise_grid(c.num_out_rows * c.dim / (vec ? 8 : 1), ds->num_cus, 8);
        uint16_t *o = static_cast<uint16_t *>(c.out);
        if (c.in_type == GNNA_BF16)
            hipLaunchKernelGGL(x16_finish_kernel<GNNA_BF16>, dim3(blocks), dim3(kBlock), 0, stream, F, ldf, o, (size_t)c.ld_out,
                               (size_t)c.num_out_rows, c.dim, c.relu ? 1 : 0, vec);
        else
            hipLaunchKernelGGL(x16_finish_kernel<GNNA_F16>, dim3(blocks), dim3(kBlock), 0, stream, F, ldf, o, (size_t)c.ld_out,
                               (size_t)c.num_out_rows, c.dim, c.relu ? 1 : 0, vec);
    } else if (c.relu) {
        launch_relu_rows(ds, stream, F, c.num_out_rows, c.dim, c.ld_out);
    }
    return launch_ok("16-bit aggregation epilogue");
}

}  // namespace gnna

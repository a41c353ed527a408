// gnna_reduce.hip -- element-wise max / min over a node's neighbours with the position of the winning edge
// (gnna_agg_reduce_ld_f32), and the backward that sends a gradient to those positions (gnna_scatter_arg_ld_f32).
// CDNA4 / gfx950 only.
//
// No counterpart in the reference (its kernels only sum, GNNAdvisor_kernel.cu:186-259); the partition arguments are those of
// gnna_agg_ld_f32.
//
// Everything here is ONE operation: the unsigned 64-bit maximum over the edges of a row of the key (gnna_keys.h)
//       (order(x) << 32) | (0xFFFFFFFF - edge position)
// where order() maps the 32 bits of a float to an unsigned that orders like the float (inverted for min).  The largest key
// holds the extreme value and, among equal values, the smallest edge position.  An unsigned maximum is associative and
// commutative and never rounds, so the result is the same bits for every partition, schedule and run, and the tie rule costs
// nothing extra.  No edge produces the key 0 (positions are below 2^31, so the low word is at least 0x80000000): 0 means
// "no edge has been seen".
//
// Shape of the computation (the gather is that of gnna_x16.hip):
//   * a wavefront takes G consecutive neighbor-groups (lane l: group l of the chunk), merges the groups that follow each other
//     in the same destination row into one run of edges, and walks the run 64 edges at a time: one coalesced load of 64 column
//     ids, then LPR wave-wide row loads of 16 bytes per lane.  A row of D floats is covered by LPR = next_pow2(ceil(D / 4))
//     lanes, so one load instruction brings 64 / LPR whole rows (D = 64: four 256-byte rows).  Rows wider than 256 floats are
//     walked in column blocks of 256.  A width that is not a multiple of 4 loads its last, partial vector element by element.
//   * every lane keeps the running key of its 4 elements in 8 registers: map, 64-bit compare, select.
//   * at the end of a run the 64 / LPR partial rows of the wavefront meet by a butterfly of key maxima over the lanes
//     (permlane32_swap, permlane16_swap, then lane shuffles), and the lanes of the first partial row send the row to scratch
//     with one 64-bit vector atomic max per element (global_atomic_umax_x2, no return value).  Atomics for every run make the
//     kernel correct for any partition -- rows split over groups and chunks, unordered part2Node, groups with
//     part_pointers[p + 1] < part_pointers[p] (taken as empty) -- without a validation pass; a run is a whole row of a chunk,
//     so there are about (rows + chunks) x D atomics per call, not one per group.
//   * reduce_finish_kernel reads every key once and writes out (value, or 0 for the key 0; ReLU) and arg (position, or -1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gnna.h"
#include "gnna_device.h"
#include "gnna_internal.h"
#include "gnna_keys.h"

namespace gnna {
namespace {

struct ReduceArgs {
    const float *X;             // source rows
    size_t ldx;                 // floats
    const int32_t *col, *pp, *p2n;
    u64 *K;                     // [num_out_rows][D] keys, zero when the kernel starts
    int64_t P;
    uint32_t num_in_rows, num_out_rows;
    int D, G, xcd_remap;
};

template <int OP, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
reduce_kernel(const ReduceArgs p)
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
            u64 best[4];
#pragma unroll
            for (int q = 0; q < 4; q++) best[q] = 0ull;
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
                            const u64 key = ok[k] ? pack(order_of<OP>(v[k][q]), npos) : 0ull;
                            best[q] = umax64(best[q], key);
                        }
                    }
                }
            }
            // ---- the R partial rows of the wavefront -> one row, in every lane ---------------------------------------------
#pragma unroll
            for (int q = 0; q < 4; q++) best[q] = partial_rows_max<R>(best[q]);
            if (sub == 0 && col_ok) {
                u64 *dst = p.K + (size_t)row * (size_t)p.D + (size_t)mycol;
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (mycol + q < p.D && best[q] != 0ull) atomicMax(dst + q, best[q]);
            }
        }
    }
}

// out[r, c] = value of K[r, c] (0 when no edge reached it; max(., 0) with relu), arg[r, c] = its edge position (-1).  Every
// element of the D columns of every row is written.
__global__ void __launch_bounds__(kBlock)
reduce_finish_kernel(const u64 *__restrict__ K, float *__restrict__ out, size_t ld_out, int32_t *__restrict__ arg, size_t ld_arg,
                     size_t rows, int D, int op, int relu)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t n = rows * (size_t)D;
    for (size_t i = tid; i < n; i += nthreads) {
        const size_t r = i / (unsigned)D, c = i - r * (unsigned)D;
        float v;
        int32_t pos;
        key_result(K[i], op, &v, &pos);
        if (relu) v = v > 0.f ? v : (v != v ? v : 0.f);         // NaN stays NaN, as torch.relu
        out[r * ld_out + c] = v;
        if (arg) arg[r * ld_arg + c] = pos;
    }
}

// no edges at all: out = 0, arg = -1
__global__ void __launch_bounds__(kBlock)
reduce_empty_kernel(float *__restrict__ out, size_t ld_out, int32_t *__restrict__ arg, size_t ld_arg, size_t rows, int D)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t n = rows * (size_t)D;
    for (size_t i = tid; i < n; i += nthreads) {
        const size_t r = i / (unsigned)D, c = i - r * (unsigned)D;
        out[r * ld_out + c] = 0.f;
        if (arg) arg[r * ld_arg + c] = -1;
    }
}

// grad_in[col[arg[r, c]], c] += grad_out[r, c]: one thread per element, one float atomic per non-negative arg
__global__ void __launch_bounds__(kBlock)
scatter_arg_kernel(const float *__restrict__ go, size_t ld_go, const int32_t *__restrict__ arg, size_t ld_arg,
                   const int32_t *__restrict__ col, float *__restrict__ gi, size_t ld_gi, uint32_t num_in_rows, size_t rows, int D)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t n = rows * (size_t)D;
    for (size_t i = tid; i < n; i += nthreads) {
        const size_t r = i / (unsigned)D, c = i - r * (unsigned)D;
        const int32_t a = arg[r * ld_arg + c];
        if (a < 0) continue;
        const int32_t src = col[a];
        if ((uint32_t)src >= num_in_rows) continue;              // (an id outside grad_in is skipped, as the forward skipped it)
        atomicAdd(gi + (size_t)(uint32_t)src * ld_gi + c, go[r * ld_go + c]);
    }
}

template <int OP>
void launch_main(int log_lpr, dim3 grid, hipStream_t stream, const ReduceArgs &a)
{
    dispatch_lpr(log_lpr, [&](auto L) {
        hipLaunchKernelGGL((reduce_kernel<OP, decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
}

// Scratch of the reduce entry: slot 5 = the keys.  Eager calls of a stream share it (grow-only), a captured call gets its
// capture's own.
constexpr int kSlotReduceKeys = 5;

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_agg_reduce_ld_f32(int op, const float *input, int64_t ld_in, int64_t num_in_rows, const int32_t *column_index,
                           const int32_t *part_pointers, const int32_t *part2Node, float *out, int64_t ld_out, int32_t *arg,
                           int64_t ld_arg, int64_t num_out_rows, int dim, int64_t num_parts, int partSize, unsigned flags,
                           void *stream_v)
{
    if (op != GNNA_REDUCE_MAX && op != GNNA_REDUCE_MIN)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "op must be GNNA_REDUCE_MAX or GNNA_REDUCE_MIN (got %d)", op);
    if (flags & ~(unsigned)(GNNA_ACCUMULATE | GNNA_EPILOGUE_RELU))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "unknown flag bits 0x%x", flags);
    if (flags & GNNA_ACCUMULATE)
        return fail(GNNA_ERR_UNSUPPORTED, "gnna_agg_reduce_ld_f32: GNNA_ACCUMULATE has no meaning for a max / min");
    if (dim < 1) return fail(GNNA_ERR_INVALID_ARGUMENT, "dim must be >= 1 (got %d)", dim);
    if (num_out_rows < 0 || num_parts < 0 || num_in_rows < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "negative size (num_out_rows=%lld num_in_rows=%lld num_parts=%lld)",
                    (long long)num_out_rows, (long long)num_in_rows, (long long)num_parts);
    if (partSize <= 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "partSize must be positive (got %d)", partSize);
    if (num_out_rows >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%lld destination rows in one call (at most 536870911): shard the rows", (long long)num_out_rows);
    // (a null arg leaves ld_arg with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld(ld_out, dim) || (arg ? bad_ld(ld_arg, dim) : ld_arg >= ((int64_t)1 << 29)))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_out=%lld ld_arg=%lld dim=%d)",
                    (long long)ld_in, (long long)ld_out, (long long)ld_arg, dim);
    if (num_out_rows == 0) return GNNA_OK;
    if (!out) return fail(GNNA_ERR_INVALID_ARGUMENT, "null output pointer");
    const bool work = num_parts > 0 && num_in_rows > 0;
    if (work && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "null feature pointer");
    if ((reinterpret_cast<uintptr_t>(input) & 3) || (reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(arg) & 3))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "feature and arg pointers must be 4-byte aligned");
    if (work && (!column_index || !part_pointers || !part2Node)) return fail(GNNA_ERR_INVALID_ARGUMENT, "null index pointer");
    if (out == input) return fail(GNNA_ERR_INVALID_ARGUMENT, "out must not alias input");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    int rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    const size_t n = (size_t)num_out_rows * (size_t)dim;
    const unsigned eblocks = elementwise_grid((int64_t)n, ds->num_cus, 8);
    const int relu = (flags & GNNA_EPILOGUE_RELU) ? 1 : 0;
    if (!work) {
        hipLaunchKernelGGL(reduce_empty_kernel, dim3(eblocks), dim3(kBlock), 0, stream, out, (size_t)ld_out, arg, (size_t)ld_arg,
                           (size_t)num_out_rows, dim);
        return launch_ok("neighbor reduce launch");
    }
    void *ws = nullptr;
    rc = get_workspace(ds, stream, kSlotReduceKeys, (n * sizeof(u64) + 255) & ~(size_t)255, &ws);
    if (rc != GNNA_OK) return rc;
    u64 *K = static_cast<u64 *>(ws);
    // (a kernel, not hipMemsetAsync: a captured call then consists of kernel nodes only)
    rc = launch_zero_fill(ds, stream, reinterpret_cast<float *>(K), num_out_rows, 2 * dim, 2 * (int64_t)dim);
    if (rc != GNNA_OK) return rc;
    ReduceArgs a;
    a.X = input; a.ldx = (size_t)ld_in; a.col = column_index; a.pp = part_pointers; a.p2n = part2Node; a.K = K;
    a.P = num_parts; a.num_in_rows = (uint32_t)std::min<int64_t>(num_in_rows, (int64_t)1 << 31);   // (ids are int32)
    a.num_out_rows = (uint32_t)num_out_rows;
    a.D = dim; a.xcd_remap = xcd_remap_on();
    const ChunkGrid cg = chunk_grid(num_parts, partSize, ds->num_cus);
    a.G = cg.G;
    if (cg.blocks > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "neighbor reduce: %lld neighbor-groups in one call", (long long)num_parts);
    const int log_lpr = log2_lanes(dim, 4);
    const dim3 grid((unsigned)cg.blocks);
    if (op == GNNA_REDUCE_MAX) launch_main<GNNA_REDUCE_MAX>(log_lpr, grid, stream, a);
    else launch_main<GNNA_REDUCE_MIN>(log_lpr, grid, stream, a);
    hipLaunchKernelGGL(reduce_finish_kernel, dim3(eblocks), dim3(kBlock), 0, stream, K, out, (size_t)ld_out, arg, (size_t)ld_arg,
                       (size_t)num_out_rows, dim, op, relu);
    return launch_ok("neighbor reduce launch");
}

int gnna_scatter_arg_ld_f32(const float *grad_out, int64_t ld_go, const int32_t *arg, int64_t ld_arg, const int32_t *column_index,
                            int64_t num_out_rows, float *grad_in, int64_t ld_gi, int64_t num_in_rows, int dim, unsigned flags,
                            void *stream_v)
{
    if (flags & ~(unsigned)GNNA_ACCUMULATE) return fail(GNNA_ERR_INVALID_ARGUMENT, "unknown flag bits 0x%x", flags);
    if (dim < 1) return fail(GNNA_ERR_INVALID_ARGUMENT, "dim must be >= 1 (got %d)", dim);
    if (num_out_rows < 0 || num_in_rows < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "negative size (num_out_rows=%lld num_in_rows=%lld)", (long long)num_out_rows,
                    (long long)num_in_rows);
    if (bad_ld(ld_go, dim) || bad_ld(ld_arg, dim) || bad_ld(ld_gi, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "row strides must be >= dim and < 2^29 elements (ld_go=%lld ld_arg=%lld ld_gi=%lld dim=%d)",
                    (long long)ld_go, (long long)ld_arg, (long long)ld_gi, dim);
    if (num_out_rows >= ((int64_t)1 << 29) || num_in_rows >= ((int64_t)1 << 31))
        return fail(GNNA_ERR_UNSUPPORTED, "too many rows in one call (num_out_rows=%lld num_in_rows=%lld)", (long long)num_out_rows,
                    (long long)num_in_rows);
    // one float atomic per element: the order of the additions into a source row is not fixed
    int rc = deterministic_refused("gnna_scatter_arg_ld_f32", "its sums meet through float atomics");
    if (rc != GNNA_OK) return rc;
    if (num_in_rows == 0) return GNNA_OK;
    if (!grad_in) return fail(GNNA_ERR_INVALID_ARGUMENT, "null grad_in pointer");
    if (num_out_rows > 0 && (!grad_out || !arg || !column_index)) return fail(GNNA_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (grad_in == grad_out) return fail(GNNA_ERR_INVALID_ARGUMENT, "grad_in must not alias grad_out");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    if (!(flags & GNNA_ACCUMULATE)) {
        rc = launch_zero_fill(ds, stream, grad_in, num_in_rows, dim, ld_gi);
        if (rc != GNNA_OK) return rc;
    }
    if (num_out_rows == 0) return GNNA_OK;
    const size_t n = (size_t)num_out_rows * (size_t)dim;
    hipLaunchKernelGGL(scatter_arg_kernel, dim3(elementwise_grid((int64_t)n, ds->num_cus, 8)), dim3(kBlock), 0, stream, grad_out,
                       (size_t)ld_go, arg, (size_t)ld_arg, column_index, grad_in, (size_t)ld_gi, (uint32_t)num_in_rows,
                       (size_t)num_out_rows, dim);
    return launch_ok("scatter_arg launch");
}

}  // extern "C"

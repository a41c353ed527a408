// gnna_edge.hip -- edge softmax over the edges of every destination row, forward and backward (the attention
// coefficients of a GAT layer, which gnna_agg_edge_ld_f32 then aggregates with).  CDNA4 / gfx950 only.
//
//   forward:  p[h, e]  = exp(s[h, e] - max_row) / sum_row exp(s - max_row)
//   backward: ds[h, e] = p[h, e] * (dp[h, e] - sum_row p * dp)
//
// Scores are head-major [heads, nnz], so a row's edges are contiguous per head.  Degrees are power-law: a block takes a
// tile of consecutive rows, and every row is handled by a SEG-lane segment of a wavefront (64 / SEG rows per wavefront;
// SEG follows the average degree) -- unless it is longer than kLongIters sweeps of its segment, in which case the whole
// block takes it after the short rows, one long row at a time.  Lanes read 4 consecutive edges per step (one dwordx4 load
// where all four are inside the row).  Every row is reduced by one segment or one block in a fixed order and written by it
// with plain stores: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "gnna.h"
#include "gnna_device.h"
#include "gnna_internal.h"

namespace gnna {
namespace {

constexpr int kLongIters = 8;     // a row of more than SEG * 4 * kLongIters edges goes to the whole block

typedef VecOf<4>::T VT;
typedef VecOf<4>::M MT;

// the 4 values at [e, e + 4) that lie before `end` (the others: `fill`)
__device__ __forceinline__ VT load4(const float *__restrict__ p, int64_t e, int64_t end, float fill)
{
    if (e + 4 <= end) return *reinterpret_cast<const MT *>(p + e);
    VT v = (VT)(fill);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (e + k < end) v[k] = p[e + k];
    return v;
}

__device__ __forceinline__ void store4(float *__restrict__ p, int64_t e, int64_t end, VT v)
{
    if (e + 4 <= end) { *reinterpret_cast<MT *>(p + e) = v; return; }
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (e + k < end) p[e + k] = v[k];
}

// running (max, sum of exp(x - max)) pairs
struct MaxSum { float m, l; };

__device__ __forceinline__ MaxSum ms_merge(MaxSum a, MaxSum b)
{
    const float m = fmaxf(a.m, b.m);
    if (m == -INFINITY) return a;
    const float fa = a.m == -INFINITY ? 0.f : expf(a.m - m);
    const float fb = b.m == -INFINITY ? 0.f : expf(b.m - m);
    return MaxSum{m, a.l * fa + b.l * fb};
}

// (the 4 values enter together: one rescale of the running sum per step, 5 exponentials per 4 edges instead of 8)
__device__ __forceinline__ MaxSum ms_add4(MaxSum a, VT x, int64_t e, int64_t end)
{
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (e + k < end) mx = fmaxf(mx, x[k]);
    const float m = fmaxf(a.m, mx);
    if (m == -INFINITY) return a;
    float l = a.m == -INFINITY ? 0.f : a.l * expf(a.m - m);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (e + k < end) l += expf(x[k] - m);
    return MaxSum{m, l};
}

// reductions over the W lanes of a segment (W a power of two <= 64; butterflies stay inside the segment)
template <int W>
__device__ __forceinline__ MaxSum seg_reduce(MaxSum v)
{
#pragma unroll
    for (int d = W / 2; d > 0; d >>= 1) v = ms_merge(v, MaxSum{__shfl_xor(v.m, d), __shfl_xor(v.l, d)});
    return v;
}

template <int W>
__device__ __forceinline__ float seg_sum(float v)
{
#pragma unroll
    for (int d = W / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// One row [beg, end) of one head, reduced over `nl` lanes (lane index `t` among them) that sweep it 4 edges at a time.
// The cross-lane reduction is passed in: a segment's butterfly or the block's.
template <bool BWD, typename MS_RED, typename SUM_RED>
__device__ __forceinline__ void softmax_row(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out,
                                            int64_t beg, int64_t end, int t, int nl, MS_RED ms_red, SUM_RED sum_red)
{
    const int64_t step = (int64_t)nl * 4;
    if constexpr (!BWD) {
        MaxSum acc{-INFINITY, 0.f};
        for (int64_t e = beg + 4 * t; e < end; e += step) acc = ms_add4(acc, load4(a, e, end, 0.f), e, end);
        acc = ms_red(acc);
        const float m = acc.m, l = acc.l;
        for (int64_t e = beg + 4 * t; e < end; e += step) {
            VT x = load4(a, e, end, 0.f);
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = expf(x[k] - m) / l;
            store4(out, e, end, x);
        }
    } else {
        float dot = 0.f;
        for (int64_t e = beg + 4 * t; e < end; e += step) {
            const VT p = load4(a, e, end, 0.f), g = load4(b, e, end, 0.f);
            dot += (p[0] * g[0] + p[1] * g[1]) + (p[2] * g[2] + p[3] * g[3]);
        }
        dot = sum_red(dot);
        for (int64_t e = beg + 4 * t; e < end; e += step) {
            const VT p = load4(a, e, end, 0.f), g = load4(b, e, end, 0.f);
            VT r;
#pragma unroll
            for (int k = 0; k < 4; k++) r[k] = p[k] * (g[k] - dot);
            store4(out, e, end, r);
        }
    }
}

// a: scores (forward) or probs (backward); b: grad_probs (backward); out: probs or grad_scores.  blockIdx.y = head.
template <int SEG, bool BWD>
__global__ void __launch_bounds__(kBlock)
edge_softmax_kernel(const float *__restrict__ a, const float *__restrict__ b, const int32_t *__restrict__ rp, int64_t N,
                    int64_t nnz, float *__restrict__ out)
{
    constexpr int RPW = kWave / SEG;                 // rows per wavefront
    constexpr int TILE = kWavesPerBlock * RPW;       // rows per block
    constexpr int LONG = SEG * 4 * kLongIters;
    __shared__ int s_long[TILE];
    __shared__ int s_nlong;
    __shared__ float s_red[2][kWavesPerBlock];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int64_t hoff = (int64_t)blockIdx.y * nnz;
    a += hoff; out += hoff;
    if constexpr (BWD) b += hoff;
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * TILE;
    const int local = wib * RPW + lane / SEG;
    const int64_t row = r0 + local;
    int64_t beg = 0, end = 0;
    if (row < N) { beg = rp[row]; end = rp[row + 1]; }
    const bool is_long = end - beg > LONG;
    if (is_long && lane % SEG == 0) s_long[atomicAdd(&s_nlong, 1)] = local;
    // short rows: the segment (empty and long rows: nothing -- every lane of a segment takes the same branch)
    if (!is_long && end > beg) {
        softmax_row<BWD>(a, b, out, beg, end, lane % SEG, SEG,
                         [](MaxSum v) { return seg_reduce<SEG>(v); }, [](float v) { return seg_sum<SEG>(v); });
    }
    __syncthreads();
    // long rows: the whole block, one after the other (LDS list order may vary; each row's result does not depend on it)
    const int nlong = s_nlong;
    for (int q = 0; q < nlong; q++) {
        const int64_t rr = r0 + s_long[q];
        const int64_t lb = rp[rr], le = rp[rr + 1];
        auto block_ms = [&](MaxSum v) {
            v = seg_reduce<kWave>(v);
            __syncthreads();
            if (lane == 0) { s_red[0][wib] = v.m; s_red[1][wib] = v.l; }
            __syncthreads();
            MaxSum r{s_red[0][0], s_red[1][0]};
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; w++) r = ms_merge(r, MaxSum{s_red[0][w], s_red[1][w]});
            return r;
        };
        auto block_sum = [&](float v) {
            v = seg_sum<kWave>(v);
            __syncthreads();
            if (lane == 0) s_red[0][wib] = v;
            __syncthreads();
            float r = s_red[0][0];
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; w++) r += s_red[0][w];
            return r;
        };
        softmax_row<BWD>(a, b, out, lb, le, tid, kBlock, block_ms, block_sum);
    }
}

template <bool BWD>
int launch_edge_softmax(const float *a, const float *b, const int32_t *rp, int64_t N, int64_t nnz, int heads, float *out,
                        void *stream_v)
{
    if (N < 0 || nnz < 0 || heads < 1)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "bad size (num_rows=%lld num_edges=%lld num_heads=%d)", (long long)N,
                    (long long)nnz, heads);
    if (nnz > 0x7fffffffLL) return fail(GNNA_ERR_UNSUPPORTED, "more than 2^31-1 edges: shard the graph");
    if (heads > 65535) return fail(GNNA_ERR_UNSUPPORTED, "at most 65535 heads (got %d)", heads);
    if (N == 0 || nnz == 0) return GNNA_OK;
    if (!a || !rp || !out || (BWD && !b)) return fail(GNNA_ERR_INVALID_ARGUMENT, "null pointer");
    if (out == a || (BWD && out == b)) return fail(GNNA_ERR_INVALID_ARGUMENT, "the output must not alias an input");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    // lanes per row: about a quarter of the average degree (every lane reads 4 edges per step), 4 .. 64
    const int64_t avg = (nnz + N - 1) / N;
    int seg = 4;
    while (seg < kWave && (int64_t)seg * 4 < avg) seg <<= 1;
    const int64_t tile = (int64_t)kWavesPerBlock * (kWave / seg);
    const int64_t blocks = (N + tile - 1) / tile;
    if (blocks > 0x7fffffffLL) return fail(GNNA_ERR_UNSUPPORTED, "too many rows (%lld)", (long long)N);
    const dim3 grid((unsigned)blocks, (unsigned)heads);
    switch (seg) {
    case 4: hipLaunchKernelGGL((edge_softmax_kernel<4, BWD>), grid, dim3(kBlock), 0, stream, a, b, rp, N, nnz, out); break;
    case 8: hipLaunchKernelGGL((edge_softmax_kernel<8, BWD>), grid, dim3(kBlock), 0, stream, a, b, rp, N, nnz, out); break;
    case 16: hipLaunchKernelGGL((edge_softmax_kernel<16, BWD>), grid, dim3(kBlock), 0, stream, a, b, rp, N, nnz, out); break;
    case 32: hipLaunchKernelGGL((edge_softmax_kernel<32, BWD>), grid, dim3(kBlock), 0, stream, a, b, rp, N, nnz, out); break;
    default: hipLaunchKernelGGL((edge_softmax_kernel<64, BWD>), grid, dim3(kBlock), 0, stream, a, b, rp, N, nnz, out); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GNNA_ERR_HIP, "edge softmax launch: %s", hipGetErrorString(e));
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_edge_softmax_f32(const float *scores, const int32_t *row_pointers, int64_t num_rows, int64_t num_edges, int num_heads,
                          float *probs, void *stream)
{
    return launch_edge_softmax<false>(scores, nullptr, row_pointers, num_rows, num_edges, num_heads, probs, stream);
}

int gnna_edge_softmax_backward_f32(const float *probs, const float *grad_probs, const int32_t *row_pointers, int64_t num_rows,
                                   int64_t num_edges, int num_heads, float *grad_scores, void *stream)
{
    return launch_edge_softmax<true>(probs, grad_probs, row_pointers, num_rows, num_edges, num_heads, grad_scores, stream);
}

#pragma GCC visibility pop
}  // extern "C"

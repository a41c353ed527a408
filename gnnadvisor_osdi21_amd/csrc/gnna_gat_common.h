// gnna_gat_common.h -- what the fused attention kernels of gnna_gat.hip (GAT: a scalar score per node and head), gnna_gatv2.hip
// (GATv2: the score is a dot product over the gathered row) and gnna_dotattn.hip (scaled dot-product attention) share: the
// lane-layout folds, the online (max, sum) of the lse passes, the dropout factor, the row-score lse pass and the (lse, c) pack pass
// of GATv2 and dot (GAT has its own: node scalars, 16-byte records), the head of the three pull kernels (the wavefront's chunk and
// its groups; each kernel keeps its own loop over the runs), their launcher and the argument checks and tails of the entries.  Not installed.
#ifndef GNNA_GAT_COMMON_H_
#define GNNA_GAT_COMMON_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "gnna_device.h"
#include "gnna_internal.h"

namespace gnna {
namespace gat {

typedef VecOf<4>::T VT;
typedef VecOf<4>::M MT;

constexpr int kLongIters = 8;     // lse pass: a row of more than (lanes or slots of its segment) * 4 * kLongIters edges goes to the whole block
constexpr int kMaxDim = 256;      // floats per head (LPH <= 64)

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : z * slope; }

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

// sum over the LPH consecutive lanes of a head; result in every lane of the head
template <int LPH>
__device__ __forceinline__ float head_sum(float v)
{
    if constexpr (LPH == 1) return v;
    else if constexpr (LPH == 2) return v + dpp_move<0xB1>(v);      // quad_perm [1,0,3,2]
    else return lane_group_sum<LPH>(v);
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

// ---- the online (max, sum) of an lse pass -----------------------------------------------------------------------------------

struct MaxSum { float m, l; };

__device__ __forceinline__ MaxSum ms_merge(MaxSum a, MaxSum b)
{
    const float m = fmaxf(a.m, b.m);
    if (m == -INFINITY) return a;
    const float fa = a.m == -INFINITY ? 0.f : expf(a.m - m);
    const float fb = b.m == -INFINITY ? 0.f : expf(b.m - m);
    return MaxSum{m, a.l * fa + b.l * fb};
}

// four scores enter together (-inf: no edge): one rescale of the running sum per step
__device__ __forceinline__ MaxSum ms_add4(MaxSum a, const float x[4])
{
    const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    const float m = fmaxf(a.m, mx);
    if (m == -INFINITY) return a;
    float l = a.m == -INFINITY ? 0.f : a.l * expf(a.m - m);
#pragma unroll
    for (int k = 0; k < 4; k++) l += x[k] == -INFINITY ? 0.f : expf(x[k] - m);
    return MaxSum{m, l};
}

// butterfly over the `w` lanes of a segment (a power of two <= 64)
__device__ __forceinline__ MaxSum seg_reduce(MaxSum v, int w)
{
    for (int d = w >> 1; d > 0; d >>= 1) v = ms_merge(v, MaxSum{__shfl_xor(v.m, d), __shfl_xor(v.l, d)});
    return v;
}

__device__ __forceinline__ float lse_of(MaxSum v) { return v.m == -INFINITY ? 0.f : v.m + logf(v.l); }

// ---- attention dropout (gnna_ext.h: the mask rule) ---------------------------------------------------------------------------

// k(i, j, h): keep_scale for a kept edge i <- j of head h, 0 for a dropped one.  A function of the two row numbers and the head
// alone, so every pass agrees without an edge position, a perm array or a reverse-edge map.
__device__ __forceinline__ float drop_factor(uint64_t rng_seed, uint32_t drop_thr, float keep_scale, uint32_t i, uint32_t j, int h)
{
    const uint64_t u = ((uint64_t)i << 35) | ((uint64_t)j << 6) | (uint64_t)(uint32_t)h;
    return (uint32_t)(key_of_position(rng_seed, u) >> 32) >= drop_thr ? keep_scale : 0.f;
}

// thr = (uint32) floor((double)attn_drop * 2^32) and k = 1 / (1 - attn_drop) in fp32, as gnna_ext.h states them; Args: the
// argument struct of a pull kernel
template <class Args>
void set_drop(Args *a, float attn_drop, uint64_t rng_seed)
{
    a->rng_seed = rng_seed;
    a->drop_thr = (uint32_t)std::floor((double)attn_drop * 4294967296.0);
    a->keep_scale = 1.0f / (1.0f - attn_drop);
}

// ---- lse[i, h] of a score made from the gathered row (GATv2, dot) ------------------------------------------------------------
//
// Args is the kernel's argument struct and says what the score is.  It has rp, col (the CSR), lse, N (rows), M (ids < M), heads,
// dim and
//     Own              what the walked row brings to the score, loaded once per row and column block ({}: an idle lane's)
//     own(row, colf, n4)       loads it: the n4 (<= 4) floats at column colf of `row`
//     gathered(id)     the row of an id
//     part(own, v)     this lane's share of the sum over a head, from the piece v of a gathered row
//     scaled(s)        z from the sum over the head

// The edges [beg, end) of `row` swept by `nl` slots of LPR lanes (this one: slot t), four edges per slot and step, for the heads
// of the column block at hb0.  Every lane of a wavefront makes the same number of steps (the folds are wave-wide).
template <class Args, int LOG_LPH, int LOG_LPR>
__device__ __forceinline__ MaxSum lse_sweep(const Args &p, int64_t row, int64_t beg, int64_t end, int t, int nl, int hb0, int cl)
{
    constexpr int LPH = 1 << LOG_LPH;
    const int h = hb0 + (cl >> LOG_LPH), fl = (cl & (LPH - 1)) * 4;
    const int n4 = h < p.heads ? p.dim - fl : 0;
    const bool ok = n4 > 0;
    const size_t colf = (size_t)(ok ? h : 0) * p.dim + (ok ? fl : 0);
    typename Args::Own own{};
    if (ok) own = p.own(row, colf, n4);
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
            if (id[k] >= 0 && ok) v[k] = load_piece(p.gathered((uint32_t)id[k]) + colf, n4);
        }
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float z = p.scaled(head_sum<LPH>(p.part(own, v[k])));
            x[k] = id[k] >= 0 ? z : -INFINITY;
        }
        acc = ms_add4(acc, x);
    }
    // the 64 / LPR slots of the wavefront meet (lanes that share lane % LPR), in a fixed order
#pragma unroll
    for (int d = kWave >> 1; d >= (1 << LOG_LPR); d >>= 1) acc = ms_merge(acc, MaxSum{__shfl_xor(acc.m, d), __shfl_xor(acc.l, d)});
    return acc;
}

// One wavefront per row (the whole block for long rows, after the short ones); N rows, ids < M.  The slots, then the waves, meet
// in a fixed order; one writer per (row, head), plain stores: the same bits on every run.
template <class Args, int LOG_LPH, int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
lse_kernel(const Args p)
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
            const MaxSum v = lse_sweep<Args, LOG_LPH, LOG_LPR>(p, row, beg, end, sub, R, hb0, cl);
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
            const MaxSum v = lse_sweep<Args, LOG_LPH, LOG_LPR>(p, rr, lb, le, wib * R + sub, kWavesPerBlock * R, hb0, cl);
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

// prefix: "<prefix> launch" is how a failed launch is reported
template <class Args>
int launch_lse(const char *prefix, hipStream_t stream, const Args &a)
{
    const dim3 grid((unsigned)((a.N + kWavesPerBlock - 1) / kWavesPerBlock));      // (N < 2^29)
    dispatch_layout(attn_layout(a.heads, a.dim), [&](auto H, auto L) {
        hipLaunchKernelGGL((lse_kernel<Args, decltype(H)::value, decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("%s launch", prefix);
}

// ---- c[i, h] = <dY[i, h, :], Y[i, h, :]>, packed with lse (GATv2, dot) -------------------------------------------------------

// SLOT: the library scratch it fills, which gives each family (a translation unit of its own) its own instance.
template <int SLOT>
__global__ void __launch_bounds__(kBlock)
lse_c_pack_kernel(const float *__restrict__ G, size_t ldg, const float *__restrict__ Y, size_t ldy, const float *__restrict__ lse,
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

// (lse, c) per (destination row, head) of a backward call, 8 bytes, in library scratch SLOT
template <int SLOT>
int launch_lse_c_pack(const char *what, DeviceState *ds, hipStream_t stream, const float *dY, int64_t ld_dy, const float *Y,
                      int64_t ld_y, const float *lse, int64_t rows, int heads, int dim, const float2 **pack)
{
    void *ws = nullptr;
    const int rc = get_workspace(ds, stream, SLOT, ((size_t)rows * heads * sizeof(float2) + 255) & ~(size_t)255, &ws);
    if (rc != GNNA_OK) return rc;
    *pack = static_cast<float2 *>(ws);
    hipLaunchKernelGGL(lse_c_pack_kernel<SLOT>, dim3(elementwise_grid(rows * heads, ds->num_cus, 8)), dim3(kBlock), 0, stream, dY,
                       (size_t)ld_dy, Y, (size_t)ld_y, lse, static_cast<float2 *>(ws), (size_t)rows, heads, dim);
    return launch_ok("%s: pack launch", what);
}

// ---- the head of a pull kernel -----------------------------------------------------------------------------------------------

// The chunk of G consecutive neighbor-groups this wavefront takes.  xcd_remap: consecutive chunks on one XCD (workgroups go round
// the 8 XCDs), so that neighbouring rows share source rows in that L2.
__device__ __forceinline__ int64_t pull_chunk(int xcd_remap)
{
    uint32_t vb = blockIdx.x;
    if (xcd_remap) {
        const uint32_t nb = gridDim.x, q = nb / kXcds, rem = nb % kXcds, x = vb % kXcds, i = vb / kXcds;
        vb = x < rem ? x * (q + 1) + i : rem * (q + 1) + (x - rem) * q + i;
    }
    return (int64_t)vb * kWavesPerBlock + (threadIdx.x >> 6);
}

// The groups [g0, g0 + cnt) of a wavefront, one per lane (cnt <= 64; a lane beyond them has none).  Consecutive groups of one row
// make a run; the kernel takes the runs off `starts` bit by bit and reads a run's first and last group with readlane.
struct PullGroups {
    int s, e, r;                    // this lane's group: the edges [s, e) of row r
    int bad;                        // the group contributes nothing and ends the run: no edges, a negative range, a row >= p.N
    unsigned long long starts;      // the lanes whose group begins a run
};
template <class Args>
__device__ __forceinline__ PullGroups pull_groups(const Args &p, int64_t g0, int cnt, int lane)
{
    int s = 0, e = 0, r = -1;
    if (lane < cnt) {
        s = p.pp[g0 + lane];
        e = p.pp[g0 + lane + 1];
        r = p.p2n[g0 + lane];
    }
    const bool bad = lane >= cnt || e <= s || s < 0 || (uint32_t)r >= p.N;
    const int prev_r = __shfl_up(r, 1);
    const int prev_bad = __shfl_up((int)bad, 1);
    const bool first = lane == 0 || bad || prev_bad != 0 || r != prev_r;
    unsigned long long starts = __ballot(first);
    if (cnt < kWave) starts &= (1ull << cnt) - 1ull;
    return PullGroups{s, e, r, bad ? 1 : 0, starts};
}

// ---- the launch of a pull kernel ---------------------------------------------------------------------------------------------

// One of a family's pull kernels over the neighbor-groups a.P.  noun: the family in the messages.  kernel_of(H, L, D): the
// instance for the layout (log_lph, log_lpr) = (H, L), with the mask (D: std::true_type) or without -- attn_drop = 0 keeps every
// edge with k = 1, so the call runs the instances without it.
template <class Args, class KernelOf>
int launch_pull(const char *noun, DeviceState *ds, hipStream_t stream, Args a, int partSize, KernelOf kernel_of)
{
    if (a.P <= 0) return GNNA_OK;
    const ChunkGrid cg = chunk_grid(a.P, partSize, ds->num_cus);
    a.G = cg.G;
    if (cg.blocks > 0x7fffffffll) return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld neighbor-groups in one call", noun, (long long)a.P);
    const dim3 grid((unsigned)cg.blocks);
    auto with_mask = [&](auto D) {
        dispatch_layout(attn_layout(a.heads, a.dim), [&](auto H, auto L) {      // (dim <= kMaxDim: log_lph is never capped)
            hipLaunchKernelGGL(kernel_of(H, L, D), grid, dim3(kBlock), 0, stream, a);
        });
    };
    if (a.drop_thr) with_mask(std::true_type());
    else with_mask(std::false_type());
    return launch_ok("%s launch", noun);
}

// ---- what the entries check alike -------------------------------------------------------------------------------------------

// rect: the rectangular entries name both row counts in their messages.
inline int check_common(const char *what, bool rect, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, int64_t num_parts,
                        int partSize, unsigned flags, unsigned allowed_flags)
{
    if (flags & GNNA_ACCUMULATE) return fail(GNNA_ERR_UNSUPPORTED, "%s: GNNA_ACCUMULATE is not supported", what);
    if (flags & ~allowed_flags) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", what, flags);
    if (num_out_rows < 0 || num_in_rows < 0 || num_parts < 0 || heads < 1 || dim < 1) {
        if (rect)
            return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (num_out_rows=%lld num_in_rows=%lld heads=%d dim=%d num_parts=%lld)",
                        what, (long long)num_out_rows, (long long)num_in_rows, heads, dim, (long long)num_parts);
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (num_nodes=%lld heads=%d dim=%d num_parts=%lld)", what,
                    (long long)num_out_rows, heads, dim, (long long)num_parts);
    }
    if (partSize <= 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must be positive (got %d)", what, partSize);
    const int64_t most = std::max(num_out_rows, num_in_rows);
    if (most >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 536870911): shard the rows", what, (long long)most);
    if (dim > kMaxDim) return fail(GNNA_ERR_UNSUPPORTED, "%s: at most %d floats per head (got %d)", what, kMaxDim, dim);
    if (heads > 64) return fail(GNNA_ERR_UNSUPPORTED, "%s: at most 64 heads (got %d)", what, heads);
    // the gathered rows are added with float atomics: the order of the additions is not fixed
    return deterministic_refused(what, "its rows are added with float atomics");
}

// attn_drop of the drop entries: [0, 1), refused before any device work (a NaN fails the first comparison)
inline int check_drop(const char *what, float attn_drop)
{
    if (!(attn_drop >= 0.f) || attn_drop >= 1.f)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: attn_drop must be in [0, 1) (got %g)", what, (double)attn_drop);
    return GNNA_OK;
}

// the backward entries: no output is an input or another output (a null output is the entry's own check)
template <size_t NI, size_t NO>
int check_alias(const char *what, const void *const (&ins)[NI], const void *const (&outs)[NO])
{
    for (const void *o : outs)
        for (const void *i : ins)
            if (o && o == i) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input", what);
    for (size_t a = 0; a < NO; a++)
        for (size_t b = a + 1; b < NO; b++)
            if (outs[a] && outs[a] == outs[b])
                return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: the outputs must not alias each other", what);
    return GNNA_OK;
}

// ---- what the forward entries do alike ---------------------------------------------------------------------------------------

// gnna_tuning with the hints of the call's graph for rows of W floats (its xcd_remap is not xcd_remap_on(): the hints apply)
inline gnna_tuning hinted_tuning(const int32_t *column_index, int W)
{
    gnna_tuning tune;
    gnna_get_tuning(&tune);
    apply_graph_hints(column_index, W, &tune);
    return tune;
}

// out = max(out, 0) when the call asks for it
inline int relu_epilogue(const char *what, DeviceState *ds, hipStream_t stream, unsigned flags, float *out, int64_t rows, int W,
                         int64_t ld_out)
{
    if (!(flags & GNNA_EPILOGUE_RELU)) return GNNA_OK;
    launch_relu_rows(ds, stream, out, rows, W, ld_out);
    return launch_ok("%s: epilogue launch", what);
}

}  // namespace gat
}  // namespace gnna

#endif  // GNNA_GAT_COMMON_H_

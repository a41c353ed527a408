// gnna_gat_common.h -- what the fused attention kernels of gnna_gat.hip (GAT: a scalar score per node and head) and
// gnna_gatv2.hip (GATv2: the score is a dot product over the gathered row) share: the lane-layout folds, the online (max, sum)
// of the lse passes, the dropout factor and the argument checks of the entries.  Not installed.
#ifndef GNNA_GAT_COMMON_H_
#define GNNA_GAT_COMMON_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

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

// thr = (uint32) floor((double)attn_drop * 2^32) and k = 1 / (1 - attn_drop) in fp32, as gnna_ext.h states them
inline uint32_t drop_threshold(float attn_drop) { return (uint32_t)std::floor((double)attn_drop * 4294967296.0); }
inline float drop_keep_scale(float attn_drop) { return 1.0f / (1.0f - attn_drop); }

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

}  // namespace gat
}  // namespace gnna

#endif  // GNNA_GAT_COMMON_H_

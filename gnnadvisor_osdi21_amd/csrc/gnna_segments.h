// gnna_segments.h -- what the kernels over the contiguous row segments of a batch of graphs share (gnna_pool.hip: sum / mean /
// max / min; gnna_attnpool.hip: attention pooling): the clamped pointers, the search for a tile's first segment, a 64-bit value
// made uniform over a wavefront, the partial store of a lane's four columns; and exp of a non-positive number, which the softmax
// states of gnna_softagg.hip and gnna_attnpool.hip weigh with.  Not installed.
#ifndef GNNA_SEGMENTS_H_
#define GNNA_SEGMENTS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gnna_gat_common.h"     // gat::VT, gat::MT

namespace gnna {
namespace seg {

// graph_pointers[g] clamped to [0, N]; the same value in every lane of a wavefront whose lanes ask for the same g
__device__ __forceinline__ int64_t seg_ptr(const int32_t *__restrict__ gp, int64_t N, int64_t g)
{
    const int64_t v = gp[g];
    return v < 0 ? 0 : (v > N ? N : v);
}

// the first segment whose end lies beyond row r (G: none): where the walk of a tile that begins at r starts
__device__ __forceinline__ int64_t first_segment(const int32_t *__restrict__ gp, int64_t G, int64_t N, int64_t r)
{
    int64_t lo = 0, hi = G;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (seg_ptr(gp, N, mid + 1) > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the first n4 (<= 4) floats of v to q
__device__ __forceinline__ void store_piece(float *__restrict__ q, const gat::VT v, int n4)
{
    if (n4 >= 4) {
        *reinterpret_cast<gat::MT *>(q) = v;
        return;
    }
    if (n4 > 0) q[0] = v[0];
    if (n4 > 1) q[1] = v[1];
    if (n4 > 2) q[2] = v[2];
}

// exp(d) for d <= 0 (and -inf -> 0): one v_exp_f32.  The product d * log2(e) is rounded once, an error of at most |d| * 2^-24 in
// the exponent, i.e. |d| * e^d * 2^-24 <= 2^-24 / e in the value: every use is a weight relative to a maximum of 1, where that is
// below half an ulp of the largest weight.
__device__ __forceinline__ float exp_nonpos(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }

}  // namespace seg
}  // namespace gnna

#endif  // GNNA_SEGMENTS_H_

// gnna_keys.h -- the 64-bit keys of the neighbor max / min, shared by gnna_reduce.hip (one extreme per call) and gnna_stats.hip
// (both extremes next to the moments): the key of an edge is
//       (order(x) << 32) | (0xFFFFFFFF - edge position)
// where order() maps the 32 bits of a float to an unsigned that orders like the float (inverted for min).  The largest key
// holds the extreme value and, among equal values, the smallest edge position.  No edge produces the key 0 (positions are
// below 2^31, so the low word is at least 0x80000000): 0 means "no edge has been seen".  Not installed.
#ifndef GNNA_KEYS_H_
#define GNNA_KEYS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gnna.h"

namespace gnna {

typedef unsigned long long u64;
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));    // global_load_dwordx4 needs dword alignment only

// the bits of a float -> an unsigned that orders like the float (OP = GNNA_REDUCE_MIN: in the opposite order)
template <int OP>
__device__ __forceinline__ uint32_t order_of(float v)
{
    const uint32_t b = __float_as_uint(v);
    const uint32_t m = (uint32_t)((int32_t)b >> 31);
    if constexpr (OP == GNNA_REDUCE_MAX) return b ^ (m | 0x80000000u);
    else return b ^ (~m & 0x7fffffffu);
}
__device__ __forceinline__ float value_of(uint32_t k, int op)
{
    if (op != GNNA_REDUCE_MAX) k = ~k;
    return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k);
}

__device__ __forceinline__ u64 pack(uint32_t hi, uint32_t lo) { return ((u64)hi << 32) | lo; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

// max of the key over the lane pair (l, l ^ STRIDE), in both lanes
template <int STRIDE>
__device__ __forceinline__ u64 pair_max(u64 k)
{
    const uint32_t hi = (uint32_t)(k >> 32), lo = (uint32_t)k;
    if constexpr (STRIDE == 32) {
        auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        return umax64(pack(h[0], l[0]), pack(h[1], l[1]));      // (own, partner) or (partner, own): the same order in both words
    } else if constexpr (STRIDE == 16) {
        auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        return umax64(pack(h[0], l[0]), pack(h[1], l[1]));
    } else {
        return umax64(k, pack((uint32_t)__shfl_xor((int)hi, STRIDE), (uint32_t)__shfl_xor((int)lo, STRIDE)));
    }
}

// max of the key over the R = 64 / LPR lanes that share lane % LPR (the partial rows of a wavefront), in every lane
template <int R>
__device__ __forceinline__ u64 partial_rows_max(u64 k)
{
    if constexpr (R >= 2) k = pair_max<32>(k);
    if constexpr (R >= 4) k = pair_max<16>(k);
    if constexpr (R >= 8) k = pair_max<8>(k);
    if constexpr (R >= 16) k = pair_max<4>(k);
    if constexpr (R >= 32) k = pair_max<2>(k);
    if constexpr (R >= 64) k = pair_max<1>(k);
    return k;
}

// the value (0 for the key 0) and the edge position (-1) a key stands for
__device__ __forceinline__ void key_result(u64 k, int op, float *v, int32_t *pos)
{
    *v = 0.f;
    *pos = -1;
    if (k != 0ull) {
        *v = value_of((uint32_t)(k >> 32), op);
        *pos = (int32_t)(0xFFFFFFFFu - (uint32_t)k);
    }
}

}  // namespace gnna

#endif

// gnna_convert16.h -- the exact conversions between fp32 registers and bf16 / fp16 storage that the 16-bit kernels share
// (gnna_x16.hip, gnna_dot_rows_x16.hip): widening is exact in both formats, narrowing rounds to nearest even.  TYPE is GNNA_BF16 or
// GNNA_F16 (gnna.h).  Not installed.
#ifndef GNNA_CONVERT16_H_
#define GNNA_CONVERT16_H_

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#include "gnna.h"

namespace gnna {
namespace cvt16 {

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

}  // namespace cvt16
}  // namespace gnna

#endif

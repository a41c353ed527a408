// gnna_prepass.h -- the passes in front of an aggregation kernel as device functions of (block index within the pass, blocks
// of the pass, threads of a block): the staging copy, the output fill with the partition validation, the packed-id sample check
// and the hub-row split of the dense block.  None of them reads what another writes, so prepass_kernel (gnna_agg.hip) runs them
// as block ranges of ONE launch; scale_rows_kernel, prologue_kernel (gnna_agg.hip) and hub_split_kernel (gnna_dense.hip) are
// thin wrappers around the same bodies for the paths that launch one pass alone.  CDNA4 / gfx950 only.
#ifndef GNNA_PREPASS_H_
#define GNNA_PREPASS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gnna_device.h"

namespace gnna {

// ---- staging copy / GCN pre-scaling: Xs[j, :] = deg[j] * X[j, :] ----------------------------------------------------------
// Lets the degree-weighted aggregation run as an unweighted gather of Xs with one multiply by deg[i] at the flush
// (deg_i * sum_j deg_j x_j), instead of one extra 4-byte gather plus a broadcast and a multiply per edge.
// Xs[r, 0:D] = (deg ? deg[r] : 1) * X[r, 0:D]; rows of X `ld_in`, rows of Xs `ld_out` floats apart (pads never read, except by
// the 4-float loads of rows narrower than 4 floats, whose padding lanes are never stored)
__device__ __forceinline__ void stage_rows(const float *__restrict__ X, int64_t ld_in, const float *__restrict__ deg,
                                           float *__restrict__ Xs, int64_t rows, int D, int ld_out, unsigned block, unsigned blocks,
                                           unsigned threads)
{
    const size_t tid = (size_t)block * threads + threadIdx.x;
    const size_t nthreads = (size_t)blocks * threads;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const bool aligned = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Xs)) & 15) == 0;
    if (ld_out == D && ld_in == D && (D & 3) == 0 && aligned) {
        const size_t n4 = ((size_t)rows * (size_t)D) >> 2;
        const int d4 = D >> 2;
        for (size_t i = tid; i < n4; i += nthreads) {
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(X) + i);
            reinterpret_cast<f32x4 *>(Xs)[i] = deg ? v * deg[i / d4] : v;
        }
    } else if ((D & 3) == 0 && (ld_out & 3) == 0 && (ld_in & 3) == 0 && aligned) {
        // padded / gapped layouts of rows whose width is a whole number of 16-byte pieces: one vector per thread
        const size_t n4 = ((size_t)rows * (size_t)D) >> 2;
        const unsigned d4 = (unsigned)D >> 2;
        const size_t ldo4 = (size_t)ld_out >> 2, ldi4 = (size_t)ld_in >> 2;
        for (size_t i = tid; i < n4; i += nthreads) {
            const size_t r = i / d4, c4 = i - r * d4;
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(X) + r * ldi4 + c4);
            reinterpret_cast<f32x4 *>(Xs)[r * ldo4 + c4] = deg ? v * deg[r] : v;
        }
    } else {
        const size_t total = (size_t)rows * (size_t)D;
        for (size_t i = tid; i < total; i += nthreads) {
            const size_t r = i / (unsigned)D, cc = i - r * (unsigned)D;
            const float v = __builtin_nontemporal_load(X + r * (size_t)ld_in + cc);
            Xs[r * (size_t)ld_out + cc] = deg ? v * deg[r] : v;
        }
    }
}

// ---- packed ids of a prepared graph: does column_index still look like the array the copy was made from? -------------------
// (1024 samples: catches a buffer that was rewritten, which is what happens when a promise of immutability is broken by
// accident.)  One block of its own, so that the zero-fill does not wait behind the sampled loads.
__device__ __forceinline__ void check_packed_ids(const int32_t *__restrict__ chk_ids, int64_t chk_n, const int32_t *__restrict__ pp,
                                                 int64_t P, const unsigned long long *__restrict__ chk_sum, int32_t *stale_flag,
                                                 int32_t seq)
{
    if (threadIdx.x < kWave) {
        const unsigned long long then = chk_sum[0], distrusted = chk_sum[4];   // [4]: a full hash differed earlier (gnna_stream.hip)
        const unsigned long long now = graph_checksum(chk_ids, chk_n, pp, P, (int)threadIdx.x);
        if (threadIdx.x == 0 && (now != then || distrusted != 0ull)) *stale_flag = seq;
    }
}

// ---- zero-fill + partition validation -------------------------------------------------------------------------------------
__device__ __forceinline__ void fill_and_validate(float *__restrict__ Y, size_t n_floats, int D, int ldy,
                                                  const int32_t *__restrict__ p2n, const int32_t *__restrict__ pp, int64_t P,
                                                  int32_t *flag, int32_t seq, int validate, int zero_fill,
                                                  uint32_t *__restrict__ clear_words, int n_clear, unsigned block, unsigned blocks,
                                                  unsigned threads)
{
    // the step counters of the sweep kernel behind this launch (<= kBlock words): cleared here instead of by a launch of their own
    if (block == 0 && (int)threadIdx.x < n_clear) clear_words[threadIdx.x] = 0u;
    const size_t tid = (size_t)block * threads + threadIdx.x;
    const size_t nthreads = (size_t)blocks * threads;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (!zero_fill) {
        // accumulate mode: Y keeps its contents
    } else if (ldy != D) {
        // rows `ldy` floats apart (the caller's leading dimension): only the D floats of every row are the library's
        if ((D & 3) == 0 && (ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0) {
            const size_t n4 = n_floats >> 2;
            const unsigned d4 = (unsigned)D >> 2, ld4 = (unsigned)ldy >> 2;
            const f32x4 z = (f32x4)(0.f);
            for (size_t i = tid; i < n4; i += nthreads) {
                const size_t r = i / d4;
                reinterpret_cast<f32x4 *>(Y)[r * ld4 + (i - r * d4)] = z;
            }
        } else {
            for (size_t i = tid; i < n_floats; i += nthreads) {
                const size_t r = i / (unsigned)D;
                Y[r * (size_t)ldy + (i - r * (unsigned)D)] = 0.f;
            }
        }
    } else if ((reinterpret_cast<uintptr_t>(Y) & 15) == 0) {
        const size_t n4 = n_floats >> 2;
        f32x4 *Y4 = reinterpret_cast<f32x4 *>(Y);
        const f32x4 z = (f32x4)(0.f);
        for (size_t i = tid; i < n4; i += nthreads) Y4[i] = z;
        for (size_t i = (n4 << 2) + tid; i < n_floats; i += nthreads) Y[i] = 0.f;
    } else {
        for (size_t i = tid; i < n_floats; i += nthreads) Y[i] = 0.f;
    }
    if (validate) {
        bool bad = false;
        for (int64_t g = (int64_t)tid; g < P; g += (int64_t)nthreads) {
            if (pp[g + 1] < pp[g]) bad = true;
            if (g + 1 < P && p2n[g + 1] < p2n[g]) bad = true;
        }
        if (bad) *flag = seq;  // every writer stores the same value
    }
}

// ---- the hub-row split of the dense block (gnna_dense.hip) ----------------------------------------------------------------
typedef typename VecOf<4>::T HubVT;
typedef int HubIT __attribute__((ext_vector_type(4)));
typedef uint32_t HubU4 __attribute__((ext_vector_type(4)));
typedef uint32_t HubU2 __attribute__((ext_vector_type(2)));

// The split image of a call: per 128-rank chunk [piece 3][32-rank step 4][column tile 4] fragments.  A fragment is the B operand
// of one MFMA, 64 lanes x 16 bytes, lane-linear: lane 16 kg + n holds the 8 ranks 8 kg .. 8 kg + 7 of the step at column n of
// the tile.  48 KB per chunk, H_pad * 384 bytes in all (dense_image_bytes).
constexpr int kHubFrag = 1024;
constexpr int kHubPiece = 16 * kHubFrag; // bytes between the hi, mid and lo pieces of a chunk (4 steps x 4 column tiles)
constexpr int kHubImage = 3 * kHubPiece; // 49,152 bytes per chunk
constexpr int kSplitThreads = 128;       // the threads of one 32-rank step of the split
constexpr int kSplitLdsBytes = 3 * 4 * kHubFrag;   // the LDS image of a step: 12 KB

// x = hi + mid + lo exactly, each with 8 significant bits in the upper half of its word (a bf16 value): hi is x truncated, mid
// the truncated remainder, lo what is left of at most 24 bits; both subtractions are exact.  A non-finite x is in hi, with NaN
// for mid and lo (the header of gnna_dense.hip: the end of hub_block_kernel deals with it).
// (A lo below 2^-126 is a bf16 subnormal whose low bits, and possibly all of it, are dropped: less than 2^-126 per term.)
__device__ __forceinline__ void hub_split(uint32_t x, uint32_t &hi, uint32_t &mid, uint32_t &lo)
{
    hi = x & 0xffff0000u;
    const float r = __uint_as_float(x) - __uint_as_float(hi);
    mid = __float_as_uint(r) & 0xffff0000u;
    lo = __float_as_uint(r - __uint_as_float(mid));
}

// the upper halves of two words as one: `first` below `second`
__device__ __forceinline__ uint32_t hub_pack(uint32_t first, uint32_t second) { return __builtin_amdgcn_perm(second, first, 0x07060302u); }

// The three bf16 pieces of the hub rows of the call's X, ONCE per call (before, each of the block's workgroups split every row
// on its way to LDS: 256 times per value).  128 threads take a 32-rank step: thread (g, pc) fetches 4 columns of the 4
// consecutive ranks 4 g .. 4 g + 3 (their ids are one 16-byte load), splits the 16 values and writes, per column and piece, the
// 4 ranks as 8 bytes into an LDS image of the step (split_step_to_lds); behind a barrier of the caller the image goes out 16
// bytes per lane, 4 KB per piece (split_step_from_lds).  A padding rank and the columns from D on are zeros.  FULL: D and ldx
// are multiples of 4 and X is 16-byte aligned, so every 16-byte piece of a row is whole and aligned; otherwise the elements are
// fetched one by one.  deg: the pre-scaled GCN form gathers deg[j] * X[j, :], so the split is of that product -- the one
// multiply of stage_rows, hence the bits of a split of the staged copy.
template <bool FULL>
__device__ __forceinline__ void split_step_to_lds(const float *__restrict__ X, int ldx, const float *__restrict__ deg,
                                                  const int32_t *__restrict__ r2n, int D, unsigned char *s_img, int step, int t)
{
    const int g = t >> 4, pc = t & 15;
    const HubIT node = *reinterpret_cast<const HubIT *>(&r2n[step * 32 + 4 * g]);
    HubVT v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int nd = node[k];
        const float *src = X + (size_t)(nd < 0 ? 0 : nd) * (size_t)ldx + 4 * pc;
        HubVT x = (HubVT)(0.f);
        if (nd >= 0) {
            if constexpr (FULL) {
                if (4 * pc < D) x = *reinterpret_cast<const HubVT *>(src);
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (4 * pc + q < D) x[q] = src[q];
            }
            if (deg) {                   // (the columns from D on stay zeros whatever the factor is)
                const float f = deg[nd];
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (4 * pc + q < D) x[q] = x[q] * f;
            }
        }
        v[k] = x;
    }
    const int wbase = (pc >> 2) * kHubFrag + (16 * (g >> 1) + 4 * (pc & 3)) * 16 + 8 * (g & 1);
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
        // column cc of the thread's 4 x 4 values: split, packed by rank pairs, 8 bytes per piece
        uint32_t pk[3][2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t a[3], b[3];
            hub_split(__float_as_uint(v[2 * h][cc]), a[0], a[1], a[2]);
            hub_split(__float_as_uint(v[2 * h + 1][cc]), b[0], b[1], b[2]);
#pragma unroll
            for (int i = 0; i < 3; i++) pk[i][h] = hub_pack(a[i], b[i]);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            HubU2 o;
            o[0] = pk[i][0];
            o[1] = pk[i][1];
            *reinterpret_cast<HubU2 *>(&s_img[wbase + i * 4 * kHubFrag + cc * 16]) = o;
        }
    }
}

__device__ __forceinline__ void split_step_from_lds(unsigned char *__restrict__ img, const unsigned char *s_img, int step, int t)
{
    unsigned char *out = img + (size_t)(step >> 2) * kHubImage + (size_t)(step & 3) * 4 * kHubFrag;
#pragma unroll
    for (int u = 0; u < kSplitLdsBytes / 16 / kSplitThreads; u++) {
        const int idx = u * kSplitThreads + t;
        const int i = idx >> 8, off = (idx & 255) * 16;
        *reinterpret_cast<HubU4 *>(&out[i * kHubPiece + off]) = *reinterpret_cast<const HubU4 *>(&s_img[i * 4 * kHubFrag + off]);
    }
}

}  // namespace gnna

#endif  // GNNA_PREPASS_H_

// gnna_dense.hip -- the dense hub-to-hub block of a prepared graph.  CDNA4 / gfx950 only.
//
// A power-law graph whose node pairs are deduplicated has a nearly full corner: for two hubs the expected number of drawn
// pairs exceeds one, so almost every hub is a neighbour of almost every other hub.  Those edges cost the gather two
// 128-byte requests each (gnna_sweep.hip) and carry one bit of information.  gnna_prepare_graph therefore splits the
// adjacency of a swept graph as A = A_res + A_hub:
//
//   * A_hub is the H x H block of the hubs (the nodes of degree >= theta, ranked by node id) as a BITMAP of H_pad^2 / 8 bytes
//     (8 MB at 8,192 hubs, 32 MB at 16,384).  A 32 x 32 tile of it is 64 16-bit halves, half l = (dst % 16) + 16 * (src % 32 / 8)
//     holding bit (src % 8) + 8 * (dst % 32 / 16): byte t of half l is what lane l of a wavefront needs of the A operand of
//     v_mfma_f32_16x16x32_bf16 for the tile's t-th 16 destination ranks (element j of the lane = source rank 8 (l / 16) + j);
//   * A_res is everything else, as a residual graph with the caller's part2Node and group count: new part_pointers
//     (groups only shrink; some become empty) and a compacted column_index.  The sweep kernel runs on it;
//   * hub_block_kernel then adds Y[node(i), :] += scale(i) * sum_j bit(i, j) * X[node(j), :] with bf16 MFMA on an EXACT
//     three-way split of X.  A fp32 value is the sum of three bf16 values: hi = x with its low 16 bits cleared, mid = (x - hi)
//     with its low 16 bits cleared, lo = x - hi - mid.  Each has 8 significant bits and both subtractions are exact (24 = 8 +
//     8 + 8 bits; a remainder has its leading bit lower, never more bits).  The bitmap operand is 0 or 1, so every product is
//     exact, and what is rounded are fp32 sums as before: the hi products in one accumulator (one rounding per 32 source
//     ranks, however the matrix unit adds inside an instruction), the mid and lo products -- 2^-8 and 2^-16 of them -- in
//     another, the two added once at the end.  (A lo piece below 2^-126 is a bf16 subnormal and may be dropped: an error
//     below 2^-126 per term.)  The split is made ONCE per call, ahead of the sweep kernel, by the split role of the pre-pass
//     launch (prepass_kernel, gnna_agg.hip; hub_split_kernel where the pass is a launch of its own: GNNA_PREPASS=0): the three
//     pieces of the hub rows of that call's X, in the order of the MFMA's B operand, in the scratch of the call's stream
//     (3 MB at 8,192 hubs, 6 MB at 16,384).  hub_block_kernel loads its operands from that image and does no arithmetic on X.
//
// Multiplicity: the C ABI accepts rows with repeated ids.  The edge that finds its bit already set (atomicOr) is a repeat
// and stays in the residual; that decision is recorded once per edge in a bit array, which the count pass and the fill
// pass of the residual both read.
//
// Everything is built inside gnna_prepare_graph and hangs on the slice plan of the caller's graph (gnna_stream.hip): it is
// released with it.  The residual graph is itself a (pinned) slice plan -- counts, statistics and the packed ids of the
// swept phase count are made by the code that makes them for any graph.
//
// Stale ids: the guard of the packed copy keeps watching the caller's arrays.  On a call that finds them changed the sweep
// kernel reads the caller's arrays and hub_block_kernel returns at once (and so does hub_split_kernel; the split role of the
// pre-pass cannot see the flag its own launch raises and writes an image that nobody reads).
//
// Environment, read at every gnna_prepare_graph: GNNA_DENSE_BLOCK = 0 never / 1 (default) the rule of gnna_agg.hip / 2 any
// prepared graph whose call sweeps (tests); GNNA_DENSE_BLOCK_THETA = the degree threshold, under mode 2 only (tests: a hub count
// of their choosing); GNNA_DENSE_BLOCK_TILE = 32 | 64, under mode 2 only: the destination ranks per workgroup of
// hub_block_kernel (tests and scans; otherwise dense_tile_ranks decides); GNNA_DENSE_BLOCK_LOG = 1 prints the block taken
// (theta, H, entries, density) to stderr.
//
// Non-finite features: 0 * Inf is NaN, so an Inf or NaN in the features of one hub reaches every hub's row through the
// block, not only its neighbours' (the gather would hand it to the neighbours alone): 1 * Inf at the neighbours, NaN at the
// others.  The split leaves a non-finite x in hi (its mid and lo are NaN); every source rank is multiplied into every
// row, so a finite hi sum says that no source was non-finite, an infinite one is the result, and a wavefront adds its mid/lo
// sum only to a hi sum that is not infinite.  (A NaN whose payload lies in its low 16 bits alone is taken for an infinity.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gnna.h"
#include "gnna_device.h"
#include "gnna_internal.h"
#include "gnna_prepass.h"

namespace gnna {
namespace {

constexpr int kHubBuckets = 64;          // half-octave degree buckets
constexpr int kHubMax = 16384;           // most hubs of a block
constexpr int kHubThreads = 512;         // hub_block_kernel: 8 wavefronts
constexpr int kHubWaves = kHubThreads / kWave;
constexpr int kHubTileM = kDenseTileRanks;    // destination ranks per workgroup of the short tile (two 16-rank MFMA tiles); the tall one: twice
constexpr int kHubKC = kDenseChunkRanks;      // source ranks of a chunk (one step per wavefront of a column half); the ranks are padded to a multiple of it
static_assert(kHubTileM == 32, "a tile row of the bitmap per 32 destination ranks");
static_assert(kHubKC % (2 * kHubTileM) == 0 && (kHubTileM * 64) % kHubThreads == 0, "whole tiles per chunk, elements per thread");
static_assert(kDenseMaxDim <= 64, "the split image holds 64 columns");

// Half-octave bucket of a degree: 2 k for 2^k <= d < sqrt(2) 2^k, 2 k + 1 for sqrt(2) 2^k <= d < 2^(k + 1); 0 for d <= 1.
// Monotone in d, so "bucket >= b" is "degree >= theta_b".
__host__ __device__ inline int hub_bucket(int64_t d)
{
    if (d <= 1) return 0;
    int k = 0;
    while ((d >> (k + 1)) != 0) k++;
    const int b = 2 * k + ((d * d >= ((int64_t)1 << (2 * k + 1))) ? 1 : 0);
    return b < kHubBuckets ? b : kHubBuckets - 1;
}

// deg[row] = edges of the row (all its neighbor-groups)
__global__ void __launch_bounds__(kBlock)
hub_degree_kernel(const int32_t *__restrict__ pp, const int32_t *__restrict__ p2n, int64_t P, int64_t N, int32_t *__restrict__ deg)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < P; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = p2n[g];
        const int len = pp[g + 1] - pp[g];
        if (r >= 0 && r < N && len > 0) atomicAdd(&deg[r], len);
    }
}

// hist[b] = nodes whose degree falls in bucket b; hist[64 + b] = edges whose min(deg[dst], deg[src]) falls in bucket b.
// Suffix sums give H(theta) and the entries of the H x H block for every bucket threshold at once.
__global__ void __launch_bounds__(kBlock)
hub_hist_kernel(const int32_t *__restrict__ col, const int32_t *__restrict__ pp, const int32_t *__restrict__ p2n, int64_t P, int64_t N,
                const int32_t *__restrict__ deg, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int s_h[2 * kHubBuckets];
    for (int i = threadIdx.x; i < 2 * kHubBuckets; i += kBlock) s_h[i] = 0u;
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < N; i += nthreads) atomicAdd(&s_h[hub_bucket(deg[i])], 1u);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = tid >> 6, nwaves = nthreads >> 6;
    for (int64_t g = wave; g < P; g += nwaves) {
        const int64_t r = p2n[g];
        if (r < 0 || r >= N) continue;
        const int dd = deg[r];
        const int a = pp[g], b = pp[g + 1];
        for (int e = a + lane; e < b; e += kWave) {
            const int64_t s = col[e];
            if (s < 0 || s >= N) continue;
            const int ds = deg[s];
            atomicAdd(&s_h[kHubBuckets + hub_bucket(dd < ds ? dd : ds)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * kHubBuckets; i += kBlock)
        if (s_h[i]) atomicAdd(&hist[i], (unsigned long long)s_h[i]);
}

// list[0 .. count) = the nodes of degree >= theta (any order; at most `cap` are stored)
__global__ void __launch_bounds__(kBlock)
hub_list_kernel(const int32_t *__restrict__ deg, int64_t N, int theta, int32_t *__restrict__ count, int32_t *__restrict__ list, int cap)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (deg[i] >= theta) {
            const int idx = atomicAdd(count, 1);
            if (idx < cap) { list[idx] = (int32_t)i; list[cap + idx] = deg[i]; }
        }
    }
}

__global__ void __launch_bounds__(kBlock)
hub_rank_kernel(const int32_t *__restrict__ r2n, int H, int64_t N, int32_t *__restrict__ n2r)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H && r2n[i] >= 0 && r2n[i] < N) n2r[r2n[i]] = i;
}

// The block's bitmap.  One wavefront per neighbor-group of a hub row; the first edge to set a bit is taken out of the
// gather (taken[e] = 1), every later edge with the same (dst, src) finds the bit set and stays in the residual.
__global__ void __launch_bounds__(kBlock)
hub_bitmap_kernel(const int32_t *__restrict__ col, const int32_t *__restrict__ pp, const int32_t *__restrict__ p2n, int64_t P, int64_t N,
                  const int32_t *__restrict__ n2r, int steps, uint32_t *__restrict__ bm,
                  uint32_t *__restrict__ taken, unsigned long long *__restrict__ total)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned int mine = 0;
    for (int64_t g = wave; g < P; g += nwaves) {
        const int64_t r = p2n[g];
        if (r < 0 || r >= N) continue;
        const int rd = n2r[r];
        if (rd < 0) continue;                                        // (wave-uniform)
        const int a = pp[g], b = pp[g + 1];
        for (int e = a + lane; e < b; e += kWave) {
            const int64_t s = col[e];
            if (s < 0 || s >= N) continue;
            const int rs = n2r[s];
            if (rs < 0) continue;
            const size_t half = ((size_t)(rd >> 5) * (size_t)steps + (size_t)(rs >> 5)) * 64 + (size_t)((rd & 15) + 16 * ((rs & 31) >> 3));
            const uint32_t bit = 1u << (16 * (int)(half & 1) + 8 * ((rd >> 4) & 1) + (rs & 7));
            const uint32_t old = atomicOr(&bm[half >> 1], bit);
            if (!(old & bit)) {
                atomicOr(&taken[(uint32_t)e >> 5], 1u << (e & 31));
                mine++;
            }
        }
    }
    unsigned long long sum = mine;
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0 && sum) atomicAdd(total, sum);
}

__device__ __forceinline__ bool hub_taken(const uint32_t *__restrict__ taken, int e)
{
    return (taken[(uint32_t)e >> 5] >> (e & 31)) & 1u;
}

// res_pp[g] = edges of group g that stay in the gather (res_pp[P] = 0: the exclusive scan behind this makes it the total)
__global__ void __launch_bounds__(kBlock)
hub_res_count_kernel(const int32_t *__restrict__ pp, int64_t P, const uint32_t *__restrict__ taken, int32_t *__restrict__ res_pp)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= P; g += (int64_t)gridDim.x * blockDim.x) {
        int n = 0;
        if (g < P) {
            const int a = pp[g], b = pp[g + 1];
            for (int e = a; e < b; e++) n += hub_taken(taken, e) ? 0 : 1;
        }
        res_pp[g] = n;
    }
}

// res_col[res_pp[g] ..] = the ids of group g that stay, in their order (one wavefront per group)
__global__ void __launch_bounds__(kBlock)
hub_res_fill_kernel(const int32_t *__restrict__ col, const int32_t *__restrict__ pp, int64_t P, const uint32_t *__restrict__ taken,
                    const int32_t *__restrict__ res_pp, int32_t *__restrict__ res_col, int64_t res_nnz)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t g = wave; g < P; g += nwaves) {
        const int a = pp[g], b = pp[g + 1];
        int64_t at = res_pp[g];
        for (int e0 = a; e0 < b; e0 += kWave) {
            const int e = e0 + lane;
            const bool keep = e < b && !hub_taken(taken, e);
            const unsigned long long K = __ballot(keep);
            const int64_t dst = at + __popcll(K & below);
            if (keep && dst < res_nnz) res_col[dst] = col[e];
            at += __popcll(K);
        }
    }
}

// ---- the block itself ---------------------------------------------------------------------------------------------
struct HubParams {
    float *Y;
    const int32_t *r2n;                  // [H_pad] rank -> node, -1 for the padding ranks
    const uint16_t *bm;                  // [H_pad / 32][H_pad / 32][64] halves (the header of this file)
    const unsigned char *img;            // the call's split image (hub_split_kernel)
    const float *row_scale;
    const int32_t *stale;
    int32_t seq;
    int H_pad, D, ldy;
    int scaled;                          // MODE_GIN: rows are multiplied by eps (* row_scale[row])
    float eps;
};

struct SplitParams {
    const float *X;
    const int32_t *r2n;
    unsigned char *img;
    const int32_t *stale;
    int32_t seq;
    int D, ldx;
};

typedef __bf16 HubFrag __attribute__((ext_vector_type(8)));
static_assert(kHubKC == 128 && kHubTileM == 32 && kHubWaves == 8, "the shape hub_block_kernel is written for");
// (HubVT, HubIT, HubU4, HubU2, the geometry of the split image -- kHubFrag, kHubPiece, kHubImage -- and hub_split / hub_pack:
// gnna_prepass.h, beside the split's body)

// 8 bitmap bits -> 8 bf16 of 0 or 1 (0x3f80), element j from bit j
__device__ __forceinline__ HubFrag hub_ones(uint32_t bits)
{
    const uint32_t y = bits | (bits << 15);          // bit j at j and at j + 15: bits 2 i and 2 i + 1 are 16 apart
    HubU4 v;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = ((y >> (2 * i)) & 0x10001u) * 0x3f80u;
    return __builtin_bit_cast(HubFrag, v);
}

// The split pass on its own (a caller's gapped layout under GNNA_PREPASS=0; otherwise the split is a block range of
// prepass_kernel, gnna_agg.hip): one workgroup of 128 threads per 32-rank step, the body of gnna_prepass.h.
template <bool FULL>
__global__ void __launch_bounds__(kSplitThreads)
hub_split_kernel(const SplitParams p)
{
    if (*p.stale == p.seq) return;       // the ids changed since the block was made: hub_block_kernel returns at once as well
    __shared__ __attribute__((aligned(16))) unsigned char s_img[kSplitLdsBytes];
    const int t = (int)threadIdx.x;
    const int step = (int)blockIdx.x;
    split_step_to_lds<FULL>(p.X, p.ldx, nullptr, p.r2n, p.D, s_img, step, t);
    __syncthreads();
    split_step_from_lds(p.img, s_img, step, t);
}

// A workgroup owns TM destination ranks (TM / 16 MFMA tiles, TM / 32 tile rows of the bitmap) and walks ALL source ranks, 128
// at a time, with v_mfma_f32_16x16x32_bf16: A is 16 destination ranks x 32 source ranks of the bitmap (0 or 1), B is 32 source
// ranks x 16 columns of ONE of the three bf16 pieces of X.  Every product is exact; the hi products are summed in one fp32
// accumulator, the mid and lo products in another, and the two are added once at the end.
//
// The kernel does no arithmetic on X and keeps no image of it in LDS.  The 8 wavefronts split a chunk as (step s = w % 4, column
// half w / 4), and a fragment of the split image IS the B operand of one MFMA: the 3 pieces of a wavefront's 2 column tiles (1
// for the upper half when NT = 3: column tile 3 is never read) are 6 wave-wide 16-byte loads straight into its registers, the
// 8 wavefronts read the chunk's 48 fragments once between them, and nothing is shared before the end -- no barrier in the
// loop.  Each fragment is multiplied with the bitmap bytes of all TM / 16 destination tiles: 12 MFMAs per chunk for TM = 32, 24
// for TM = 64, which halves the bytes of the image a destination rank pulls through the L2.  Three register stages take the
// chunks in turn (chunk c lives in stage c % 3): a piece's fragments are asked for again, three chunks ahead, as soon as its
// MFMAs are issued, so about two chunks (12 KB per wavefront) are on their way at any time.
//
// At the end the four steps' partial tiles are laid side by side in LDS and summed in step order, and the workgroup -- the
// only writer of its TM rows in this launch, behind the sweep kernel of the same call -- adds the tile to Y with plain loads
// and stores: no atomics, and a result that does not depend on timing.  The order in which a destination element's products
// are added is the same for both tile heights.
template <int NT, int TM>
__global__ void __launch_bounds__(kHubThreads)
hub_block_kernel(const HubParams p)
{
    if (*p.stale == p.seq) return;       // the ids changed since the block was made: the sweep kernel does the whole call
    constexpr int TR = TM / 32;          // tile rows of the bitmap
    static_assert((TM == kHubTileM || TM == 2 * kHubTileM) && (NT == 3 || NT == 4), "tile shapes");
    __shared__ __attribute__((aligned(16))) float s_part[4 * TM * 64];
    const int tid = (int)threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = p.H_pad / kHubKC;
    const int steps = p.H_pad >> 5;      // 32-rank steps of a row of the bitmap
    const int D = p.D;
    const int cs = wib & 3, ch = wib >> 2;                  // this wavefront's step of a chunk and its half of the columns
    const bool two = NT == 4 || ch == 0;                    // (wave-uniform) the half has a second column tile
    const unsigned char *frag0 = p.img + (size_t)(cs * 4 + 2 * ch) * kHubFrag + (size_t)lane * 16;
    const uint16_t *word0 = p.bm + ((size_t)blockIdx.x * TR * (size_t)steps + (size_t)cs) * 64 + (size_t)lane;
    struct Stage {
        HubFrag b[2][3];                 // [column tile of the half][piece]
        uint32_t w[TR];                  // this wavefront's step of the bitmap per tile row: byte 0 the first destination tile, byte 1 the second
    };
    // (a chunk beyond the last is the last one again: fetched, never multiplied)
    auto fetch_piece = [&](int c, int i, Stage &st) {
        const unsigned char *src = frag0 + (size_t)(c < chunks ? c : chunks - 1) * kHubImage + i * kHubPiece;
        st.b[0][i] = *reinterpret_cast<const HubFrag *>(src);
        if (two) st.b[1][i] = *reinterpret_cast<const HubFrag *>(src + kHubFrag);
    };
    auto fetch_words = [&](int c, Stage &st) {
        const int cc = c < chunks ? c : chunks - 1;
#pragma unroll
        for (int tr = 0; tr < TR; tr++) st.w[tr] = word0[((size_t)tr * (size_t)steps + (size_t)(cc * 4)) * 64];
    };
    HubVT acc_hi[2 * TR][2], acc_lo[2 * TR][2];             // [destination tile][column tile of the half]
#pragma unroll
    for (int t = 0; t < 2 * TR; t++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc_hi[t][q] = acc_lo[t][q] = (HubVT)(0.f);

    // Chunk c out of stage st, which then starts on chunk c + 3.  A turn is three parts, pinned in this order: the MFMAs of one
    // piece (hi, mid, lo), then the loads that fill that piece's registers again.
    auto turn = [&](int c, Stage &st) {
        HubFrag a[2 * TR];
#pragma unroll
        for (int t = 0; t < 2 * TR; t++) a[t] = hub_ones((st.w[t >> 1] >> (8 * (t & 1))) & 0xffu);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int q = 0; q < 2; q++)
                if (q == 0 || two) {
#pragma unroll
                    for (int t = 0; t < 2 * TR; t++) {
                        if (k == 0) acc_hi[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], st.b[q][0], acc_hi[t][q], 0, 0, 0);
                        else acc_lo[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], st.b[q][k], acc_lo[t][q], 0, 0, 0);
                    }
                }
            fetch_piece(c + 3, k, st);
            __builtin_amdgcn_sched_barrier(0);
        }
        fetch_words(c + 3, st);
        __builtin_amdgcn_sched_barrier(0);
    };
    Stage s0, s1, s2;
    // (the order of the loads is that of the turns, and pinned: the counted waits of the loop are those of its entry as well)
    auto fetch = [&](int c, Stage &st) {
#pragma unroll
        for (int i = 0; i < 3; i++) fetch_piece(c, i, st);
        fetch_words(c, st);
        __builtin_amdgcn_sched_barrier(0);
    };
    fetch(0, s0);
    fetch(1, s1);
    fetch(2, s2);
    int c = 0;
    for (; c + 3 <= chunks; c += 3) {
        turn(c, s0);
        turn(c + 1, s1);
        turn(c + 2, s2);
    }
    if (c < chunks) {
        turn(c, s0);
        if (c + 1 < chunks) turn(c + 1, s1);
    }

    // the 4 partial tiles of the workgroup's TM rows, side by side, then summed in step order
    float *part = s_part;                // [step][TM ranks][64 columns]; the columns from 16 NT on stay unwritten and unread
#pragma unroll
    for (int t = 0; t < 2 * TR; t++)
#pragma unroll
        for (int q = 0; q < 2; q++)
            if (q == 0 || two) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    part[(cs * TM + t * 16 + (lane >> 4) * 4 + r) * 64 + (2 * ch + q) * 16 + (lane & 15)] =
                        __builtin_isinf(acc_hi[t][q][r]) ? acc_hi[t][q][r] : acc_hi[t][q][r] + acc_lo[t][q][r];
            }
    __syncthreads();
    // one plain read-add-write of Y per element
#pragma unroll
    for (int i = 0; i < TM * 64 / kHubThreads; i++) {
        const int idx = i * kHubThreads + tid;
        const int row = idx >> 6, col = idx & 63;
        if (col >= D) continue;
        float sum = part[idx];
#pragma unroll
        for (int s = 1; s < 4; s++) sum += part[s * TM * 64 + idx];
        const int node = p.r2n[(int)blockIdx.x * TM + row];
        if (node < 0 || sum == 0.f) continue;
        float scale = 1.f;
        if (p.scaled) {
            scale = p.eps;
            if (p.row_scale) scale *= p.row_scale[node];
        }
        float *dst = p.Y + (size_t)node * (size_t)p.ldy + col;
        *dst += sum * scale;
    }
}

int smallest_degree_of_bucket(int b)
{
    if (b <= 0) return 0;
    int64_t d = (int64_t)std::floor(std::pow(2.0, b / 2.0)) - 2;
    if (d < 1) d = 1;
    while (hub_bucket(d) < b) d++;
    return (int)std::min<int64_t>(d, 0x7fffffff);
}

struct DenseTemp {
    void *ptr = nullptr;
    ~DenseTemp() { if (ptr) { (void)hipFree(ptr); count_event(CTR_LAUNCH_FREES); } }
};

}  // namespace

int dense_block_mode()
{
    const char *s = std::getenv("GNNA_DENSE_BLOCK");
    if (!s || !*s) return 1;
    const int v = std::atoi(s);
    return v == 0 ? 0 : (v == 2 ? 2 : 1);
}

int build_dense_block(DeviceState *ds, hipStream_t stream, const int32_t *col, const int32_t *pp, const int32_t *p2n, int64_t P,
                      int64_t N, int64_t nnz, int mode, DenseBlock *out)
{
    *out = DenseBlock();
    if (mode == 0 || P <= 0 || N <= 0 || nnz <= 0 || nnz > 0x7fffffffLL || N > 0x7fffffffLL) return GNNA_OK;
    // ---- degrees and the two histograms ----
    const size_t deg_b = align256((size_t)N * 4), hist_b = align256(2 * kHubBuckets * 8), cnt_b = 256;
    const size_t list_b = align256((size_t)kHubMax * 8), taken_b = align256((((size_t)nnz + 31) / 32 + 1) * 4);
    const size_t part_b = align256((size_t)std::max<int64_t>(1, scan_tiles(P + 1)) * 4), n2r_b = align256((size_t)N * 4);
    DenseTemp tmp;           // (scratch of the build, the node -> rank map included: freed on return)
    hipError_t e = hipMalloc(&tmp.ptr, deg_b + hist_b + cnt_b + list_b + taken_b + part_b + n2r_b);
    count_event(CTR_LAUNCH_MALLOCS);
    if (e != hipSuccess) { tmp.ptr = nullptr; (void)hipGetLastError(); return GNNA_OK; }       // no memory: no block
    char *base = static_cast<char *>(tmp.ptr);
    int32_t *deg = reinterpret_cast<int32_t *>(base);
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(base + deg_b);
    int32_t *hub_count = reinterpret_cast<int32_t *>(base + deg_b + hist_b);
    unsigned long long *taken_total = reinterpret_cast<unsigned long long *>(base + deg_b + hist_b + 8);
    int32_t *hub_list = reinterpret_cast<int32_t *>(base + deg_b + hist_b + cnt_b);
    uint32_t *taken = reinterpret_cast<uint32_t *>(base + deg_b + hist_b + cnt_b + list_b);
    int32_t *partial = reinterpret_cast<int32_t *>(base + deg_b + hist_b + cnt_b + list_b + taken_b);
    int32_t *n2r = reinterpret_cast<int32_t *>(base + deg_b + hist_b + cnt_b + list_b + taken_b + part_b);
    (void)hipMemsetAsync(tmp.ptr, 0, deg_b + hist_b + cnt_b + list_b + taken_b, stream);
    const unsigned gblocks = elementwise_grid(P, ds->num_cus, 8);
    const unsigned wblocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((P + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ds->num_cus * 16));
    hipLaunchKernelGGL(hub_degree_kernel, dim3(gblocks), dim3(kBlock), 0, stream, pp, p2n, P, N, deg);
    hipLaunchKernelGGL(hub_hist_kernel, dim3(wblocks), dim3(kBlock), 0, stream, col, pp, p2n, P, N, deg, hist);
    unsigned long long h[2 * kHubBuckets];
    e = hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(GNNA_ERR_HIP, "dense block (histograms): %s", hipGetErrorString(e));

    // ---- theta: the bucket threshold with the largest modelled saving ----
    int best_b = -1;
    double best_gain = 0.0;
    double Hs = 0.0, Es = 0.0;
    int fallback_b = -1;
    for (int b = kHubBuckets - 1; b >= 1; b--) {
        Hs += (double)h[b];
        Es += (double)h[kHubBuckets + b];
        if (Hs <= 0.0) continue;
        if (Hs > (double)kHubMax) break;
        if (Es > 0.0) fallback_b = b;
        const double gain = dense_block_saving(Hs, Es, ds->num_cus);
        const bool ok = mode == 2 ? Es > 0.0 : dense_block_pays(gain, Es, (double)nnz);
        if (ok && (best_b < 0 || gain > best_gain)) { best_b = b; best_gain = gain; }
    }
    int theta = best_b >= 0 ? smallest_degree_of_bucket(best_b) : 0;
    if (mode == 2) {
        if (best_b < 0 && fallback_b >= 0) theta = smallest_degree_of_bucket(fallback_b);
        const char *s = std::getenv("GNNA_DENSE_BLOCK_THETA");      // (tests: a hub count of their choosing)
        if (s && *s && std::atoi(s) > 0) theta = std::atoi(s);
    }
    if (theta <= 0) return GNNA_OK;

    // ---- hub ranks (by node id) ----
    hipLaunchKernelGGL(hub_list_kernel, dim3(elementwise_grid(N, ds->num_cus, 8)), dim3(kBlock), 0, stream, deg, N, theta, hub_count,
                       hub_list, kHubMax);
    // the count and the (id, degree) lists come back together: one copy, one synchronisation
    std::vector<int32_t> fetched((cnt_b + list_b) / 4);
    e = hipMemcpyAsync(fetched.data(), hub_count, cnt_b + list_b, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(GNNA_ERR_HIP, "dense block (hub ids): %s", hipGetErrorString(e));
    int32_t H = fetched[0];
    if (H <= 0 || H > kHubMax) return GNNA_OK;
    const int32_t *got = fetched.data() + cnt_b / 4;
    std::vector<int32_t> ids(got, got + H), degs(got + kHubMax, got + kHubMax + H);
    if (trimmed_hubs(H, ds->num_cus) != H) {
        std::vector<int32_t> order((size_t)H);
        for (int i = 0; i < H; i++) order[(size_t)i] = i;
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return degs[(size_t)a] != degs[(size_t)b] ? degs[(size_t)a] > degs[(size_t)b] : ids[(size_t)a] < ids[(size_t)b];
        });
        H = trimmed_hubs(H, ds->num_cus);
        std::vector<int32_t> kept((size_t)H);
        for (int i = 0; i < H; i++) kept[(size_t)i] = ids[(size_t)order[(size_t)i]];
        ids.swap(kept);
    }
    const int H_pad = (H + kHubKC - 1) / kHubKC * kHubKC;
    std::vector<int32_t> ranks((size_t)H_pad, -1);
    std::copy(ids.begin(), ids.end(), ranks.begin());
    std::sort(ranks.begin(), ranks.begin() + H);

    const size_t r2n_b = align256((size_t)H_pad * 4);
    const size_t bm_b = align256((size_t)H_pad * (size_t)H_pad / 8), rpp_b = align256((size_t)(P + 1) * 4);
    void *blk = nullptr;
    e = hipMalloc(&blk, r2n_b + bm_b + rpp_b);
    count_event(CTR_LAUNCH_MALLOCS);
    if (e != hipSuccess) { (void)hipGetLastError(); return GNNA_OK; }
    char *bb = static_cast<char *>(blk);
    int32_t *r2n = reinterpret_cast<int32_t *>(bb);
    uint32_t *bm = reinterpret_cast<uint32_t *>(bb + r2n_b);
    int32_t *res_pp = reinterpret_cast<int32_t *>(bb + r2n_b + bm_b);
    int32_t *res_col = nullptr;
    auto give_up = [&](int rc) { (void)hipStreamSynchronize(stream); (void)hipFree(blk); if (res_col) (void)hipFree(res_col); return rc; };
    e = hipMemcpy(r2n, ranks.data(), (size_t)H_pad * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return give_up(fail(GNNA_ERR_HIP, "dense block (ranks): %s", hipGetErrorString(e)));
    (void)hipMemsetAsync(n2r, 0xff, n2r_b, stream);
    (void)hipMemsetAsync(bm, 0, bm_b, stream);
    hipLaunchKernelGGL(hub_rank_kernel, dim3((unsigned)((H + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, r2n, (int)H, N, n2r);
    hipLaunchKernelGGL(hub_bitmap_kernel, dim3(wblocks), dim3(kBlock), 0, stream, col, pp, p2n, P, N, n2r, H_pad / 32, bm, taken, taken_total);
    hipLaunchKernelGGL(hub_res_count_kernel, dim3(elementwise_grid(P + 1, ds->num_cus, 8)), dim3(kBlock), 0, stream, pp, P, taken, res_pp);
    int rc = launch_exclusive_scan(stream, res_pp, P + 1, partial);
    if (rc != GNNA_OK) return give_up(rc);
    unsigned long long entries = 0;
    e = hipMemcpyAsync(&entries, taken_total, sizeof(entries), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return give_up(fail(GNNA_ERR_HIP, "dense block (bitmap): %s", hipGetErrorString(e)));
    const int64_t res_nnz = nnz - (int64_t)entries;
    if (entries == 0 || res_nnz <= 0) return give_up(GNNA_OK);      // nothing to take out / nothing left to sweep: no block
    e = hipMalloc(reinterpret_cast<void **>(&res_col), ((size_t)res_nnz + 16) * 4);
    count_event(CTR_LAUNCH_MALLOCS);
    if (e != hipSuccess) { (void)hipGetLastError(); res_col = nullptr; return give_up(GNNA_OK); }
    (void)hipMemsetAsync(res_col + res_nnz, 0, 16 * 4, stream);
    hipLaunchKernelGGL(hub_res_fill_kernel, dim3(wblocks), dim3(kBlock), 0, stream, col, pp, P, taken, res_pp, res_col, res_nnz);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);           // (the scratch of these passes is freed on return)
    if (e != hipSuccess) return give_up(fail(GNNA_ERR_HIP, "dense block (residual): %s", hipGetErrorString(e)));
    out->buf = blk; out->r2n = r2n; out->bm = bm; out->res_pp = res_pp; out->res_col = res_col;
    out->H = H; out->H_pad = H_pad; out->theta = theta; out->entries = (int64_t)entries; out->res_nnz = res_nnz;
    out->forced = mode == 2;
    out->tile = dense_block_tile_env(mode);
    const char *log = std::getenv("GNNA_DENSE_BLOCK_LOG");
    if (log && *log && *log != '0')
        std::fprintf(stderr, "gnna dense block: theta %d, H %d (padded %d), entries %lld of %lld edges, density %.3f\n", theta, (int)H,
                     H_pad, (long long)entries, (long long)nnz, (double)entries / ((double)H * (double)H));
    count_event(CTR_DENSE_BUILDS);
    return GNNA_OK;
}

int dense_block_tile_env(int mode)
{
    const char *s = mode == 2 ? std::getenv("GNNA_DENSE_BLOCK_TILE") : nullptr;
    const int v = s && *s ? std::atoi(s) : 0;
    return v == kHubTileM || v == 2 * kHubTileM ? v : 0;
}

int launch_hub_split(hipStream_t stream, const DenseBlock &db, const float *X, int ldx, int dim, void *image, const int32_t *stale_flag,
                     int32_t seq)
{
    if (dim < kDenseMinDim || dim > kDenseMaxDim) return fail(GNNA_ERR_INVALID_ARGUMENT, "hub block: width %d", dim);
    SplitParams p;
    p.X = X; p.r2n = db.r2n; p.img = static_cast<unsigned char *>(image); p.stale = stale_flag; p.seq = seq; p.D = dim; p.ldx = ldx;
    const bool full = dim % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    const dim3 grid((unsigned)(db.H_pad / 32)), block(kSplitThreads);
    if (full) hipLaunchKernelGGL((hub_split_kernel<true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((hub_split_kernel<false>), grid, block, 0, stream, p);
    return launch_ok("hub split launch");
}

int launch_hub_block(DeviceState *ds, hipStream_t stream, const DenseBlock &db, const void *image, float *Y, int ldy, int dim,
                     bool scaled, float eps, const float *row_scale, const int32_t *stale_flag, int32_t seq)
{
    HubParams p;
    p.Y = Y; p.r2n = db.r2n; p.bm = static_cast<const uint16_t *>(db.bm); p.img = static_cast<const unsigned char *>(image);
    p.row_scale = row_scale; p.stale = stale_flag; p.seq = seq; p.H_pad = db.H_pad; p.D = dim; p.ldy = ldy;
    p.scaled = scaled ? 1 : 0; p.eps = eps;
    if (dim < kDenseMinDim || dim > kDenseMaxDim) return fail(GNNA_ERR_INVALID_ARGUMENT, "hub block: width %d", dim);
    const int tile = dense_tile_ranks(db.H_pad, ds->num_cus, db.tile);
    const dim3 grid((unsigned)(db.H_pad / tile)), block(kHubThreads);
    if (tile == kHubTileM) {
        if (dim <= 48) hipLaunchKernelGGL((hub_block_kernel<3, kHubTileM>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((hub_block_kernel<4, kHubTileM>), grid, block, 0, stream, p);
    } else {
        if (dim <= 48) hipLaunchKernelGGL((hub_block_kernel<3, 2 * kHubTileM>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((hub_block_kernel<4, 2 * kHubTileM>), grid, block, 0, stream, p);
    }
    const int rc = launch_ok("hub block launch");
    if (rc == GNNA_OK) count_event(CTR_DENSE_LAUNCHES);      // (one per call: the split pass is counted with it)
    return rc;
}

}  // namespace gnna

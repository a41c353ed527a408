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
//     below 2^-126 per term.)
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
// kernel reads the caller's arrays and hub_block_kernel returns at once.
//
// Environment, read at every gnna_prepare_graph: GNNA_DENSE_BLOCK = 0 never / 1 (default) the rule of gnna_agg.hip / 2 any
// prepared graph whose call sweeps (tests); GNNA_DENSE_BLOCK_THETA = the degree threshold, under mode 2 only (tests: a hub count
// of their choosing); GNNA_DENSE_BLOCK_LOG = 1 prints the block taken (theta, H, entries, density) to stderr.
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

namespace gnna {
namespace {

constexpr int kHubBuckets = 64;          // half-octave degree buckets
constexpr int kHubMax = 16384;           // most hubs of a block
constexpr int kHubThreads = 512;         // hub_block_kernel: 8 wavefronts
constexpr int kHubWaves = kHubThreads / kWave;
constexpr int kHubTileM = kDenseTileRanks;    // destination ranks per workgroup (two 16-rank MFMA tiles)
constexpr int kHubKC = kDenseChunkRanks;      // source ranks staged in LDS at a time; the ranks are padded to a multiple of it
static_assert(kHubTileM == 32, "two MFMA tiles per workgroup");
constexpr int kHubStage = kHubKC / 32;   // 16-byte pieces a thread stages per chunk
constexpr int kHubZeros = 64;            // zero floats behind the ranks of a block: the row a padding rank reads
static_assert(kHubKC % kHubTileM == 0 && kHubKC * 16 == kHubThreads * kHubStage && (kHubTileM * 64) % kHubThreads == 0, "staging, elements per thread");
static_assert(kHubZeros >= kDenseMaxDim, "the zeros are a whole row");

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
    const float *X;
    float *Y;
    const int32_t *r2n;                  // [H_pad] rank -> node, -1 for the padding ranks; then kHubZeros zero floats
    const uint16_t *bm;                  // [H_pad / 32][H_pad / 32][64] halves (the header of this file)
    const float *row_scale;
    const int32_t *stale;
    int32_t seq;
    int H_pad, D, ldx, ldy;
    int scaled;                          // MODE_GIN: rows are multiplied by eps (* row_scale[row])
    float eps;
};

typedef typename VecOf<4>::T HubVT;
typedef typename VecOf<4>::M HubMT;
typedef int HubIT __attribute__((ext_vector_type(4)));

constexpr int kHubFrag = 1088;           // bytes between the B fragments of an image: 64 lanes x 16 bytes, and 64 (see the LDS image)
constexpr int kHubPiece = 16 * kHubFrag; // bytes between the hi, mid and lo images of a chunk (4 steps x 4 column tiles)
constexpr int kHubImage = 3 * kHubPiece; // 52,224 bytes per chunk
static_assert(kHubKC == 128 && kHubTileM == 32 && kHubWaves == 8 && kHubStage == 4, "the shape hub_block_kernel is written for");

typedef __bf16 HubFrag __attribute__((ext_vector_type(8)));
typedef uint32_t HubU4 __attribute__((ext_vector_type(4)));
typedef uint32_t HubU2 __attribute__((ext_vector_type(2)));

// x = hi + mid + lo exactly, each with 8 significant bits in the upper half of its word (a bf16 value): hi is x truncated, mid
// the truncated remainder, lo what is left of at most 24 bits; both subtractions are exact.  A non-finite x is in hi, with NaN
// for mid and lo (the header of this file: the end of hub_block_kernel deals with it).
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

// 8 bitmap bits -> 8 bf16 of 0 or 1 (0x3f80), element j from bit j
__device__ __forceinline__ HubFrag hub_ones(uint32_t bits)
{
    const uint32_t y = bits | (bits << 15);          // bit j at j and at j + 15: bits 2 i and 2 i + 1 are 16 apart
    HubU4 v;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = ((y >> (2 * i)) & 0x10001u) * 0x3f80u;
    return __builtin_bit_cast(HubFrag, v);
}

// A workgroup owns 32 destination ranks (two 16-rank MFMA tiles) and walks ALL source ranks, 128 at a time, with
// v_mfma_f32_16x16x32_bf16: A is 16 destination ranks x 32 source ranks of the bitmap (0 or 1), B is 32 source ranks x 16
// columns of ONE of the three bf16 pieces of X.  Every product is exact; the hi products are summed in one fp32 accumulator, the
// mid and lo products in another, and the two are added once at the end.
//
// Staging.  Thread t fetches 16 bytes (4 columns) of each of 4 consecutive ranks (their four ids are one 16-byte load), splits
// the 16 values as they go to LDS and writes, per column and piece, the 4 ranks as 8 bytes.  No branch on the way and nothing
// to mask: a padding rank reads the zeros behind the ranks, and a piece beyond D reads piece 0 into columns of the image whose
// products are never written to Y.  Within a wavefront, lanes 8 apart take adjacent rank groups and lanes 16 apart take
// columns 32 apart (below: why).
//
// The LDS image of a chunk: [piece 3][step 4][column tile 4] fragments of 64 x 16 bytes, kHubFrag bytes apart.  A fragment is the B
// operand of one MFMA: 16 bytes = the 8 ranks 8 kg .. 8 kg + 7 of a step at one column n, in slot 16 kg + 4 (n % 4) + n / 4.
// Read (ds_read_b128, lane = 16 kg + n): the 16 lanes of a service group fall on 16 different slots modulo 16: no conflict.
// Written (ds_write_b64; a service group is 16 consecutive lanes = columns 4 i + cc of two adjacent column tiles for i = 0 .. 3,
// and both halves h of the slots): byte 64 (tile + cc) + 16 i + 8 h modulo 128, the 64 from kHubFrag: all 32 banks once.
//
// The 8 wavefronts split a chunk as (step s = w % 4, column half w / 4): a wavefront reads the 3 pieces of its 2 column tiles (1
// for the upper half when NT = 3) and multiplies each with the bitmap bytes of both destination tiles: 12 MFMAs.  Two images
// take the chunks in turn: while chunk c is multiplied out of one, chunk c + 1 goes into the other, chunk c + 2 is in
// registers or on its way and chunk c + 3 is asked for (three register stages); one barrier per chunk.  At the end the
// four steps' partial tiles are laid side by side in LDS (over the images) and summed in step order, and the workgroup --
// the only writer of its 32 rows in this launch, behind the sweep kernel of the same call -- adds the tile to Y with plain
// loads and stores: no atomics, and a result that does not depend on timing.  FULL: D and ldx are multiples of 4, so every
// staged 16-byte piece is whole.
template <int NT, bool FULL>
__global__ void __launch_bounds__(kHubThreads)
hub_block_kernel(const HubParams p)
{
    if (*p.stale == p.seq) return;       // the ids changed since the block was made: the sweep kernel does the whole call
    __shared__ __attribute__((aligned(16))) unsigned char s_x[2][kHubImage];
    static_assert(4 * kHubTileM * 64 * 4 <= kHubImage, "the partial tiles fit over the first image");
    const uint16_t *bm = p.bm;
    const int tid = (int)threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = p.H_pad / kHubKC;
    const int steps = p.H_pad >> 5;      // 32-rank steps of a row of the bitmap
    const int D = p.D;

    // staging: 4 ranks from 4 g, 4 columns from 4 pc
    const int g = 4 * (tid >> 6) + ((lane >> 3) & 1) + 2 * (lane >> 5), pc = (lane & 7) + 8 * ((lane >> 4) & 1);
    const int srow = 4 * g, spiece = 4 * pc;
    const int scol = spiece < D ? spiece : 0;                // (a piece beyond D feeds columns that are never written to Y)
    const int wbase = ((g >> 3) * 4 + (pc >> 2)) * kHubFrag + (16 * ((g & 7) >> 1) + (pc & 3)) * 16 + 8 * (g & 1);
    const float *zero_row = reinterpret_cast<const float *>(p.r2n + p.H_pad);    // 64 zeros behind the ranks: what a padding rank reads
    const uintptr_t zero_at = reinterpret_cast<uintptr_t>(zero_row + scol);
    auto load_piece = [&](int node) -> HubVT {
        // (one address, chosen without a branch: a padding rank reads the zeros)
        const uintptr_t row = reinterpret_cast<uintptr_t>(p.X + (size_t)(node < 0 ? 0 : node) * (size_t)p.ldx + scol);
        const float *src = reinterpret_cast<const float *>(node < 0 ? zero_at : row);
        HubVT v;
        if constexpr (FULL) {
            v = *reinterpret_cast<const HubMT *>(src);
        } else if (spiece + 4 <= D) {
            v = *reinterpret_cast<const HubMT *>(src);
        } else {
            v = (HubVT)(0.f);
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (spiece + q < D) v[q] = src[q];
        }
        return v;
    };
    // Three stages take the chunks in turn (chunk c lives in stage c % 3): rows, bitmap bytes and the node ids of the chunk
    // that FOLLOWS in the same stage, fetched behind the rows, so a row address never waits for an id that is younger than
    // the rows the same wait is for.  A chunk beyond the last is the last one again: fetched, never multiplied.
    struct Stage {
        HubVT r[kHubStage];
        HubIT node;
        uint32_t w;                      // this wavefront's step of the bitmap: byte 0 the first destination tile, byte 1 the second
    };
    auto fetch_ids = [&](int c, Stage &st) {
        const int cc = c < chunks ? c : chunks - 1;
        st.node = *reinterpret_cast<const HubIT *>(&p.r2n[cc * kHubKC + srow]);
    };
    auto fetch_words = [&](int c, Stage &st) {
        const int cc = c < chunks ? c : chunks - 1;
        st.w = bm[((size_t)blockIdx.x * (size_t)steps + (size_t)(cc * 4 + (wib & 3))) * 64 + (size_t)lane];
    };
    auto fetch_row = [&](int i, Stage &st) {                 // row i of the chunk whose ids are in st.node
        st.r[i] = load_piece(st.node[i]);
    };
    // column cc of the thread's 4 x 4 values: split, packed by rank pairs, 8 bytes per piece
    auto stage_out = [&](int cc, const Stage &st, unsigned char *image) {
        uint32_t pk[3][2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t a[3], b[3];
            hub_split(__float_as_uint(st.r[2 * h][cc]), a[0], a[1], a[2]);
            hub_split(__float_as_uint(st.r[2 * h + 1][cc]), b[0], b[1], b[2]);
#pragma unroll
            for (int i = 0; i < 3; i++) pk[i][h] = hub_pack(a[i], b[i]);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            HubU2 v;
            v[0] = pk[i][0];
            v[1] = pk[i][1];
            *reinterpret_cast<HubU2 *>(&image[wbase + i * kHubPiece + cc * 64]) = v;
        }
    };

    const int cs = wib & 3, ch = wib >> 2;                  // this wavefront's step of a chunk and its half of the columns
    const int rbase = (cs * 4 + 2 * ch) * kHubFrag + (16 * (lane >> 4) + 4 * (lane & 3) + ((lane & 15) >> 2)) * 16;
    HubVT acc_hi[2][2], acc_lo[2][2];                           // [destination tile][column tile of the half]
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc_hi[t][q] = acc_lo[t][q] = (HubVT)(0.f);

    // Chunk c out of image c % 2 with the bitmap bytes of stage L, which then starts on chunk c + 3; stage S holds chunk c + 1,
    // which goes into the other image.  A turn is four parts, pinned in this order: a load of L, the MFMAs of one piece (hi, mid,
    // lo, none), one column of S split and written.  The loads are spread like this because the compute unit's address unit
    // takes about as long for a chunk's 32 KB as the rest of the turn does: issued in one burst by all eight wavefronts they
    // fill its queue, a wavefront stands at its next load until the queue has room, and nothing else is issued meanwhile.
    auto turn = [&](int c, Stage &L, const Stage &S) {
        const unsigned char *cur = s_x[c & 1];
        unsigned char *nxt = s_x[(c & 1) ^ 1];
        __builtin_amdgcn_sched_barrier(0);
        HubFrag b[2][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int q = 0; q < 2; q++)
                if (NT == 4 || q == 0 || ch == 0) b[q][i] = *reinterpret_cast<const HubFrag *>(&cur[rbase + q * kHubFrag + i * kHubPiece]);
        HubFrag a[2];
        a[0] = hub_ones(L.w & 0xffu);
        a[1] = hub_ones((L.w >> 8) & 0xffu);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            fetch_row(k, L);
            if (k < 3) {
#pragma unroll
                for (int q = 0; q < 2; q++)
                    if (NT == 4 || q == 0 || ch == 0) {
#pragma unroll
                        for (int t = 0; t < 2; t++) {
                            if (k == 0) acc_hi[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[q][0], acc_hi[t][q], 0, 0, 0);
                            else acc_lo[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[q][k], acc_lo[t][q], 0, 0, 0);
                        }
                    }
            }
            stage_out(k, S, nxt);
            __builtin_amdgcn_sched_barrier(0);
        }
        fetch_words(c + 3, L);
        fetch_ids(c + 6, L);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                     // `nxt` is whole, and `cur` has been read by every wavefront
    };
    Stage s0, s1, s2;
    fetch_ids(0, s0);
    fetch_ids(1, s1);
    fetch_ids(2, s2);
    // (the order of the loads is that of the turns, and pinned: the counted waits of the loop are those of its entry as well)
    auto fetch = [&](int c, Stage &st) {
#pragma unroll
        for (int i = 0; i < kHubStage; i++) fetch_row(i, st);
        fetch_words(c, st);
        fetch_ids(c + 3, st);
        __builtin_amdgcn_sched_barrier(0);
    };
    fetch(0, s0);
    fetch(1, s1);
    fetch(2, s2);
#pragma unroll
    for (int cc = 0; cc < 4; cc++) stage_out(cc, s0, s_x[0]);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    int c = 0;
    for (; c + 3 <= chunks; c += 3) {
        turn(c, s0, s1);
        turn(c + 1, s1, s2);
        turn(c + 2, s2, s0);
    }
    if (c < chunks) {
        turn(c, s0, s1);
        if (c + 1 < chunks) turn(c + 1, s1, s2);
    }

    // the 4 partial tiles of the workgroup's 32 rows, side by side, then summed in step order
    // (the last turn ended with a barrier: nobody reads the images any more)
    float *part = reinterpret_cast<float *>(&s_x[0][0]);     // [step][32 ranks][64 columns]; the columns from 16 NT on stay unwritten and unread
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < 2; q++)
            if (NT == 4 || q == 0 || ch == 0) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    part[(cs * kHubTileM + t * 16 + (lane >> 4) * 4 + r) * 64 + (2 * ch + q) * 16 + (lane & 15)] =
                        __builtin_isinf(acc_hi[t][q][r]) ? acc_hi[t][q][r] : acc_hi[t][q][r] + acc_lo[t][q][r];
            }
    __syncthreads();
    // one plain read-add-write of Y per element
#pragma unroll
    for (int i = 0; i < kHubTileM * 64 / kHubThreads; i++) {
        const int idx = i * kHubThreads + tid;
        const int row = idx >> 6, col = idx & 63;
        if (col >= D) continue;
        float sum = part[idx];
#pragma unroll
        for (int s = 1; s < 4; s++) sum += part[s * kHubTileM * 64 + idx];
        const int node = p.r2n[(int)blockIdx.x * kHubTileM + row];
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

    const size_t r2n_b = align256((size_t)H_pad * 4 + kHubZeros * 4);
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
    (void)hipMemsetAsync(r2n + H_pad, 0, kHubZeros * 4, stream);
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
    const char *log = std::getenv("GNNA_DENSE_BLOCK_LOG");
    if (log && *log && *log != '0')
        std::fprintf(stderr, "gnna dense block: theta %d, H %d (padded %d), entries %lld of %lld edges, density %.3f\n", theta, (int)H,
                     H_pad, (long long)entries, (long long)nnz, (double)entries / ((double)H * (double)H));
    count_event(CTR_DENSE_BUILDS);
    return GNNA_OK;
}

int launch_hub_block(DeviceState *ds, hipStream_t stream, const DenseBlock &db, const float *X, int ldx, float *Y, int ldy, int dim,
                     bool scaled, float eps, const float *row_scale, const int32_t *stale_flag, int32_t seq)
{
    HubParams p;
    p.X = X; p.Y = Y; p.r2n = db.r2n; p.bm = static_cast<const uint16_t *>(db.bm); p.row_scale = row_scale;
    p.stale = stale_flag; p.seq = seq; p.H_pad = db.H_pad; p.D = dim; p.ldx = ldx; p.ldy = ldy;
    p.scaled = scaled ? 1 : 0; p.eps = eps;
    (void)ds;
    if (dim < kDenseMinDim || dim > kDenseMaxDim) return fail(GNNA_ERR_INVALID_ARGUMENT, "hub block: width %d", dim);
    const bool full = dim % 4 == 0 && ldx % 4 == 0;
    const dim3 grid((unsigned)(db.H_pad / kHubTileM)), block(kHubThreads);
    if (dim <= 48) {
        if (full) hipLaunchKernelGGL((hub_block_kernel<3, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((hub_block_kernel<3, false>), grid, block, 0, stream, p);
    } else {
        if (full) hipLaunchKernelGGL((hub_block_kernel<4, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((hub_block_kernel<4, false>), grid, block, 0, stream, p);
    }
    const int rc = launch_ok("hub block launch");
    if (rc == GNNA_OK) count_event(CTR_DENSE_LAUNCHES);
    return rc;
}

}  // namespace gnna

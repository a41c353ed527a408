// gnna_dense.hip -- the dense hub-to-hub block of a prepared graph.  CDNA4 / gfx950 only.
//
// A power-law graph whose node pairs are deduplicated has a nearly full corner: for two hubs the expected number of drawn
// pairs exceeds one, so almost every hub is a neighbour of almost every other hub.  Those edges cost the gather two
// 128-byte requests each (gnna_sweep.hip) and carry one bit of information.  gnna_prepare_graph therefore splits the
// adjacency of a swept graph as A = A_res + A_hub:
//
//   * A_hub is the H x H block of the hubs (the nodes of degree >= theta, ranked by node id) as a BITMAP.  One 64-bit
//     word holds 16 destination ranks x 4 source ranks -- bit (dst % 16) + 16 * (src % 4) -- which is the lane order of
//     the A operand of v_mfma_f32_16x16x4_f32: the operand of a wavefront is 1.0f where its lane's bit is set;
//   * A_res is everything else, as a residual graph with the caller's part2Node and group count: new part_pointers
//     (groups only shrink; some become empty) and a compacted column_index.  The sweep kernel runs on it;
//   * hub_block_kernel then adds Y[node(i), :] += scale(i) * sum_j bit(i, j) * X[node(j), :] with f32 MFMA (inputs and
//     accumulation in fp32: the products are exact, the sums are fp32 sums in another order).
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
// block, not only its neighbours' (the gather would hand it to the neighbours alone).
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
constexpr int kHubRowStride = 80;        // floats between staged rows (16-byte aligned; the 4 rows of a step start 16 banks apart)
static_assert(kHubKC % kHubTileM == 0 && kHubKC * 16 == kHubThreads * kHubStage && kHubKC / 4 * 2 == kWave, "staging; one bitmap word per lane");
static_assert((kHubKC / 4) % kHubWaves == 0 && (kHubTileM * 64) % kHubThreads == 0, "steps per wavefront, elements per thread");

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
                  const int32_t *__restrict__ n2r, int words_per_tile_row, unsigned long long *__restrict__ bm,
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
            const size_t word = (size_t)(rd >> 4) * (size_t)words_per_tile_row + (size_t)(rs >> 2);
            const unsigned long long bit = 1ull << ((rd & 15) + 16 * (rs & 3));
            const unsigned long long old = atomicOr(&bm[word], bit);
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
    const int32_t *r2n;                  // [H_pad] rank -> node, -1 for the padding ranks
    const unsigned long long *bm;        // [H_pad / 16][H_pad / 4] words
    const float *row_scale;
    const int32_t *stale;
    int32_t seq;
    int H_pad, D, ldx, ldy;
    int scaled;                          // MODE_GIN: rows are multiplied by eps (* row_scale[row])
    float eps;
};

// A workgroup owns 32 destination ranks (two MFMA tiles) and walks ALL source ranks, 128 at a time.  The 128 source rows of a
// chunk are staged in one of TWO LDS images (zero beyond D and for padding ranks): while chunk c is multiplied out of one
// image, the rows of chunk c + 1 are written into the other, and the loads of chunks c + 2 and c + 3 are in flight -- one
// barrier per chunk, and a load has two chunks' time to arrive.  Its 8 wavefronts split the 32 four-rank steps of a chunk:
// wavefront w takes steps 4 w .. 4 w + 3 of both tiles.  Per step lane (k, j) = (lane / 16, lane % 16) reads
// X[rank k0 + k][16 q + j] for q = 0 .. NT - 1: the B operands of NT MFMAs, MFMA q covering the columns 16 q .. 16 q + 15
// (NT = 3 for D <= 48, 4 beyond).  A wavefront issues the B reads of all its four steps first; its 8 NT MFMAs then follow with
// no branch between them, and the LDS writes of the next chunk and the loads of the chunk after the next two sit one by one
// between the half steps, in the shadow of the matrix unit.  The A operand is the tile's bitmap word.  Accumulator register r of MFMA q
// holds Y[rank 4 (lane / 16) + r][16 q + lane % 16].  At the end the 8 partial tiles are laid side by side in LDS (over the
// images) and summed in wavefront order, and the workgroup -- the only writer of its 32 rows in this launch, behind the sweep
// kernel of the same call -- adds the tile to Y with plain loads and stores: no atomics, and a result that does not depend
// on timing.  FULL: D and ldx are multiples of 4, so every staged 16-byte piece is whole.
// (Measured on the headline's block of 8,192 hubs, profiles/dense_block and profiles/hub_block_rate: partial tiles of a
// split over source ranks added with float atomics -- 183 us; 64-rank chunks, one chunk in flight -- 367 us; one image, two
// barriers per chunk, an LDS read waited for before every pair of MFMAs -- 130 us.)
template <int NT, bool FULL>
__global__ void __launch_bounds__(kHubThreads)
hub_block_kernel(const HubParams p)
{
    typedef typename VecOf<4>::T VT;
    typedef typename VecOf<4>::M MT;
    if (*p.stale == p.seq) return;       // the ids changed since the block was made: the sweep kernel does the whole call
    __shared__ __attribute__((aligned(16))) float s_x[2][kHubKC * kHubRowStride];
    static_assert(kHubWaves * kHubTileM * 64 <= 2 * kHubKC * kHubRowStride, "the partial tiles fit over the images");
    const int tid = (int)threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = p.H_pad / kHubKC;
    const int words_per_tile_row = p.H_pad >> 2;
    const int tile0 = (int)blockIdx.x * (kHubTileM / 16);  // the workgroup's first 16-rank tile
    const int D = p.D;

    // staging: thread t fetches piece t % 16 of the chunk's rows 4 (t / 16) .. 4 (t / 16) + 3 (their four ids are one 16-byte
    // load).  No branch on the way: a padding rank reads row 0 and a piece beyond D reads piece 0; what they fetched is masked
    // away when the piece goes to LDS (not before: touching a loaded value where it is loaded would wait for it there)
    typedef int IT __attribute__((ext_vector_type(4)));
    const int srow = (tid >> 4) * kHubStage, spiece = (tid & 15) * 4;
    const bool live = spiece < D;
    const int scol = live ? spiece : 0;
    auto load_piece = [&](int node) -> VT {
        const float *src = p.X + (size_t)(node < 0 ? 0 : node) * (size_t)p.ldx + scol;
        VT v;
        if constexpr (FULL) {
            v = *reinterpret_cast<const MT *>(src);
        } else if (spiece + 4 <= D) {
            v = *reinterpret_cast<const MT *>(src);
        } else {
            v = vzero<4>();
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (spiece + q < D) v[q] = src[q];
        }
        return v;
    };
    // Two stages take the chunks in turn (s0 the even ones, s1 the odd ones); the node ids of a stage's NEXT chunk are
    // fetched behind the rows of the current one, so a row address never waits for an id that is younger than the rows the
    // same wait is for.  A chunk beyond the last is the last one again: fetched, never multiplied.
    struct Stage {
        VT r[kHubStage];
        IT node;
        uint32_t keep[kHubStage];        // all ones, or zero for a padding rank and for a piece beyond D
    };
    auto fetch_ids = [&](int c, Stage &st) {
        const int cc = c < chunks ? c : chunks - 1;
        st.node = *reinterpret_cast<const IT *>(&p.r2n[cc * kHubKC + srow]);
    };
    auto fetch_row = [&](int i, Stage &st) {                 // piece i of the chunk whose ids are in st.node
        st.r[i] = load_piece(st.node[i]);
        st.keep[i] = (st.node[i] >= 0 && live) ? 0xffffffffu : 0u;
    };
    // the bitmap words of chunk c: lanes 0 .. 31 the 32 words of the first tile, lanes 32 .. 63 of the second
    auto fetch_words = [&](int c) -> unsigned long long {
        const int cc = c < chunks ? c : chunks - 1;
        return p.bm[(size_t)(tile0 + (lane >> 5)) * (size_t)words_per_tile_row + (size_t)(cc * (kHubKC / 4) + (lane & 31))];
    };
    // rows of chunk c (its ids are in st.node), the words of chunk cw, the ids of chunk c + 2: the order of a turn's loads
    auto fetch = [&](int c, Stage &st, unsigned long long &w, int cw) {
#pragma unroll
        for (int i = 0; i < kHubStage; i++) fetch_row(i, st);
        w = fetch_words(cw);
        fetch_ids(c + 2, st);
    };
    auto stage_out = [&](int i, const Stage &st, float *image) {
        VT v = st.r[i];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = __uint_as_float(__float_as_uint(v[q]) & st.keep[i]);
        *reinterpret_cast<VT *>(&image[(srow + i) * kHubRowStride + spiece]) = v;
    };

    VT acc[2][NT];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < NT; q++) acc[t][q] = vzero<4>();

    // Chunk c out of `cur` with the words w, which then become those of chunk c + 2 (a wavefront moves its eight words to
    // scalar registers first: no copy of a loaded register, which would wait for the load where the copy stands); st holds
    // chunk c + 1, which goes into `nxt`, and then starts on chunk c + 3.  The ten memory
    // operations of a turn (4 LDS writes, 6 loads) are spread over the gaps between the eight half steps of MFMAs and
    // pinned there: issued in one burst by all eight wavefronts they fill the queue of the compute unit's address unit (a
    // chunk's 32 KB keep it busy for about half of a chunk's MFMA time), a wavefront stands at its next load until the
    // queue has room, and no MFMA is issued meanwhile (stamped: 600 - 1,100 cycles per chunk for the nine loads of a burst).
    auto turn = [&](int c, Stage &st, unsigned long long &w, const float *cur, float *nxt) {
        constexpr int kSteps = kHubKC / 4 / kHubWaves;
        static_assert(kSteps == 4 && kHubStage == 4, "the places of the memory operations between the half steps");
        float b[kSteps][NT];
#pragma unroll
        for (int j = 0; j < kSteps; j++) {
            const float *xs = &cur[((wib * kSteps + j) * 4 + (lane >> 4)) * kHubRowStride + (lane & 15)];
#pragma unroll
            for (int q = 0; q < NT; q++) b[j][q] = xs[q * 16];
        }
        __builtin_amdgcn_sched_barrier(0);                   // every B read is issued before the first MFMA
        const int w_lo = (int)(uint32_t)w, w_hi = (int)(uint32_t)(w >> 32);
        unsigned long long m[2][kSteps];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int j = 0; j < kSteps; j++) {
                const int s = 32 * t + wib * kSteps + j;
                m[t][j] = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(w_hi, s) << 32) | (uint32_t)__builtin_amdgcn_readlane(w_lo, s);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kSteps; j++) {
            const float a0 = __builtin_amdgcn_inverse_ballot_w64(m[0][j]) ? 1.f : 0.f;   // (one v_cndmask on the scalar word)
            const float a1 = __builtin_amdgcn_inverse_ballot_w64(m[1][j]) ? 1.f : 0.f;
#pragma unroll
            for (int h = 0; h < 2; h++) {
#pragma unroll
                for (int q = 2 * h; q < 2 * h + 2 && q < NT; q++) {
                    acc[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[j][q], acc[0][q], 0, 0, 0);
                    acc[1][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[j][q], acc[1][q], 0, 0, 0);
                }
                const int k = 2 * j + h;
                if (k < 2) {
                    stage_out(2 * k, st, nxt);
                    stage_out(2 * k + 1, st, nxt);
                } else if (k < 6) {
                    fetch_row(k - 2, st);
                } else if (k == 6) {
                    w = fetch_words(c + 2);
                    fetch_ids(c + 5, st);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();                                     // `nxt` is whole, and `cur` has been read by every wavefront
    };
    Stage s0, s1;
    fetch_ids(0, s0);
    fetch_ids(1, s1);
    unsigned long long w0, w1;           // the words of the even and of the odd chunks
    fetch(0, s0, w0, 0);
    fetch(1, s1, w0, 0);
#pragma unroll
    for (int i = 0; i < kHubStage; i++) stage_out(i, s0, s_x[0]);
    fetch(2, s0, w1, 1);
    __syncthreads();
    // (two turns per trip and the odd last chunk outside: a branch inside the loop would make the waits of the trip after it
    // cover the loads of both stages)
    for (int c = 0; c + 1 < chunks; c += 2) {
        turn(c, s1, w0, s_x[0], s_x[1]);
        turn(c + 1, s0, w1, s_x[1], s_x[0]);
    }
    if (chunks & 1) turn(chunks - 1, s1, w0, s_x[0], s_x[1]);

    // the 8 partial tiles of the workgroup's 32 rows, side by side, then summed in wavefront order
    // (the last turn ended with a barrier: nobody reads the images any more)
    float *part = &s_x[0][0];            // [wavefront][32 ranks][64 columns]; the columns from 16 NT on stay unwritten and unread
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < NT; q++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                part[(wib * kHubTileM + t * 16 + (lane >> 4) * 4 + r) * 64 + q * 16 + (lane & 15)] = acc[t][q][r];
    __syncthreads();
    // one plain read-add-write of Y per element
#pragma unroll
    for (int i = 0; i < kHubTileM * 64 / kHubThreads; i++) {
        const int idx = i * kHubThreads + tid;
        const int row = idx >> 6, col = idx & 63;
        if (col >= D) continue;
        float sum = part[idx];
#pragma unroll
        for (int w = 1; w < kHubWaves; w++) sum += part[w * kHubTileM * 64 + idx];
        const int node = p.r2n[tile0 * 16 + row];
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
    const size_t bm_b = align256((size_t)(H_pad / 16) * (size_t)(H_pad / 4) * 8), rpp_b = align256((size_t)(P + 1) * 4);
    void *blk = nullptr;
    e = hipMalloc(&blk, r2n_b + bm_b + rpp_b);
    count_event(CTR_LAUNCH_MALLOCS);
    if (e != hipSuccess) { (void)hipGetLastError(); return GNNA_OK; }
    char *bb = static_cast<char *>(blk);
    int32_t *r2n = reinterpret_cast<int32_t *>(bb);
    unsigned long long *bm = reinterpret_cast<unsigned long long *>(bb + r2n_b);
    int32_t *res_pp = reinterpret_cast<int32_t *>(bb + r2n_b + bm_b);
    int32_t *res_col = nullptr;
    auto give_up = [&](int rc) { (void)hipStreamSynchronize(stream); (void)hipFree(blk); if (res_col) (void)hipFree(res_col); return rc; };
    e = hipMemcpy(r2n, ranks.data(), (size_t)H_pad * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return give_up(fail(GNNA_ERR_HIP, "dense block (ranks): %s", hipGetErrorString(e)));
    (void)hipMemsetAsync(n2r, 0xff, n2r_b, stream);
    (void)hipMemsetAsync(bm, 0, bm_b, stream);
    hipLaunchKernelGGL(hub_rank_kernel, dim3((unsigned)((H + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, r2n, (int)H, N, n2r);
    hipLaunchKernelGGL(hub_bitmap_kernel, dim3(wblocks), dim3(kBlock), 0, stream, col, pp, p2n, P, N, n2r, H_pad / 4, bm, taken, taken_total);
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
    p.X = X; p.Y = Y; p.r2n = db.r2n; p.bm = static_cast<const unsigned long long *>(db.bm); p.row_scale = row_scale;
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

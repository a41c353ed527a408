// hub_block_bf16_probe.hip -- stand-alone measurement of the hub block kernel in its two forms (profiles/hub_block_bf16 section 0).
//
// A synthetic block of the headline's shape: H hubs among 232,965 rows of X, D = 64, a random bitmap of a given density.  The
// program runs
//   * f32:  a copy of hub_block_kernel<4, true> as it stood before the bf16 form (v_mfma_f32_16x16x4_f32, one 64-bit word per
//           16 destination x 4 source ranks), and
//   * bf16: a copy of hub_block_kernel<4, true> of csrc/gnna_dense.hip (X split exactly into three bf16 pieces at staging,
//           v_mfma_f32_16x16x32_bf16, two bitmap bytes per lane of a 32 x 32 tile),
// 50 launches each back to back, and prints the time per launch and the largest difference of the bf16 result from an fp64
// sum (on a sample of the rows) and from the f32 kernel (on all rows).  Measurement only: nothing in the library uses it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 hub_block_bf16_probe.hip -o hub_block_bf16_probe && ./hub_block_bf16_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                         \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) {                                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));              \
            std::exit(1);                                                                                \
        }                                                                                                \
    } while (0)

namespace {

constexpr int kWave = 64;
constexpr int kHubThreads = 512;
constexpr int kHubWaves = kHubThreads / kWave;
constexpr int kHubTileM = 32;
constexpr int kHubKC = 128;
constexpr int kHubStage = kHubKC / 32;

typedef float VT __attribute__((ext_vector_type(4)));
typedef VT MT __attribute__((aligned(4)));
typedef int IT __attribute__((ext_vector_type(4)));

struct HubParams {
    const float *X;
    float *Y;
    const int32_t *r2n;
    const uint16_t *bm;                  // (the f32 form reads it as 64-bit words)
    const float *row_scale;
    const int32_t *stale;
    int32_t seq;
    int H_pad, D, ldx, ldy;
    int scaled;
    float eps;
};

// ---- the f32 form (copy; NT = 4, FULL) -----------------------------------------------------------------------------
constexpr int kF32RowStride = 80;

__global__ void __launch_bounds__(kHubThreads)
hub_block_f32(const HubParams p)
{
    constexpr int NT = 4;
    if (*p.stale == p.seq) return;
    __shared__ __attribute__((aligned(16))) float s_x[2][kHubKC * kF32RowStride];
    const unsigned long long *bm = reinterpret_cast<const unsigned long long *>(p.bm);
    const int tid = (int)threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = p.H_pad / kHubKC;
    const int words_per_tile_row = p.H_pad >> 2;
    const int tile0 = (int)blockIdx.x * (kHubTileM / 16);
    const int D = p.D;
    const int srow = (tid >> 4) * kHubStage, spiece = (tid & 15) * 4;
    const bool live = spiece < D;
    const int scol = live ? spiece : 0;
    auto load_piece = [&](int node) -> VT {
        const float *src = p.X + (size_t)(node < 0 ? 0 : node) * (size_t)p.ldx + scol;
        return *reinterpret_cast<const MT *>(src);
    };
    struct Stage {
        VT r[kHubStage];
        IT node;
        uint32_t keep[kHubStage];
    };
    auto fetch_ids = [&](int c, Stage &st) {
        const int cc = c < chunks ? c : chunks - 1;
        st.node = *reinterpret_cast<const IT *>(&p.r2n[cc * kHubKC + srow]);
    };
    auto fetch_row = [&](int i, Stage &st) {
        st.r[i] = load_piece(st.node[i]);
        st.keep[i] = (st.node[i] >= 0 && live) ? 0xffffffffu : 0u;
    };
    auto fetch_words = [&](int c) -> unsigned long long {
        const int cc = c < chunks ? c : chunks - 1;
        return bm[(size_t)(tile0 + (lane >> 5)) * (size_t)words_per_tile_row + (size_t)(cc * (kHubKC / 4) + (lane & 31))];
    };
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
        *reinterpret_cast<VT *>(&image[(srow + i) * kF32RowStride + spiece]) = v;
    };
    VT acc[2][NT];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < NT; q++) acc[t][q] = (VT)(0.f);
    auto turn = [&](int c, Stage &st, unsigned long long &w, const float *cur, float *nxt) {
        constexpr int kSteps = kHubKC / 4 / kHubWaves;
        float b[kSteps][NT];
#pragma unroll
        for (int j = 0; j < kSteps; j++) {
            const float *xs = &cur[((wib * kSteps + j) * 4 + (lane >> 4)) * kF32RowStride + (lane & 15)];
#pragma unroll
            for (int q = 0; q < NT; q++) b[j][q] = xs[q * 16];
        }
        __builtin_amdgcn_sched_barrier(0);
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
            const float a0 = __builtin_amdgcn_inverse_ballot_w64(m[0][j]) ? 1.f : 0.f;
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
        __syncthreads();
    };
    Stage s0, s1;
    fetch_ids(0, s0);
    fetch_ids(1, s1);
    unsigned long long w0, w1;
    fetch(0, s0, w0, 0);
    fetch(1, s1, w0, 0);
#pragma unroll
    for (int i = 0; i < kHubStage; i++) stage_out(i, s0, s_x[0]);
    fetch(2, s0, w1, 1);
    __syncthreads();
    for (int c = 0; c + 1 < chunks; c += 2) {
        turn(c, s1, w0, s_x[0], s_x[1]);
        turn(c + 1, s0, w1, s_x[1], s_x[0]);
    }
    if (chunks & 1) turn(chunks - 1, s1, w0, s_x[0], s_x[1]);
    float *part = &s_x[0][0];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < NT; q++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                part[(wib * kHubTileM + t * 16 + (lane >> 4) * 4 + r) * 64 + q * 16 + (lane & 15)] = acc[t][q][r];
    __syncthreads();
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

// ---- the bf16 form (copy of csrc/gnna_dense.hip) -------------------------------------------------------------------
constexpr int kHubZeros = 64;            // zero floats behind the ranks: the row a padding rank reads
typedef VT HubVT;
typedef MT HubMT;
typedef IT HubIT;

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

// ---- the synthetic block -------------------------------------------------------------------------------------------
inline uint64_t mix(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

struct Result {
    double us_f32, us_bf16, err64, ref64, errf32;
};

Result run(int H, int inv_density, int N, int D, const float *dX, const std::vector<float> &X, int launches)
{
    const int H_pad = (H + kHubKC - 1) / kHubKC * kHubKC;
    // hubs: every (N / H)-th node, in id order
    std::vector<int32_t> r2n((size_t)H_pad, -1);
    for (int i = 0; i < H; i++) r2n[(size_t)i] = (int32_t)((int64_t)i * N / H);
    std::vector<unsigned long long> bm64((size_t)(H_pad / 16) * (size_t)(H_pad / 4), 0ull);
    std::vector<uint32_t> bm16((size_t)H_pad * (size_t)H_pad / 32, 0u);
    const int steps = H_pad / 32;
    for (int d = 0; d < H; d++)
        for (int s0 = 0; s0 < H; s0 += 64) {
            uint64_t r = mix((uint64_t)d * 1000003ull + (uint64_t)s0), r2 = mix(r);
            uint64_t bits = inv_density == 4 ? (r & r2) : (r & r2 & mix(r2));
            for (int b = 0; b < 64 && s0 + b < H; b++) {
                if (!((bits >> b) & 1ull)) continue;
                const int s = s0 + b;
                bm64[(size_t)(d >> 4) * (size_t)(H_pad / 4) + (size_t)(s >> 2)] |= 1ull << ((d & 15) + 16 * (s & 3));
                const size_t half = ((size_t)(d >> 5) * steps + (size_t)(s >> 5)) * 64 + (size_t)((d & 15) + 16 * ((s & 31) >> 3));
                bm16[half >> 1] |= 1u << (16 * (half & 1) + 8 * ((d >> 4) & 1) + (s & 7));
            }
        }
    int32_t *d_r2n, *d_stale;
    void *d_bm64, *d_bm16;
    float *dY0, *dY1;
    CHECK(hipMalloc(&d_r2n, (size_t)H_pad * 4 + kHubZeros * 4));       // (the ranks, and the zeros behind them)
    CHECK(hipMemset(d_r2n, 0, (size_t)H_pad * 4 + kHubZeros * 4));
    CHECK(hipMalloc(&d_stale, 4));
    CHECK(hipMalloc(&d_bm64, bm64.size() * 8));
    CHECK(hipMalloc(&d_bm16, bm16.size() * 4));
    CHECK(hipMalloc(&dY0, (size_t)N * D * 4));
    CHECK(hipMalloc(&dY1, (size_t)N * D * 4));
    CHECK(hipMemcpy(d_r2n, r2n.data(), (size_t)H_pad * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_stale, 0, 4));
    CHECK(hipMemcpy(d_bm64, bm64.data(), bm64.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_bm16, bm16.data(), bm16.size() * 4, hipMemcpyHostToDevice));
    HubParams p;
    p.X = dX; p.r2n = d_r2n; p.row_scale = nullptr; p.stale = d_stale; p.seq = 1; p.H_pad = H_pad; p.D = D; p.ldx = D; p.ldy = D;
    p.scaled = 0; p.eps = 0.f;
    const dim3 grid((unsigned)(H_pad / kHubTileM)), block(kHubThreads);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    Result res{};
    std::vector<float> y0((size_t)N * D), y1((size_t)N * D);
    for (int form = 0; form < 2; form++) {
        p.Y = form ? dY1 : dY0;
        p.bm = static_cast<const uint16_t *>(form ? d_bm16 : d_bm64);
        auto launch = [&]() {
            if (form) hipLaunchKernelGGL((hub_block_kernel<4, true>), grid, block, 0, 0, p);
            else hipLaunchKernelGGL(hub_block_f32, grid, block, 0, 0, p);
        };
        // the result of ONE launch into zeros
        CHECK(hipMemset(p.Y, 0, (size_t)N * D * 4));
        launch();
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(form ? y1.data() : y0.data(), p.Y, (size_t)N * D * 4, hipMemcpyDeviceToHost));
        double best = 1e30;
        for (int rep = 0; rep < 3; rep++) {
            CHECK(hipMemset(p.Y, 0, (size_t)N * D * 4));
            CHECK(hipEventRecord(e0, 0));
            for (int i = 0; i < launches; i++) launch();
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            best = std::min(best, (double)ms * 1e3 / launches);
        }
        (form ? res.us_bf16 : res.us_f32) = best;
    }
    for (size_t i = 0; i < y0.size(); i++) res.errf32 = std::max(res.errf32, (double)std::fabs(y0[i] - y1[i]));
    // fp64 sums of every 61st hub row
    for (int d = 0; d < H; d += 61) {
        std::vector<double> sum((size_t)D, 0.0);
        for (int s = 0; s < H; s++)
            if ((bm64[(size_t)(d >> 4) * (size_t)(H_pad / 4) + (size_t)(s >> 2)] >> ((d & 15) + 16 * (s & 3))) & 1ull)
                for (int c = 0; c < D; c++) sum[(size_t)c] += (double)X[(size_t)r2n[(size_t)s] * D + c];
        for (int c = 0; c < D; c++) {
            res.err64 = std::max(res.err64, std::fabs(sum[(size_t)c] - (double)y1[(size_t)r2n[(size_t)d] * D + c]));
            res.ref64 = std::max(res.ref64, std::fabs(sum[(size_t)c]));
        }
    }
    CHECK(hipFree(d_r2n)); CHECK(hipFree(d_stale)); CHECK(hipFree(d_bm64)); CHECK(hipFree(d_bm16)); CHECK(hipFree(dY0)); CHECK(hipFree(dY1));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    return res;
}

}  // namespace

int main()
{
    const int N = 232965, D = 64;
    std::vector<float> X((size_t)N * D);
    for (size_t i = 0; i < X.size(); i++) {
        // roughly normal, full mantissas: the sum of four uniforms
        const uint64_t r = mix(i);
        const double u = ((double)(r & 0xffff) + (double)((r >> 16) & 0xffff) + (double)((r >> 32) & 0xffff) + (double)(r >> 48)) / 65536.0 - 2.0;
        X[i] = (float)(u * 1.7320508 + (double)(mix(r) & 0xffffff) * 1e-9);
    }
    float *dX;
    CHECK(hipMalloc(&dX, X.size() * 4));
    CHECK(hipMemcpy(dX, X.data(), X.size() * 4, hipMemcpyHostToDevice));
    std::printf("| H | density | f32 us | bf16 us | bf16 / f32 | max abs diff from fp64 (max abs fp64 sum) | max abs diff from f32 kernel |\n|---|---|---|---|---|---|---|\n");
    const int Hs[2] = {8192, 16384}, inv[2] = {4, 8};
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const Result r = run(Hs[a], inv[b], N, D, dX, X, 50);
            std::printf("| %d | 1/%d | %.1f | %.1f | %.3f | %.3e (%.1f) | %.3e |\n", Hs[a], inv[b], r.us_f32, r.us_bf16, r.us_bf16 / r.us_f32,
                        r.err64, r.ref64, r.errf32);
            std::fflush(stdout);
        }
    CHECK(hipFree(dX));
    return 0;
}

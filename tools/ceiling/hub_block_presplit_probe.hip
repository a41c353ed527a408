// hub_block_presplit_probe.hip -- stand-alone go / no-go measurement for splitting the hub rows once per call
// (profiles/hub_block_presplit section 0).
//
// A synthetic block of the headline's shape: H hubs among 232,965 rows of X, D = 64, a random bitmap of a given density.  In one
// process:
//   * today:  a copy of hub_block_kernel<4, true> as it stood before this change (every workgroup splits every hub row of X
//             into its three bf16 pieces on the way to LDS);
//   * split:  hub_split_kernel, one pass that writes the three pieces of the hub rows once, in the B-operand order, with one
//             or four 32-rank steps per workgroup;
//   * image:  the kernel that reads that image and does no arithmetic on X, with 32 and 64 destination ranks per workgroup:
//             copying it to LDS with register staging and with LDS-DMA, and (hub_block_direct, the form the library has) loading
//             each wavefront's fragments straight into its registers.
// 50 launches each back to back, best of three (and the spread of the three beside it), the largest difference from an fp64
// sum on every 61st hub row, and from today's kernel on all rows (0 = the same bits).  Measurement only: nothing in the
// library uses it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 hub_block_presplit_probe.hip -o hub_block_presplit_probe && ./hub_block_presplit_probe
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
    const uint16_t *bm;
    const unsigned char *img;            // the split image (the image-reading kernels)
    const float *row_scale;
    const int32_t *stale;
    int32_t seq;
    int H_pad, D, ldx, ldy;
    int scaled;
    float eps;
};

// ---- today's kernel (copy of csrc/gnna_dense.hip before the split pass) -------------------------------------------------------------------
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
hub_block_today(const HubParams p)
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

// ---- the split pass and the image-reading kernel (as in csrc/gnna_dense.hip) ---------------------------------------
constexpr int kImgFrag = 1024;                 // one B fragment: 64 lanes x 16 bytes, lane-linear
constexpr int kImgPiece = 16 * kImgFrag;       // [step 4][column tile 4] fragments of one of the three pieces
constexpr int kImgChunk = 3 * kImgPiece;       // 49,152 bytes per 128-rank chunk
constexpr int kSplitThreads = 128;             // threads per 32-rank step of hub_split_kernel

struct SplitParams {
    const float *X;
    const int32_t *r2n;
    unsigned char *img;
    const int32_t *stale;
    int32_t seq;
    int H_pad, D, ldx;
};

// The three bf16 pieces of the hub rows of X, once per call, in the order hub_block_kernel multiplies them: per 128-rank chunk
// [piece 3][step 4][column tile 4] fragments of 64 lanes x 16 bytes, lane 16 kg + n = the ranks 8 kg .. 8 kg + 7 of the step at
// column n of the tile.  A padding rank and the columns from D on are zeros.  128 threads take a step: thread (g, pc) fetches 4
// columns of 4 consecutive ranks, splits them into an LDS image of the step, and the image goes out 16 bytes per lane.
// FULL: D and ldx are multiples of 4 and X is 16-byte aligned, so every 16-byte piece is whole and aligned.
template <bool FULL, int SPB>
__global__ void __launch_bounds__(kSplitThreads * SPB)
hub_split_kernel(const SplitParams p)
{
    if (*p.stale == p.seq) return;
    __shared__ __attribute__((aligned(16))) unsigned char s_img[SPB][3 * 4 * kImgFrag];
    const int tid = (int)threadIdx.x;
    const int sl = tid >> 7, t = tid & (kSplitThreads - 1);
    const int g = t >> 4, pc = t & 15;
    const int step = (int)blockIdx.x * SPB + sl;
    const int D = p.D;
    const HubIT node = *reinterpret_cast<const HubIT *>(&p.r2n[step * 32 + 4 * g]);
    HubVT v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int nd = node[k];
        const float *src = p.X + (size_t)(nd < 0 ? 0 : nd) * (size_t)p.ldx + 4 * pc;
        HubVT x = (HubVT)(0.f);
        if (nd >= 0) {
            if constexpr (FULL) {
                if (4 * pc < D) x = *reinterpret_cast<const HubVT *>(src);
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (4 * pc + q < D) x[q] = src[q];
            }
        }
        v[k] = x;
    }
    unsigned char *mine = s_img[sl];
    const int wbase = (pc >> 2) * kImgFrag + (16 * (g >> 1) + 4 * (pc & 3)) * 16 + 8 * (g & 1);
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
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
            *reinterpret_cast<HubU2 *>(&mine[wbase + i * 4 * kImgFrag + cc * 16]) = o;
        }
    }
    __syncthreads();
    unsigned char *out = p.img + (size_t)(step >> 2) * kImgChunk + (size_t)(step & 3) * 4 * kImgFrag;
#pragma unroll
    for (int u = 0; u < 6; u++) {
        const int idx = u * kSplitThreads + t;
        const int i = idx >> 8, off = (idx & 255) * 16;
        *reinterpret_cast<HubU4 *>(&out[i * kImgPiece + off]) = *reinterpret_cast<const HubU4 *>(&mine[i * 4 * kImgFrag + off]);
    }
}

// A workgroup owns TM destination ranks (TM / 16 MFMA tiles, TM / 32 tile rows of the bitmap) and walks ALL source ranks, 128
// at a time: per chunk it copies the 48 KB of the split image (36 for NT = 3: column tile 3 is never read) into one of two LDS
// images, fragment by fragment over the wavefronts, and does no arithmetic on X.  DMA = 0: through registers, three stages --
// the global_load_dwordx4 of chunk c + 3 and the ds_write_b128 of chunk c + 1 one by one between the MFMAs.  DMA = 1: LDS-DMA of
// chunk c + 1, one by one between the MFMAs, drained before the barrier.  The wavefront split (step w % 4, column half w / 4),
// the two accumulators, the order of a destination element's sums and the end of the kernel are those of the kernel above.
// (Measured and not taken: hub_block_direct below needs no LDS image.)
template <int NT, int TM, int DMA>
__global__ void __launch_bounds__(kHubThreads)
hub_block_kernel(const HubParams p)
{
    if (*p.stale == p.seq) return;       // the ids changed since the block was made: the sweep kernel does the whole call
    constexpr int TR = TM / 32;          // tile rows of the bitmap
    constexpr int kFrags = 12 * NT, kCopies = (kFrags + kHubWaves - 1) / kHubWaves;
    static_assert((TM == 32 || TM == 64) && (NT == 3 || NT == 4), "tile shapes");
    __shared__ __attribute__((aligned(16))) unsigned char s_x[2][kImgChunk];
    static_assert(4 * TM * 64 * 4 <= 2 * kImgChunk, "the partial tiles fit over the images");
    const uint16_t *bm = p.bm;
    const int tid = (int)threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = p.H_pad / kHubKC;
    const int steps = p.H_pad >> 5;      // 32-rank steps of a row of the bitmap
    const int D = p.D;
    const int cs = wib & 3, ch = wib >> 2;                  // this wavefront's step of a chunk and its half of the columns

    // the copy: fragment f = 8 k + w of the NT column tiles of the 12 (piece, step) pairs
    int cbase[kCopies];
#pragma unroll
    for (int k = 0; k < kCopies; k++) {
        const int f = k * kHubWaves + wib;
        cbase[k] = ((f / NT) * 4 + f % NT) * kImgFrag;
    }
    auto copies = [&](int k) { return (k + 1) * kHubWaves <= kFrags || k * kHubWaves + wib < kFrags; };
    struct Stage {
        HubU4 r[kCopies];
        uint32_t w[TR];                  // this wavefront's step of the bitmap per tile row: byte 0 the first destination tile, byte 1 the second
    };
    auto chunk_at = [&](int c) {                             // (a chunk beyond the last is the last one again: fetched, never multiplied)
        return p.img + (size_t)(c < chunks ? c : chunks - 1) * kImgChunk + lane * 16;
    };
    auto fetch_row = [&](const unsigned char *src, int k, Stage &st) {
        if (k < kCopies && copies(k)) st.r[k] = *reinterpret_cast<const HubU4 *>(src + cbase[k]);
    };
    auto fetch_words = [&](int c, Stage &st) {
        const int cc = c < chunks ? c : chunks - 1;
#pragma unroll
        for (int tr = 0; tr < TR; tr++)
            st.w[tr] = bm[((size_t)((int)blockIdx.x * TR + tr) * (size_t)steps + (size_t)(cc * 4 + cs)) * 64 + (size_t)lane];
    };
    auto write_row = [&](int k, const Stage &st, unsigned char *image) {
        if (k < kCopies && copies(k)) *reinterpret_cast<HubU4 *>(&image[cbase[k] + lane * 16]) = st.r[k];
    };
    auto dma_row = [&](const unsigned char *src, int k, unsigned char *image) {
        if (k < kCopies && copies(k))
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + cbase[k]),
                                             (__attribute__((address_space(3))) void *)(&image[cbase[k]]), 16, 0, 0);
    };

    const int rbase = (cs * 4 + 2 * ch) * kImgFrag + lane * 16;
    HubVT acc_hi[2 * TR][2], acc_lo[2 * TR][2];             // [destination tile][column tile of the half]
#pragma unroll
    for (int t = 0; t < 2 * TR; t++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc_hi[t][q] = acc_lo[t][q] = (HubVT)(0.f);

    // Chunk c out of image c % 2 with the bitmap bytes of stage L, which then starts on chunk c + 3; stage S holds chunk c + 1,
    // which goes into the other image.  A turn is six parts, pinned in this order: the MFMAs of one piece (hi, mid, lo) and one
    // column tile, one load of L, one fragment of S written.  The loads are spread like this because the compute unit's address
    // unit takes about as long for a chunk's 48 KB (48 wave-wide 16-byte loads) as the matrix units do for a 64-rank tile: issued
    // in one burst by all eight wavefronts they fill its queue, a wavefront stands at its next load until the queue has room, and
    // nothing else is issued meanwhile.
    auto turn = [&](int c, Stage &L, const Stage &S) {
        const unsigned char *cur = s_x[c & 1];
        unsigned char *nxt = s_x[(c & 1) ^ 1];
        const unsigned char *src = chunk_at(DMA ? c + 1 : c + 3);
        __builtin_amdgcn_sched_barrier(0);
        HubFrag b[2][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int q = 0; q < 2; q++)
                if (NT == 4 || q == 0 || ch == 0) b[q][i] = *reinterpret_cast<const HubFrag *>(&cur[rbase + q * kImgFrag + i * kImgPiece]);
        HubFrag a[2 * TR];
#pragma unroll
        for (int t = 0; t < 2 * TR; t++) a[t] = hub_ones((L.w[t >> 1] >> (8 * (t & 1))) & 0xffu);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (NT == 4 || q == 0 || ch == 0) {
#pragma unroll
                    for (int t = 0; t < 2 * TR; t++) {
                        if (k == 0) acc_hi[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[q][0], acc_hi[t][q], 0, 0, 0);
                        else acc_lo[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[q][k], acc_lo[t][q], 0, 0, 0);
                    }
                }
                if (DMA) {
                    dma_row(src, 2 * k + q, nxt);
                } else {
                    fetch_row(src, 2 * k + q, L);
                    write_row(2 * k + q, S, nxt);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        fetch_words(c + 3, L);
        __builtin_amdgcn_sched_barrier(0);
        if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                     // `nxt` is whole, and `cur` has been read by every wavefront
    };
    // Three stages take the chunks in turn (chunk c lives in stage c % 3): while chunk c is multiplied out of one image, chunk
    // c + 1 goes from its stage into the other image, chunk c + 2 is on its way and chunk c + 3 is asked for.
    Stage s0, s1, s2;
    // (the order of the loads is that of the turns, and pinned: the counted waits of the loop are those of its entry as well)
    if (DMA) {
#pragma unroll
        for (int k = 0; k < kCopies; k++) dma_row(chunk_at(0), k, s_x[0]);
        fetch_words(0, s0);
        fetch_words(1, s1);
        fetch_words(2, s2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
#pragma unroll
        for (int k = 0; k < kCopies; k++) fetch_row(chunk_at(0), k, s0);
        fetch_words(0, s0);
#pragma unroll
        for (int k = 0; k < kCopies; k++) fetch_row(chunk_at(1), k, s1);
        fetch_words(1, s1);
#pragma unroll
        for (int k = 0; k < kCopies; k++) fetch_row(chunk_at(2), k, s2);
        fetch_words(2, s2);
#pragma unroll
        for (int k = 0; k < kCopies; k++) write_row(k, s0, s_x[0]);
    }
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

    // the 4 partial tiles of the workgroup's TM rows, side by side, then summed in step order
    // (the last turn ended with a barrier: nobody reads the images any more)
    float *part = reinterpret_cast<float *>(&s_x[0][0]);     // [step][TM ranks][64 columns]; the columns from 16 NT on stay unwritten and unread
#pragma unroll
    for (int t = 0; t < 2 * TR; t++)
#pragma unroll
        for (int q = 0; q < 2; q++)
            if (NT == 4 || q == 0 || ch == 0) {
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

// The same sums with no LDS image at all.  The 8 wavefronts of a workgroup split a chunk as (step w % 4, column half w / 4), and a
// fragment of the split image IS the B operand of one MFMA: the 6 fragments a wavefront multiplies are 6 wave-wide 16-byte loads
// straight into its registers, the 8 wavefronts read the chunk's 48 fragments once between them, and nothing is shared before
// the partial tiles at the end -- no barrier in the loop.  Three register stages take the chunks in turn (chunk c lives in
// stage c % 3): a piece's two fragments are asked for again, three chunks ahead, as soon as its MFMAs are issued.
template <int NT, int TM>
__global__ void __launch_bounds__(kHubThreads)
hub_block_direct(const HubParams p)
{
    if (*p.stale == p.seq) return;       // the ids changed since the block was made: the sweep kernel does the whole call
    constexpr int TR = TM / 32;          // tile rows of the bitmap
    static_assert((TM == 32 || TM == 64) && (NT == 3 || NT == 4), "tile shapes");
    __shared__ __attribute__((aligned(16))) float s_part[4 * TM * 64];
    const int tid = (int)threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = p.H_pad / kHubKC;
    const int steps = p.H_pad >> 5;      // 32-rank steps of a row of the bitmap
    const int D = p.D;
    const int cs = wib & 3, ch = wib >> 2;                  // this wavefront's step of a chunk and its half of the columns
    const bool two = NT == 4 || ch == 0;                    // (wave-uniform) the half has a second column tile
    const unsigned char *frag0 = p.img + (size_t)(cs * 4 + 2 * ch) * kImgFrag + (size_t)lane * 16;
    const uint16_t *word0 = p.bm + ((size_t)blockIdx.x * TR * (size_t)steps + (size_t)cs) * 64 + (size_t)lane;
    struct Stage {
        HubFrag b[2][3];                 // [column tile of the half][piece]
        uint32_t w[TR];                  // this wavefront's step of the bitmap per tile row: byte 0 the first destination tile, byte 1 the second
    };
    // (a chunk beyond the last is the last one again: fetched, never multiplied)
    auto fetch_piece = [&](int c, int i, Stage &st) {
        const unsigned char *src = frag0 + (size_t)(c < chunks ? c : chunks - 1) * kImgChunk + i * kImgPiece;
        st.b[0][i] = *reinterpret_cast<const HubFrag *>(src);
        if (two) st.b[1][i] = *reinterpret_cast<const HubFrag *>(src + kImgFrag);
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

// ---- the synthetic block -------------------------------------------------------------------------------------------
inline uint64_t mix(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

struct Timing {
    double best = 1e30, worst = 0.0;     // us per launch: the best and the worst of the three repetitions
};

template <class F>
Timing time_launches(F launch, int launches, hipEvent_t e0, hipEvent_t e1)
{
    Timing t;
    for (int rep = 0; rep < 3; rep++) {
        CHECK(hipEventRecord(e0, 0));
        for (int i = 0; i < launches; i++) launch();
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const double us = (double)ms * 1e3 / launches;
        t.best = std::min(t.best, us);
        t.worst = std::max(t.worst, us);
    }
    return t;
}

void run(int H, int inv_density, int N, int D, const float *dX, const std::vector<float> &X, int launches)
{
    const int H_pad = (H + kHubKC - 1) / kHubKC * kHubKC;
    // hubs: every (N / H)-th node, in id order
    std::vector<int32_t> r2n((size_t)H_pad, -1);
    for (int i = 0; i < H; i++) r2n[(size_t)i] = (int32_t)((int64_t)i * N / H);
    std::vector<uint32_t> bm16((size_t)H_pad * (size_t)H_pad / 32, 0u);
    const int steps = H_pad / 32;
    auto bit_at = [&](int d, int s, size_t *word, uint32_t *bit) {
        const size_t half = ((size_t)(d >> 5) * steps + (size_t)(s >> 5)) * 64 + (size_t)((d & 15) + 16 * ((s & 31) >> 3));
        *word = half >> 1;
        *bit = 1u << (16 * (half & 1) + 8 * ((d >> 4) & 1) + (s & 7));
    };
    for (int d = 0; d < H; d++)
        for (int s0 = 0; s0 < H; s0 += 64) {
            uint64_t r = mix((uint64_t)d * 1000003ull + (uint64_t)s0), r2 = mix(r);
            uint64_t bits = inv_density == 4 ? (r & r2) : (r & r2 & mix(r2));
            for (int b = 0; b < 64 && s0 + b < H; b++) {
                if (!((bits >> b) & 1ull)) continue;
                size_t word; uint32_t bit;
                bit_at(d, s0 + b, &word, &bit);
                bm16[word] |= bit;
            }
        }
    int32_t *d_r2n, *d_stale;
    void *d_bm16, *d_img;
    float *dY;
    CHECK(hipMalloc(&d_r2n, (size_t)H_pad * 4 + kHubZeros * 4));       // (the ranks, and the zeros behind them)
    CHECK(hipMemset(d_r2n, 0, (size_t)H_pad * 4 + kHubZeros * 4));
    CHECK(hipMalloc(&d_stale, 4));
    CHECK(hipMalloc(&d_bm16, bm16.size() * 4));
    CHECK(hipMalloc(&d_img, (size_t)(H_pad / kHubKC) * kImgChunk));
    CHECK(hipMalloc(&dY, (size_t)N * D * 4));
    CHECK(hipMemcpy(d_r2n, r2n.data(), (size_t)H_pad * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_stale, 0, 4));
    CHECK(hipMemcpy(d_bm16, bm16.data(), bm16.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_img, 0xff, (size_t)(H_pad / kHubKC) * kImgChunk));
    HubParams p;
    p.X = dX; p.Y = dY; p.r2n = d_r2n; p.bm = static_cast<const uint16_t *>(d_bm16); p.img = static_cast<const unsigned char *>(d_img);
    p.row_scale = nullptr; p.stale = d_stale; p.seq = 1; p.H_pad = H_pad; p.D = D; p.ldx = D; p.ldy = D;
    p.scaled = 0; p.eps = 0.f;
    SplitParams sp;
    sp.X = dX; sp.r2n = d_r2n; sp.img = static_cast<unsigned char *>(d_img); sp.stale = d_stale; sp.seq = 1; sp.H_pad = H_pad; sp.D = D; sp.ldx = D;
    const dim3 block(kHubThreads);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));

    // the split pass, with one and with four steps per workgroup (the image of the second stays for the kernels below)
    auto split1 = [&]() { hipLaunchKernelGGL((hub_split_kernel<true, 1>), dim3((unsigned)(H_pad / 32)), dim3(kSplitThreads), 0, 0, sp); };
    auto split4 = [&]() { hipLaunchKernelGGL((hub_split_kernel<true, 4>), dim3((unsigned)(H_pad / 128)), dim3(4 * kSplitThreads), 0, 0, sp); };
    const Timing ts1 = time_launches(split1, launches, e0, e1);
    std::vector<unsigned char> img1((size_t)(H_pad / kHubKC) * kImgChunk), img4(img1.size());
    CHECK(hipMemcpy(img1.data(), d_img, img1.size(), hipMemcpyDeviceToHost));
    CHECK(hipMemset(d_img, 0xff, img1.size()));
    const Timing ts4 = time_launches(split4, launches, e0, e1);
    CHECK(hipMemcpy(img4.data(), d_img, img4.size(), hipMemcpyDeviceToHost));
    const bool same_img = img1 == img4;

    std::vector<float> y_today((size_t)N * D), y((size_t)N * D);
    auto one = [&](auto launch, std::vector<float> &into) {               // the result of ONE launch into zeros
        CHECK(hipMemset(dY, 0, (size_t)N * D * 4));
        launch();
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(into.data(), dY, (size_t)N * D * 4, hipMemcpyDeviceToHost));
    };
    auto today = [&]() { hipLaunchKernelGGL((hub_block_today<4, true>), dim3((unsigned)(H_pad / 32)), block, 0, 0, p); };
    one(today, y_today);
    const Timing tt = time_launches(today, launches, e0, e1);
    // fp64 sums of every 61st hub row
    double err64 = 0.0, ref64 = 0.0;
    std::vector<std::vector<double>> sums;
    for (int d = 0; d < H; d += 61) {
        std::vector<double> sum((size_t)D, 0.0);
        for (int s = 0; s < H; s++) {
            size_t word; uint32_t bit;
            bit_at(d, s, &word, &bit);
            if (bm16[word] & bit)
                for (int c = 0; c < D; c++) sum[(size_t)c] += (double)X[(size_t)r2n[(size_t)s] * D + c];
        }
        sums.push_back(sum);
    }
    auto err_of = [&](const std::vector<float> &got) {
        double e = 0.0;
        size_t k = 0;
        for (int d = 0; d < H; d += 61, k++)
            for (int c = 0; c < D; c++) {
                e = std::max(e, std::fabs(sums[k][(size_t)c] - (double)got[(size_t)r2n[(size_t)d] * D + c]));
                ref64 = std::max(ref64, std::fabs(sums[k][(size_t)c]));
            }
        return e;
    };
    err64 = err_of(y_today);
    std::printf("| %d | 1/%d | today | %.1f (+%.1f) | | %.3e (%.1f) | |\n", H, inv_density, tt.best, tt.worst - tt.best, err64, ref64);
    std::printf("| %d | 1/%d | split, 1 step per workgroup | %.1f (+%.1f) | | | |\n", H, inv_density, ts1.best, ts1.worst - ts1.best);
    std::printf("| %d | 1/%d | split, 4 steps per workgroup | %.1f (+%.1f) | | | images %s |\n", H, inv_density, ts4.best, ts4.worst - ts4.best,
                same_img ? "equal" : "DIFFER");
    const double tsplit = std::min(ts1.best, ts4.best);
    auto variant = [&](const char *name, auto launch) {
        one(launch, y);
        const Timing t = time_launches(launch, launches, e0, e1);
        double diff = 0.0;
        for (size_t i = 0; i < y.size(); i++) diff = std::max(diff, (double)std::fabs(y[i] - y_today[i]));
        std::printf("| %d | 1/%d | %s | %.1f (+%.1f) | %.1f | %.3e | %.3e |\n", H, inv_density, name, t.best, t.worst - t.best, t.best + tsplit,
                    err_of(y), diff);
        std::fflush(stdout);
    };
    variant("image, 32 ranks, registers", [&]() { hipLaunchKernelGGL((hub_block_kernel<4, 32, 0>), dim3((unsigned)(H_pad / 32)), block, 0, 0, p); });
    variant("image, 32 ranks, LDS-DMA", [&]() { hipLaunchKernelGGL((hub_block_kernel<4, 32, 1>), dim3((unsigned)(H_pad / 32)), block, 0, 0, p); });
    variant("image, 64 ranks, registers", [&]() { hipLaunchKernelGGL((hub_block_kernel<4, 64, 0>), dim3((unsigned)(H_pad / 64)), block, 0, 0, p); });
    variant("image, 64 ranks, LDS-DMA", [&]() { hipLaunchKernelGGL((hub_block_kernel<4, 64, 1>), dim3((unsigned)(H_pad / 64)), block, 0, 0, p); });
    variant("image, 32 ranks, no LDS", [&]() { hipLaunchKernelGGL((hub_block_direct<4, 32>), dim3((unsigned)(H_pad / 32)), block, 0, 0, p); });
    variant("image, 64 ranks, no LDS", [&]() { hipLaunchKernelGGL((hub_block_direct<4, 64>), dim3((unsigned)(H_pad / 64)), block, 0, 0, p); });
    CHECK(hipFree(d_r2n)); CHECK(hipFree(d_stale)); CHECK(hipFree(d_bm16)); CHECK(hipFree(d_img)); CHECK(hipFree(dY));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
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
    std::printf("| H | density | kernel | us per launch: best of three (+ spread) | with the split pass | max abs diff from fp64 (max abs fp64 sum) | max abs diff from today's kernel |\n|---|---|---|---|---|---|---|\n");
    const int Hs[5] = {4096, 6144, 8192, 12416, 16384}, inv[2] = {4, 8};
    for (int a = 0; a < 5; a++)
        for (int b = 0; b < 2; b++) run(Hs[a], inv[b], N, D, dX, X, 50);
    CHECK(hipFree(dX));
    return 0;
}

// gnna_launch.h -- launch geometry of the kernels of libgnna.so: the block shape and the host arithmetic that turns a call's
// sizes into a grid and a lane layout.  Every kernel family calls these and does not copy them.  Plain host functions without
// a HIP type, so a test compiles this header with the host compiler alone (tests/test_launch_geometry.py).
#ifndef GNNA_LAUNCH_H_
#define GNNA_LAUNCH_H_

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace gnna {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kXcds = 8;

// Grid of a gather whose wavefronts take chunks of G consecutive neighbor-groups: G = 64 (about 2048 edges per wavefront at
// most), fewer while that leaves compute units without a chunk; kWavesPerBlock chunks per block.  The caller refuses
// blocks > 0x7fffffff in its own words.
struct ChunkGrid {
    int G;
    int64_t blocks;
};
inline ChunkGrid chunk_grid(int64_t num_parts, int partSize, int num_cus)
{
    int G = std::max(1, std::min(kWave, 2048 / std::max(1, partSize)));
    while (G > 1 && (num_parts + G - 1) / G < (int64_t)num_cus * 16) G >>= 1;
    const int64_t chunks = (num_parts + G - 1) / G;
    return {G, (chunks + kWavesPerBlock - 1) / kWavesPerBlock};
}

// log2 of the lanes that cover `dim` elements at elems_per_lane each: the smallest power of two that does, 2^cap at most
// (wider rows are taken in column blocks).
inline int log2_lanes(int dim, int elems_per_lane, int cap = 6)
{
    int l = 0;
    while (l < cap && (elems_per_lane << l) < dim) l++;
    return l;
}

// f(std::integral_constant<int, L>) for L = log_lpr in 0 .. 6 (above: 6): a run-time lane count becomes a template argument.
template <class F>
void dispatch_lpr(int log_lpr, F &&f)
{
    switch (log_lpr) {
    case 0: f(std::integral_constant<int, 0>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    default: f(std::integral_constant<int, 6>()); break;
    }
}

// Lane layout of the fused attention kernels (gnna_gat.hip, gnna_gatv2.hip, gnna_dotattn.hip): 2^log_lph lanes of 4 floats cover
// a head of `dim` floats, 2^log_lpr lanes a row of a column block -- as many whole heads as fit in a wavefront, `heads` at most.
struct AttnLayout {
    int log_lph, log_lpr;
};
inline AttnLayout attn_layout(int heads, int dim)
{
    const int log_lph = log2_lanes(dim, 4);
    int log_lpr = log_lph;
    while (log_lpr < 6 && (1 << (log_lpr - log_lph)) < heads) log_lpr++;
    return {log_lph, log_lpr};
}

// f(std::integral_constant<int, log_lph>, std::integral_constant<int, log_lpr>) for the layouts that exist (a row has at least
// the lanes of one head).
template <class F>
void dispatch_layout(AttnLayout layout, F &&f)
{
    dispatch_lpr(layout.log_lph, [&](auto H) {
        dispatch_lpr(layout.log_lpr, [&](auto L) {
            if constexpr (decltype(L)::value >= decltype(H)::value) f(H, L);
        });
    });
}

// Blocks of a grid-stride kernel over `items` work items: one thread each, blocks_per_cu blocks per compute unit at most.
inline unsigned elementwise_grid(int64_t items, int num_cus, int blocks_per_cu)
{
    const int64_t blocks = (items + kBlock - 1) / kBlock;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)num_cus * blocks_per_cu));
}

// the smallest power of two >= x (1 for x <= 1)
inline int pow2_at_least(int64_t x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// a row stride that is narrower than the row or does not fit the kernels' 32-bit element offsets
inline bool bad_ld(int64_t ld, int64_t width) { return ld < width || ld >= ((int64_t)1 << 29); }
// the stride of an operand that may be null: checked against its width only where something is strided by it
inline bool bad_ld_of(const void *ptr, int64_t ld, int64_t width) { return ptr ? bad_ld(ld, width) : ld >= ((int64_t)1 << 29); }

}  // namespace gnna

#endif

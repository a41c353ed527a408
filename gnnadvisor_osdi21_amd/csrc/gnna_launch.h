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

// ---- the pre-pass launch of an aggregation call (prepass_kernel, gnna_agg.hip) ----------------------------------------------
// One grid whose blocks are divided among up to four roles: staging copy, output fill (+ partition validation), packed-id check
// and hub-row split.  A role without work has no blocks.  The grid begins with the split blocks (short blocks with a barrier:
// first, so that they are not the tail), then the check block, then the stage and fill blocks -- alternating block by block
// while both roles have blocks left (`interleave`), else the stage range ahead of the fill range.  Plain arithmetic: the launcher
// fills a PrepassGrid and the kernel asks prepass_role_of for its block; a host program asks both (tests/test_prepass_grid.py).
#if defined(__HIPCC__)
#define GNNA_HOST_DEVICE __host__ __device__
#else
#define GNNA_HOST_DEVICE
#endif
enum { PREPASS_STAGE = 0, PREPASS_FILL = 1, PREPASS_CHECK = 2, PREPASS_SPLIT = 3, PREPASS_ROLES = 4 };
struct PrepassGrid {
    unsigned count[PREPASS_ROLES];   // blocks of each role
    unsigned check_begin;            // = count[PREPASS_SPLIT]
    unsigned pass_begin;             // the first stage / fill block
    unsigned pairs;                  // stage and fill blocks that alternate: min(stage, fill) when interleaved, else 0
    unsigned total;
};
struct PrepassRole {
    int role;
    unsigned index, count;           // the block's index among the blocks of its role, and how many those are
};
// Blocks of a grid-stride pass over `items` work items, one thread each: none for no items, at most 8 per compute unit.
inline unsigned prepass_pass_blocks(uint64_t items, int num_cus)
{
    if (items == 0) return 0u;
    const uint64_t blocks = items / (uint64_t)kBlock + (items % (uint64_t)kBlock != 0 ? 1 : 0);    // (no sum that could wrap)
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(1, num_cus) * 8));
}
// stage_items: 16-byte pieces of the rows to copy; fill_items: max(16-byte pieces of the output, neighbor-groups to validate);
// check: the packed-id sample check runs (one block); split_steps: 32-rank steps of the hub-row split (one block each).
inline PrepassGrid prepass_grid(uint64_t stage_items, uint64_t fill_items, bool check, unsigned split_steps, int num_cus, bool interleave)
{
    PrepassGrid g;
    g.count[PREPASS_STAGE] = prepass_pass_blocks(stage_items, num_cus);
    g.count[PREPASS_FILL] = prepass_pass_blocks(fill_items, num_cus);
    g.count[PREPASS_CHECK] = check ? 1u : 0u;
    g.count[PREPASS_SPLIT] = split_steps;
    g.check_begin = g.count[PREPASS_SPLIT];
    g.pass_begin = g.check_begin + g.count[PREPASS_CHECK];
    g.pairs = interleave ? std::min(g.count[PREPASS_STAGE], g.count[PREPASS_FILL]) : 0u;
    g.total = g.pass_begin + g.count[PREPASS_STAGE] + g.count[PREPASS_FILL];
    return g;
}
// The role of block `block` < g.total.
GNNA_HOST_DEVICE inline PrepassRole prepass_role_of(const PrepassGrid &g, unsigned block)
{
    if (block < g.check_begin) return {PREPASS_SPLIT, block, g.count[PREPASS_SPLIT]};
    if (block < g.pass_begin) return {PREPASS_CHECK, block - g.check_begin, g.count[PREPASS_CHECK]};
    unsigned j = block - g.pass_begin;
    if (j < 2u * g.pairs) {
        const int role = (j & 1u) ? PREPASS_FILL : PREPASS_STAGE;
        return {role, j >> 1, g.count[role]};
    }
    j -= 2u * g.pairs;                // what is left of the two ranges, stage first
    const unsigned stage_left = g.count[PREPASS_STAGE] - g.pairs;
    if (j < stage_left) return {PREPASS_STAGE, g.pairs + j, g.count[PREPASS_STAGE]};
    return {PREPASS_FILL, g.pairs + (j - stage_left), g.count[PREPASS_FILL]};
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

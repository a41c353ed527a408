// gnna_segments.h -- what the kernels over the contiguous row segments of a batch of graphs share (gnna_pool.hip: sum / mean /
// max / min; gnna_attnpool.hip: attention pooling; gnna_segnorm.hip: GraphNorm).  The geometry: a wavefront owns a tile of kTile
// consecutive rows, a workgroup four tiles; kRowsInFlight rows per slot and step; a segment of more than kLongSteps join steps
// goes to the whole workgroup.  On the device: the clamped pointers, the search for a tile's first segment, a 64-bit value made
// uniform over a wavefront, the partial store of a lane's four columns (gnna_topk.hip uses these too), exp of a non-positive
// number (with gnna_softagg.hip).  The kernels keep their loops in their own files: a walk and a join shared through
// force-inlined functions compiled to slower code for some lane layouts (profiles/segment_walk/).  On the host: the size checks of every entry, the carving of the two pieces
// per tile from a scratch slot, and the pair of launches (tiles, then finish).  Not installed.
#ifndef GNNA_SEGMENTS_H_
#define GNNA_SEGMENTS_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "gnna_pool.h"           // GNNA_POOL_TILE_ROWS, GNNA_POOL_LONG_STEPS: the geometry all three share
#include "gnna_gat_common.h"     // gat::VT, gat::MT
#include "gnna_internal.h"

namespace gnna {
namespace seg {

constexpr int kTile = GNNA_POOL_TILE_ROWS;
constexpr int kRowsInFlight = 4;     // rows per slot and step of a row walk: 16-byte loads in flight per lane and array loaded
// A segment whose pieces would keep its wavefront for more than kLongSteps steps of the join goes to the whole block.
constexpr int kLongSteps = GNNA_POOL_LONG_STEPS;

// graph_pointers[g] clamped to [0, N]; the same value in every lane of a wavefront whose lanes ask for the same g
__device__ __forceinline__ int64_t seg_ptr(const int32_t *__restrict__ gp, int64_t N, int64_t g)
{
    const int64_t v = gp[g];
    return v < 0 ? 0 : (v > N ? N : v);
}

// the first segment whose end lies beyond row r (G: none): where the walk of a tile that begins at r starts
__device__ __forceinline__ int64_t first_segment(const int32_t *__restrict__ gp, int64_t G, int64_t N, int64_t r)
{
    int64_t lo = 0, hi = G;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (seg_ptr(gp, N, mid + 1) > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the first n4 (<= 4) floats of v to q
__device__ __forceinline__ void store_piece(float *__restrict__ q, const gat::VT v, int n4)
{
    if (n4 >= 4) {
        *reinterpret_cast<gat::MT *>(q) = v;
        return;
    }
    if (n4 > 0) q[0] = v[0];
    if (n4 > 1) q[1] = v[1];
    if (n4 > 2) q[2] = v[2];
}

// exp(d) for d <= 0 (and -inf -> 0): one v_exp_f32.  The product d * log2(e) is rounded once, an error of at most |d| * 2^-24 in
// the exponent, i.e. |d| * e^d * 2^-24 <= 2^-24 / e in the value: every use is a weight relative to a maximum of 1, where that is
// below half an ulp of the largest weight.
__device__ __forceinline__ float exp_nonpos(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }

// ---- host ---------------------------------------------------------------------------------------------------------------------

// what every entry checks alike after its flags, before any device work: the width (attention pooling checks its gate_dim
// between the two), then the counts
inline int check_dim(const char *what, int dim)
{
    return dim < 1 ? fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dim must be >= 1 (got %d)", what, dim) : GNNA_OK;
}
inline int check_counts(const char *what, int64_t num_rows, int64_t num_segments)
{
    if (num_rows < 0 || num_segments < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_rows=%lld num_segments=%lld)", what, (long long)num_rows,
                    (long long)num_segments);
    if (num_segments >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld segments in one call (at most 536870911): shard the batch", what,
                    (long long)num_segments);
    if (num_rows > 0x7fffffffll)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 2147483647: graph_pointers is int32)", what,
                    (long long)num_rows);
    return GNNA_OK;
}

// The pieces of a call's tiles, two per tile, in scratch slot `slot`: K arrays one after the other, array i with piece_bytes[i]
// bytes per piece (the caller puts 8-byte cells first).  out[i]: null for an array of no bytes and for a call without rows.
// Eager calls of a stream share the slot (grow-only), a captured call gets its capture's own.
template <size_t K>
int get_pieces(DeviceState *ds, hipStream_t stream, int slot, int64_t num_rows, const size_t (&piece_bytes)[K], void *(&out)[K])
{
    const size_t pieces = (size_t)((num_rows + kTile - 1) / kTile) * 2;
    size_t bytes = 0;
    for (size_t i = 0; i < K; i++) { out[i] = nullptr; bytes += pieces * piece_bytes[i]; }
    if (pieces == 0) return GNNA_OK;
    void *ws = nullptr;
    const int rc = get_workspace(ds, stream, slot, align256(bytes), &ws);
    if (rc != GNNA_OK) return rc;
    char *at = static_cast<char *>(ws);
    for (size_t i = 0; i < K; i++) {
        if (piece_bytes[i]) out[i] = at;
        at += pieces * piece_bytes[i];
    }
    return GNNA_OK;
}

// The tile kernels, then the finish kernels of a call with G > 0 (a.N rows, a.G segments).  kernels_of(L) gives the pair
// (tile kernel, finish kernel) for LOG_LPR = L.
template <class Args, class KernelsOf>
int launch_tiles_then_finish(const char *noun, int log_lpr, hipStream_t stream, const Args &a, KernelsOf kernels_of)
{
    const int64_t tiles = (a.N + kTile - 1) / kTile;
    int rc = GNNA_OK;
    dispatch_lpr(log_lpr, [&](auto L) {
        const auto kernels = kernels_of(L);
        if (tiles > 0) {
            hipLaunchKernelGGL(kernels.first, dim3((unsigned)((tiles + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, stream, a);
            if ((rc = launch_ok("%s: tile launch", noun)) != GNNA_OK) return;
        }
        hipLaunchKernelGGL(kernels.second, dim3((unsigned)((a.G + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, stream, a);
        rc = launch_ok("%s: finish launch", noun);
    });
    return rc;
}

}  // namespace seg
}  // namespace gnna

#endif  // GNNA_SEGMENTS_H_

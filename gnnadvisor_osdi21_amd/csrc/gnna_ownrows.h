// gnna_ownrows.h -- what the "rows" kernels of fused attention (gnna_gat_rows.hip, gnna_dot_rows.hip) share today: the two ownership
// limits and the host side of their entries.  The kernel skeleton itself (row classification, the three walks, the long-row
// exchange through LDS) is still written out in both files: one driver for both was built, gave the same bits and no worse
// resources, and was left out because the GAT passes ran slower under it (profiles/ownrows/README.md).  gnna_edgefeat.hip, where
// the scheme came from, shares nothing here: its limits are macros that tools/probe_edge_features.py rebuilds with.
#ifndef GNNA_OWNROWS_H_
#define GNNA_OWNROWS_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gnna_gat_common.h"     // gat::kMaxDim
#include "gnna_internal.h"
#include "gnna_launch.h"

namespace gnna {
namespace own {

// a row of up to this many edges is walked by its own slot (wavefronts of more than one slot only): gnna_edgefeat.hip's limit
constexpr int kSlotEdges = 8;
// a row that would keep its wavefront for more than kLongSteps steps of EDGES edges per slot goes to the whole block: more than
// (slots of a wavefront) * 128 = (64 / LPR) * 128 edges.  First choices, not tuned.
template <int EDGES>
constexpr int kLongSteps = 128 / EDGES;
static_assert(kSlotEdges == 8 && 4 * kLongSteps<4> == 128 && 2 * kLongSteps<2> == 128,
              "include/gnna_gat_rows.h and include/gnna_dot_rows.h state the limits as 8 edges for a slot and (64 / LPR) * 128 edges "
              "for a wavefront");

// what every rows entry checks alike, before any device work: the checks of the rect entries without the partition, and without
// their refusal under gnna_tuning.deterministic = 1
inline int check_rows_sizes(const char *what, int64_t num_out_rows, int64_t num_in_rows, int heads, int dim, unsigned flags,
                            unsigned allowed_flags)
{
    if (flags & GNNA_ACCUMULATE) return fail(GNNA_ERR_UNSUPPORTED, "%s: GNNA_ACCUMULATE is not supported", what);
    if (flags & ~allowed_flags) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", what, flags);
    if (num_out_rows < 0 || num_in_rows < 0 || heads < 1 || dim < 1)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad size (num_out_rows=%lld num_in_rows=%lld heads=%d dim=%d)", what,
                    (long long)num_out_rows, (long long)num_in_rows, heads, dim);
    const int64_t most = std::max(num_out_rows, num_in_rows);
    if (most >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 536870911): shard the rows", what, (long long)most);
    if (dim > gat::kMaxDim) return fail(GNNA_ERR_UNSUPPORTED, "%s: at most %d floats per head (got %d)", what, gat::kMaxDim, dim);
    if (heads > 64) return fail(GNNA_ERR_UNSUPPORTED, "%s: at most 64 heads (got %d)", what, heads);
    return GNNA_OK;
}

// the blocks of a rows launch: a block owns (64 / LPR) * kWavesPerBlock rows (rows < 2^29)
inline dim3 rows_grid(int64_t rows, const AttnLayout &layout)
{
    const int64_t rows_per_block = (int64_t)(kWave >> layout.log_lpr) * kWavesPerBlock;
    return dim3((unsigned)std::max<int64_t>(1, (rows + rows_per_block - 1) / rows_per_block));
}

// the library scratch of a backward call: `bytes` for the records that the destination side leaves for the source side
inline int record_scratch(hipStream_t stream, int slot, size_t bytes, void **out)
{
    DeviceState *ds = nullptr;
    const int rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    return get_workspace(ds, stream, slot, align256(bytes), out);
}

}  // namespace own
}  // namespace gnna

#endif

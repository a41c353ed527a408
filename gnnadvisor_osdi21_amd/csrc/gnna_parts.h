// gnna_parts.h -- the neighbor-group partition as the device builders write it: the ONE device statement of the rule of
// gnna_build_part_i32.  A row of deg > 0 edges owns ceil(deg / partSize) consecutive groups of partSize edges from its start on
// (the last one what is left), a row without edges owns none.  The aggregation kernels trust partPtr / part2Node unchecked, so
// gnna_transpose.hip, gnna_sample.hip, gnna_topk.hip and gnna_walk.hip differ in where a row starts and what it is called,
// never in this rule.  They say so with a `Rows` functor that their fill kernel takes by value:
//   rows()    the rows that own groups (the rows first_part was counted over)
//   start(i)  the first position of row i among the result's edges
//   id(i)     what part2Node calls row i
//   end()     the result's edge count, the closing entry of partPtr
#ifndef GNNA_PARTS_H_
#define GNNA_PARTS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gnna_launch.h"

namespace gnna {

// neighbor-groups of a row of `deg` edges (none for a row whose pointers decrease)
__host__ __device__ __forceinline__ int32_t groups_of(int64_t deg, int partSize)
{
    return deg > 0 ? (int32_t)((deg + partSize - 1) / partSize) : 0;
}

// The owner of group p: the last of `rows` rows whose first group is <= p (rows without groups share their first group with
// the next row).  first_part: the exclusive scan of the rows' group counts.
__device__ __forceinline__ int64_t part_owner(const int32_t *__restrict__ first_part, int64_t rows, int64_t p)
{
    int64_t lo = 0, hi = rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (first_part[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// pp[0 .. num_parts] and p2n[0 .. num_parts) by the whole grid (grid-stride: any launch shape).  The caller has made sure that
// num_parts groups fit pp / p2n; nothing of first_part is read beyond [rows()), nothing of `r` beyond what its members name.
template <class Rows>
__device__ __forceinline__ void fill_parts(const Rows &r, const int32_t *__restrict__ first_part, int partSize, int64_t num_parts,
                                           int32_t *__restrict__ pp, int32_t *__restrict__ p2n)
{
    const int64_t rows = r.rows();
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p <= num_parts; p += (int64_t)gridDim.x * kBlock) {
        if (p == num_parts) { pp[p] = r.end(); continue; }
        const int64_t i = part_owner(first_part, rows, p);
        pp[p] = (int32_t)((int64_t)r.start(i) + (p - first_part[i]) * partSize);
        p2n[p] = r.id(i);
    }
}

// The n rows of the row pointers rp, row i called i: the partition entry of gnna_transpose.hip, a sampled block, an induced
// subgraph (whose kernel reads n on the device).
struct CsrRows {
    const int32_t *rp;
    int64_t n;
    __device__ int64_t rows() const { return n; }
    __device__ int32_t start(int64_t i) const { return rp[i]; }
    __device__ int32_t id(int64_t i) const { return (int32_t)i; }
    __device__ int32_t end() const { return n > 0 ? rp[n] : 0; }
};

}  // namespace gnna

#endif

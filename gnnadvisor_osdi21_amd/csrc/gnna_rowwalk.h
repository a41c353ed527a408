// gnna_rowwalk.h -- how the device structure builders walk a row with wavefront ballots: the ONE statement of the lane-group
// geometry, the placement by ballot prefix, the most-significant-bit-first selection of the k-th smallest 64-bit key and the
// long-row walk of a whole block.  gnna_sample.hip, gnna_walk.hip and gnna_spatial.hip differ in what a position of a row is (a
// sampling key, a column id to look up, a distance) and what a survivor is written as, never in these walks.  They say so with
// callables that take a position t of the row: "is t a survivor", "emit survivor t at `pos`", "the key of t, if t has one".
// Everything here is a ballot or a barrier, so every user keeps two invariants:
//   * every loop bound that steers a ballot is uniform over the wavefront -- rounds come from wave_max, a search goes on while
//     ANY lane group of the wavefront is searching -- so all 64 lanes reach every ballot, whatever their own row needs;
//   * every barrier is reached by the whole block: what steers for_each_flagged's callable and exchange_counts (the flags, the
//     ordinal, a row's extent and selection state) is uniform over the block, and no thread of a block leaves early.
// A slip in either is a hang, not a wrong number.
#ifndef GNNA_ROWWALK_H_
#define GNNA_ROWWALK_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gnna_launch.h"

namespace gnna {

// Every lane holds the maximum after the butterfly; reading it from the first lane tells the compiler so.  A loop bound then
// lives in a scalar register and the loop is a scalar loop: without this the long-row walks, whose bounds are uniform before
// they come here, were 13 % slower per sampling call (profiles/rowwalk/README.md).
__device__ __forceinline__ int wave_max(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return __builtin_amdgcn_readfirstlane(v);
}

// ---- lane groups ------------------------------------------------------------------------------------------------------------

// L consecutive lanes (a power of two, 4 .. 64) of a wavefront share a row: 256 / L rows per block.  L = kWave is a wavefront
// as one group, whatever row it is then given.
struct LaneGroup {
    int L, lis;                            // the lane's index in its group
    unsigned long long segmask, below;     // the group's lanes; those of them below this lane
    int64_t row;                           // of a grid with a lane group per row
    __device__ __forceinline__ explicit LaneGroup(int lanes) : L(lanes)
    {
        const int lane = threadIdx.x & (kWave - 1);
        lis = lane & (L - 1);
        segmask = (L == kWave ? ~0ull : ((1ull << L) - 1ull)) << (lane & ~(L - 1));
        below = segmask & ((1ull << lane) - 1ull);
        row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / L;
    }
};

// The survivors among positions [0, d) of the group's row, in position order without a sort: emit(pos, t) for the n-th survivor
// t with pos = out0 + n.  Returns their count (every lane of the group).  survivor(t) is asked once per position, just before
// that position's emit.
template <class Survivor, class Emit>
__device__ __forceinline__ int place_by_ballot(const LaneGroup &g, int d, int64_t out0, Survivor &&survivor, Emit &&emit)
{
    const int rounds = wave_max((d + g.L - 1) / g.L);
    int written = 0;
    for (int j = 0; j < rounds; j++) {
        const int t = j * g.L + g.lis;
        const bool p = t < d && survivor(t);
        const unsigned long long picks = __ballot(p) & g.segmask;
        if (p) emit(out0 + written + __popcll(picks & g.below), t);
        written += __popcll(picks);
    }
    return written;
}

template <class Survivor>
__device__ __forceinline__ int count_by_ballot(const LaneGroup &g, int d, Survivor &&survivor)
{
    return place_by_ballot(g, d, 0, survivor, [](int64_t, int) {});
}

// ---- the k-th smallest key ----------------------------------------------------------------------------------------------------

// The state of a most-significant-bit-first search: after bit `sh`, the wanted key agrees with `prefix` on bits 63 .. sh.  Once
// one key is left it is found, and the keys up to it are those that `keeps`.
struct Selection {
    uint64_t prefix;
    int sh;
    __device__ __forceinline__ bool agrees(uint64_t key, int b) const { return ((key ^ prefix) >> b) == 0; }
    __device__ __forceinline__ bool keeps(uint64_t key) const { return (key >> sh) <= (prefix >> sh); }
};

// One step of the search for the k-th smallest of m keys that agree with the prefix above bit b, c0 of them with bit b clear.
__device__ __forceinline__ void select_step(int b, int c0, int *k, int *m, Selection *s)
{
    if (*k <= c0) {
        *m = c0;
    } else {
        *k -= c0;
        *m -= c0;
        s->prefix |= 1ull << b;
    }
    s->sh = b;
}

// The k-th smallest of the m distinct keys among positions [0, d) of the group's row; m <= 1: nothing to search (the group
// still goes through the ballots of its wavefront).  key(t, &v): does position t have a key, and which -- a key is 64 free
// bits, so none of its values can say "no key".
template <class Key>
__device__ __forceinline__ Selection select_kth(const LaneGroup &g, int d, int k, int m, Key &&key)
{
    Selection s{0, 0};
    const int rounds = wave_max(m > 1 ? (d + g.L - 1) / g.L : 0);
    for (int b = 63; b >= 0; b--) {
        const bool act = m > 1;
        if (!__any(act)) break;
        int c0 = 0;
        for (int j = 0; j < rounds; j++) {
            const int t = j * g.L + g.lis;
            uint64_t v;
            const bool p = act && t < d && key(t, &v) && s.agrees(v, b);
            c0 += __popcll(__ballot(p) & g.segmask);
        }
        if (act) select_step(b, c0, &k, &m, &s);
    }
    return s;
}

// ---- long rows: a whole block per row -----------------------------------------------------------------------------------------

struct LongRowLds {
    unsigned long long flagged[kWavesPerBlock];
    int cnt[kWavesPerBlock];
};

// f(slot, ordinal) by the whole block for every thread `slot` of it that came with `flag`, one after another in thread order;
// ordinal counts them from 0.
template <class F>
__device__ __forceinline__ void for_each_flagged(LongRowLds &lds, bool flag, F &&f)
{
    const unsigned long long mine = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0) lds.flagged[threadIdx.x / kWave] = mine;
    __syncthreads();
    int ordinal = 0;
    for (int w = 0; w < kWavesPerBlock; w++) {
        unsigned long long todo = lds.flagged[w];
        while (todo) {
            const int bitpos = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            f(w * kWave + bitpos, ordinal++);
        }
    }
}

// The contiguous quarter [lo, hi) of a row of d positions that this thread's wavefront walks.
struct Quarter {
    int lo, hi;
};
__device__ __forceinline__ Quarter my_quarter(int d)
{
    const int chunk = ((d + kBlock - 1) / kBlock) * kWave;
    const int lo = min(d, (int)(threadIdx.x / kWave) * chunk);
    return {lo, min(d, lo + chunk)};
}

// Every wavefront brings the count of its quarter: the counts of the quarters before it, and of the whole row.
struct QuarterCounts {
    int before, total;
};
static_assert(kWavesPerBlock == 4, "exchange_counts sums four wavefront counts");
__device__ __forceinline__ QuarterCounts exchange_counts(LongRowLds &lds, int mine)
{
    const int wave = threadIdx.x / kWave;
    __syncthreads();                                           // (the previous readers of cnt are done)
    if ((threadIdx.x & (kWave - 1)) == 0) lds.cnt[wave] = mine;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int v = 0; v < kWavesPerBlock; v++)
        if (v < wave) before += lds.cnt[v];
    return {before, lds.cnt[0] + lds.cnt[1] + lds.cnt[2] + lds.cnt[3]};
}

}  // namespace gnna

#endif

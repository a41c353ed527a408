// gnna_edgefeat.hip -- message passing with a feature row per edge: out[i] = sum over the edges of row i of act(x_j (+ | *) E_e), and
// its two backward passes (gnna_agg_edge_feat_ld_f32, gnna_agg_edge_feat_backward_ld_f32; gnna_edgefeat.h).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its kernels sum x_j alone, GNNAdvisor_kernel.cu:186-259).
//
// One kernel body, three passes.  Each walks the rows of a CSR the way gnna_softagg.hip does -- slots of LPR = next_pow2(ceil(D / 4))
// lanes, 16-byte loads, ids one step ahead, column blocks of 256 floats, element-wise loads for a partial last vector, no
// neighbor-group partition, no atomics, no zero-fill, no scratch -- and differs in what a row holds, gathers and writes:
//   * forward (rows of A):      gathers x[j] and streams E[e];            writes out[i] = the sum of the messages
//   * d_edge  (rows of A):      holds dY[i], gathers x[j], streams E[e];  writes d_edge[e] per edge, sums nothing
//   * d_input (rows of A^T):    holds x[j], gathers dY[i] and E[t_edge_pos[p]];  writes d_input[j] = the sum
// A pass loads only what its (combine, act) needs: d_edge of ADD without an activation is a copy of dY[i] and loads neither x nor E.
//
// The rows of the target workload (batches of molecules) have 2 .. 4 edges, so a wavefront per row would leave most slots of a narrow
// row idle.  A wavefront owns 64 / LPR consecutive rows instead and every row takes one of three paths by its degree alone:
//   * up to kSlotEdges edges: the row's own slot walks it, kEdges edges per step; the 64 / LPR rows of a wavefront run side by side
//     and their E rows are one contiguous range;
//   * up to (64 / LPR) * kEdges * kLongSteps edges: the slots of the wavefront share the row and meet by slots_sum;
//   * beyond: the whole workgroup shares it, and the wavefronts meet through LDS in the order of the wavefronts.
// The path and the order of every sum depend on the degree only: the same bits on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gnna_edgefeat.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::load_piece, gat::slots_sum, gat::check_alias
#include "gnna_internal.h"
#include "gnna_segments.h"       // seg::store_piece

namespace gnna {
namespace {

using gat::VT;
using gat::load_piece;
using seg::store_piece;

// Both constants were chosen on one MI355X (profiles/edge_features/README.md; the macros exist so that tools/probe_edge_features.py
// can time libraries built with other values):
// edges per slot and step = pairs of 16-byte loads (a gathered row piece and an E row piece) in flight per lane.  2, not 4: with 4
// the passes need 80 .. 104 registers (6 .. 4 waves per SIMD) and every one of the twelve timed passes was slower, the source-side
// pass by a fifth to a quarter; 3 lies between, and 1 ties on the batch of small graphs and loses up to a tenth on the
// amazon0505-like graph.  With 2 the passes need 50 .. 72 registers (8 .. 7 waves per SIMD): the loads in flight that count come
// from more wavefronts, not from a longer step.
#ifndef GNNA_EDGEFEAT_EDGES
#define GNNA_EDGEFEAT_EDGES 2
#endif
// a row of up to this many edges is walked by its own slot (wavefronts of more than one slot only).  On 65,536 graphs of 8 .. 72
// nodes (mean degree 3.8, at most 17) at D = 64 the forward took 1.23 ms without this path, 1.07 ms with 4 and 0.87 ms with 8 or
// 16 (measured with 4 edges per step); on the amazon0505-like graph (mean degree 11.9) the four were within 3 % of each other.  8 keeps the rows of a molecule on the
// path and leaves everything longer to the slots of a whole wavefront.
#ifndef GNNA_EDGEFEAT_SLOT_EDGES
#define GNNA_EDGEFEAT_SLOT_EDGES 8
#endif
constexpr int kEdges = GNNA_EDGEFEAT_EDGES;
constexpr int kSlotEdges = GNNA_EDGEFEAT_SLOT_EDGES;
// a row that would keep its wavefront for more than kLongSteps steps goes to the whole block (gnna_softagg.hip's threshold)
constexpr int kLongSteps = 32;

enum Pass { kFwd = 0, kDEdge = 1, kSrc = 2 };

struct Args {
    const float *A;             // the rows gathered by id: x (forward, d_edge), dY (d_input)
    size_t lda;
    const float *E;             // edge rows
    size_t lde;
    const float *H;             // the row held while its edges are walked: dY (d_edge), x (d_input); unused by the forward
    size_t ldh;
    const int32_t *rp, *col;    // the CSR walked: A, or A^T in the d_input pass
    const int32_t *pos;         // d_input pass: t_edge_pos
    float *out;                 // out | d_edge | d_input
    size_t ldo;
    int64_t rows;               // rows walked
    uint32_t limit;             // ids < limit
    uint32_t nnz;               // positions < nnz
    int D;
    bool mul, relu;
    bool need_a, need_e, need_h;
    bool walk;                  // false: no edge can count (no edges or no source rows): the index arrays are not read
};

// The kEdges edges of slot t in the step at `base` (positions base + t + k * nl): the id gathered by and the E row of each.
// gid = -1: no position; -2: a position whose edge is skipped (an id outside [0, limit), an E row outside [0, nnz)).
template <int PASS>
__device__ __forceinline__ void load_ids(const Args &p, uint32_t base, uint32_t end, int t, int nl, int (&gid)[kEdges],
                                         uint32_t (&eid)[kEdges])
{
#pragma unroll
    for (int k = 0; k < kEdges; k++) {
        const uint32_t at = base + (uint32_t)(t + k * nl);      // (end < 2^31: no wrap)
        int g = -1;
        uint32_t e = at;
        if (at < end) {
            g = p.col[at];
            if constexpr (PASS == kSrc) e = (uint32_t)p.pos[at];
            if ((uint32_t)g >= p.limit || e >= p.nnz) g = -2;
        }
        gid[k] = g;
        eid[k] = e;
    }
}

// The positions [beg, end) swept by `nl` slots (this one: slot t), kEdges edges per slot and step, for the n4 (<= 4; <= 0: an idle
// lane) columns at mycol; h: this lane's piece of the held row.  -> this slot's sum (forward, d_input); the d_edge pass stores here.
template <int PASS>
__device__ __forceinline__ VT sweep(const Args &p, uint32_t beg, uint32_t end, int t, int nl, int mycol, int n4, const VT h)
{
    const bool ok = n4 > 0;
    VT acc = (VT)(0.f);
    int ng[kEdges];
    uint32_t ne[kEdges];
    load_ids<PASS>(p, beg, end, t, nl, ng, ne);
#pragma unroll 1
    for (uint32_t base = beg; base < end; base += (uint32_t)(nl * kEdges)) {
        int gid[kEdges];
        uint32_t eid[kEdges];
        VT a[kEdges], b[kEdges];
#pragma unroll
        for (int k = 0; k < kEdges; k++) {
            gid[k] = ng[k];
            eid[k] = ne[k];
            a[k] = b[k] = (VT)(0.f);
            if (gid[k] >= 0 && ok) {
                if (p.need_a) a[k] = load_piece(p.A + (size_t)(uint32_t)gid[k] * p.lda + (size_t)mycol, n4);
                if (p.need_e) b[k] = load_piece(p.E + (size_t)eid[k] * p.lde + (size_t)mycol, n4);
            }
        }
        load_ids<PASS>(p, base + (uint32_t)(nl * kEdges), end, t, nl, ng, ne);
#pragma unroll
        for (int k = 0; k < kEdges; k++) {
            const VT x = PASS == kSrc ? h : a[k];
            const VT g = PASS == kSrc ? a[k] : h;
            VT v;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float pre = p.mul ? x[c] * b[k][c] : x[c] + b[k][c];
                const bool on = gid[k] >= 0 && (!p.relu || pre > 0.f);
                float r;
                if constexpr (PASS == kFwd) r = pre;
                else if constexpr (PASS == kDEdge) r = p.mul ? g[c] * x[c] : g[c];
                else r = p.mul ? g[c] * b[k][c] : g[c];
                v[c] = on ? r : 0.f;
            }
            if constexpr (PASS == kDEdge) {
                if (gid[k] != -1 && ok) store_piece(p.out + (size_t)eid[k] * p.ldo + (size_t)mycol, v, n4);
            } else {
                acc += v;
            }
        }
    }
    return acc;
}

template <int PASS>
__device__ __forceinline__ VT held_piece(const Args &p, int64_t row, int mycol, int n4)
{
    if (PASS == kFwd || !p.need_h || n4 <= 0) return (VT)(0.f);
    return load_piece(p.H + (size_t)row * p.ldh + (size_t)mycol, n4);
}

template <int LOG_LPR, int PASS>
__global__ void __launch_bounds__(kBlock)
edgefeat_kernel(const Args p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR, RB = R * kWavesPerBlock;
    constexpr bool kSum = PASS != kDEdge;
    constexpr uint32_t kLong = (uint32_t)(R * kEdges * kLongSteps);
    __shared__ int s_long[RB];
    __shared__ int s_nlong;
    __shared__ float s_red[4][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    // this slot's row: R consecutive rows per wavefront, RB per block
    const int64_t r0 = (int64_t)blockIdx.x * RB;
    const int64_t row = r0 + wib * R + sub;
    const bool live = row < p.rows;
    uint32_t beg = 0, end = 0;
    // A range of the structure itself is cut to [0, nnz]: a position >= num_edges is skipped.  The positions of A^T are not edge
    // positions (t_edge_pos holds those, and is checked per edge): its ranges are cut to int32 only.  Either way no position wraps.
    const uint32_t cap = PASS == kSrc ? 0x7fffffffu : p.nnz;
    if (live && p.walk) {
        beg = std::min((uint32_t)p.rp[row], cap);
        end = std::min((uint32_t)p.rp[row + 1], cap);
        if (beg > end) beg = end;
    }
    const uint32_t deg = end - beg;
    const bool is_long = deg > kLong;
    const bool is_short = R > 1 && deg <= (uint32_t)kSlotEdges;         // (a wavefront of one slot: the slot is the wavefront)
    if (is_long && cl == 0) s_long[atomicAdd(&s_nlong, 1)] = wib * R + sub;
    __syncthreads();

    // ---- the short rows (and, in wavefronts of several slots, the rows without edges): every slot its own row --------------------
    if constexpr (R > 1) {
        if (live && is_short) {
            for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
                const int mycol = c0 + cl * 4, n4 = p.D - mycol;
                const VT h = held_piece<PASS>(p, row, mycol, n4);
                const VT acc = sweep<PASS>(p, beg, end, 0, 1, mycol, n4, h);
                if (kSum && n4 > 0) store_piece(p.out + (size_t)row * p.ldo + (size_t)mycol, acc, n4);
            }
        }
    }

    // ---- the rows in between: the slots of the wavefront share one row after the other ------------------------------------------
    {
        constexpr uint64_t slot_lanes = LPR == 64 ? ~0ull : ((1ull << (LPR & 63)) - 1ull);
        uint64_t todo = __ballot(live && !is_long && !is_short);
        while (todo) {
            const int s = (__ffsll((unsigned long long)todo) - 1) >> LOG_LPR;
            todo &= ~(slot_lanes << (s * LPR));
            const int64_t rr = r0 + wib * R + s;
            const uint32_t lb = (uint32_t)__shfl((int)beg, s * LPR), le = (uint32_t)__shfl((int)end, s * LPR);
            for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
                const int mycol = c0 + cl * 4, n4 = p.D - mycol;
                const VT h = held_piece<PASS>(p, rr, mycol, n4);
                VT acc = sweep<PASS>(p, lb, le, sub, R, mycol, n4, h);
                if constexpr (kSum) {
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[c] = gat::slots_sum<LPR>(acc[c]);
                    if (sub == 0 && n4 > 0) store_piece(p.out + (size_t)rr * p.ldo + (size_t)mycol, acc, n4);
                }
            }
        }
    }

    // ---- the long rows: the whole block, one after the other (the list's order may vary; a row's result does not depend on it) ---
    const int nlong = s_nlong;
    for (int k = 0; k < nlong; k++) {
        const int64_t rr = r0 + s_long[k];
        const uint32_t lb = std::min((uint32_t)p.rp[rr], cap), le = std::min((uint32_t)p.rp[rr + 1], cap);
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            const VT h = held_piece<PASS>(p, rr, mycol, n4);
            VT acc = sweep<PASS>(p, lb, le, wib * R + sub, RB, mycol, n4, h);
            if constexpr (kSum) {
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c] = gat::slots_sum<LPR>(acc[c]);
                // the wavefronts' sums are added in the order of the wavefronts
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int c = 0; c < 4; c++) s_red[c][wib][cl] = acc[c];
                }
                __syncthreads();
                if (wib == 0 && sub == 0 && n4 > 0) {
                    acc = (VT)(0.f);
                    for (int w = 0; w < kWavesPerBlock; w++) {
#pragma unroll
                        for (int c = 0; c < 4; c++) acc[c] += s_red[c][w][cl];
                    }
                    store_piece(p.out + (size_t)rr * p.ldo + (size_t)mycol, acc, n4);
                }
            }
        }
    }

    // ---- d_edge: the rows of d_edge that no row of the structure reaches, [row_pointers[rows], nnz), are 0 -----------------------
    if constexpr (PASS == kDEdge) {
        const uint32_t done = p.rows > 0 ? std::min((uint32_t)p.rp[p.rows], p.nnz) : 0u;
        const size_t n = (size_t)(p.nnz - done) * (size_t)p.D;
        for (size_t i = (size_t)blockIdx.x * kBlock + (size_t)tid; i < n; i += (size_t)gridDim.x * kBlock) {
            const size_t r = i / (unsigned)p.D, c = i - r * (unsigned)p.D;
            p.out[((size_t)done + r) * p.ldo + c] = 0.f;
        }
    }
}

template <int PASS>
int launch(const Args &a, hipStream_t stream, const char *noun)
{
    const int log_lpr = log2_lanes(a.D, 4);
    const int64_t rows_per_block = (int64_t)(kWave >> log_lpr) * kWavesPerBlock;
    const dim3 grid((unsigned)std::max<int64_t>(1, (a.rows + rows_per_block - 1) / rows_per_block));       // (rows < 2^29)
    dispatch_lpr(log_lpr, [&](auto L) {
        hipLaunchKernelGGL((edgefeat_kernel<decltype(L)::value, PASS>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("%s launch", noun);
}

// what both entries check alike, before any device work
int check_sizes(const char *what, int64_t num_out_rows, int64_t num_in_rows, int64_t num_edges, int dim, int combine, int act,
                unsigned flags)
{
    if (flags != 0u)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s takes no flags (got 0x%x): GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning "
                    "for an edge-feature aggregation, whose activation is `act`", what, flags);
    if (dim < 1) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dim must be >= 1 (got %d)", what, dim);
    if (num_out_rows < 0 || num_in_rows < 0 || num_edges < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_out_rows=%lld num_in_rows=%lld num_edges=%lld)", what,
                    (long long)num_out_rows, (long long)num_in_rows, (long long)num_edges);
    if (combine != GNNA_EDGE_ADD && combine != GNNA_EDGE_MUL)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: combine must be GNNA_EDGE_ADD (0) or GNNA_EDGE_MUL (1) (got %d)", what, combine);
    if (act != GNNA_EDGE_ACT_NONE && act != GNNA_EDGE_ACT_RELU)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: act must be GNNA_EDGE_ACT_NONE (0) or GNNA_EDGE_ACT_RELU (1) (got %d)", what, act);
    const int64_t most = std::max(num_out_rows, num_in_rows);
    if (most >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 536870911): shard the rows", what, (long long)most);
    if (num_edges >= ((int64_t)1 << 31))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld edges in one call (at most 2147483647): shard the rows", what, (long long)num_edges);
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_agg_edge_feat_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows, const float *edge_feat, int64_t ld_e,
                              int64_t num_edges, const int32_t *row_pointers, const int32_t *column_index, float *out, int64_t ld_out,
                              int64_t num_out_rows, int dim, int combine, int act, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_agg_edge_feat_ld_f32";
    int rc = check_sizes(what, num_out_rows, num_in_rows, num_edges, dim, combine, act, flags);
    if (rc != GNNA_OK) return rc;
    if (bad_ld(ld_in, dim) || bad_ld(ld_e, dim) || bad_ld(ld_out, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_e=%lld ld_out=%lld "
                    "dim=%d)", what, (long long)ld_in, (long long)ld_e, (long long)ld_out, dim);
    const void *const ins[2] = {input, edge_feat};
    const void *const outs[1] = {out};
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(out);
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, edge-feature and output pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;
    if (!out) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer", what);
    const bool walk = num_edges > 0 && num_in_rows > 0;
    if (walk && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    if (walk && !edge_feat) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null edge-feature pointer", what);
    if (walk && (!row_pointers || !column_index)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    Args a{};
    a.A = input; a.lda = (size_t)ld_in; a.E = edge_feat; a.lde = (size_t)ld_e; a.H = nullptr; a.ldh = 0;
    a.rp = row_pointers; a.col = column_index; a.pos = nullptr; a.out = out; a.ldo = (size_t)ld_out;
    a.rows = num_out_rows; a.limit = (uint32_t)num_in_rows; a.nnz = (uint32_t)num_edges; a.D = dim;
    a.mul = combine == GNNA_EDGE_MUL; a.relu = act == GNNA_EDGE_ACT_RELU;
    a.need_a = a.need_e = true; a.need_h = false; a.walk = walk;
    return launch<kFwd>(a, static_cast<hipStream_t>(stream_v), "edge-feature aggregation");
}

int gnna_agg_edge_feat_backward_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows, const float *edge_feat, int64_t ld_e,
                                       int64_t num_edges, const float *dY, int64_t ld_dy, const int32_t *row_pointers,
                                       const int32_t *column_index, const int32_t *t_row_pointers, const int32_t *t_column_index,
                                       const int32_t *t_edge_pos, float *d_input, int64_t ld_din, float *d_edge, int64_t ld_de,
                                       int64_t num_out_rows, int dim, int combine, int act, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_agg_edge_feat_backward_ld_f32";
    int rc = check_sizes(what, num_out_rows, num_in_rows, num_edges, dim, combine, act, flags);
    if (rc != GNNA_OK) return rc;
    // (a null output leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld(ld_e, dim) || bad_ld(ld_dy, dim) || bad_ld_of(d_input, ld_din, dim) || bad_ld_of(d_edge, ld_de, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_e=%lld ld_dy=%lld "
                    "ld_din=%lld ld_de=%lld dim=%d)", what, (long long)ld_in, (long long)ld_e, (long long)ld_dy, (long long)ld_din,
                    (long long)ld_de, dim);
    const void *const ins[3] = {input, edge_feat, dY};
    const void *const outs[2] = {d_input, d_edge};
    uintptr_t low_bits = 0;
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    for (const void *q : outs) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, edge-feature and gradient pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    const bool mul = combine == GNNA_EDGE_MUL, relu = act == GNNA_EDGE_ACT_RELU;
    const bool want_din = d_input && num_in_rows > 0, want_de = d_edge && num_edges > 0;
    if (!want_din && !want_de) return GNNA_OK;
    // an edge counts only where all three sizes are positive; without one, the outputs are 0 and nothing else is read
    const bool walk = num_edges > 0 && num_in_rows > 0 && num_out_rows > 0;
    if (walk && !dY) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null dY pointer", what);
    if (walk && (mul || relu) && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    if (walk && (mul || relu) && !edge_feat) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null edge-feature pointer", what);
    if (walk && want_de && (!row_pointers || !column_index)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (walk && want_din && (!t_row_pointers || !t_column_index || !t_edge_pos))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null transposed index pointer (t_row_pointers, t_column_index and t_edge_pos are "
                    "needed for d_input)", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (want_de) {
        // destination side: row i holds dY[i]; x[j] is gathered for the product or the mask, E[e] streamed for the mask
        Args a{};
        a.A = input; a.lda = (size_t)ld_in; a.E = edge_feat; a.lde = (size_t)ld_e; a.H = dY; a.ldh = (size_t)ld_dy;
        a.rp = row_pointers; a.col = column_index; a.pos = nullptr; a.out = d_edge; a.ldo = (size_t)ld_de;
        a.rows = walk ? num_out_rows : 0; a.limit = (uint32_t)num_in_rows; a.nnz = (uint32_t)num_edges; a.D = dim;
        a.mul = mul; a.relu = relu; a.need_a = mul || relu; a.need_e = relu; a.need_h = true; a.walk = walk;
        if ((rc = launch<kDEdge>(a, stream, "edge-feature aggregation backward: d_edge")) != GNNA_OK) return rc;
    }
    if (want_din) {
        // source side: row j of A^T holds x[j] (for the mask); dY[i] is gathered, E[e] gathered through t_edge_pos
        Args a{};
        a.A = dY; a.lda = (size_t)ld_dy; a.E = edge_feat; a.lde = (size_t)ld_e; a.H = input; a.ldh = (size_t)ld_in;
        a.rp = t_row_pointers; a.col = t_column_index; a.pos = t_edge_pos; a.out = d_input; a.ldo = (size_t)ld_din;
        a.rows = num_in_rows; a.limit = (uint32_t)num_out_rows; a.nnz = (uint32_t)num_edges; a.D = dim;
        a.mul = mul; a.relu = relu; a.need_a = true; a.need_e = mul || relu; a.need_h = relu; a.walk = walk;
        if ((rc = launch<kSrc>(a, stream, "edge-feature aggregation backward: d_input")) != GNNA_OK) return rc;
    }
    return GNNA_OK;
}

}  // extern "C"

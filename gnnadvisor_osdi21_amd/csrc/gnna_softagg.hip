// gnna_softagg.hip -- softmax neighbor aggregation with a temperature, per channel, and its backward pass
// (gnna_agg_softmax_ld_f32, gnna_agg_softmax_backward_ld_f32; include/gnna_softagg.h).  CDNA4 / gfx950 only.
//
// No counterpart in the reference (its kernels only sum, GNNAdvisor_kernel.cu:186-259).
//
// Both passes walk the rows of a CSR the way the lse pass of the fused attention does (gat::lse_kernel): one wavefront per row,
// the whole workgroup for the long rows of its four, 64 / LPR slots of LPR = next_pow2(ceil(D / 4)) lanes that take several edges
// per step with 16-byte loads, column blocks of 256 floats for wider rows, element-wise loads for a partial last vector.  No
// neighbor-group partition, no atomics, no zero-fill: a row has one writer per element, and slots and wavefronts meet in a fixed
// order, so the same bits come out on every run.
//   * forward: per lane and element the online state (m, l, a, q) -- the running max of s = t * x, and sum e, sum e * x and
//     sum e * x^2 with e = exp(s - m) -- 16 registers.  The edges of a step enter together: one exp to rescale the state, one
//     per edge.  The slots meet by a butterfly of state merges, the wavefronts of a long row through LDS.  lse = m + log l,
//     out = a / l, sq = q / l.
//   * backward: a pack pass writes (dY, dY * Y, lse) per (destination row, channel) into library scratch, 12 bytes, so that a
//     transposed edge j <- i costs one contiguous gather.  Row j keeps u = sum alpha * dY and w = sum alpha * dY * Y with
//     alpha = exp(t * x_j - lse_i) <= 1 computed per edge, and writes dX = (1 + t * x_j) * u - t * w.  (The factored form
//     exp(t * x_j) * sum exp(-lse_i) ... overflows fp32 once |lse| > 88 and is not used.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gnna_softagg.h"
#include "gnna_device.h"
#include "gnna_gat_common.h"     // gat::load_piece, gat::slots_sum, gat::check_alias
#include "gnna_internal.h"
#include "gnna_segments.h"

namespace gnna {
namespace {

using gat::VT;
using gat::load_piece;

// edges per slot and step of the forward gather = 16-byte loads in flight per lane: with 4 every instance needs 132 .. 144
// registers (3 waves per SIMD), with 3 at most 118 (4 waves)
constexpr int kFwdEdges = 3;
constexpr int kBwdEdges = 2;     // records (three 16-byte loads each) per slot and step of the backward gather
// A row that would keep its wavefront for more than kLongSteps steps of the gather goes to the whole block: more than
// (slots of a wavefront) * (edges per slot and step) * kLongSteps edges.
constexpr int kLongSteps = 32;

// (exp of a non-positive number, one v_exp_f32, and the partial store of a lane's four columns: gnna_segments.h)
using seg::exp_nonpos;
using seg::store_piece;

// this lane's four temperatures: the one value of a scalar temperature, or the piece of the per-channel vector
__device__ __forceinline__ VT temp_piece(const float *__restrict__ temp, int temp_len, int mycol, int n4)
{
    if (temp_len == 1) return (VT)(temp[0]);
    return load_piece(temp + mycol, n4);
}

// The ids of the E edges of slot t in the step at `base` (edges base + t + k * nl, k < E); -1 past the end of the row and for an id
// outside [0, limit): such an edge is skipped, in every pass alike.
template <int E>
__device__ __forceinline__ void load_ids(const int32_t *__restrict__ col, uint32_t base, uint32_t end, int t, int nl, uint32_t limit,
                                         int (&id)[E])
{
#pragma unroll
    for (int k = 0; k < E; k++) {
        const uint32_t ee = base + (uint32_t)(t + k * nl);      // (positions are int32 row pointers: no wrap below 2^32)
        id[k] = ee < end ? col[ee] : -1;
        if ((uint32_t)id[k] >= limit) id[k] = -1;
    }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------

struct FwdArgs {
    const float *X;             // source rows
    size_t ldx;
    const float *temp;
    int temp_len;
    const int32_t *rp, *col;
    float *out, *lse, *sq;      // sq may be null
    size_t ldo, ldl, ldq;
    int64_t N;                  // destination rows
    uint32_t M;                 // ids < M
    int D;
};

// (m, l, a, q) of four elements; m = -inf: no edge yet (l = a = q = 0)
struct State {
    VT m, l, a, q;
};

__device__ __forceinline__ State state_empty()
{
    return State{(VT)(-INFINITY), (VT)(0.f), (VT)(0.f), (VT)(0.f)};
}

__device__ __forceinline__ void state_merge(State &s, const State &o)
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float m = fmaxf(s.m[c], o.m[c]);
        const float fa = s.m[c] == -INFINITY ? 0.f : exp_nonpos(s.m[c] - m);
        const float fb = o.m[c] == -INFINITY ? 0.f : exp_nonpos(o.m[c] - m);
        s.l[c] = s.l[c] * fa + o.l[c] * fb;
        s.a[c] = s.a[c] * fa + o.a[c] * fb;
        s.q[c] = s.q[c] * fa + o.q[c] * fb;
        s.m[c] = m;
    }
}

// E edges enter together (id < 0: no edge): one rescale of the state per step
template <int E>
__device__ __forceinline__ void state_add(State &s, const VT t, const VT (&v)[E], const int (&id)[E])
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float z[E];
        float m = s.m[c];
#pragma unroll
        for (int k = 0; k < E; k++) {
            z[k] = id[k] >= 0 ? t[c] * v[k][c] : -INFINITY;
            m = fmaxf(m, z[k]);
        }
        const float r = s.m[c] == -INFINITY ? 0.f : exp_nonpos(s.m[c] - m);
        float l = s.l[c] * r, a = s.a[c] * r, q = s.q[c] * r;
#pragma unroll
        for (int k = 0; k < E; k++) {
            const float e = z[k] == -INFINITY ? 0.f : exp_nonpos(z[k] - m);
            const float ex = e * v[k][c];
            l += e;
            a += ex;
            q += ex * v[k][c];
        }
        s.m[c] = m; s.l[c] = l; s.a[c] = a; s.q[c] = q;
    }
}

// The edges [beg, end) swept by `nl` slots of LPR lanes (this one: slot t), kFwdEdges edges per slot and step, for the n4 (<= 4;
// <= 0: an idle lane) columns at mycol.  Every lane of a wavefront makes the same number of steps; the slots of the wavefront then
// meet.
template <int LOG_LPR>
__device__ __forceinline__ State fwd_sweep(const FwdArgs &p, uint32_t beg, uint32_t end, int t, int nl, int mycol, int n4, const VT tv)
{
    constexpr int E = kFwdEdges;
    const bool ok = n4 > 0;
    State st = state_empty();
    // the ids of a step are loaded one step ahead, so that a step's row loads do not wait for them
    int next[E];
    load_ids<E>(p.col, beg, end, t, nl, p.M, next);
#pragma unroll 1
    for (uint32_t base = beg; base < end; base += (uint32_t)(nl * E)) {
        int id[E];
        VT v[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            id[k] = next[k];
            v[k] = (VT)(0.f);
            if (id[k] >= 0 && ok) v[k] = load_piece(p.X + (size_t)(uint32_t)id[k] * p.ldx + (size_t)mycol, n4);
        }
        load_ids<E>(p.col, base + (uint32_t)(nl * E), end, t, nl, p.M, next);
        state_add<E>(st, tv, v, id);
    }
#pragma unroll
    for (int d = kWave >> 1; d >= (1 << LOG_LPR); d >>= 1) {
        State o;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            o.m[c] = __shfl_xor(st.m[c], d);
            o.l[c] = __shfl_xor(st.l[c], d);
            o.a[c] = __shfl_xor(st.a[c], d);
            o.q[c] = __shfl_xor(st.q[c], d);
        }
        state_merge(st, o);
    }
    return st;
}

__device__ __forceinline__ void fwd_write(const FwdArgs &p, int64_t row, int mycol, int n4, const State &st)
{
    VT o, ls, sq;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const bool any = st.m[c] != -INFINITY;                      // a row without edges: out = lse = sq = 0
        o[c] = any ? st.a[c] / st.l[c] : 0.f;
        sq[c] = any ? st.q[c] / st.l[c] : 0.f;
        ls[c] = any ? st.m[c] + logf(st.l[c]) : 0.f;
    }
    store_piece(p.out + (size_t)row * p.ldo + (size_t)mycol, o, n4);
    store_piece(p.lse + (size_t)row * p.ldl + (size_t)mycol, ls, n4);
    if (p.sq) store_piece(p.sq + (size_t)row * p.ldq + (size_t)mycol, sq, n4);
}

template <int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
softagg_fwd_kernel(const FwdArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR;
    __shared__ int s_long[kWavesPerBlock];
    __shared__ int s_nlong;
    __shared__ float s_red[16][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * kWavesPerBlock;
    const int64_t row = r0 + wib;
    int64_t beg = 0, end = 0;
    if (row < p.N && p.M > 0) { beg = p.rp[row]; end = p.rp[row + 1]; }
    const bool is_long = end - beg > R * kFwdEdges * kLongSteps;
    if (is_long && lane == 0) s_long[atomicAdd(&s_nlong, 1)] = wib;
    __syncthreads();
    // k = -1: the short rows (and rows without edges), a wavefront each; k >= 0: the long rows, the whole block, one after the
    // other (the list's order may vary; a row's result does not depend on it)
    const int nlong = s_nlong;
    for (int k = -1; k < nlong; k++) {
        const bool whole = k >= 0;
        const int64_t rr = whole ? r0 + s_long[k] : row;
        int64_t lb = beg, le = is_long ? beg : end;
        if (whole) { lb = p.rp[rr]; le = p.rp[rr + 1]; }
        const int t = whole ? wib * R + sub : sub, nl = whole ? kWavesPerBlock * R : R;
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            const VT tv = n4 > 0 ? temp_piece(p.temp, p.temp_len, mycol, n4) : (VT)(0.f);
            State st = fwd_sweep<LOG_LPR>(p, (uint32_t)lb, (uint32_t)le, t, nl, mycol, n4, tv);
            if (whole) {
                // the wavefronts meet through LDS, in the order of the wavefronts
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        s_red[c][wib][cl] = st.m[c];
                        s_red[4 + c][wib][cl] = st.l[c];
                        s_red[8 + c][wib][cl] = st.a[c];
                        s_red[12 + c][wib][cl] = st.q[c];
                    }
                }
                __syncthreads();
                st = state_empty();
#pragma unroll 1
                for (int w = 0; w < kWavesPerBlock; w++) {
                    State o;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        o.m[c] = s_red[c][w][cl];
                        o.l[c] = s_red[4 + c][w][cl];
                        o.a[c] = s_red[8 + c][w][cl];
                        o.q[c] = s_red[12 + c][w][cl];
                    }
                    state_merge(st, o);
                }
            }
            const bool writer = whole ? wib == 0 : (row < p.N && !is_long);
            if (writer && sub == 0 && n4 > 0) fwd_write(p, rr, mycol, n4, st);
        }
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------

// (dY, dY * Y, lse) of every (destination row, channel), 12 bytes: what row i brings to each of its transposed edges
__global__ void __launch_bounds__(kBlock)
softagg_pack_kernel(const float *__restrict__ G, size_t ldg, const float *__restrict__ Y, size_t ldy, const float *__restrict__ lse,
                    size_t ldl, float *__restrict__ pack, size_t N, int D)
{
    const size_t n = N * (size_t)D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (unsigned)D, c = i - r * (unsigned)D;
        const float g = G[r * ldg + c];
        pack[3 * i] = g;
        pack[3 * i + 1] = g * Y[r * ldy + c];
        pack[3 * i + 2] = lse[r * ldl + c];
    }
}

struct BwdArgs {
    const float *X;             // source rows: the rows this pass walks
    size_t ldx;
    const float *temp;
    int temp_len;
    const float *pack;          // [N][D][3]
    const int32_t *rp, *col;    // A^T: M rows, ids < N
    float *dX;
    size_t lddx;
    int64_t M;                  // source rows
    uint32_t N;                 // destination rows: ids < N
    int D;
};

struct Sums {
    VT u, w;
};

// the records of the n4 (<= 4) channels at `at`: 3 * n4 floats
__device__ __forceinline__ void load_records(const float *__restrict__ at, int n4, VT &g, VT &gy, VT &ls)
{
    float r[12];
    if (n4 >= 4) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const VT t = *reinterpret_cast<const gat::MT *>(at + 4 * k);
#pragma unroll
            for (int c = 0; c < 4; c++) r[4 * k + c] = t[c];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) r[k] = k < 3 * n4 ? at[k] : 0.f;
        r[9] = r[10] = r[11] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        g[c] = r[3 * c];
        gy[c] = r[3 * c + 1];
        ls[c] = r[3 * c + 2];
    }
}

// The transposed edges [beg, end) swept as in fwd_sweep, kBwdEdges edges per slot and step (a record is three loads); the sums of this
// lane's slot.  z = t * x_j of this lane's columns.
__device__ __forceinline__ Sums bwd_sweep(const BwdArgs &p, uint32_t beg, uint32_t end, int t, int nl, int mycol, int n4, const VT z)
{
    const bool ok = n4 > 0;
    Sums s{(VT)(0.f), (VT)(0.f)};
    int next[kBwdEdges];
    load_ids<kBwdEdges>(p.col, beg, end, t, nl, p.N, next);
#pragma unroll 1
    for (uint32_t base = beg; base < end; base += (uint32_t)(nl * kBwdEdges)) {
        int id[kBwdEdges];
        VT g[kBwdEdges], gy[kBwdEdges], ls[kBwdEdges];
#pragma unroll
        for (int k = 0; k < kBwdEdges; k++) {
            id[k] = next[k];
            g[k] = gy[k] = ls[k] = (VT)(0.f);
            if (id[k] >= 0 && ok) load_records(p.pack + ((size_t)(uint32_t)id[k] * (size_t)p.D + (size_t)mycol) * 3, n4, g[k], gy[k], ls[k]);
        }
        load_ids<kBwdEdges>(p.col, base + (uint32_t)(nl * kBwdEdges), end, t, nl, p.N, next);
#pragma unroll
        for (int k = 0; k < kBwdEdges; k++) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float alpha = id[k] >= 0 ? exp_nonpos(z[c] - ls[k][c]) : 0.f;
                s.u[c] += alpha * g[k][c];
                s.w[c] += alpha * gy[k][c];
            }
        }
    }
    return s;
}

template <int LOG_LPR>
__global__ void __launch_bounds__(kBlock)
softagg_bwd_kernel(const BwdArgs p)
{
    constexpr int LPR = 1 << LOG_LPR, R = kWave / LPR;
    __shared__ int s_long[kWavesPerBlock];
    __shared__ int s_nlong;
    __shared__ float s_red[8][kWavesPerBlock][LPR];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wib = tid >> 6;
    const int sub = lane >> LOG_LPR, cl = lane & (LPR - 1);
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * kWavesPerBlock;
    const int64_t row = r0 + wib;
    int64_t beg = 0, end = 0;
    if (row < p.M && p.N > 0) { beg = p.rp[row]; end = p.rp[row + 1]; }
    const bool is_long = end - beg > R * kBwdEdges * kLongSteps;
    if (is_long && lane == 0) s_long[atomicAdd(&s_nlong, 1)] = wib;
    __syncthreads();
    // k = -1: the short rows (and rows without transposed edges: d_input = 0), a wavefront each; k >= 0: the long rows, the whole
    // block, one after the other
    const int nlong = s_nlong;
    for (int k = -1; k < nlong; k++) {
        const bool whole = k >= 0;
        const int64_t rr = whole ? r0 + s_long[k] : row;
        int64_t lb = beg, le = is_long ? beg : end;
        if (whole) { lb = p.rp[rr]; le = p.rp[rr + 1]; }
        const int t = whole ? wib * R + sub : sub, nl = whole ? kWavesPerBlock * R : R;
        for (int c0 = 0; c0 < p.D; c0 += LPR * 4) {
            const int mycol = c0 + cl * 4, n4 = p.D - mycol;
            VT tv = (VT)(0.f), x = (VT)(0.f);
            if (n4 > 0 && rr < p.M) {
                tv = temp_piece(p.temp, p.temp_len, mycol, n4);
                x = load_piece(p.X + (size_t)rr * p.ldx + (size_t)mycol, n4);
            }
            const VT z = tv * x;
            Sums s = bwd_sweep(p, (uint32_t)lb, (uint32_t)le, t, nl, mycol, n4, z);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                s.u[c] = gat::slots_sum<LPR>(s.u[c]);
                s.w[c] = gat::slots_sum<LPR>(s.w[c]);
            }
            if (whole) {
                // the wavefronts' sums are added in the order of the wavefronts
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        s_red[c][wib][cl] = s.u[c];
                        s_red[4 + c][wib][cl] = s.w[c];
                    }
                }
                __syncthreads();
                s.u = s.w = (VT)(0.f);
                for (int v = 0; v < kWavesPerBlock; v++) {
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        s.u[c] += s_red[c][v][cl];
                        s.w[c] += s_red[4 + c][v][cl];
                    }
                }
            }
            const bool writer = whole ? wib == 0 : (row < p.M && !is_long);
            if (writer && sub == 0 && n4 > 0) store_piece(p.dX + (size_t)rr * p.lddx + (size_t)mycol, (1.0f + z) * s.u - tv * s.w, n4);
        }
    }
}

// Scratch of the backward entry: slot 12 = the records.  Eager calls of a stream share it (grow-only), a captured call gets its
// capture's own.
constexpr int kSlotSoftaggPack = 12;

// what both entries check alike, before any device work
int check_sizes(const char *what, int64_t num_out_rows, int64_t num_in_rows, int dim, int temp_len, unsigned flags)
{
    if (flags != 0u)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s takes no flags (got 0x%x): GNNA_ACCUMULATE and GNNA_EPILOGUE_RELU have no meaning "
                    "for a softmax aggregation", what, flags);
    if (dim < 1) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: dim must be >= 1 (got %d)", what, dim);
    if (num_out_rows < 0 || num_in_rows < 0)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: negative size (num_out_rows=%lld num_in_rows=%lld)", what, (long long)num_out_rows,
                    (long long)num_in_rows);
    if (temp_len != 1 && temp_len != dim)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: temp_len must be 1 or dim = %d (got %d)", what, dim, temp_len);
    const int64_t most = std::max(num_out_rows, num_in_rows);
    if (most >= ((int64_t)1 << 29))
        return fail(GNNA_ERR_UNSUPPORTED, "%s: %lld rows in one call (at most 536870911): shard the rows", what, (long long)most);
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {

int gnna_agg_softmax_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows, const float *temp, int temp_len,
                            const int32_t *row_pointers, const int32_t *column_index, float *out, int64_t ld_out, float *lse,
                            int64_t ld_lse, float *sq, int64_t ld_sq, int64_t num_out_rows, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_agg_softmax_ld_f32";
    int rc = check_sizes(what, num_out_rows, num_in_rows, dim, temp_len, flags);
    if (rc != GNNA_OK) return rc;
    // (a null sq leaves its stride with its upper bound only: nothing is strided by it)
    if (bad_ld(ld_in, dim) || bad_ld(ld_out, dim) || bad_ld(ld_lse, dim) || (sq ? bad_ld(ld_sq, dim) : ld_sq >= ((int64_t)1 << 29)))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_out=%lld ld_lse=%lld "
                    "ld_sq=%lld dim=%d)", what, (long long)ld_in, (long long)ld_out, (long long)ld_lse, (long long)ld_sq, dim);
    const void *const ins[2] = {input, temp};
    const void *const outs[3] = {out, lse, sq};
    uintptr_t low_bits = 0;
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    for (const void *q : outs) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, temperature and output pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_out_rows == 0) return GNNA_OK;
    if (!out || !lse) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer (out and lse are always written)", what);
    if (!temp) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null temperature pointer", what);
    if (num_in_rows > 0 && !input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    if (num_in_rows > 0 && (!row_pointers || !column_index)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    FwdArgs a;
    a.X = input; a.ldx = (size_t)ld_in; a.temp = temp; a.temp_len = temp_len; a.rp = row_pointers; a.col = column_index;
    a.out = out; a.lse = lse; a.sq = sq; a.ldo = (size_t)ld_out; a.ldl = (size_t)ld_lse; a.ldq = (size_t)ld_sq;
    a.N = num_out_rows; a.M = (uint32_t)num_in_rows; a.D = dim;
    const dim3 grid((unsigned)((num_out_rows + kWavesPerBlock - 1) / kWavesPerBlock));       // (num_out_rows < 2^29)
    dispatch_lpr(log2_lanes(dim, 4), [&](auto L) {
        hipLaunchKernelGGL((softagg_fwd_kernel<decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("softmax aggregation launch");
}

int gnna_agg_softmax_backward_ld_f32(const float *input, int64_t ld_in, int64_t num_in_rows, const float *temp, int temp_len,
                                     const float *lse, int64_t ld_lse, const float *Y, int64_t ld_y, const float *dY, int64_t ld_dy,
                                     const int32_t *t_row_pointers, const int32_t *t_column_index, float *d_input, int64_t ld_din,
                                     int64_t num_out_rows, int dim, unsigned flags, void *stream_v)
{
    static const char what[] = "gnna_agg_softmax_backward_ld_f32";
    int rc = check_sizes(what, num_out_rows, num_in_rows, dim, temp_len, flags);
    if (rc != GNNA_OK) return rc;
    if (bad_ld(ld_in, dim) || bad_ld(ld_lse, dim) || bad_ld(ld_y, dim) || bad_ld(ld_dy, dim) || bad_ld(ld_din, dim))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row strides must be >= dim and < 2^29 elements (ld_in=%lld ld_lse=%lld ld_y=%lld "
                    "ld_dy=%lld ld_din=%lld dim=%d)", what, (long long)ld_in, (long long)ld_lse, (long long)ld_y, (long long)ld_dy,
                    (long long)ld_din, dim);
    const void *const ins[5] = {input, temp, lse, Y, dY};
    const void *const outs[1] = {d_input};
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(d_input);
    for (const void *q : ins) low_bits |= reinterpret_cast<uintptr_t>(q);
    if (low_bits & 3) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: feature, temperature and gradient pointers must be 4-byte aligned", what);
    if ((rc = gat::check_alias(what, ins, outs)) != GNNA_OK) return rc;
    if (num_in_rows == 0) return GNNA_OK;
    if (!d_input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer", what);
    if (!input) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null feature pointer", what);
    if (!temp) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null temperature pointer", what);
    if (num_out_rows > 0 && (!lse || !Y || !dY)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null lse, Y or dY pointer", what);
    if (num_out_rows > 0 && (!t_row_pointers || !t_column_index)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceState *ds = nullptr;
    if ((rc = get_device_state(&ds)) != GNNA_OK) return rc;
    float *pack = nullptr;
    if (num_out_rows > 0) {
        void *ws = nullptr;
        const size_t bytes = (size_t)num_out_rows * (size_t)dim * 3 * sizeof(float);
        if ((rc = get_workspace(ds, stream, kSlotSoftaggPack, (bytes + 255) & ~(size_t)255, &ws)) != GNNA_OK) return rc;
        pack = static_cast<float *>(ws);
        hipLaunchKernelGGL(softagg_pack_kernel, dim3(elementwise_grid(num_out_rows * dim, ds->num_cus, 8)), dim3(kBlock), 0, stream, dY,
                           (size_t)ld_dy, Y, (size_t)ld_y, lse, (size_t)ld_lse, pack, (size_t)num_out_rows, dim);
        if ((rc = launch_ok("softmax aggregation backward: pack launch")) != GNNA_OK) return rc;
    }
    BwdArgs a;
    a.X = input; a.ldx = (size_t)ld_in; a.temp = temp; a.temp_len = temp_len; a.pack = pack; a.rp = t_row_pointers;
    a.col = t_column_index; a.dX = d_input; a.lddx = (size_t)ld_din; a.M = num_in_rows; a.N = (uint32_t)num_out_rows; a.D = dim;
    const dim3 grid((unsigned)((num_in_rows + kWavesPerBlock - 1) / kWavesPerBlock));        // (num_in_rows < 2^29)
    dispatch_lpr(log2_lanes(dim, 4), [&](auto L) {
        hipLaunchKernelGGL((softagg_bwd_kernel<decltype(L)::value>), grid, dim3(kBlock), 0, stream, a);
    });
    return launch_ok("softmax aggregation backward launch");
}

}  // extern "C"

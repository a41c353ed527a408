// gnna_transpose.hip -- device builders of a graph's structure: the transposed CSR with its edge permutation
// (gnna_transpose_csr_i32) and the neighbor-group partition of device row pointers (gnna_count_parts_device_i32,
// gnna_build_part_device_i32).  Prepare-time calls: they read one number back (and so synchronise the stream) and
// refuse to run inside a stream capture.  DESIGN.md 7e.
//
// Transpose = a stable sort of the edge positions e by their column id.  The positions start in increasing order, so a
// least-significant-digit radix sort with 8-bit digits over the ids gives exactly numpy.argsort(column_index, kind="stable"):
//   per pass   transpose_hist_kernel     tile of 4,096 edges -> 256 digit counts (LDS integer atomics) -> hist[digit][tile]
//              scan_* kernels            exclusive scan of hist in digit-major order = where every (digit, tile) run starts
//              transpose_scatter_kernel  the tile again, 256 edges per round in order: the rank of an edge among the edges of
//                                        its digit that precede it in the tile (wave ballots + per-wave counts in LDS)
//   then       transpose_rows_kernel     t_row_pointers[j] = lower bound of j among the sorted ids
//              transpose_finish_kernel   t_column_index[p] = the row of edge t_perm[p] (search in row_pointers); -1 tails
// An id outside [0, num_in_rows) sorts as num_in_rows, behind every real id.  Counts are integers and every position is
// computed, none is handed out by a global atomic: the result is the same bits on every run and for every launch shape.
// The passes ping-pong between library scratch and the two output arrays, so the scratch is 8 bytes per edge (12 when the
// caller wants no t_perm) plus 1 KiB per tile.
// The partition = part_count_kernel, the scan, a read-back of the total, part_fill_kernel; the rule is gnna_parts.h's.  Here
// is also what gnna_sample.hip, gnna_topk.hip and gnna_walk.hip take from gnna_internal.h: the scan, refuse_capture, the clear,
// the group count of row pointers, the read-back of a call's record and the lanes-per-row choice.
#include <algorithm>

#include "gnna_device.h"
#include "gnna_internal.h"
#include "gnna_parts.h"

namespace gnna {
namespace {

constexpr int kSlotTranspose = 7;                            // library scratch: sort buffers + digit counts / parts per row
constexpr int kScanItems = 16, kScanTile = kBlock * kScanItems;
constexpr int kSortItems = 16, kSortTile = kBlock * kSortItems;
constexpr int kDigits = 256;
static_assert(kDigits == kBlock, "one thread per digit");

// ---- exclusive scan of int32 counts whose total fits int32 (in place) -------------------------------------------------

// Exclusive prefix of `v` over the block's threads; *total = the block's sum (every thread).  All threads must call it.
__device__ __forceinline__ int block_exclusive_scan(int v, int *total)
{
    __shared__ int s_wave[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int incl = wave_inclusive_scan(v);
    __syncthreads();                                           // (the previous call's readers are done with s_wave)
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        const int t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + incl - v;
}

__global__ void __launch_bounds__(kBlock)
scan_reduce_kernel(const int32_t *__restrict__ data, int64_t n, int32_t *__restrict__ partial)
{
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) sum += base + k < n ? data[base + k] : 0;
    int total;
    (void)block_exclusive_scan(sum, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one block: partial[b] <- sum of partial[0 .. b)
__global__ void __launch_bounds__(kBlock)
scan_partials_kernel(int32_t *__restrict__ partial, int64_t num)
{
    int carry = 0;
    for (int64_t base = 0; base < num; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const int v = i < num ? partial[i] : 0;
        int total;
        const int excl = block_exclusive_scan(v, &total);
        if (i < num) partial[i] = carry + excl;
        carry += total;
    }
}

__global__ void __launch_bounds__(kBlock)
scan_apply_kernel(int32_t *__restrict__ data, int64_t n, const int32_t *__restrict__ partial)
{
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int v[kScanItems];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) { v[k] = base + k < n ? data[base + k] : 0; sum += v[k]; }
    int total;
    int run = partial[blockIdx.x] + block_exclusive_scan(sum, &total);
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < n) data[base + k] = run;
        run += v[k];
    }
}

}  // namespace

// (shared through gnna_internal.h)
int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

// data[i] <- sum of data[0 .. i) for i < n; `partial` holds scan_tiles(n) ints.
int launch_exclusive_scan(hipStream_t stream, int32_t *data, int64_t n, int32_t *partial)
{
    if (n <= 0) return GNNA_OK;
    const int64_t tiles = scan_tiles(n);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, stream, data, n, partial);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kBlock), 0, stream, partial, tiles);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, stream, data, n, partial);
    return launch_ok("scan launch");
}

namespace {

// ---- the radix passes -------------------------------------------------------------------------------------------------

// The sort key of a column id: the id, or num_in_rows for an id that names no source row.
__device__ __forceinline__ uint32_t key_of(int32_t id, uint32_t num_in_rows)
{
    return (uint32_t)id < num_in_rows ? (uint32_t)id : num_in_rows;
}

// FIRST: `keys` is the caller's column_index (ids are mapped by key_of, the value of edge i is i itself).
template <bool FIRST>
__global__ void __launch_bounds__(kBlock)
transpose_hist_kernel(const int32_t *__restrict__ keys, int64_t nnz, uint32_t num_in_rows, int shift,
                      int32_t *__restrict__ hist, int64_t tiles)
{
    __shared__ int s_count[kDigits];
    s_count[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSortTile + threadIdx.x;
#pragma unroll 4
    for (int r = 0; r < kSortItems; r++) {
        const int64_t i = base + (int64_t)r * kBlock;
        if (i < nnz) {
            const uint32_t key = FIRST ? key_of(keys[i], num_in_rows) : (uint32_t)keys[i];
            atomicAdd(&s_count[(key >> shift) & (kDigits - 1)], 1);
        }
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * tiles + blockIdx.x] = s_count[threadIdx.x];
}

template <bool FIRST>
__global__ void __launch_bounds__(kBlock)
transpose_scatter_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t nnz, uint32_t num_in_rows,
                         int shift, const int32_t *__restrict__ hist, int64_t tiles, int32_t *__restrict__ keys_out,
                         int32_t *__restrict__ vals_out)
{
    __shared__ int s_run[kDigits];                        // where the next edge of a digit goes
    __shared__ int s_cnt[kWavesPerBlock][kDigits];        // this round's edges per wave and digit
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    s_run[tid] = hist[(int64_t)tid * tiles + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t base = (int64_t)blockIdx.x * kSortTile + tid;
    for (int r = 0; r < kSortItems; r++) {
        const int64_t i = base + (int64_t)r * kBlock;
        const bool valid = i < nnz;
        uint32_t key = 0;
        int32_t val = 0;
        if (valid) {
            key = FIRST ? key_of(keys[i], num_in_rows) : (uint32_t)keys[i];
            val = FIRST ? (int32_t)i : vals[i];
        }
        const uint32_t d = (key >> shift) & (kDigits - 1);
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; w++) s_cnt[w][tid] = 0;
        // the lanes of this wave that hold an edge of the same digit
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long set = __ballot(bit);
            same &= bit ? set : ~set;
        }
        const int rank = __popcll(same & below);
        __syncthreads();
        if (valid && rank == 0) s_cnt[wave][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            int pos = s_run[d] + rank;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; w++)
                if (w < wave) pos += s_cnt[w][d];
            if ((uint32_t)pos < (uint64_t)nnz) {              // (always, for a histogram of these very keys)
                keys_out[pos] = (int32_t)key;
                vals_out[pos] = val;
            }
        }
        __syncthreads();
        int add = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; w++) add += s_cnt[w][tid];
        s_run[tid] += add;
    }
}

// t_row_pointers[j] = how many sorted keys are below j, j in [0, num_in_rows]
__global__ void __launch_bounds__(kBlock)
transpose_rows_kernel(const int32_t *__restrict__ sorted_keys, int64_t nnz, int64_t num_in_rows, int32_t *__restrict__ t_rp)
{
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j <= num_in_rows; j += (int64_t)gridDim.x * kBlock) {
        int64_t lo = 0, hi = nnz;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(uint32_t)sorted_keys[mid] < j) lo = mid + 1; else hi = mid;
        }
        t_rp[j] = (int32_t)lo;
    }
}

// keys_ids: the sorted keys on entry, t_column_index on exit.  perm: the sorted positions; perm_is_output: it is the caller's
// t_perm, whose tail (the dropped edges) becomes -1.
__global__ void __launch_bounds__(kBlock)
transpose_finish_kernel(const int32_t *__restrict__ rp, int64_t num_out_rows, uint32_t num_in_rows, int64_t nnz,
                        int32_t *__restrict__ keys_ids, int32_t *__restrict__ perm, bool perm_is_output)
{
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * kBlock) {
        int32_t row = -1;
        if ((uint32_t)keys_ids[p] < num_in_rows) {
            const int32_t e = perm[p];
            // the last row i with rp[i] <= e (rows without edges share their start with the next row)
            int64_t lo = 0, hi = num_out_rows - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (rp[mid] <= e) lo = mid; else hi = mid - 1;
            }
            row = (int32_t)lo;
        } else if (perm_is_output) {
            perm[p] = -1;
        }
        keys_ids[p] = row;
    }
}

__global__ void __launch_bounds__(kBlock)
clear_kernel(int32_t *__restrict__ words, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) words[i] = 0;
}

// ---- neighbor-group partition (the rule: gnna_parts.h) ------------------------------------------------------------------

// count[i] = groups of row i for i < rows (0 for a row whose pointers decrease), 0 from there to n, which the scan turns into
// the total.  rows = *rows_word, or n without one.
__global__ void __launch_bounds__(kBlock)
part_count_kernel(const int32_t *__restrict__ rp, int64_t n, const long long *__restrict__ rows_word, int partSize,
                  int32_t *__restrict__ count)
{
    const int64_t rows = rows_word ? (int64_t)*rows_word : n;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (int64_t)gridDim.x * kBlock)
        count[i] = groups_of(i < rows ? (int64_t)rp[i + 1] - (int64_t)rp[i] : 0, partSize);
}

// the partition of device row pointers; num_parts is the host's (scan_parts read it back)
__global__ void __launch_bounds__(kBlock)
part_fill_kernel(const CsrRows rows, const int32_t *__restrict__ first_part, int partSize, int64_t num_parts,
                 int32_t *__restrict__ pp, int32_t *__restrict__ p2n)
{
    fill_parts(rows, first_part, partSize, num_parts, pp, p2n);
}

}  // namespace

// ---- shared with gnna_sample.hip, gnna_topk.hip and gnna_walk.hip through gnna_internal.h ---------------------------------

int refuse_capture(const char *what, hipStream_t stream)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(GNNA_ERR_UNSUPPORTED, "%s reads a count back and cannot run inside a stream capture: call it before capturing", what);
    return GNNA_OK;
}

void launch_clear_words(DeviceState *ds, hipStream_t stream, int32_t *words, int64_t n)
{
    hipLaunchKernelGGL(clear_kernel, dim3(elementwise_grid(n, ds->num_cus, 16)), dim3(kBlock), 0, stream, words, n);
}

void launch_part_count(DeviceState *ds, hipStream_t stream, const int32_t *rp, int64_t n, const long long *rows_word, int partSize,
                       int32_t *count)
{
    hipLaunchKernelGGL(part_count_kernel, dim3(elementwise_grid(n + 1, ds->num_cus, 16)), dim3(kBlock), 0, stream, rp, n, rows_word,
                       partSize, count);
}

int read_record(const char *what, hipStream_t stream, const long long *rec, long long *host, int words)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GNNA_ERR_HIP, "%s: launch: %s", what, hipGetErrorString(e));
    e = hipMemcpyAsync(host, rec, (size_t)words * sizeof(long long), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(GNNA_ERR_HIP, "%s: reading the counts back: %s", what, hipGetErrorString(e));
    return GNNA_OK;
}

int lanes_per_row(const int32_t *column_index, int64_t fallback_avg)
{
    gnna_tuning tune;
    gnna_get_tuning(&tune);
    apply_graph_hints(column_index, 0, &tune);
    return std::max(4, std::min(kWave, pow2_at_least(tune.avg_degree > 0 ? tune.avg_degree : fallback_avg)));
}

namespace {

int read_back_i32(const char *what, hipStream_t stream, const int32_t *src, int32_t *value)
{
    hipError_t e = hipMemcpyAsync(value, src, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(GNNA_ERR_HIP, "%s: reading a count back: %s", what, hipGetErrorString(e));
    return GNNA_OK;
}

// first_part[i] (scratch, [num_nodes + 1]) = groups of the rows before i; *num_parts = their total (synchronises).
int scan_parts(const char *what, DeviceState *ds, hipStream_t stream, int partSize, const int32_t *rp, int64_t num_nodes,
               int32_t **first_part, int64_t *num_parts)
{
    const int64_t n = num_nodes + 1;
    Carver c;
    const size_t o_count = c.add((size_t)n * 4), o_partial = c.add((size_t)scan_tiles(n) * 4);
    void *ws = nullptr;
    int rc = get_workspace(ds, stream, kSlotTranspose, c.bytes, &ws);
    if (rc != GNNA_OK) return rc;
    int32_t *count = Carver::at<int32_t>(ws, o_count), *partial = Carver::at<int32_t>(ws, o_partial);
    launch_part_count(ds, stream, rp, num_nodes, nullptr, partSize, count);
    rc = launch_exclusive_scan(stream, count, n, partial);
    if (rc != GNNA_OK) return rc;
    int32_t total = 0;
    rc = read_back_i32(what, stream, count + num_nodes, &total);
    if (rc != GNNA_OK) return rc;
    if (total < 0) return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 neighbor-groups", what);
    *first_part = count;
    *num_parts = total;
    return GNNA_OK;
}

int check_part_args(const char *what, int partSize, const int32_t *indptr, int64_t num_nodes)
{
    if (partSize <= 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: partSize must be positive (got %d)", what, partSize);
    if (num_nodes < 0 || !indptr) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad indptr / num_nodes", what);
    if (num_nodes >= 0x7fffffffLL) return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 rows", what);
    return GNNA_OK;
}

}  // namespace
}  // namespace gnna

using namespace gnna;

extern "C" {
#pragma GCC visibility push(default)

int gnna_transpose_csr_i32(const int32_t *row_pointers, const int32_t *column_index, int64_t num_out_rows, int64_t num_in_rows,
                           int32_t *t_row_pointers, int32_t *t_column_index, int32_t *t_perm, void *stream_v)
{
    const char *what = "gnna_transpose_csr_i32";
    if (num_out_rows < 0 || num_in_rows < 0 || !t_row_pointers || (num_out_rows > 0 && !row_pointers))
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: bad sizes or a null pointer (num_out_rows=%lld num_in_rows=%lld)", what,
                    (long long)num_out_rows, (long long)num_in_rows);
    if (num_out_rows >= 0x7fffffffLL || num_in_rows >= 0x7fffffffLL)
        return fail(GNNA_ERR_UNSUPPORTED, "%s: more than 2^31 - 2 rows", what);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = refuse_capture(what, stream);
    if (rc != GNNA_OK) return rc;
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    int32_t nnz32 = 0;
    if (num_out_rows > 0) {
        rc = read_back_i32(what, stream, row_pointers + num_out_rows, &nnz32);
        if (rc != GNNA_OK) return rc;
    }
    const int64_t nnz = nnz32;
    if (nnz < 0) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: row_pointers[num_out_rows] = %d", what, nnz32);
    if (nnz == 0) {
        launch_clear_words(ds, stream, t_row_pointers, num_in_rows + 1);
        return launch_ok("%s: launch", what);
    }
    if (!column_index || !t_column_index) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null index pointer", what);
    if (t_column_index == column_index || t_perm == column_index || t_perm == t_column_index ||
        t_row_pointers == row_pointers)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: an output must not alias an input or another output", what);

    // digits that tell the keys 0 .. num_in_rows apart
    int passes = 1;
    while (passes < 4 && ((uint64_t)num_in_rows >> (8 * passes)) != 0) passes++;
    const int64_t tiles = (nnz + kSortTile - 1) / kSortTile;
    const int64_t hist_len = tiles * kDigits;
    // scratch: [keys][positions] (one side of the ping-pong) [positions of the other side, without a t_perm][hist][scan partials]
    Carver c;
    const size_t o_keys = c.add((size_t)nnz * 4), o_vals = c.add((size_t)nnz * 4), o_vals_b = t_perm ? 0 : c.add((size_t)nnz * 4);
    const size_t o_hist = c.add((size_t)hist_len * 4), o_partial = c.add((size_t)scan_tiles(hist_len) * 4);
    void *ws = nullptr;
    rc = get_workspace(ds, stream, kSlotTranspose, c.bytes, &ws);
    if (rc != GNNA_OK) return rc;
    int32_t *keys_a = Carver::at<int32_t>(ws, o_keys), *vals_a = Carver::at<int32_t>(ws, o_vals);
    int32_t *keys_b = t_column_index, *vals_b = t_perm ? t_perm : Carver::at<int32_t>(ws, o_vals_b);
    int32_t *hist = Carver::at<int32_t>(ws, o_hist), *partial = Carver::at<int32_t>(ws, o_partial);

    const int32_t *keys_in = column_index, *vals_in = nullptr;
    const uint32_t n_in = (uint32_t)num_in_rows;
    const dim3 grid((unsigned)tiles), block(kBlock);
    for (int k = 0; k < passes; k++) {
        const bool to_b = ((passes - 1 - k) & 1) == 0;       // the last pass writes into the output arrays
        int32_t *keys_out = to_b ? keys_b : keys_a, *vals_out = to_b ? vals_b : vals_a;
        const int shift = 8 * k;
        if (k == 0) hipLaunchKernelGGL(transpose_hist_kernel<true>, grid, block, 0, stream, keys_in, nnz, n_in, shift, hist, tiles);
        else hipLaunchKernelGGL(transpose_hist_kernel<false>, grid, block, 0, stream, keys_in, nnz, n_in, shift, hist, tiles);
        rc = launch_exclusive_scan(stream, hist, hist_len, partial);
        if (rc != GNNA_OK) return rc;
        if (k == 0)
            hipLaunchKernelGGL(transpose_scatter_kernel<true>, grid, block, 0, stream, keys_in, vals_in, nnz, n_in, shift, hist, tiles,
                               keys_out, vals_out);
        else
            hipLaunchKernelGGL(transpose_scatter_kernel<false>, grid, block, 0, stream, keys_in, vals_in, nnz, n_in, shift, hist, tiles,
                               keys_out, vals_out);
        keys_in = keys_out;
        vals_in = vals_out;
    }
    hipLaunchKernelGGL(transpose_rows_kernel, dim3(elementwise_grid(num_in_rows + 1, ds->num_cus, 16)), block, 0, stream, keys_b,
                       nnz, num_in_rows, t_row_pointers);
    hipLaunchKernelGGL(transpose_finish_kernel, dim3(elementwise_grid(nnz, ds->num_cus, 16)), block, 0, stream, row_pointers,
                       num_out_rows, n_in, nnz, keys_b, vals_b, t_perm != nullptr);
    return launch_ok("%s: launch", what);
}

int64_t gnna_count_parts_device_i32(int partSize, const int32_t *indptr, int64_t num_nodes, void *stream_v)
{
    const char *what = "gnna_count_parts_device_i32";
    int rc = check_part_args(what, partSize, indptr, num_nodes);
    if (rc != GNNA_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    rc = refuse_capture(what, stream);
    if (rc != GNNA_OK) return rc;
    if (num_nodes == 0) return 0;
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    int32_t *first_part = nullptr;
    int64_t parts = 0;
    rc = scan_parts(what, ds, stream, partSize, indptr, num_nodes, &first_part, &parts);
    return rc != GNNA_OK ? rc : parts;
}

int gnna_build_part_device_i32(int partSize, const int32_t *indptr, int64_t num_nodes, int32_t *partPtr, int32_t *part2Node,
                               int64_t num_parts, void *stream_v)
{
    const char *what = "gnna_build_part_device_i32";
    int rc = check_part_args(what, partSize, indptr, num_nodes);
    if (rc != GNNA_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    rc = refuse_capture(what, stream);
    if (rc != GNNA_OK) return rc;
    if (!partPtr || (num_parts > 0 && !part2Node)) return fail(GNNA_ERR_INVALID_ARGUMENT, "%s: null output pointer", what);
    DeviceState *ds = nullptr;
    rc = get_device_state(&ds);
    if (rc != GNNA_OK) return rc;
    int32_t *first_part = nullptr;
    int64_t expect = 0;
    if (num_nodes > 0) {
        rc = scan_parts(what, ds, stream, partSize, indptr, num_nodes, &first_part, &expect);
        if (rc != GNNA_OK) return rc;
    }
    if (expect != num_parts)
        return fail(GNNA_ERR_INVALID_ARGUMENT, "num_parts=%lld but the CSR has %lld groups at partSize=%d", (long long)num_parts,
                    (long long)expect, partSize);
    hipLaunchKernelGGL(part_fill_kernel, dim3(elementwise_grid(num_parts + 1, ds->num_cus, 16)), dim3(kBlock), 0, stream,
                       CsrRows{indptr, num_nodes}, first_part, partSize, num_parts, partPtr, part2Node);
    return launch_ok("%s: launch", what);
}

#pragma GCC visibility pop
}  // extern "C"

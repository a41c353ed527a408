// gnna_internal.h -- shared by the translation units of libgnna.so (not installed).
#ifndef GNNA_INTERNAL_H_
#define GNNA_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "gnna.h"
#include "gnna_launch.h"

namespace gnna {

// Records a formatted message for gnna_last_error() on this thread and returns `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Host worker threads the library's CPU passes (CSR builder, renumbering) should start: the hardware threads, capped by the
// CPUs the container is actually GRANTED (cgroup v2 cpu.max / v1 cfs quota) and by GNNA_HOST_THREADS.  The GPU boxes show
// 256 hardware threads and grant 16 CPUs: 64 threads there spend most of every scheduling period throttled (round 5: the
// community renumbering of the Reddit-like graph took 90 s with 64 threads on a 16-CPU quota).
int host_thread_budget(int cap);

// Per-graph hints registered with gnna_set_graph_hints(), keyed by the column_index pointer of the
// call; overrides tune->avg_degree / nonlocal_ids when there is an entry, and tune->column_phases when a
// measured schedule for this feature width was registered with gnna_set_graph_phases().  (gnna_host.cpp)
void apply_graph_hints(const void *column_index, int dim, gnna_tuning *tune);

// ---- what the launchers of the kernel families share (grids and lane layouts: gnna_launch.h) ------
// After a launch: GNNA_OK, or GNNA_ERR_HIP with the message "<prefix>: <HIP's error string>"; the prefix is printf-style.
// (gnna_runtime.hip)
int launch_ok(const char *prefix_fmt, ...) __attribute__((format(printf, 1, 2)));
// gnna_tuning.xcd_remap as the kernels take it
inline int xcd_remap_on()
{
    gnna_tuning tune;
    gnna_get_tuning(&tune);
    return tune.xcd_remap != 0 ? 1 : 0;
}
// An entry whose sums meet through float atomics, under gnna_tuning.deterministic = 1: GNNA_ERR_UNSUPPORTED and
// "<what> has no deterministic schedule (gnna_tuning.deterministic = 1): <reason>".
inline int deterministic_refused(const char *what, const char *reason)
{
    gnna_tuning tune;
    gnna_get_tuning(&tune);
    if (tune.deterministic != 1) return GNNA_OK;
    return fail(GNNA_ERR_UNSUPPORTED, "%s has no deterministic schedule (gnna_tuning.deterministic = 1): %s", what, reason);
}

// ---- per-device runtime state (gnna_runtime.hip) -------------------------------------------------
struct Workspace {
    void *ptr = nullptr;
    size_t bytes = 0;
};
// Scratch of a call that is being captured: keyed by the capture (hipStreamGetCaptureInfo's id), the stream and the slot.  A
// graph runs whenever and wherever it is replayed -- next to any eager call and any other graph -- so these buffers are handed
// to the calls of that one capture on that one stream only, and are never freed.
struct CaptureKey {
    unsigned long long capture_id;
    hipStream_t stream;
    int slot;
    bool operator<(const CaptureKey &o) const
    {
        if (capture_id != o.capture_id) return capture_id < o.capture_id;
        if (stream != o.stream) return stream < o.stream;
        return slot < o.slot;
    }
};
struct DeviceState {
    std::atomic<bool> init{false};
    int num_cus = 256;
    int32_t *flags = nullptr;  // two arrays of kFlagSlots ints, zero-initialised: [slot] "partition is not canonical",
                               // [kFlagSlots + slot] "the packed ids are stale" -- each holds the sequence number of the call
                               // that raised it; slot = the call's block (call_block_of)
    unsigned long long *gap_lists = nullptr;   // kCallBlocks lists of kGapWords words (call_block_of)
    uint32_t *sweep_sync = nullptr;  // kCallBlocks counter blocks for the sweep kernel's soft barrier (call_block_of)
    std::map<hipStream_t, int> stream_block;   // streams that own one of the first kStreamBlocks call blocks
    int captured_blocks = 0;                   // call blocks handed to captured calls so far (never returned)
    std::map<std::pair<hipStream_t, int>, Workspace> ws;  // eager calls, per stream: slot 1 staged / pre-scaled X, slot 2 partial
                                                          // rows of the deterministic schedule / slabs of the weight-gradient kernel
    std::map<CaptureKey, Workspace> capture_ws;           // captured calls: the same slots, per capture and stream (never freed)
    std::vector<void *> capture_outgrown;                 // buffers a capture outgrew: earlier calls of its graph still point at them
};
constexpr int kFlagSlots = 1024;
// per-call lists of long runs of rows without edges that the sparse prologue leaves to a grid-wide pass
constexpr int kGapEntries = 63, kGapWords = 2 + 2 * kGapEntries;   // word 0: count, pairs (first row, rows)
// Per-call device scratch that is NOT tagged with the call's sequence number (the gap list of the sparse prologue, the sweep
// kernel's step counters and ReLU list) lives in "call blocks".  Work on one stream is ordered, so a stream needs one block:
//   * the first kStreamBlocks streams that call the library get a block of their own (no allocation);
//   * a call that is being CAPTURED into a graph runs whenever and wherever its graph is replayed -- not in the order of the
//     capture stream (torch.cuda.graph captures every graph on one shared side stream) and possibly next to a replay of another
//     graph: each of the first kCapturedBlocks captured calls of a device gets a block of its own FOR GOOD (the graph may be
//     replayed at any time; round 6, ADVICE r5 -- before, they shared the ring below by sequence number);
//   * calls on further streams, and captured calls beyond those, share a ring of the remaining blocks by call count: graphs
//     captured after the first kCapturedBlocks calls must not be replayed concurrently with each other (include/gnna.h).
// (A ring alone, shared by all streams, lets a call on one stream clear the block of a call that is still running on another.)
constexpr int kStreamBlocks = 64, kCapturedBlocks = 160, kCallBlocks = 256;
static_assert(kCallBlocks <= kFlagSlots && kStreamBlocks + kCapturedBlocks < kCallBlocks, "call blocks");

// State of the current device (lazily created: CU count, flag ring).
int get_device_state(DeviceState **out);
// Scratch buffer `slot` of `stream` for an eager call (grow-only, shared by the eager calls on that stream), or -- while `stream`
// is being captured -- of that capture on that stream (allocated at capture time, never freed, never handed to another call).
int get_workspace(DeviceState *ds, hipStream_t stream, int slot, size_t bytes, void **out);
// The layout of a call's scratch buffer: add() declares a region of b bytes ONCE and gives its 256-byte aligned offset, in the
// order of the calls; `bytes` is what get_workspace is asked for, at<T>(base, offset) the region's pointer.
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Carver {
    size_t bytes = 0;
    size_t add(size_t b) { const size_t offset = bytes; bytes += align256(b); return offset; }
    template <class T>
    static T *at(void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(base) + offset); }
};
// Fresh non-zero sequence number of an aggregation call on `stream` and its slot among the flags (the call block's index).
int32_t next_call_seq(DeviceState *ds, hipStream_t stream, int32_t **flag_slot);
// Index of the call block (see kCallBlocks) of a call with sequence number `seq` on `stream`.
int call_block_of(DeviceState *ds, hipStream_t stream, int32_t seq);

// ---- streaming kernel + sliced schedule (gnna_stream.hip) ----------------------------------------------
constexpr int kMaxSlices = 32;    // fine source slices of a slice plan (one byte of cumulative count per group and boundary)
constexpr int kSliceLevels = 5;   // cells[l]: non-empty (group, slice) cells when the fine slices are merged into kMaxSlices >> l
struct SlicePlanStats {
    bool valid = false;
    double cells[kSliceLevels] = {0, 0, 0, 0, 0};
    double edges = 0, groups = 0;
    double span = 0;                 // sum over the edges of |column id - destination row|
    double unsorted = 0;             // neighbor-groups whose column ids are not in non-decreasing order
    double near[24] = {0};           // near[k]: edges with |column id - destination row| < 256 * 2^(k / 2)
};
struct SlicePlan {
    const uint8_t *cnt = nullptr;    // [S - 1][P] cumulative slice counts (phase-major), null: no plan right now
    int S = 0;                       // fine slices of the plan
    uint32_t slice_rows = 0;         // source rows per fine slice
    SlicePlanStats stats;
    void *handle = nullptr;          // the plan itself (get_packed_ids)
    bool pinned = false;             // made by gnna_prepare_graph (the caller promised not to change the graph)
};
// Fine slicing of `num_in_rows` source rows: S = kMaxSlices slices of ceil(num_in_rows / S) rows.
inline uint32_t slice_rows_for(int64_t num_in_rows)
{
    const int64_t r = (num_in_rows + kMaxSlices - 1) / kMaxSlices;
    return (uint32_t)(r < 1 ? 1 : r);
}
// Slice plan of the partition for gathers from `num_in_rows` source rows (library cache keyed by the device
// addresses; a miss enqueues the counting kernel on `stream`, and with want_stats synchronises it once to read
// the statistics).  out->cnt stays null when the plan cannot be built right now (stream capture, or the
// back-off for partitions that are never seen twice).  A plan made by gnna_prepare_graph is never evicted.
int get_slice_plan(DeviceState *ds, hipStream_t stream, const int32_t *column_index, const int32_t *part_pointers,
                   const int32_t *part2Node, int64_t num_parts, int64_t num_in_rows, bool want_stats, bool pin,
                   SlicePlan *out, uint32_t window_rows = 0);
void drop_slice_plans();
// Packed column ids of a plan for (B phases, G groups per chunk): see gnna_stream.hip.  *ids == null: none.  The
// caller decides whether the plan may have them (pinned, or gnna_tuning.pack_ids = 1).
int get_packed_ids(DeviceState *ds, hipStream_t stream, void *plan_handle, int B, int G, bool may_build, bool force,
                   const int32_t **ids, const uint32_t **item_off, const unsigned long long **checksum = nullptr,
                   int64_t *num_ids = nullptr, int32_t *stale_flag = nullptr, int32_t seq = 0, int check_every = 0);
// One-wavefront comparison of the graph's samples with a packed copy's state words (for calls without a prologue).
int launch_ids_sample_check(hipStream_t stream, const int32_t *col, int64_t n, const int32_t *pp, int64_t P,
                            const unsigned long long *state, int32_t *stale_flag, int32_t seq);
// Forgets the plans whose column_index starts at this address (all plans when null).  -> number of plans dropped.
// deferred: the device buffers are not freed now (no synchronisation: safe from a finalizer on any thread, during a
// stream capture) but at the next gnna_prepare_graph / gnna_release_graph / plan allocation with no launch in flight.
int release_slice_plans(const void *column_index, bool deferred);
void drain_dead_buffers();
// An aggregation call holds plan buffers between looking them up and enqueueing its kernels: dropped plans are not freed
// in between (RAII: LaunchGuard).
void begin_launch();
void end_launch();
struct LaunchGuard {
    LaunchGuard() { begin_launch(); }
    ~LaunchGuard() { end_launch(); }
    LaunchGuard(const LaunchGuard &) = delete;
    LaunchGuard &operator=(const LaunchGuard &) = delete;
};
// Number of phases of the sliced schedule from the statistics of the partition (gnna_agg.hip).
// Where to gather `dim`-float source rows from: the caller's layout or a staged copy in the stream's scratch (gnna_agg.hip).
int stage_rows_for_gather(DeviceState *ds, hipStream_t stream, const gnna_tuning &tune, const float *input, int64_t ld_in,
                          int64_t num_in_rows, int dim, int64_t est_edges, const float **X, int *ldx_out);
int choose_slices(const SlicePlanStats &st, size_t x_bytes, int S, uint32_t slice_rows, int64_t num_out_rows,
                  bool square, bool hinted_scattered);
// Events on the launch path that the contract promises not to happen after gnna_prepare_graph (gnna_runtime_counters).
enum { CTR_PLAN_BUILDS = 0, CTR_LAUNCH_SYNCS = 1, CTR_LAUNCH_FREES = 2, CTR_LAUNCH_MALLOCS = 3, CTR_BACKOFF_SKIPS = 4,
       CTR_SWEEP_LAUNCHES = 5, CTR_PACK_BUILDS = 6, CTR_PACKED_LAUNCHES = 7, CTR_FULL_HASHES = 8, CTR_CAPTURE_SCRATCH = 9,
       CTR_DENSE_BUILDS = 10, CTR_DENSE_LAUNCHES = 11, CTR_COUNT = 12 };
void count_event(int which);
// While one lives on this thread, plan and packed-copy builds are not counted: the residual graph of a dense block is made by
// the caller's ONE gnna_prepare_graph, whose own plan and copies are what plan_builds / pack_builds count.
struct QuietBuilds {
    QuietBuilds();
    ~QuietBuilds();
    QuietBuilds(const QuietBuilds &) = delete;
    QuietBuilds &operator=(const QuietBuilds &) = delete;
};

// ---- dense hub-to-hub block of a prepared graph (gnna_dense.hip) ----------------------------------------------------
struct DenseBlock {
    void *buf = nullptr;              // one allocation: r2n, node -> rank map, bm, res_pp
    const int32_t *r2n = nullptr;     // [H_pad] rank -> node (-1: padding)
    const void *bm = nullptr;         // [H_pad / 32][H_pad / 32][64] 16-bit halves: 2 x 16 destination ranks x 8 source ranks each
    const int32_t *res_pp = nullptr;  // part_pointers of the residual graph (same part2Node, same group count)
    int32_t *res_col = nullptr;       // its column ids (an allocation of its own)
    const uint8_t *res_cnt = nullptr; // its slice counts: those of its slice plan
    void *res_plan = nullptr;         // the residual graph's (pinned) slice plan
    int H = 0, H_pad = 0, theta = 0;
    int64_t entries = 0, res_nnz = 0;
    bool forced = false;              // built under GNNA_DENSE_BLOCK=2: also taken by a forced sweep
    bool off = false;                 // the graph's latest gnna_prepare_graph ran under GNNA_DENSE_BLOCK=0
    int tile = 0;                     // destination ranks per workgroup forced by GNNA_DENSE_BLOCK_TILE (32 | 64); 0: dense_tile_ranks
    int declined_mode = -1;           // buf == null: the GNNA_DENSE_BLOCK mode under which the graph was counted and got no block
};
// Geometry of hub_block_kernel that the block rule needs: destination ranks per workgroup (the short tile; the tall one is
// twice that), source ranks per chunk (= padding).
constexpr int kDenseTileRanks = 32, kDenseChunkRanks = 128;
// Destination ranks per workgroup that a launch on H_pad ranks takes: the short tile while its workgroups are one round (one per
// compute unit), the tall one beyond -- half the workgroups, and half the bytes of the split image through the L2 per
// destination rank.  (Behind the sweep kernel of the headline, at 8,192 ranks on 256 compute units: short 46.6 us, tall 51.1;
// back to back in the stand-alone probe, with a warm L2, the tall tile is already ahead there: profiles/hub_block_presplit.)
// `forced`: DenseBlock::tile.
inline int dense_tile_ranks(int H_pad, int num_cus, int forced = 0)
{
    if (forced == kDenseTileRanks || forced == 2 * kDenseTileRanks) return forced;
    return H_pad / kDenseTileRanks <= (num_cus > 1 ? num_cus : 1) ? kDenseTileRanks : 2 * kDenseTileRanks;
}
// The split image of a call (hub_split_kernel): the three bf16 pieces of the H_pad hub rows at 64 columns, in the stream's
// scratch slot kSlotDenseImage -- per call and per stream, never on the plan.
constexpr int kSlotDenseImage = 18;
inline size_t dense_image_bytes(int H_pad) { return (size_t)H_pad * 3 * 64 * 2; }
// Row widths the block is taken at: two 128-byte lines per gathered row, what the rule's constants were measured for.  (A row
// of <= 32 floats is one request per edge: the sweep saves about half per edge taken out while the block costs the same.)
constexpr int kDenseMinDim = 33, kDenseMaxDim = 64;
// The block rule (gnna_agg.hip, beside sweep_auto_phases): hubs a block of `H` nodes keeps (whole rounds of workgroups), its
// modelled saving in seconds, and whether that is worth a block.
int trimmed_hubs(int H, int num_cus);
double dense_block_saving(double hubs, double entries, int num_cus);
bool dense_block_pays(double saving, double entries, double edges);
// GNNA_DENSE_BLOCK: 0 never, 1 (default) where the block rule finds a saving, 2 for any prepared graph whose call sweeps.
int dense_block_mode();
// Degrees, histograms, the rule's theta, hub ranks, bitmap and residual arrays of the graph, on `stream` (synchronises; only
// from gnna_prepare_graph).  out->buf stays null when the graph gets no block.
int build_dense_block(DeviceState *ds, hipStream_t stream, const int32_t *col, const int32_t *pp, const int32_t *p2n, int64_t P,
                      int64_t N, int64_t nnz, int mode, DenseBlock *out);
// GNNA_DENSE_BLOCK_TILE under GNNA_DENSE_BLOCK=2 (tests and scans): 32 or 64, anything else 0.
int dense_block_tile_env(int mode);
// image = the three bf16 pieces of X[node(j), :] for every rank j, in hub_block_kernel's operand order (dense_image_bytes(H_pad)
// bytes of the call's scratch), ahead of the sweep kernel of the same call; returns at once on the device when *stale_flag == seq.
int launch_hub_split(hipStream_t stream, const DenseBlock &db, const float *X, int ldx, int dim, void *image, const int32_t *stale_flag,
                     int32_t seq);
// Y[node(i), :] += scale(i) * sum_j bit(i, j) * X[node(j), :] from that image, behind the sweep kernel of the same call; returns
// at once on the device when *stale_flag == seq.
int launch_hub_block(DeviceState *ds, hipStream_t stream, const DenseBlock &db, const void *image, float *Y, int ldy, int dim,
                     bool scaled, float eps, const float *row_scale, const int32_t *stale_flag, int32_t seq);
// The block that hangs on a slice plan (gnna_stream.hip): a copy of it (false: none) / hang `db` on the plan, which owns its
// buffers and the residual plan from then on.
bool plan_dense_block(void *plan_handle, DenseBlock *out);
void plan_set_dense_block(void *plan_handle, const DenseBlock &db);

struct StreamLaunch {
    int mode;                 // MODE_SAG, MODE_GIN (also the pre-scaled GCN form: GIN + row_scale), MODE_GCN (per-edge) or MODE_EDGE
    const float *X; const int32_t *col; const int32_t *pp; const int32_t *p2n; float *Y;
    const uint8_t *cnt;       // slice counts or nullptr (single phase)
    const float *row_scale;
    const float *deg_row; const float *deg_col;   // MODE_GCN
    const float *A = nullptr;                      // MODE_SDDMM: destination-side features (Y = edge_out)
    const float *edge_w = nullptr;                 // MODE_EDGE: per-edge weights, indexed like column_index
    const int32_t *flag; int32_t seq; int32_t trust;
    int64_t P;
    int D, ldx, G, U, S, B;
    int lda = 0;                                   // MODE_SDDMM: row stride of A in floats (0: D)
    int ldy = 0;                                   // row stride of Y in floats (0: D)
    int win_lo = 0, win_hi = 0;                    // windowed call: the fine slices (= source windows) it covers; win_hi == S: the rest
    bool relu = false;                             // epilogue: out = max(out, 0)
    int64_t num_out_rows = 0;                      // rows of Y (the epilogue's whole-output pass)
    bool wide, plain_ok, xcd_remap;
    float eps;
    bool det = false;                              // deterministic schedule (ordered phase launches, no atomics)
    float *det_part = nullptr; int32_t *det_stamp = nullptr;   // [num_chunks][2][D] partial rows / [num_chunks][2] stamps
    const int32_t *ids_packed = nullptr; const uint32_t *item_off = nullptr;   // packed ids of a prepared graph for (B, G)
    const int32_t *packed_stale = nullptr;   // *packed_stale == seq: column_index no longer matches the copy, read column_index
};
int launch_stream(const StreamLaunch &a, hipStream_t stream);
// The ReLU epilogue over the whole output on its own (a call that has nothing to aggregate but accumulates into `out`).
int launch_stream_epilogue_only(const StreamLaunch &a, hipStream_t stream);

// ---- destination-blocked sweep kernel (gnna_sweep.hip) ------------------------------------------------------
struct SweepLaunch {
    int mode;                 // MODE_SAG or MODE_GIN (also the pre-scaled GCN form: GIN + row_scale)
    const float *X; const int32_t *col; const int32_t *pp; const int32_t *p2n; float *Y;
    const uint8_t *cnt;       // slice counts (required)
    const float *row_scale;
    const int32_t *flag; int32_t seq; int32_t trust;
    uint32_t *sync;           // kXcds counters, 64 bytes apart, + the shared-row list's two header words: zero when the kernel starts
    int64_t P;
    int D, ldx, U, S, B;
    int ldy = 0;              // row stride of Y in floats (0: D)
    bool relu = false;        // epilogue: out = max(out, 0)
    int64_t num_out_rows = 0;
    int rounds = 0;           // sets per workgroup (0: from rows_with_edges and the accumulator capacity)
    int64_t rows_with_edges = 0;
    int slack = 0;            // soft-barrier slack in steps (0: built-in, >= 1000: none)
    int wgs_per_cu = 0;       // 2: two 16-wavefront workgroups per CU (64 VGPRs, half the accumulators each); else one
    bool dynamic = true;      // item pool with chunk locks (false: fixed share of the groups per wavefront)
    bool plain_ok;
    float eps;
    const int32_t *ids_packed = nullptr; const uint32_t *item_off = nullptr;   // packed ids for (B, 64 groups per chunk)
    const int32_t *packed_stale = nullptr;
    // the residual graph of a dense block (same p2n and P), or null: the kernel walks it instead of col / pp / cnt / the packed
    // copy unless *packed_stale == seq
    const int32_t *res_col = nullptr; const int32_t *res_pp = nullptr; const uint8_t *res_cnt = nullptr;
    const int32_t *res_ids_packed = nullptr; const uint32_t *res_item_off = nullptr;
};
bool sweep_supports(int mode, int dim, size_t x_bytes);
int sweep_acc_rows(int dim, int wgs_per_cu);   // destination rows a workgroup's LDS accumulators hold at this width
int launch_sweep(DeviceState *ds, const SweepLaunch &a, hipStream_t stream);
// Phases of the sweep kernel when the library picks it on its own (gnna_tuning.sweep = 0) for this call, else 0 (gnna_agg.hip).
int sweep_auto_phases(const gnna_tuning &t, int mode, int dim, size_t x_bytes, int64_t num_out_rows, int64_t num_in_rows,
                      const SlicePlanStats &st, int B, int num_cus, bool deterministic, int part_size);
// a call block of the sweep kernel: kXcds step counters 64 bytes apart, then the ReLU epilogue's
constexpr int kSweepListCap = 1023;    // list of row ranges the kernel did not store once: [count][overflow][(first, rows) ...]
constexpr int kSweepSlotWords = 8 * 16 + 2 + 2 * kSweepListCap;

// ---- 16-bit storage, fp32 accumulation (gnna_x16.hip) ----------------------------------------------------------
struct X16Launch {
    int mode;                 // MODE_SAG, MODE_GCN (per-edge fp32 source degree, fp32 destination degree at the flush) or MODE_GIN
    int in_type, out_type;    // GNNA_BF16 / GNNA_F16; out_type may also be GNNA_F32
    const void *input; int64_t ld_in, num_in_rows;          // leading dimensions in ELEMENTS
    const int32_t *column_index; const float *degrees_out; const float *degrees_in; float epsilon;
    const int32_t *part_pointers; const int32_t *part2Node;
    void *out; int64_t ld_out, num_out_rows;
    int dim; int64_t num_parts; int partSize;
    bool accumulate, relu, xcd_remap;
    int prof_call = -1;
};
int launch_x16(DeviceState *ds, hipStream_t stream, const X16Launch &c);
// Sizes the stream's scratch of the 16-bit path for one width (staged source rows, fp32 sums of a 16-bit output).
int reserve_x16(DeviceState *ds, hipStream_t stream, int64_t num_in_rows, int64_t num_out_rows, int dim);
// out[r, 0:dim] = 0 for every row (rows `ld` floats apart): the dense prologue without its validation (gnna_agg.hip).
int launch_zero_fill(DeviceState *ds, hipStream_t stream, float *out, int64_t rows, int dim, int64_t ld);
// out[r, 0:dim] = max(out[r, 0:dim], 0) for every row (NaN stays NaN, as torch.relu): the ReLU epilogue of the entries that do
// not fuse it.  Enqueues only: the caller's launch_ok reports a failed launch in the entry's own words (gnna_agg.hip).
void launch_relu_rows(DeviceState *ds, hipStream_t stream, float *out, int64_t rows, int dim, int64_t ld);

// ---- device structure builders: what gnna_transpose.hip, gnna_sample.hip, gnna_topk.hip and gnna_walk.hip share ---------
// (defined in gnna_transpose.hip; the partition rule itself -- groups per row, owner search, fill -- is gnna_parts.h)
// Tiles of the exclusive scan over n ints: the ints of `partial` that launch_exclusive_scan needs.
int64_t scan_tiles(int64_t n);
// data[i] <- sum of data[0 .. i) for i < n, in place (int32 counts whose total fits int32); three launches, no read-back.
int launch_exclusive_scan(hipStream_t stream, int32_t *data, int64_t n, int32_t *partial);
// GNNA_ERR_UNSUPPORTED when `stream` is being captured (the prepare-time calls read a count back).
int refuse_capture(const char *what, hipStream_t stream);
// words[0 .. n) = 0: one launch (a call's record and the scratch that is cleared together with it).
void launch_clear_words(DeviceState *ds, hipStream_t stream, int32_t *words, int64_t n);
// count[i] = the neighbor-groups of row i of `rp` for i < rows, 0 for rows <= i <= n (the scan makes the last one the total):
// one launch over n + 1 items.  rows = *rows_word, read on the device, or n when rows_word is null.
void launch_part_count(DeviceState *ds, hipStream_t stream, const int32_t *rp, int64_t n, const long long *rows_word, int partSize,
                       int32_t *count);
// The tail of a call that reports through a record of `words` int64: "<what>: launch: ..." for a launch that failed, else
// host[0 .. words) = rec by one copy and one synchronisation ("<what>: reading the counts back: ...").  The words are the entry's.
int read_record(const char *what, hipStream_t stream, const long long *rec, long long *host, int words);
// Lanes per row (a power of two, 4 .. 64) from the edges an average row has: the hint of `column_index`, else fallback_avg.
int lanes_per_row(const int32_t *column_index, int64_t fallback_avg);

// ---- optional per-call kernel timing (gnna_profile_begin/end) ---------------------------------------
// Returns the index of this call in the active profile (-1 when not profiling).
int profile_acquire_call(bool has_work);
// Records event `which` (0 before the prologue, 1 between, 2 after the aggregation) of call `call`.
void profile_record(int call, int which, hipStream_t stream);

}  // namespace gnna

#endif

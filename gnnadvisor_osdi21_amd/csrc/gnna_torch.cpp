// gnna_torch.cpp -- the Python extension module `GNNAdvisor` on PyTorch-ROCm.
//
// Mirrors the reference's extension boundary one-to-one (GNNAdvisor/GNNConv/GNNAdvisor.cpp:
// SAG :75-96, forward :99-122, backward :124-150, forward_gin :156-178,
// backward_gin :183-207, build_part :210-251, module table :253-263): same function
// names, positional arguments, return shapes and the same CHECK_INPUT error texts.
// The five host launchers keep the reference's names (SAG_cuda, spmm_forward_cuda, ...,
// GNNAdvisor_kernel.cu:110,267,422,559,696) but are thin shims over the C ABI of
// libgnna.so (include/gnna.h); the dense updates X W and G W^T stay torch::mm (rocBLAS /
// hipBLASLt) exactly where the reference calls it, the weight gradient X^T G goes to libgnna's
// MFMA kernel (gnna_xtg_f32).  Extension functions beyond the reference's six: backward_weight,
// aggregate_gin, xtg, aggregate_ld (used by ops.py).
//
// Differences from the reference, all deliberate (DESIGN.md "Boundary"):
//   * work is enqueued on PyTorch's *current* HIP stream of the input's device (the
//     reference launches on the legacy default stream, .cu:149);
//   * a failed launch raises RuntimeError (the reference printf()s and exit(-1)s);
//   * dtype is checked up front (the reference fails later inside packed_accessor32);
//   * build_part returns int32 tensors (the reference returns float32, inexact > 2^24;
//     its caller's `.int()` is a no-op on these) and always writes the closing sentinel.
#include <cstdlib>
#include <limits>
#include <torch/extension.h>
#include <torch/csrc/Dtype.h>

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <cmath>
#include <vector>

#include "gnna_ext.h"
#include "gnna_gatv2.h"
#include "gnna_dotattn.h"
#include "gnna_gat_edge.h"
#include "gnna_stats.h"
#include "gnna_softagg.h"
#include "gnna_pool.h"
#include "gnna_attnpool.h"
#include "gnna_topk.h"
#include "gnna_segnorm.h"
#include "gnna_walk.h"
#include "gnna_spatial.h"
#include "gnna_edgefeat.h"

#define CHECK_CUDA(x) TORCH_CHECK(x.is_cuda(), #x " must be a CUDA tensor")
#define CHECK_CONTIGUOUS(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")
#define CHECK_INPUT(x) CHECK_CUDA(x); CHECK_CONTIGUOUS(x)
#define CHECK_F32(x) TORCH_CHECK(x.scalar_type() == at::kFloat, #x " must be float32 (got ", x.scalar_type(), ")")
#define CHECK_I32(x) TORCH_CHECK(x.scalar_type() == at::kInt, #x " must be int32 (got ", x.scalar_type(), ")")

namespace {

enum AggKind { AGG_SAG, AGG_GCN, AGG_GIN };

// ---- automatic graph lifecycle for callers of the six reference functions ------------------------------------------
// The reference API has no "this graph is immutable" call, so a drop-in caller (GNNA_main.py, unitest.py) never reaches
// gnna_prepare_graph and its aggregations read the column ids one cache line per neighbor-group and phase instead of
// from the packed copy (1.442 against 1.36 ms on the Reddit-like headline).  This module knows more
// than a raw-pointer caller can tell the C ABI: a torch tensor carries a VERSION COUNTER that every in-place write
// through torch bumps, and a storage that outlives or dies with it.  A graph -- the (column_index, part_pointers,
// part2Node) triple -- that is seen a THIRD time with the same storages, data pointers, sizes and version counters, while no
// stream of new graphs is passing through (see note_graph), is the same immutable graph the first call saw, and is prepared
// then (one stream synchronisation + the packed copy, nnz x 4 bytes, per width; never inside a stream capture).  Any change -- a version bump, a new storage at the old address,
// another size or partSize -- forgets the library's plan for that address first (gnna_forget_graph) and starts over.  The
// packed copy's own checks stay as a second guard for writes that bypass torch: 2 x 1,024 samples at every call and a 64-bit hash of
// all ids at every 64th (gnna_tuning.ids_check_every; GNNA.forget_graph(column_index) tells the module at once).  GNNA_AUTO_PREPARE=0
// turns the automatic lifecycle off.
struct SeenGraph {
    const void *ci = nullptr, *pp = nullptr, *p2n = nullptr;
    c10::weak_intrusive_ptr<c10::StorageImpl> s_ci{c10::intrusive_ptr<c10::StorageImpl>()},
        s_pp{c10::intrusive_ptr<c10::StorageImpl>()}, s_p2n{c10::intrusive_ptr<c10::StorageImpl>()};
    uint32_t v_ci = 0, v_pp = 0, v_p2n = 0;
    int64_t nnz = 0, parts = 0, rows = 0;
    int partSize = 0, device = -1;
    int sightings = 0;
    uint64_t stamp = 0, born = 0;     // call numbers (g_seen_clock) of the latest and of the first sighting
    std::vector<int> dims_done;       // widths gnna_prepare_graph has been called for (successfully or not: one attempt each)
};
constexpr int kSeenGraphs = 16;
SeenGraph g_seen[kSeenGraphs];
std::mutex g_seen_mutex;
uint64_t g_seen_clock = 0;
std::atomic<long long> g_auto_prepared{0};

bool same_storage(const c10::weak_intrusive_ptr<c10::StorageImpl> &w, const torch::Tensor &t)
{
    return !w.expired() && w._unsafe_get_target() == t.storage().unsafeGetStorageImpl();
}

// gnna_forget_plans() drops every plan keyed by this column_index -- those of the other partitions over the same array too:
// their entries must prepare again (at their next call) instead of believing their plans are still pinned.  Only what this
// module pinned goes: hints and measured schedules the CALLER registered for a graph that is still alive (gnna_set_graph_hints,
// gnna_set_graph_phases) are not this module's to wipe.  Caller holds the mutex.
void forget_plans_of(const void *ci)
{
    (void)gnna_forget_plans(static_cast<const int32_t *>(ci));
    for (auto &g : g_seen)
        if (g.ci == ci) g.dims_done.clear();
}

// When is a graph "the same immutable graph again"?  Not at its second sighting (round 5's rule): in sampled / mini-batch
// training every step's fresh subgraph is seen several times within the step (second layer, backward) and would be prepared --
// a stream synchronisation, a counting pass, hipMalloc of the packed copy -- only to be dropped with a hipFree when its tensors
// die.  The rule now:
//   * at least kSightings calls with unchanged storages and version counters,
//   * at least kMinEdges edges (the packed copy pays on the sliced schedules of large graphs only),
//   * and the set of graphs is standing still: no OTHER graph made its first appearance within the last kQuietWindow calls
//     (the module's counterpart of the library's own back-off for partitions that keep changing).  A second standing graph
//     (train / validation) is therefore prepared kQuietWindow calls after it turned up; of a stream of mini-batches only the
//     very first is.
constexpr int kSightings = 3;
constexpr int64_t kMinEdges = 1 << 18;
constexpr uint64_t kQuietWindow = 32;
constexpr int kQuietOthers = 0;
uint64_t g_first_seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // call numbers of the latest first appearances (ring)
int g_first_seen_at = 0;

void note_graph(const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node,
                int64_t rows, int partSize, int dim, void *stream)
{
    // GNNA_AUTO_PREPARE (read at every call): 0 = off, 1 / unset = the rule above, 2 = eager -- the second sighting, any size,
    // whatever else is passing through (round 5's rule: for callers who know their graphs are few and fixed, and for the tests)
    const char *env = std::getenv("GNNA_AUTO_PREPARE");
    const int policy = env ? std::atoi(env) : 1;
    if (policy == 0 || part2Node.size(0) == 0 || column_index.numel() == 0 || dim <= 0) return;
    const bool eager = policy == 2;
    if (column_index.is_inference() || part_pointers.is_inference() || part2Node.is_inference()) return;   // (no version counter)
    const void *ci = column_index.data_ptr();
    const int device = column_index.get_device();
    std::lock_guard<std::mutex> lock(g_seen_mutex);
    const uint64_t now = ++g_seen_clock;
    // graphs whose tensors are gone: their plans (and packed copies: nnz x 4 bytes each) must not stay pinned in the library
    for (auto &g : g_seen)
        if (g.ci && (g.s_ci.expired() || g.s_pp.expired() || g.s_p2n.expired())) {
            const void *gone = g.ci;
            const bool pinned = !g.dims_done.empty();
            g = SeenGraph();
            if (pinned) forget_plans_of(gone);
        }
    SeenGraph *e = nullptr, *victim = &g_seen[0];
    // (an entry is one PARTITION of a graph -- the three arrays together: two partitions over one column_index, e.g. two
    // neighbor-group sizes, are two entries and do not evict each other call by call)
    for (auto &g : g_seen) {
        if (g.ci == ci && g.pp == part_pointers.data_ptr() && g.p2n == part2Node.data_ptr() && g.device == device) { e = &g; break; }
        if (g.stamp < victim->stamp) victim = &g;
    }
    const bool same = e && same_storage(e->s_ci, column_index) && same_storage(e->s_pp, part_pointers) &&
                      same_storage(e->s_p2n, part2Node) && e->v_ci == column_index._version() &&
                      e->v_pp == part_pointers._version() && e->v_p2n == part2Node._version() &&
                      e->nnz == column_index.numel() && e->parts == part2Node.size(0) && e->rows == rows &&
                      e->partSize == partSize;
    if (!same) {
        if (e) {
            if (!e->dims_done.empty()) forget_plans_of(ci);               // another graph lives at this address now
        } else {
            e = victim;                                                    // (the least recently seen entry makes room:
            if (e->ci && !e->dims_done.empty()) forget_plans_of(e->ci);    // unpin what it pinned)
        }
        *e = SeenGraph();
        e->ci = ci; e->pp = part_pointers.data_ptr(); e->p2n = part2Node.data_ptr();
        e->s_ci = column_index.storage().getWeakStorageImpl();
        e->s_pp = part_pointers.storage().getWeakStorageImpl();
        e->s_p2n = part2Node.storage().getWeakStorageImpl();
        e->v_ci = column_index._version(); e->v_pp = part_pointers._version(); e->v_p2n = part2Node._version();
        e->nnz = column_index.numel(); e->parts = part2Node.size(0); e->rows = rows; e->partSize = partSize; e->device = device;
        e->born = now;
        g_first_seen[g_first_seen_at] = now;
        g_first_seen_at = (g_first_seen_at + 1) % 8;
    }
    e->sightings++;
    e->stamp = now;
    if (e->sightings < (eager ? 2 : kSightings) || (!eager && e->nnz < kMinEdges)) return;
    for (int d : e->dims_done) if (d == dim) return;
    int others = 0;
    for (uint64_t born : g_first_seen)
        if (born != 0 && born != e->born && now - born < kQuietWindow) others++;
    if (!eager && others > kQuietOthers) return;   // the graphs keep changing (sampled training): nothing is pinned for them
    int phases = 0;
    const int rc = gnna_prepare_graph(static_cast<const int32_t *>(ci), part_pointers.data_ptr<int32_t>(),
                                      part2Node.data_ptr<int32_t>(), e->parts, rows, rows, partSize, &dim, 1, &phases, stream);
    if (rc == GNNA_ERR_UNSUPPORTED) return;        // inside a stream capture: try again at the next eager call
    e->dims_done.push_back(dim);                   // (a failed attempt -- no memory for the copy -- is not repeated per call)
    if (rc == GNNA_OK) g_auto_prepared.fetch_add(1);
}

// The module-level counterpart of gnna_forget_graph for callers that write into a graph's arrays behind torch's back
// (`column_index.data[k] = v`, a raw pointer, another library): forgets what this module remembers about every partition over
// this column_index and everything the library holds for it -- the next call sees the graph for the first time.
void forget_graph(const torch::Tensor &column_index)
{
    CHECK_CUDA(column_index);
    const void *ci = column_index.data_ptr();
    std::lock_guard<std::mutex> lock(g_seen_mutex);
    for (auto &g : g_seen)
        if (g.ci == ci) g = SeenGraph();
    (void)gnna_forget_graph(static_cast<const int32_t *>(ci));
}

// ---- shared by the wrappers below: one copy of the tensor checks, the output allocation and the call tail -------------
// A wrapper for a new operator goes next to the one it resembles and is made of these.  Where the CHECK_* macros would have
// stringified their argument, a helper is handed the name: the text is the same ("column_index must be a CUDA tensor").

// leading dimension of a [rows, dim] view with contiguous rows (a single row may carry any stride(0))
int64_t ld_of(const torch::Tensor &t) { return t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(t.size(1), t.stride(0)); }

// GNNA_DEBUG_POISON=1 (the test suite sets it): every fresh output starts as NaN, an int32 one as `int_fill`, so that an
// element the library fails to write cannot go unnoticed (NaN in every float type: the 16-bit outputs are covered as well)
bool poisoned()
{
    static const bool poison = std::getenv("GNNA_DEBUG_POISON") && std::atoi(std::getenv("GNNA_DEBUG_POISON")) != 0;
    return poison;
}
torch::Tensor fresh(at::IntArrayRef sizes, const at::TensorOptions &options, int32_t int_fill = std::numeric_limits<int32_t>::min())
{
    if (!poisoned()) return torch::empty(sizes, options);
    if (c10::typeMetaToScalarType(options.dtype()) == at::kInt) return torch::full(sizes, int_fill, options);
    return torch::full(sizes, std::numeric_limits<float>::quiet_NaN(), options);
}

void check_input(const torch::Tensor &t, const char *name)
{
    TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
void check_i32(const torch::Tensor &t, const char *name) { TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32 (got ", t.scalar_type(), ")"); }
void check_f32(const torch::Tensor &t, const char *name) { TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32 (got ", t.scalar_type(), ")"); }
void check_ids(const torch::Tensor &t, const char *name) { check_input(t, name); check_i32(t, name); }
void check_floats(const torch::Tensor &t, const char *name) { check_input(t, name); check_f32(t, name); }
void check_partition(const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node)
{
    check_ids(column_index, "column_index");
    check_ids(part_pointers, "part_pointers");
    check_ids(part2Node, "part2Node");
}
void check_rows(const torch::Tensor &t, const char *name)
{
    TORCH_CHECK(t.size(1) <= 1 || t.stride(1) == 1, name, ": the floats of a row must be contiguous (stride(1) == 1)");
}

// The caller's `out` ([n, dim], rows contiguous; float32, or whatever `check_dtype` accepts where one is given) or, without one, a
// fresh tensor -- which there is nothing to accumulate into.
torch::Tensor out_or_fresh(const c10::optional<torch::Tensor> &out_opt, int64_t n, int64_t dim, const at::TensorOptions &options,
                           bool accumulate, const std::function<void(const torch::Tensor &)> &check_dtype = nullptr)
{
    if (!out_opt.has_value()) {
        TORCH_CHECK(!accumulate, "accumulate needs an existing `out`");
        return fresh({n, dim}, options);
    }
    const torch::Tensor &out = *out_opt;
    CHECK_CUDA(out);
    if (check_dtype) check_dtype(out); else CHECK_F32(out);
    TORCH_CHECK(out.dim() == 2 && out.size(0) == n && out.size(1) == dim, "out must be [num_nodes, dim] like input");
    check_rows(out, "out");
    return out;
}

// PyTorch's current stream of the current device: call it under the device guard of the tensors
void *current_stream() { return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }
void check_rc(int64_t rc) { TORCH_CHECK(rc == GNNA_OK, "GNNAdvisor (libgnna) error ", rc, ": ", gnna_last_error()); }

// Runs one aggregation of `input` ([N, dim]) into a fresh tensor on input's device/stream.
torch::Tensor aggregate(AggKind kind, const torch::Tensor &input, const torch::Tensor &row_pointers,
                        const torch::Tensor &column_index, const torch::Tensor *degrees, float epsilon,
                        const torch::Tensor &part_pointers, const torch::Tensor &part2Node,
                        int partSize, int dimWorker, int warpPerBlock)
{
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    CHECK_I32(row_pointers);
    CHECK_I32(column_index);
    CHECK_I32(part_pointers);
    CHECK_I32(part2Node);
    if (degrees) CHECK_F32((*degrees));
    const int64_t num_parts = part2Node.size(0);
    TORCH_CHECK(part_pointers.size(0) == num_parts + 1 || (num_parts == 0 && part_pointers.size(0) >= 0),
                "part_pointers must have part2Node.size(0) + 1 entries");
    if (kind == AGG_GCN) TORCH_CHECK(degrees->size(0) >= input.size(0), "degrees shorter than num_nodes");

    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    // fully overwritten by the library (prologue + stores / atomics)
    auto out = poisoned() ? torch::full_like(input, std::numeric_limits<float>::quiet_NaN()) : torch::empty_like(input);
    void *stream = current_stream();

    const float *x = input.data_ptr<float>();
    const int32_t *rp = row_pointers.data_ptr<int32_t>();
    const int32_t *ci = column_index.data_ptr<int32_t>();
    const int32_t *pp = part_pointers.data_ptr<int32_t>();
    const int32_t *p2n = part2Node.data_ptr<int32_t>();
    float *y = out.data_ptr<float>();
    const int64_t n = input.size(0);
    const int dim = (int)input.size(1);
    note_graph(column_index, part_pointers, part2Node, n, partSize, dim, stream);

    int rc = GNNA_OK;
    switch (kind) {
    case AGG_SAG:
        rc = gnna_sag_f32(x, rp, ci, degrees ? degrees->data_ptr<float>() : nullptr, pp, p2n, y, n, dim,
                          num_parts, partSize, dimWorker, warpPerBlock, stream);
        break;
    case AGG_GCN:
        rc = gnna_agg_gcn_f32(x, rp, ci, degrees->data_ptr<float>(), pp, p2n, y, n, dim, num_parts,
                              partSize, dimWorker, warpPerBlock, stream);
        break;
    case AGG_GIN:
        rc = gnna_agg_gin_f32(x, rp, ci, epsilon, pp, p2n, y, n, dim, num_parts, partSize, dimWorker,
                              warpPerBlock, stream);
        break;
    }
    check_rc(rc);
    return out;
}

// The general entry (gnna_agg_ld_f32): `input` and `out` may be row-strided views (stride(1) == 1; stride(0) is the leading
// dimension), the result can be added to `out` and clamped at zero in the same call.
torch::Tensor aggregate_general(int mode, const torch::Tensor &input, const torch::Tensor &column_index,
                                const c10::optional<torch::Tensor> &degrees, double epsilon,
                                const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
                                c10::optional<torch::Tensor> out_opt, bool accumulate, bool relu, pybind11::object out_dtype_obj)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    const bool x16 = input.scalar_type() == at::kBFloat16 || input.scalar_type() == at::kHalf;
    TORCH_CHECK(x16 || input.scalar_type() == at::kFloat, "input must be float32, bfloat16 or float16 (got ", input.scalar_type(), ")");
    // out_dtype (bf16 / fp16 input only): float32 or the input's dtype; default: the input's dtype
    at::ScalarType out_dtype = input.scalar_type();
    if (!out_dtype_obj.is_none()) {
        TORCH_CHECK(THPDtype_Check(out_dtype_obj.ptr()), "out_dtype must be a torch.dtype");
        out_dtype = reinterpret_cast<THPDtype *>(out_dtype_obj.ptr())->scalar_type;
        TORCH_CHECK(out_dtype == input.scalar_type() || (x16 && out_dtype == at::kFloat),
                    "out_dtype must be float32 or the input's dtype ", input.scalar_type(), " (got ", out_dtype, ")");
    }
    check_partition(column_index, part_pointers, part2Node);
    TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0 (sag), 1 (gcn) or 2 (gin)");
    check_rows(input, "input");
    const int64_t n = input.size(0), dim = input.size(1);
    if (mode == 1) {
        TORCH_CHECK(degrees.has_value(), "mode 1 (gcn) needs the degree norms");
        check_floats(*degrees, "(*degrees)");
        TORCH_CHECK(degrees->size(0) >= n, "degrees shorter than num_nodes");
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = out_or_fresh(out_opt, n, dim, input.options().dtype(out_dtype), accumulate, [&](const torch::Tensor &out) {
        if (!x16) {
            CHECK_F32(out);
            return;
        }
        TORCH_CHECK(out.scalar_type() == at::kFloat || out.scalar_type() == input.scalar_type(),
                    "out must be float32 or have the input's dtype ", input.scalar_type(), " (got ", out.scalar_type(), ")");
        TORCH_CHECK(out_dtype_obj.is_none() || out.scalar_type() == out_dtype, "out is ", out.scalar_type(), ", out_dtype says ", out_dtype);
    });
    void *stream = current_stream();
    const float *deg = degrees.has_value() ? degrees->data_ptr<float>() : nullptr;
    const unsigned flags = (accumulate ? GNNA_ACCUMULATE : 0u) | (relu ? GNNA_EPILOGUE_RELU : 0u);
    if (x16) {
        // features stored in 16 bits, accumulated in fp32 (gnna_agg_ld_x16); the degrees stay fp32
        const int in_type = input.scalar_type() == at::kBFloat16 ? GNNA_BF16 : GNNA_F16;
        const int out_type = out.scalar_type() == at::kFloat ? GNNA_F32 : in_type;
        check_rc(gnna_agg_ld_x16(mode, in_type, input.data_ptr(), ld_of(input), n, column_index.data_ptr<int32_t>(), deg, deg,
                                 (float)epsilon, part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(),
                                 out.data_ptr(), out_type, ld_of(out), n, (int)dim, part2Node.size(0), partSize, flags, stream));
        return out;
    }
    check_rc(gnna_agg_ld_f32(mode, input.data_ptr<float>(), ld_of(input), n, column_index.data_ptr<int32_t>(), deg, deg,
                             (float)epsilon, part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(),
                             out.data_ptr<float>(), ld_of(out), n, (int)dim, part2Node.size(0), partSize, flags, stream));
    return out;
}

// Edge-weighted aggregation (gnna_agg_edge_ld_f32): out[i] (+)= sum_e w[e] X[column_index[e]], strided X / out as aggregate_ld.
torch::Tensor aggregate_edge(const torch::Tensor &input, const torch::Tensor &column_index, const torch::Tensor &edge_weight,
                             const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
                             c10::optional<torch::Tensor> out_opt, bool accumulate, bool relu)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    check_ids(column_index, "column_index");
    check_floats(edge_weight, "edge_weight");
    check_ids(part_pointers, "part_pointers");
    check_ids(part2Node, "part2Node");
    TORCH_CHECK(edge_weight.dim() == 1 && edge_weight.size(0) == column_index.numel(),
                "edge_weight must be [nnz], indexed like column_index");
    TORCH_CHECK(edge_weight.device() == input.device() && column_index.device() == input.device(),
                "input, column_index and edge_weight must be on one device");
    check_rows(input, "input");
    const int64_t n = input.size(0), dim = input.size(1);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = out_or_fresh(out_opt, n, dim, input.options(), accumulate);
    const unsigned flags = (accumulate ? GNNA_ACCUMULATE : 0u) | (relu ? GNNA_EPILOGUE_RELU : 0u);
    check_rc(gnna_agg_edge_ld_f32(input.data_ptr<float>(), ld_of(input), n, column_index.data_ptr<int32_t>(),
                                  edge_weight.data_ptr<float>(), part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(),
                                  out.data_ptr<float>(), ld_of(out), n, (int)dim, part2Node.size(0), partSize, flags, current_stream()));
    return out;
}

// Element-wise max / min over every row's neighbours (gnna_agg_reduce_ld_f32) -> (out, arg); strided X / out as aggregate_ld.
// arg [num_nodes, dim] int32: the position in column_index that supplied each element (-1: the row has no edge); an undefined
// tensor (None in Python) with want_arg = false.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>>
aggregate_reduce(int op, const torch::Tensor &input, const torch::Tensor &column_index, const torch::Tensor &part_pointers,
                 const torch::Tensor &part2Node, int partSize, c10::optional<torch::Tensor> out_opt, bool want_arg, bool relu)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    check_partition(column_index, part_pointers, part2Node);
    TORCH_CHECK(op == GNNA_REDUCE_MAX || op == GNNA_REDUCE_MIN, "op must be 0 (max) or 1 (min)");
    TORCH_CHECK(column_index.device() == input.device(), "input and column_index must be on one device");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    check_rows(input, "input");
    const int64_t n = input.size(0), dim = input.size(1);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = out_or_fresh(out_opt, n, dim, input.options(), /*accumulate=*/false);
    c10::optional<torch::Tensor> arg;
    if (want_arg) arg = fresh({n, dim}, input.options().dtype(at::kInt));
    check_rc(gnna_agg_reduce_ld_f32(op, input.data_ptr<float>(), ld_of(input), n, column_index.data_ptr<int32_t>(),
                                    part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), out.data_ptr<float>(),
                                    ld_of(out), arg.has_value() ? arg->data_ptr<int32_t>() : nullptr, dim, n, (int)dim,
                                    part2Node.size(0), partSize, relu ? GNNA_EPILOGUE_RELU : 0u, current_stream()));
    return std::make_tuple(out, arg);
}

// Sum, sum of squares, max and min over every row's neighbours from one gather (gnna_agg_stats_ld_f32) -> (sum, sumsq, max, argmax,
// min, argmin), each [num_out_rows, dim]; None for a statistic that was not asked for (argmax / argmin come with max / min).
// Strided X as aggregate_ld; num_out_rows < 0: as many rows as X has.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
aggregate_stats(const torch::Tensor &input, const torch::Tensor &column_index, const torch::Tensor &part_pointers,
                const torch::Tensor &part2Node, int partSize, int64_t num_out_rows, bool want_sum, bool want_sumsq, bool want_max,
                bool want_min)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    check_partition(column_index, part_pointers, part2Node);
    TORCH_CHECK(want_sum || want_sumsq || want_max || want_min, "no statistic asked for");
    TORCH_CHECK(column_index.device() == input.device(), "input and column_index must be on one device");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    check_rows(input, "input");
    const int64_t n_in = input.size(0), dim = input.size(1), n = num_out_rows < 0 ? n_in : num_out_rows;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    c10::optional<torch::Tensor> sum, sumsq, mx, amx, mn, amn;
    if (want_sum) sum = fresh({n, dim}, input.options());
    if (want_sumsq) sumsq = fresh({n, dim}, input.options());
    if (want_max) { mx = fresh({n, dim}, input.options()); amx = fresh({n, dim}, input.options().dtype(at::kInt)); }
    if (want_min) { mn = fresh({n, dim}, input.options()); amn = fresh({n, dim}, input.options().dtype(at::kInt)); }
    auto fp = [](const c10::optional<torch::Tensor> &t) { return t.has_value() ? t->data_ptr<float>() : nullptr; };
    auto ip = [](const c10::optional<torch::Tensor> &t) { return t.has_value() ? t->data_ptr<int32_t>() : nullptr; };
    check_rc(gnna_agg_stats_ld_f32(input.data_ptr<float>(), ld_of(input), n_in, column_index.data_ptr<int32_t>(),
                                   part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), fp(sum), dim, fp(sumsq), dim,
                                   fp(mx), dim, ip(amx), dim, fp(mn), dim, ip(amn), dim, n, (int)dim, part2Node.size(0), partSize, 0u,
                                   current_stream()));
    return std::make_tuple(sum, sumsq, mx, amx, mn, amn);
}

// Softmax aggregation with a temperature, per channel, in one gather (gnna_agg_softmax_ld_f32) -> (out, lse, sq), each
// [num_out_rows, dim] with num_out_rows = row_pointers.size(0) - 1; sq is None unless want_sq.  temp: 1 or dim floats on the
// device.  Strided X as aggregate_ld.
static const int32_t *softagg_ids(const torch::Tensor &column_index, const torch::Tensor &row_pointers)
{
    // (a graph without edges has no column_index address: row_pointers' stands for it, no id is ever read)
    return column_index.numel() > 0 ? column_index.data_ptr<int32_t>() : row_pointers.data_ptr<int32_t>();
}
static void softagg_check(const torch::Tensor &input, const torch::Tensor &temp, const torch::Tensor &row_pointers,
                          const torch::Tensor &column_index)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    check_floats(temp, "temp");
    check_ids(row_pointers, "row_pointers");
    check_ids(column_index, "column_index");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    TORCH_CHECK(temp.numel() == 1 || temp.numel() == input.size(1), "temp must have 1 or dim = ", input.size(1), " elements (got ",
                temp.numel(), ")");
    TORCH_CHECK(row_pointers.dim() == 1 && row_pointers.size(0) >= 1, "row_pointers must be [rows + 1]");
    TORCH_CHECK(temp.device() == input.device() && row_pointers.device() == input.device() && column_index.device() == input.device(),
                "input, temp, row_pointers and column_index must be on one device");
    check_rows(input, "input");
}
std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>>
aggregate_softmax(const torch::Tensor &input, const torch::Tensor &temp, const torch::Tensor &row_pointers,
                  const torch::Tensor &column_index, bool want_sq)
{
    softagg_check(input, temp, row_pointers, column_index);
    const int64_t n_in = input.size(0), dim = input.size(1), n = row_pointers.size(0) - 1;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = fresh({n, dim}, input.options()), lse = fresh({n, dim}, input.options());
    c10::optional<torch::Tensor> sq;
    if (want_sq) sq = fresh({n, dim}, input.options());
    check_rc(gnna_agg_softmax_ld_f32(input.data_ptr<float>(), ld_of(input), n_in, temp.data_ptr<float>(), (int)temp.numel(),
                                     row_pointers.data_ptr<int32_t>(), softagg_ids(column_index, row_pointers), out.data_ptr<float>(), dim,
                                     lse.data_ptr<float>(), dim, sq.has_value() ? sq->data_ptr<float>() : nullptr, dim, n, (int)dim, 0u,
                                     current_stream()));
    return std::make_tuple(out, lse, sq);
}

// Backward of aggregate_softmax (gnna_agg_softmax_backward_ld_f32) -> d_input like input.  (t_row_pointers, t_column_index): A^T,
// input.size(0) rows whose ids are destination rows.  Strided input, lse, Y and dY as aggregate_ld.
torch::Tensor aggregate_softmax_backward(const torch::Tensor &input, const torch::Tensor &temp, const torch::Tensor &lse,
                                         const torch::Tensor &Y, const torch::Tensor &dY, const torch::Tensor &t_row_pointers,
                                         const torch::Tensor &t_column_index)
{
    softagg_check(input, temp, t_row_pointers, t_column_index);
    const int64_t n_in = input.size(0), dim = input.size(1);
    TORCH_CHECK(t_row_pointers.size(0) == n_in + 1, "t_row_pointers must be [num_in_rows + 1] (the transposed structure has input's rows)");
    const int64_t n = lse.dim() == 2 ? lse.size(0) : -1;
    for (const torch::Tensor *t : {&lse, &Y, &dY}) {
        CHECK_CUDA((*t));
        CHECK_F32((*t));
        TORCH_CHECK(t->dim() == 2 && t->size(0) == n && t->size(1) == dim && t->device() == input.device(),
                    "lse, Y and dY must be [num_out_rows, dim] on input's device");
        check_rows(*t, "lse / Y / dY");
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = fresh({n_in, dim}, input.options());
    check_rc(gnna_agg_softmax_backward_ld_f32(input.data_ptr<float>(), ld_of(input), n_in, temp.data_ptr<float>(), (int)temp.numel(),
                                              lse.data_ptr<float>(), ld_of(lse), Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(),
                                              ld_of(dY), t_row_pointers.data_ptr<int32_t>(), softagg_ids(t_column_index, t_row_pointers),
                                              out.data_ptr<float>(), dim, n, (int)dim, 0u, current_stream()));
    return out;
}

// Message passing with a feature row per edge (gnna_agg_edge_feat_ld_f32, include/gnna_edgefeat.h) -> out [num_out_rows, dim] with
// num_out_rows = row_pointers.size(0) - 1: the sum over a row's positions e of act(X[column_index[e]] (+ | *) E[e]).  E: [nnz, dim],
// edge-major.  Strided X and E as aggregate_ld.
static void edgefeat_check(const torch::Tensor &input, const torch::Tensor &edge_feat, const torch::Tensor &row_pointers,
                           const torch::Tensor &column_index)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    CHECK_CUDA(edge_feat);
    CHECK_F32(edge_feat);
    check_ids(row_pointers, "row_pointers");
    check_ids(column_index, "column_index");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    TORCH_CHECK(edge_feat.dim() == 2 && edge_feat.size(0) == column_index.numel() && edge_feat.size(1) == input.size(1),
                "edge_feat must be [nnz = ", column_index.numel(), ", dim = ", input.size(1), "] in the order of column_index");
    TORCH_CHECK(row_pointers.dim() == 1 && row_pointers.size(0) >= 1, "row_pointers must be [rows + 1]");
    TORCH_CHECK(edge_feat.device() == input.device() && row_pointers.device() == input.device() &&
                column_index.device() == input.device(), "input, edge_feat, row_pointers and column_index must be on one device");
    check_rows(input, "input");
    if (edge_feat.size(0) > 0) check_rows(edge_feat, "edge_feat");       // (no row: nothing is strided by whatever an empty tensor carries)
}
torch::Tensor aggregate_edge_feat(const torch::Tensor &input, const torch::Tensor &edge_feat, const torch::Tensor &row_pointers,
                                  const torch::Tensor &column_index, int combine, int act)
{
    edgefeat_check(input, edge_feat, row_pointers, column_index);
    const int64_t n_in = input.size(0), dim = input.size(1), n = row_pointers.size(0) - 1, nnz = column_index.numel();
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = fresh({n, dim}, input.options());
    check_rc(gnna_agg_edge_feat_ld_f32(input.data_ptr<float>(), ld_of(input), n_in, edge_feat.data_ptr<float>(), ld_of(edge_feat), nnz,
                                       row_pointers.data_ptr<int32_t>(), softagg_ids(column_index, row_pointers), out.data_ptr<float>(), dim,
                                       n, (int)dim, combine, act, 0u, current_stream()));
    return out;
}

// Backward of aggregate_edge_feat (gnna_agg_edge_feat_backward_ld_f32) -> (d_input | None, d_edge | None).  The transposed structure
// and t_edge_pos (transpose_csr's perm, or the reverse-edge map of a symmetric structure) are needed only with want_dx.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
aggregate_edge_feat_backward(const torch::Tensor &input, const torch::Tensor &edge_feat, const torch::Tensor &dY,
                             const torch::Tensor &row_pointers, const torch::Tensor &column_index,
                             const c10::optional<torch::Tensor> &t_row_pointers, const c10::optional<torch::Tensor> &t_column_index,
                             const c10::optional<torch::Tensor> &t_edge_pos, int combine, int act, bool want_dx, bool want_de)
{
    edgefeat_check(input, edge_feat, row_pointers, column_index);
    const int64_t n_in = input.size(0), dim = input.size(1), n = row_pointers.size(0) - 1, nnz = column_index.numel();
    CHECK_CUDA(dY);
    CHECK_F32(dY);
    TORCH_CHECK(dY.dim() == 2 && dY.size(0) == n && dY.size(1) == dim && dY.device() == input.device(),
                "dY must be [num_out_rows, dim] on input's device");
    check_rows(dY, "dY");
    const int32_t *trp = nullptr, *tci = nullptr, *tpos = nullptr;
    if (want_dx) {
        TORCH_CHECK(t_row_pointers.has_value() && t_column_index.has_value() && t_edge_pos.has_value(),
                    "want_dx needs t_row_pointers, t_column_index and t_edge_pos");
        check_ids(*t_row_pointers, "t_row_pointers");
        check_ids(*t_column_index, "t_column_index");
        check_ids(*t_edge_pos, "t_edge_pos");
        TORCH_CHECK(t_row_pointers->numel() == n_in + 1 && t_column_index->numel() == nnz && t_edge_pos->numel() == nnz,
                    "t_row_pointers must be [num_in_rows + 1], t_column_index and t_edge_pos [nnz]");
        TORCH_CHECK(t_row_pointers->device() == input.device() && t_column_index->device() == input.device() &&
                    t_edge_pos->device() == input.device(), "the transposed structure must be on input's device");
        trp = t_row_pointers->data_ptr<int32_t>();
        tci = softagg_ids(*t_column_index, *t_row_pointers);
        tpos = softagg_ids(*t_edge_pos, *t_row_pointers);
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    c10::optional<torch::Tensor> dX, dE;
    if (want_dx) dX = fresh({n_in, dim}, input.options());
    if (want_de) dE = fresh({nnz, dim}, input.options());
    check_rc(gnna_agg_edge_feat_backward_ld_f32(input.data_ptr<float>(), ld_of(input), n_in, edge_feat.data_ptr<float>(), ld_of(edge_feat),
                                                nnz, dY.data_ptr<float>(), ld_of(dY), row_pointers.data_ptr<int32_t>(),
                                                softagg_ids(column_index, row_pointers), trp, tci, tpos,
                                                dX.has_value() ? dX->data_ptr<float>() : nullptr, dim,
                                                dE.has_value() ? dE->data_ptr<float>() : nullptr, dim, n, (int)dim, combine, act, 0u,
                                                current_stream()));
    return std::make_tuple(dX, dE);
}

// Graph-level readout (gnna_segment_pool_ld_f32) -> (sum, max, argmax, min, argmin), each [num_graphs, dim] with num_graphs =
// graph_pointers.size(0) - 1; None for a statistic that was not asked for (argmax / argmin, the winning rows, come with max / min).
// mean: the sum divided by the rows of the graph.  Strided input as aggregate_ld.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>>
segment_pool(const torch::Tensor &input, const torch::Tensor &graph_pointers, bool want_sum, bool want_max, bool want_min, bool mean)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    check_ids(graph_pointers, "graph_pointers");
    TORCH_CHECK(want_sum || want_max || want_min, "no statistic asked for");
    TORCH_CHECK(graph_pointers.dim() == 1 && graph_pointers.size(0) >= 1, "graph_pointers must be [num_graphs + 1]");
    TORCH_CHECK(graph_pointers.device() == input.device(), "input and graph_pointers must be on one device");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    check_rows(input, "input");
    const int64_t n = input.size(0), dim = input.size(1), g = graph_pointers.size(0) - 1;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    c10::optional<torch::Tensor> sum, mx, amx, mn, amn;
    if (want_sum) sum = fresh({g, dim}, input.options());
    if (want_max) { mx = fresh({g, dim}, input.options()); amx = fresh({g, dim}, input.options().dtype(at::kInt)); }
    if (want_min) { mn = fresh({g, dim}, input.options()); amn = fresh({g, dim}, input.options().dtype(at::kInt)); }
    auto fp = [](const c10::optional<torch::Tensor> &t) { return t.has_value() ? t->data_ptr<float>() : nullptr; };
    auto ip = [](const c10::optional<torch::Tensor> &t) { return t.has_value() ? t->data_ptr<int32_t>() : nullptr; };
    if (g == 0) return std::make_tuple(sum, mx, amx, mn, amn);     // (empty outputs have no address)
    check_rc(gnna_segment_pool_ld_f32(n > 0 ? input.data_ptr<float>() : nullptr, ld_of(input), n, graph_pointers.data_ptr<int32_t>(), g,
                                      fp(sum), dim, fp(mx), dim, ip(amx), dim, fp(mn), dim, ip(amn), dim, (int)dim,
                                      mean ? GNNA_POOL_MEAN : 0u, current_stream()));
    return std::make_tuple(sum, mx, amx, mn, amn);
}

// Backward of segment_pool (gnna_segment_pool_backward_ld_f32) -> d_input [num_rows, dim]: every row gets the gradient of its
// graph's sum (divided by the graph's rows with mean) plus those of the max / min it won; a row of no graph gets 0.  Any of d_sum,
// (d_max, argmax), (d_min, argmin) may be None, not all.
torch::Tensor segment_pool_backward(const c10::optional<torch::Tensor> &d_sum, const c10::optional<torch::Tensor> &d_max,
                                    const c10::optional<torch::Tensor> &argmax, const c10::optional<torch::Tensor> &d_min,
                                    const c10::optional<torch::Tensor> &argmin, const torch::Tensor &graph_pointers, int64_t num_rows,
                                    bool mean)
{
    check_ids(graph_pointers, "graph_pointers");
    TORCH_CHECK(graph_pointers.dim() == 1 && graph_pointers.size(0) >= 1, "graph_pointers must be [num_graphs + 1]");
    TORCH_CHECK(d_sum.has_value() || d_max.has_value() || d_min.has_value(), "no gradient given");
    TORCH_CHECK(d_max.has_value() == argmax.has_value() && d_min.has_value() == argmin.has_value(), "d_max comes with argmax, d_min with argmin");
    TORCH_CHECK(num_rows >= 0, "num_rows must not be negative");
    const int64_t g = graph_pointers.size(0) - 1;
    const torch::Tensor &first = d_sum.has_value() ? *d_sum : d_max.has_value() ? *d_max : *d_min;
    TORCH_CHECK(first.dim() == 2 && first.size(1) >= 1, "the gradients must be 2-D [num_graphs, dim]");
    const int64_t dim = first.size(1);
    for (const c10::optional<torch::Tensor> *t : {&d_sum, &d_max, &d_min}) {
        if (!t->has_value()) continue;
        CHECK_CUDA((**t));
        CHECK_F32((**t));
        TORCH_CHECK((*t)->dim() == 2 && (*t)->size(0) == g && (*t)->size(1) == dim && (*t)->device() == graph_pointers.device(),
                    "d_sum, d_max and d_min must be [num_graphs, dim] on graph_pointers' device");
        check_rows(**t, "d_sum / d_max / d_min");
    }
    for (const c10::optional<torch::Tensor> *t : {&argmax, &argmin}) {
        if (!t->has_value()) continue;
        CHECK_CUDA((**t));
        CHECK_I32((**t));
        TORCH_CHECK((*t)->dim() == 2 && (*t)->size(0) == g && (*t)->size(1) == dim && (*t)->device() == graph_pointers.device(),
                    "argmax and argmin must be int32 [num_graphs, dim] on graph_pointers' device");
        check_rows(**t, "argmax / argmin");
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(first.device());
    const torch::Tensor out = fresh({num_rows, dim}, first.options());
    auto fp = [](const c10::optional<torch::Tensor> &t) { return t.has_value() ? t->data_ptr<float>() : nullptr; };
    auto ip = [](const c10::optional<torch::Tensor> &t) { return t.has_value() ? t->data_ptr<int32_t>() : nullptr; };
    auto ld = [&](const c10::optional<torch::Tensor> &t) { return t.has_value() ? ld_of(*t) : dim; };
    check_rc(gnna_segment_pool_backward_ld_f32(fp(d_sum), ld(d_sum), fp(d_max), ld(d_max), ip(argmax), ld(argmax), fp(d_min), ld(d_min),
                                               ip(argmin), ld(argmin), graph_pointers.data_ptr<int32_t>(), g,
                                               num_rows > 0 ? out.data_ptr<float>() : nullptr, dim, num_rows, (int)dim,
                                               mean ? GNNA_POOL_MEAN : 0u, current_stream()));
    return out;
}

// Attention readout (gnna_segment_attn_pool_ld_f32) -> (out [num_graphs, dim], lse [num_graphs, gate_dim]) with num_graphs =
// graph_pointers.size(0) - 1: the softmax-weighted sum of the rows of every graph.  gate: [num_rows, 1] (a score per row) or
// [num_rows, dim] (a score per element); it may be input itself.  Strided input and gate as aggregate_ld.
static void attn_pool_check(const torch::Tensor &input, const torch::Tensor &gate, const torch::Tensor &graph_pointers)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    CHECK_CUDA(gate);
    CHECK_F32(gate);
    check_ids(graph_pointers, "graph_pointers");
    TORCH_CHECK(graph_pointers.dim() == 1 && graph_pointers.size(0) >= 1, "graph_pointers must be [num_graphs + 1]");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    TORCH_CHECK(gate.dim() == 2 && gate.size(0) == input.size(0) && (gate.size(1) == 1 || gate.size(1) == input.size(1)),
                "gate must be [num_nodes, 1] or [num_nodes, dim = ", input.size(1), "]");
    TORCH_CHECK(graph_pointers.device() == input.device() && gate.device() == input.device(),
                "input, gate and graph_pointers must be on one device");
    check_rows(input, "input");
    check_rows(gate, "gate");
}
std::tuple<torch::Tensor, torch::Tensor> segment_attn_pool(const torch::Tensor &input, const torch::Tensor &gate,
                                                           const torch::Tensor &graph_pointers)
{
    attn_pool_check(input, gate, graph_pointers);
    const int64_t n = input.size(0), dim = input.size(1), gd = gate.size(1), g = graph_pointers.size(0) - 1;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = fresh({g, dim}, input.options()), lse = fresh({g, gd}, input.options());
    if (g == 0) return std::make_tuple(out, lse);                  // (empty outputs have no address)
    check_rc(gnna_segment_attn_pool_ld_f32(n > 0 ? input.data_ptr<float>() : nullptr, ld_of(input), n,
                                           n > 0 ? gate.data_ptr<float>() : nullptr, ld_of(gate), (int)gd,
                                           graph_pointers.data_ptr<int32_t>(), g, out.data_ptr<float>(), dim, lse.data_ptr<float>(), gd,
                                           (int)dim, 0u, current_stream()));
    return std::make_tuple(out, lse);
}

// Backward of segment_attn_pool (gnna_segment_attn_pool_backward_ld_f32) -> (d_input like input, d_gate like gate), None for the
// one that is not needed: with alpha = exp(gate - lse), d_input = alpha dY and d_gate = alpha dY (input - Y), summed over the
// columns for a score per row; a row of no graph gets 0.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
segment_attn_pool_backward(const torch::Tensor &input, const torch::Tensor &gate, const torch::Tensor &lse, const torch::Tensor &Y,
                           const torch::Tensor &dY, const torch::Tensor &graph_pointers, bool need_input, bool need_gate)
{
    attn_pool_check(input, gate, graph_pointers);
    TORCH_CHECK(need_input || need_gate, "neither d_input nor d_gate asked for");
    const int64_t n = input.size(0), dim = input.size(1), gd = gate.size(1), g = graph_pointers.size(0) - 1;
    for (const torch::Tensor *t : {&lse, &Y, &dY}) {
        CHECK_CUDA((*t));
        CHECK_F32((*t));
        TORCH_CHECK(t->dim() == 2 && t->size(0) == g && t->size(1) == (t == &lse ? gd : dim) && t->device() == input.device(),
                    "lse must be [num_graphs, gate_dim], Y and dY [num_graphs, dim], on input's device");
        check_rows(*t, "lse / Y / dY");
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    c10::optional<torch::Tensor> d_input, d_gate;
    if (need_input) d_input = fresh({n, dim}, input.options());
    if (need_gate) d_gate = fresh({n, gd}, input.options());
    if (n == 0) return std::make_tuple(d_input, d_gate);
    auto fp = [&](const torch::Tensor &t) { return g > 0 ? t.data_ptr<float>() : nullptr; };     // (empty tensors have no address)
    check_rc(gnna_segment_attn_pool_backward_ld_f32(input.data_ptr<float>(), ld_of(input), gate.data_ptr<float>(), ld_of(gate), (int)gd,
                                                    fp(lse), ld_of(lse), fp(Y), ld_of(Y), fp(dY), ld_of(dY),
                                                    graph_pointers.data_ptr<int32_t>(), g,
                                                    d_input.has_value() ? d_input->data_ptr<float>() : nullptr, dim,
                                                    d_gate.has_value() ? d_gate->data_ptr<float>() : nullptr, gd, n, (int)dim, 0u,
                                                    current_stream()));
    return std::make_tuple(d_input, d_gate);
}

// Per-graph normalisation (gnna_segnorm.h).  What the three functions check alike: input [num_rows, dim] float32 with contiguous
// rows, graph_pointers int32 [num_graphs + 1] on its device.
static void segnorm_check(const torch::Tensor &input, const torch::Tensor &graph_pointers)
{
    CHECK_CUDA(input);
    TORCH_CHECK(input.dim() == 2, "input must be 2-D [num_nodes, dim]");
    CHECK_F32(input);
    check_ids(graph_pointers, "graph_pointers");
    TORCH_CHECK(graph_pointers.dim() == 1 && graph_pointers.size(0) >= 1, "graph_pointers must be [num_graphs + 1]");
    TORCH_CHECK(graph_pointers.device() == input.device(), "input and graph_pointers must be on one device");
    TORCH_CHECK(input.size(1) >= 1, "input must have at least one column");
    check_rows(input, "input");
}
// the address of a per-column parameter [dim] on input's device; null for None (the default)
static const float *segnorm_param(const c10::optional<torch::Tensor> &t, const torch::Tensor &input, const char *name)
{
    if (!t.has_value()) return nullptr;
    check_floats(*t, name);
    TORCH_CHECK(t->dim() == 1 && t->size(0) == input.size(1) && t->device() == input.device(), name, " must be [dim = ", input.size(1),
                "] on input's device");
    return t->data_ptr<float>();
}

// Centred moments of the rows of every graph (gnna_segment_moments_ld_f32) -> (mean, m2), each [num_graphs, dim].
std::tuple<torch::Tensor, torch::Tensor> segment_moments(const torch::Tensor &input, const torch::Tensor &graph_pointers)
{
    segnorm_check(input, graph_pointers);
    const int64_t n = input.size(0), dim = input.size(1), g = graph_pointers.size(0) - 1;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor mean = fresh({g, dim}, input.options()), m2 = fresh({g, dim}, input.options());
    if (g == 0) return std::make_tuple(mean, m2);                  // (empty outputs have no address)
    check_rc(gnna_segment_moments_ld_f32(n > 0 ? input.data_ptr<float>() : nullptr, ld_of(input), n, graph_pointers.data_ptr<int32_t>(), g,
                                         mean.data_ptr<float>(), dim, m2.data_ptr<float>(), dim, (int)dim, 0u, current_stream()));
    return std::make_tuple(mean, m2);
}

// GraphNorm forward (gnna_segment_norm_ld_f32) -> (out like input, mean, rstd [num_graphs, dim]); weight / bias / alpha: [dim] or
// None for 1 / 0 / 1.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
segment_norm(const torch::Tensor &input, const torch::Tensor &graph_pointers, const c10::optional<torch::Tensor> &weight,
             const c10::optional<torch::Tensor> &bias, const c10::optional<torch::Tensor> &alpha, double eps)
{
    segnorm_check(input, graph_pointers);
    const int64_t n = input.size(0), dim = input.size(1), g = graph_pointers.size(0) - 1;
    const float *wp = segnorm_param(weight, input, "weight"), *bp = segnorm_param(bias, input, "bias"),
                *ap = segnorm_param(alpha, input, "alpha");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = fresh({n, dim}, input.options()), mean = fresh({g, dim}, input.options()),
                        rstd = fresh({g, dim}, input.options());
    if (n == 0 && g == 0) return std::make_tuple(out, mean, rstd);
    check_rc(gnna_segment_norm_ld_f32(n > 0 ? input.data_ptr<float>() : nullptr, ld_of(input), n, graph_pointers.data_ptr<int32_t>(), g,
                                      wp, bp, ap, (float)eps, n > 0 ? out.data_ptr<float>() : nullptr, dim,
                                      g > 0 ? mean.data_ptr<float>() : nullptr, dim, g > 0 ? rstd.data_ptr<float>() : nullptr, dim,
                                      (int)dim, 0u, current_stream()));
    return std::make_tuple(out, mean, rstd);
}

// GraphNorm backward (gnna_segment_norm_backward_ld_f32) -> (d_input like input | None, seg_a, seg_b [num_graphs, dim]).
std::tuple<c10::optional<torch::Tensor>, torch::Tensor, torch::Tensor>
segment_norm_backward(const torch::Tensor &dY, const torch::Tensor &input, const torch::Tensor &mean, const torch::Tensor &rstd,
                      const torch::Tensor &graph_pointers, const c10::optional<torch::Tensor> &weight,
                      const c10::optional<torch::Tensor> &alpha, bool need_input)
{
    segnorm_check(input, graph_pointers);
    const int64_t n = input.size(0), dim = input.size(1), g = graph_pointers.size(0) - 1;
    for (const torch::Tensor *t : {&dY, &mean, &rstd}) {
        CHECK_CUDA((*t));
        CHECK_F32((*t));
        TORCH_CHECK(t->dim() == 2 && t->size(0) == (t == &dY ? n : g) && t->size(1) == dim && t->device() == input.device(),
                    "dY must be [num_nodes, dim], mean and rstd [num_graphs, dim], on input's device");
        check_rows(*t, "dY / mean / rstd");
    }
    const float *wp = segnorm_param(weight, input, "weight"), *ap = segnorm_param(alpha, input, "alpha");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    c10::optional<torch::Tensor> d_input;
    if (need_input) d_input = fresh({n, dim}, input.options());
    const torch::Tensor seg_a = fresh({g, dim}, input.options()), seg_b = fresh({g, dim}, input.options());
    if (g == 0 && (n == 0 || !need_input)) return std::make_tuple(d_input, seg_a, seg_b);
    auto gptr = [&](const torch::Tensor &t) { return g > 0 ? t.data_ptr<float>() : nullptr; };      // (empty tensors have no address)
    check_rc(gnna_segment_norm_backward_ld_f32(n > 0 ? dY.data_ptr<float>() : nullptr, ld_of(dY), n > 0 ? input.data_ptr<float>() : nullptr,
                                               ld_of(input), gptr(mean), ld_of(mean), gptr(rstd), ld_of(rstd), wp, ap,
                                               graph_pointers.data_ptr<int32_t>(), g,
                                               d_input.has_value() && n > 0 ? d_input->data_ptr<float>() : nullptr, dim, gptr(seg_a), dim,
                                               gptr(seg_b), dim, n, (int)dim, 0u, current_stream()));
    return std::make_tuple(d_input, seg_a, seg_b);
}

// Backward of aggregate_reduce (gnna_scatter_arg_ld_f32): grad_in[column_index[arg[i, f]], f] += grad_out[i, f], arg >= 0.
torch::Tensor scatter_arg(const torch::Tensor &grad_out, const torch::Tensor &arg, const torch::Tensor &column_index,
                          int64_t num_in_rows)
{
    CHECK_CUDA(grad_out);
    TORCH_CHECK(grad_out.dim() == 2, "grad_out must be 2-D [num_nodes, dim]");
    CHECK_F32(grad_out);
    check_ids(arg, "arg");
    check_ids(column_index, "column_index");
    TORCH_CHECK(arg.dim() == 2 && arg.size(0) == grad_out.size(0) && arg.size(1) == grad_out.size(1), "arg must be [num_nodes, dim] like grad_out");
    TORCH_CHECK(arg.device() == grad_out.device() && column_index.device() == grad_out.device(),
                "grad_out, arg and column_index must be on one device");
    TORCH_CHECK(grad_out.size(1) >= 1, "grad_out must have at least one column");
    check_rows(grad_out, "grad_out");
    TORCH_CHECK(num_in_rows >= 0, "num_in_rows must not be negative");
    const int64_t n = grad_out.size(0), dim = grad_out.size(1);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(grad_out.device());
    auto out = fresh({num_in_rows, dim}, grad_out.options());
    check_rc(gnna_scatter_arg_ld_f32(grad_out.data_ptr<float>(), ld_of(grad_out), arg.data_ptr<int32_t>(), dim,
                                     column_index.data_ptr<int32_t>(), n, out.data_ptr<float>(), dim, num_in_rows, (int)dim, 0u, current_stream()));
    return out;
}

// Edge softmax and its backward: scores [nnz] or head-major [heads, nnz] over the rows of row_pointers.
torch::Tensor edge_softmax(const torch::Tensor &scores, const torch::Tensor &row_pointers)
{
    check_floats(scores, "scores");
    check_ids(row_pointers, "row_pointers");
    TORCH_CHECK(scores.dim() == 1 || scores.dim() == 2, "scores must be [nnz] or [heads, nnz]");
    TORCH_CHECK(row_pointers.dim() == 1 && row_pointers.size(0) >= 1, "row_pointers must be [num_rows + 1]");
    TORCH_CHECK(row_pointers.device() == scores.device(), "scores and row_pointers must be on one device");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(scores.device());
    auto probs = torch::empty_like(scores);
    const int heads = scores.dim() == 2 ? (int)scores.size(0) : 1;
    const int64_t nnz = scores.size(scores.dim() - 1);
    check_rc(gnna_edge_softmax_f32(scores.data_ptr<float>(), row_pointers.data_ptr<int32_t>(), row_pointers.size(0) - 1, nnz, heads,
                                   probs.data_ptr<float>(), current_stream()));
    return probs;
}

torch::Tensor edge_softmax_backward(const torch::Tensor &probs, const torch::Tensor &grad, const torch::Tensor &row_pointers)
{
    check_floats(probs, "probs");
    check_floats(grad, "grad");
    check_ids(row_pointers, "row_pointers");
    TORCH_CHECK(probs.dim() == 1 || probs.dim() == 2, "probs must be [nnz] or [heads, nnz]");
    TORCH_CHECK(grad.sizes() == probs.sizes(), "grad must have the shape of probs");
    TORCH_CHECK(row_pointers.dim() == 1 && row_pointers.size(0) >= 1, "row_pointers must be [num_rows + 1]");
    TORCH_CHECK(grad.device() == probs.device() && row_pointers.device() == probs.device(), "probs, grad and row_pointers must be on one device");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(probs.device());
    auto gs = torch::empty_like(probs);
    const int heads = probs.dim() == 2 ? (int)probs.size(0) : 1;
    const int64_t nnz = probs.size(probs.dim() - 1);
    check_rc(gnna_edge_softmax_backward_f32(probs.data_ptr<float>(), grad.data_ptr<float>(), row_pointers.data_ptr<int32_t>(),
                                            row_pointers.size(0) - 1, nnz, heads, gs.data_ptr<float>(), current_stream()));
    return gs;
}

// Fused multi-head GAT attention (gnna_gat_forward_f32 / gnna_gat_backward_f32 and their rectangular forms): H [num_in_rows,
// heads * dim], er [num_in_rows, heads], el [num_out_rows, heads] with num_out_rows = row_pointers.numel() - 1 (a square graph:
// both are num_nodes; a sampled block: num_dst and num_src).  No per-edge tensor is made.  H, Y and dY go through their leading
// dimension (copied only when the inner stride is not 1).  Every shape is checked before any device work.
static torch::Tensor gat_rows(const torch::Tensor &t, const char *what, int64_t n, int64_t width)
{
    CHECK_CUDA(t); CHECK_F32(t);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == n && t.size(1) == width, what, " must be [", n, ", heads * dim = ", width,
                "] (num_nodes rows; on a rectangular structure H has num_in_rows rows, Y and dY num_out_rows)");
    const bool rows_ok = (width <= 1 || t.stride(1) == 1) && (n <= 1 || t.stride(0) >= width);
    return rows_ok ? t : t.contiguous();
}

// the structure walked by rows of `rows` rows (the graph: num_out_rows; its transpose: num_in_rows)
static void gat_check_graph(const torch::Tensor &H, int64_t rows, const torch::Tensor &row_pointers,
                            const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node)
{
    check_ids(row_pointers, "row_pointers");
    check_partition(column_index, part_pointers, part2Node);
    TORCH_CHECK(row_pointers.dim() == 1 && row_pointers.size(0) == rows + 1, "row_pointers must be [num_nodes + 1] (", rows + 1,
                " entries: one more than the rows of the side it walks)");
    TORCH_CHECK(part_pointers.numel() == part2Node.numel() + 1, "part_pointers must be [num_parts + 1]");
    TORCH_CHECK(row_pointers.device() == H.device() && column_index.device() == H.device() &&
                part_pointers.device() == H.device() && part2Node.device() == H.device(), "H and the graph must be on one device");
}

static int gat_heads(const torch::Tensor &H, const torch::Tensor &el, const torch::Tensor &er)
{
    check_floats(el, "el");
    check_floats(er, "er");
    TORCH_CHECK(H.dim() == 2, "H must be 2-D [num_nodes, heads * dim]");
    TORCH_CHECK(el.dim() == 2 && el.size(1) >= 1 && er.dim() == 2 && er.size(0) == H.size(0) && er.size(1) == el.size(1),
                "el and er must be [num_nodes, heads] (rectangular: el [num_out_rows, heads], er [num_in_rows = H.size(0), heads])");
    TORCH_CHECK(H.size(1) >= el.size(1) && H.size(1) % el.size(1) == 0, "H must be [num_nodes, heads * dim]");
    TORCH_CHECK(el.device() == H.device() && er.device() == H.device(), "H, el and er must be on one device");
    return (int)el.size(1);
}

// (attn_drop, rng_seed) of gat_forward_drop / gat_backward_drop: the mask rule of gnna_ext.h, whose entries take every structure
// in the rectangular form
struct GatDrop { float attn_drop; uint64_t rng_seed; };

static std::tuple<torch::Tensor, torch::Tensor>
gat_forward_any(const torch::Tensor &H_in, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &row_pointers,
                const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
                double negative_slope, const GatDrop *drop)
{
    const int heads = gat_heads(H_in, el, er);
    const int64_t n_in = H_in.size(0), n_out = el.size(0), width = H_in.size(1);
    const torch::Tensor H = gat_rows(H_in, "H", n_in, width);
    gat_check_graph(H, n_out, row_pointers, column_index, part_pointers, part2Node);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(H.device());
    auto Y = fresh({n_out, width}, el.options()), lse = fresh({n_out, (int64_t)heads}, el.options());
    void *stream = current_stream();
    if (drop)
        check_rc(gnna_gat_forward_drop_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(),
                                           row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                           part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), (float)negative_slope,
                                           drop->attn_drop, drop->rng_seed, Y.data_ptr<float>(), width, lse.data_ptr<float>(), n_out,
                                           n_in, heads, (int)(width / heads), part2Node.size(0), partSize, 0u, stream));
    else if (n_out == n_in)
        check_rc(gnna_gat_forward_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(),
                                      row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                      part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), (float)negative_slope,
                                      Y.data_ptr<float>(), width, lse.data_ptr<float>(), n_out, heads, (int)(width / heads),
                                      part2Node.size(0), partSize, 0u, stream));
    else
        check_rc(gnna_gat_forward_rect_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(),
                                           row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                           part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), (float)negative_slope,
                                           Y.data_ptr<float>(), width, lse.data_ptr<float>(), n_out, n_in, heads,
                                           (int)(width / heads), part2Node.size(0), partSize, 0u, stream));
    return std::make_tuple(Y, lse);
}

std::tuple<torch::Tensor, torch::Tensor>
gat_forward(const torch::Tensor &H, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &row_pointers,
            const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
            double negative_slope)
{
    return gat_forward_any(H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope, nullptr);
}

std::tuple<torch::Tensor, torch::Tensor>
gat_forward_drop(const torch::Tensor &H, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &row_pointers,
                 const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
                 double negative_slope, double attn_drop, uint64_t rng_seed)
{
    const GatDrop drop{(float)attn_drop, rng_seed};
    return gat_forward_any(H, el, er, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope, &drop);
}

static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
gat_backward_any(const torch::Tensor &H_in, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &lse,
                 const torch::Tensor &Y_in, const torch::Tensor &dY_in, const torch::Tensor &row_pointers,
                 const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
                 double negative_slope, const c10::optional<std::vector<torch::Tensor>> &transposed, const GatDrop *drop)
{
    const int heads = gat_heads(H_in, el, er);
    const int64_t n_in = H_in.size(0), n_out = el.size(0), width = H_in.size(1);
    const bool rect = n_out != n_in;
    TORCH_CHECK(!rect || transposed.has_value(), "gat_backward on a rectangular structure (", n_out, " destination rows, ", n_in,
                " source rows) needs `transposed`: a rectangular structure is never its own transpose");
    const torch::Tensor H = gat_rows(H_in, "H", n_in, width), Y = gat_rows(Y_in, "Y", n_out, width),
                        dY = gat_rows(dY_in, "dY", n_out, width);
    // transposed = (t_row_pointers, t_column_index, t_part_pointers, t_part2Node): the source-side pass walks it (directed graphs,
    // blocks): num_in_rows rows
    const torch::Tensor *t_rp = &row_pointers, *t_ci = &column_index, *t_pp = &part_pointers, *t_p2n = &part2Node;
    if (transposed.has_value()) {
        TORCH_CHECK(transposed->size() == 4, "transposed must be (t_row_pointers, t_column_index, t_part_pointers, t_part2Node)");
        t_rp = &(*transposed)[0]; t_ci = &(*transposed)[1]; t_pp = &(*transposed)[2]; t_p2n = &(*transposed)[3];
        gat_check_graph(H, n_in, *t_rp, *t_ci, *t_pp, *t_p2n);
    }
    check_floats(lse, "lse");
    TORCH_CHECK(lse.sizes() == el.sizes() && lse.device() == H.device(), "lse must be [num_nodes, heads] (the shape of el) on H's device");
    TORCH_CHECK(Y.device() == H.device() && dY.device() == H.device(), "H, Y and dY must be on one device");
    gat_check_graph(H, n_out, row_pointers, column_index, part_pointers, part2Node);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(H.device());
    auto dH = fresh({n_in, width}, el.options()), d_el = fresh({n_out, (int64_t)heads}, el.options()),
         d_er = fresh({n_in, (int64_t)heads}, el.options());
    void *stream = current_stream();
    if (drop)       // (a symmetric graph without `transposed`: its own structure, given twice)
        check_rc(gnna_gat_backward_drop_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(), lse.data_ptr<float>(),
                                            Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(), ld_of(dY),
                                            row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                            part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), part2Node.size(0),
                                            t_rp->data_ptr<int32_t>(), t_ci->data_ptr<int32_t>(), t_pp->data_ptr<int32_t>(),
                                            t_p2n->data_ptr<int32_t>(), t_p2n->size(0), (float)negative_slope, drop->attn_drop,
                                            drop->rng_seed, dH.data_ptr<float>(), width, d_el.data_ptr<float>(),
                                            d_er.data_ptr<float>(), n_out, n_in, heads, (int)(width / heads), partSize, 0u, stream));
    else if (!rect)
        check_rc(gnna_gat_backward_dir_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(), lse.data_ptr<float>(),
                                           Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(), ld_of(dY),
                                           row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                           part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), part2Node.size(0),
                                           t_rp->data_ptr<int32_t>(), t_ci->data_ptr<int32_t>(), t_pp->data_ptr<int32_t>(),
                                           t_p2n->data_ptr<int32_t>(), t_p2n->size(0), (float)negative_slope,
                                           dH.data_ptr<float>(), width, d_el.data_ptr<float>(), d_er.data_ptr<float>(), n_out, heads,
                                           (int)(width / heads), partSize, 0u, stream));
    else
        check_rc(gnna_gat_backward_rect_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(), lse.data_ptr<float>(),
                                            Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(), ld_of(dY),
                                            row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                            part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), part2Node.size(0),
                                            t_rp->data_ptr<int32_t>(), t_ci->data_ptr<int32_t>(), t_pp->data_ptr<int32_t>(),
                                            t_p2n->data_ptr<int32_t>(), t_p2n->size(0), (float)negative_slope,
                                            dH.data_ptr<float>(), width, d_el.data_ptr<float>(), d_er.data_ptr<float>(), n_out, n_in,
                                            heads, (int)(width / heads), partSize, 0u, stream));
    return std::make_tuple(dH, d_el, d_er);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
gat_backward(const torch::Tensor &H, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &lse,
             const torch::Tensor &Y, const torch::Tensor &dY, const torch::Tensor &row_pointers, const torch::Tensor &column_index,
             const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize, double negative_slope,
             const c10::optional<std::vector<torch::Tensor>> &transposed)
{
    return gat_backward_any(H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope,
                            transposed, nullptr);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
gat_backward_drop(const torch::Tensor &H, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &lse,
                  const torch::Tensor &Y, const torch::Tensor &dY, const torch::Tensor &row_pointers, const torch::Tensor &column_index,
                  const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize, double negative_slope,
                  double attn_drop, uint64_t rng_seed, const c10::optional<std::vector<torch::Tensor>> &transposed)
{
    const GatDrop drop{(float)attn_drop, rng_seed};
    return gat_backward_any(H, el, er, lse, Y, dY, row_pointers, column_index, part_pointers, part2Node, partSize, negative_slope,
                            transposed, &drop);
}

// Fused GAT attention with a per-edge score term (gnna_gat_edge.h): gat_forward_drop / gat_backward_drop with ee [num_edges,
// heads] (edge-major, indexed like column_index) in the score, its gradient d_ee, and the coefficients edge for edge.
static void gat_check_edge_term(const torch::Tensor &t, const char *name, const torch::Tensor &column_index, int heads)
{
    check_floats(t, name);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == column_index.numel() && t.size(1) == heads, name, " must be [num_edges = ",
                column_index.numel(), ", heads = ", heads, "] (edge-major, indexed like column_index)");
    TORCH_CHECK(t.device() == column_index.device(), name, " and the graph must be on one device");
}

std::tuple<torch::Tensor, torch::Tensor>
gat_edge_forward(const torch::Tensor &H_in, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &ee,
                 const torch::Tensor &row_pointers, const torch::Tensor &column_index, const torch::Tensor &part_pointers,
                 const torch::Tensor &part2Node, int partSize, double negative_slope, double attn_drop, uint64_t rng_seed)
{
    const int heads = gat_heads(H_in, el, er);
    const int64_t n_in = H_in.size(0), n_out = el.size(0), width = H_in.size(1);
    const torch::Tensor H = gat_rows(H_in, "H", n_in, width);
    gat_check_graph(H, n_out, row_pointers, column_index, part_pointers, part2Node);
    gat_check_edge_term(ee, "ee", column_index, heads);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(H.device());
    auto Y = fresh({n_out, width}, el.options()), lse = fresh({n_out, (int64_t)heads}, el.options());
    check_rc(gnna_gat_edge_forward_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(), ee.data_ptr<float>(),
                                       row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                       part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), (float)negative_slope,
                                       (float)attn_drop, rng_seed, Y.data_ptr<float>(), width, lse.data_ptr<float>(), n_out, n_in,
                                       column_index.numel(), heads, (int)(width / heads), part2Node.size(0), partSize, 0u,
                                       current_stream()));
    return std::make_tuple(Y, lse);
}

// t_edge_pos [num_edges]: the forward position of every position of the transposed structure -- transpose_csr's t_perm with
// `transposed`, the reverse-edge map of a symmetric graph without (its own structure is then given twice)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
gat_edge_backward(const torch::Tensor &H_in, const torch::Tensor &el, const torch::Tensor &er, const torch::Tensor &ee,
                  const torch::Tensor &lse, const torch::Tensor &Y_in, const torch::Tensor &dY_in, const torch::Tensor &row_pointers,
                  const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node,
                  const torch::Tensor &t_edge_pos, int partSize, double negative_slope, double attn_drop, uint64_t rng_seed,
                  const c10::optional<std::vector<torch::Tensor>> &transposed)
{
    const int heads = gat_heads(H_in, el, er);
    const int64_t n_in = H_in.size(0), n_out = el.size(0), width = H_in.size(1), nnz = column_index.numel();
    TORCH_CHECK(n_out == n_in || transposed.has_value(), "gat_edge_backward on a rectangular structure (", n_out, " destination rows, ",
                n_in, " source rows) needs `transposed`: a rectangular structure is never its own transpose");
    const torch::Tensor H = gat_rows(H_in, "H", n_in, width), Y = gat_rows(Y_in, "Y", n_out, width),
                        dY = gat_rows(dY_in, "dY", n_out, width);
    const torch::Tensor *t_rp = &row_pointers, *t_ci = &column_index, *t_pp = &part_pointers, *t_p2n = &part2Node;
    if (transposed.has_value()) {
        TORCH_CHECK(transposed->size() == 4, "transposed must be (t_row_pointers, t_column_index, t_part_pointers, t_part2Node)");
        t_rp = &(*transposed)[0]; t_ci = &(*transposed)[1]; t_pp = &(*transposed)[2]; t_p2n = &(*transposed)[3];
        gat_check_graph(H, n_in, *t_rp, *t_ci, *t_pp, *t_p2n);
    }
    check_floats(lse, "lse");
    TORCH_CHECK(lse.sizes() == el.sizes() && lse.device() == H.device(), "lse must be [num_nodes, heads] (the shape of el) on H's device");
    TORCH_CHECK(Y.device() == H.device() && dY.device() == H.device(), "H, Y and dY must be on one device");
    gat_check_graph(H, n_out, row_pointers, column_index, part_pointers, part2Node);
    gat_check_edge_term(ee, "ee", column_index, heads);
    check_ids(t_edge_pos, "t_edge_pos");
    TORCH_CHECK(t_edge_pos.dim() == 1 && t_edge_pos.numel() == nnz && t_ci->numel() == nnz && t_edge_pos.device() == H.device(),
                "t_edge_pos and the transposed column_index must be [num_edges = ", nnz, "] on H's device");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(H.device());
    auto dH = fresh({n_in, width}, el.options()), d_el = fresh({n_out, (int64_t)heads}, el.options()),
         d_er = fresh({n_in, (int64_t)heads}, el.options()), d_ee = fresh({nnz, (int64_t)heads}, el.options());
    check_rc(gnna_gat_edge_backward_f32(H.data_ptr<float>(), ld_of(H), el.data_ptr<float>(), er.data_ptr<float>(), ee.data_ptr<float>(),
                                        lse.data_ptr<float>(), Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(), ld_of(dY),
                                        row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                        part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), part2Node.size(0),
                                        t_rp->data_ptr<int32_t>(), t_ci->data_ptr<int32_t>(), t_pp->data_ptr<int32_t>(),
                                        t_p2n->data_ptr<int32_t>(), t_p2n->size(0), t_edge_pos.data_ptr<int32_t>(),
                                        (float)negative_slope, (float)attn_drop, rng_seed, dH.data_ptr<float>(), width,
                                        d_el.data_ptr<float>(), d_er.data_ptr<float>(), d_ee.data_ptr<float>(), n_out, n_in, nnz, heads,
                                        (int)(width / heads), partSize, 0u, current_stream()));
    return std::make_tuple(dH, d_el, d_er, d_ee);
}

torch::Tensor gat_alpha(const torch::Tensor &el, const torch::Tensor &er, const c10::optional<torch::Tensor> &ee, const torch::Tensor &lse,
                        const torch::Tensor &row_pointers, const torch::Tensor &column_index, double negative_slope)
{
    check_floats(el, "el");
    check_floats(er, "er");
    check_floats(lse, "lse");
    check_ids(row_pointers, "row_pointers");
    check_ids(column_index, "column_index");
    TORCH_CHECK(el.dim() == 2 && el.size(1) >= 1 && er.dim() == 2 && er.size(1) == el.size(1) && lse.sizes() == el.sizes(),
                "el and lse must be [num_out_rows, heads], er [num_in_rows, heads]");
    TORCH_CHECK(row_pointers.dim() == 1 && row_pointers.size(0) == el.size(0) + 1, "row_pointers must be [num_out_rows + 1]");
    TORCH_CHECK(er.device() == el.device() && lse.device() == el.device() && row_pointers.device() == el.device() &&
                column_index.device() == el.device(), "el, er, lse and the graph must be on one device");
    const int heads = (int)el.size(1);
    if (ee.has_value()) gat_check_edge_term(*ee, "ee", column_index, heads);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(el.device());
    auto alpha = fresh({column_index.numel(), (int64_t)heads}, el.options());
    check_rc(gnna_gat_alpha_f32(el.data_ptr<float>(), er.data_ptr<float>(), ee.has_value() ? ee->data_ptr<float>() : nullptr,
                                lse.data_ptr<float>(), row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                (float)negative_slope, alpha.data_ptr<float>(), el.size(0), er.size(0), column_index.numel(), heads,
                                current_stream()));
    return alpha;
}

// Fused GATv2 attention (gnna_gatv2_forward_f32 / gnna_gatv2_backward_f32, gnna_gatv2.h): Hs [num_in_rows, heads * dim] (the source
// side and the message), Hd [num_out_rows, heads * dim] with num_out_rows = row_pointers.numel() - 1, att [heads, dim].  One
// (rectangular) entry for every structure; attn_drop = 0 is the plain function.  Hs and Hd may be the same tensor.
static int gatv2_heads(const torch::Tensor &Hs, const torch::Tensor &Hd, const torch::Tensor &att)
{
    check_floats(att, "att");
    TORCH_CHECK(Hs.dim() == 2 && Hd.dim() == 2 && Hs.size(1) == Hd.size(1), "Hs must be [num_in_rows, heads * dim] and Hd [num_out_rows, heads * dim]");
    TORCH_CHECK(att.dim() == 2 && att.size(0) >= 1 && att.size(1) >= 1 && att.size(0) * att.size(1) == Hs.size(1),
                "att must be [heads, dim] with heads * dim = Hs.size(1)");
    TORCH_CHECK(Hd.device() == Hs.device() && att.device() == Hs.device(), "Hs, Hd and att must be on one device");
    return (int)att.size(0);
}

std::tuple<torch::Tensor, torch::Tensor>
gatv2_forward(const torch::Tensor &Hs_in, const torch::Tensor &Hd_in, const torch::Tensor &att, const torch::Tensor &row_pointers,
              const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
              double negative_slope, double attn_drop, uint64_t rng_seed)
{
    const int heads = gatv2_heads(Hs_in, Hd_in, att);
    const int64_t n_in = Hs_in.size(0), n_out = Hd_in.size(0), width = Hs_in.size(1);
    const torch::Tensor Hs = gat_rows(Hs_in, "Hs", n_in, width), Hd = gat_rows(Hd_in, "Hd", n_out, width);
    gat_check_graph(Hs, n_out, row_pointers, column_index, part_pointers, part2Node);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(Hs.device());
    auto Y = fresh({n_out, width}, att.options()), lse = fresh({n_out, (int64_t)heads}, att.options());
    check_rc(gnna_gatv2_forward_f32(Hs.data_ptr<float>(), ld_of(Hs), Hd.data_ptr<float>(), ld_of(Hd), att.data_ptr<float>(),
                                    row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                    part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), (float)negative_slope,
                                    (float)attn_drop, rng_seed, Y.data_ptr<float>(), width, lse.data_ptr<float>(), n_out, n_in, heads,
                                    (int)(width / heads), part2Node.size(0), partSize, 0u, current_stream()));
    return std::make_tuple(Y, lse);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
gatv2_backward(const torch::Tensor &Hs_in, const torch::Tensor &Hd_in, const torch::Tensor &att, const torch::Tensor &lse,
               const torch::Tensor &Y_in, const torch::Tensor &dY_in, const torch::Tensor &row_pointers,
               const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
               double negative_slope, double attn_drop, uint64_t rng_seed,
               const c10::optional<std::vector<torch::Tensor>> &transposed)
{
    const int heads = gatv2_heads(Hs_in, Hd_in, att);
    const int64_t n_in = Hs_in.size(0), n_out = Hd_in.size(0), width = Hs_in.size(1);
    TORCH_CHECK(n_out == n_in || transposed.has_value(), "gatv2_backward on a rectangular structure (", n_out, " destination rows, ",
                n_in, " source rows) needs `transposed`: a rectangular structure is never its own transpose");
    const torch::Tensor Hs = gat_rows(Hs_in, "Hs", n_in, width), Hd = gat_rows(Hd_in, "Hd", n_out, width),
                        Y = gat_rows(Y_in, "Y", n_out, width), dY = gat_rows(dY_in, "dY", n_out, width);
    // (a symmetric graph without `transposed`: its own structure, given twice)
    const torch::Tensor *t_rp = &row_pointers, *t_ci = &column_index, *t_pp = &part_pointers, *t_p2n = &part2Node;
    if (transposed.has_value()) {
        TORCH_CHECK(transposed->size() == 4, "transposed must be (t_row_pointers, t_column_index, t_part_pointers, t_part2Node)");
        t_rp = &(*transposed)[0]; t_ci = &(*transposed)[1]; t_pp = &(*transposed)[2]; t_p2n = &(*transposed)[3];
        gat_check_graph(Hs, n_in, *t_rp, *t_ci, *t_pp, *t_p2n);
    }
    check_floats(lse, "lse");
    TORCH_CHECK(lse.dim() == 2 && lse.size(0) == n_out && lse.size(1) == heads && lse.device() == Hs.device(),
                "lse must be [num_out_rows, heads] on Hs's device");
    TORCH_CHECK(Y.device() == Hs.device() && dY.device() == Hs.device(), "Hs, Y and dY must be on one device");
    gat_check_graph(Hs, n_out, row_pointers, column_index, part_pointers, part2Node);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(Hs.device());
    auto dHs = fresh({n_in, width}, att.options()), dHd = fresh({n_out, width}, att.options()), d_att = fresh(att.sizes(), att.options());
    check_rc(gnna_gatv2_backward_f32(Hs.data_ptr<float>(), ld_of(Hs), Hd.data_ptr<float>(), ld_of(Hd), att.data_ptr<float>(),
                                     lse.data_ptr<float>(), Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(), ld_of(dY),
                                     row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                     part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), part2Node.size(0),
                                     t_rp->data_ptr<int32_t>(), t_ci->data_ptr<int32_t>(), t_pp->data_ptr<int32_t>(),
                                     t_p2n->data_ptr<int32_t>(), t_p2n->size(0), (float)negative_slope, (float)attn_drop, rng_seed,
                                     dHs.data_ptr<float>(), width, dHd.data_ptr<float>(), width, d_att.data_ptr<float>(), n_out, n_in,
                                     heads, (int)(width / heads), partSize, 0u, current_stream()));
    return std::make_tuple(dHs, dHd, d_att);
}

// Fused scaled dot-product graph attention (gnna_dot_attn_forward_f32 / gnna_dot_attn_backward_f32, gnna_dotattn.h): Q [num_out_rows,
// heads * dim] with num_out_rows = row_pointers.numel() - 1, K and V [num_in_rows, heads * dim].  One (rectangular) entry for every
// structure; attn_drop = 0 is the plain function.  Q, K and V go through their leading dimensions: column slices of one projection
// matrix are passed as they are.
static void dot_attn_shapes(const torch::Tensor &Q, const torch::Tensor &K, const torch::Tensor &V, int64_t heads, double scale)
{
    TORCH_CHECK(Q.dim() == 2 && K.dim() == 2 && V.dim() == 2 && K.size(1) == Q.size(1) && V.size(1) == Q.size(1) && V.size(0) == K.size(0),
                "Q must be [num_out_rows, heads * dim], K and V [num_in_rows, heads * dim]");
    TORCH_CHECK(heads >= 1 && Q.size(1) >= 1 && Q.size(1) % heads == 0, "heads (", heads, ") must divide heads * dim = ", Q.size(1));
    TORCH_CHECK(std::isfinite(scale), "scale must be finite (got ", scale, ")");
    TORCH_CHECK(K.device() == Q.device() && V.device() == Q.device(), "Q, K and V must be on one device");
}

std::tuple<torch::Tensor, torch::Tensor>
dot_attn_forward(const torch::Tensor &Q_in, const torch::Tensor &K_in, const torch::Tensor &V_in, int64_t heads,
                 const torch::Tensor &row_pointers, const torch::Tensor &column_index, const torch::Tensor &part_pointers,
                 const torch::Tensor &part2Node, int partSize, double scale, double attn_drop, uint64_t rng_seed)
{
    dot_attn_shapes(Q_in, K_in, V_in, heads, scale);
    const int64_t n_in = K_in.size(0), n_out = Q_in.size(0), width = Q_in.size(1);
    const torch::Tensor Q = gat_rows(Q_in, "Q", n_out, width), K = gat_rows(K_in, "K", n_in, width), V = gat_rows(V_in, "V", n_in, width);
    gat_check_graph(Q, n_out, row_pointers, column_index, part_pointers, part2Node);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(Q.device());
    auto Y = fresh({n_out, width}, Q.options()), lse = fresh({n_out, heads}, Q.options());
    check_rc(gnna_dot_attn_forward_f32(Q.data_ptr<float>(), ld_of(Q), K.data_ptr<float>(), ld_of(K), V.data_ptr<float>(), ld_of(V),
                                       row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                       part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), (float)scale,
                                       (float)attn_drop, rng_seed, Y.data_ptr<float>(), width, lse.data_ptr<float>(), n_out, n_in,
                                       (int)heads, (int)(width / heads), part2Node.size(0), partSize, 0u, current_stream()));
    return std::make_tuple(Y, lse);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
dot_attn_backward(const torch::Tensor &Q_in, const torch::Tensor &K_in, const torch::Tensor &V_in, int64_t heads,
                  const torch::Tensor &lse, const torch::Tensor &Y_in, const torch::Tensor &dY_in, const torch::Tensor &row_pointers,
                  const torch::Tensor &column_index, const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize,
                  double scale, double attn_drop, uint64_t rng_seed, const c10::optional<std::vector<torch::Tensor>> &transposed)
{
    dot_attn_shapes(Q_in, K_in, V_in, heads, scale);
    const int64_t n_in = K_in.size(0), n_out = Q_in.size(0), width = Q_in.size(1);
    TORCH_CHECK(n_out == n_in || transposed.has_value(), "dot_attn_backward on a rectangular structure (", n_out, " destination rows, ",
                n_in, " source rows) needs `transposed`: a rectangular structure is never its own transpose");
    const torch::Tensor Q = gat_rows(Q_in, "Q", n_out, width), K = gat_rows(K_in, "K", n_in, width), V = gat_rows(V_in, "V", n_in, width),
                        Y = gat_rows(Y_in, "Y", n_out, width), dY = gat_rows(dY_in, "dY", n_out, width);
    // (a symmetric graph without `transposed`: its own structure, given twice)
    const torch::Tensor *t_rp = &row_pointers, *t_ci = &column_index, *t_pp = &part_pointers, *t_p2n = &part2Node;
    if (transposed.has_value()) {
        TORCH_CHECK(transposed->size() == 4, "transposed must be (t_row_pointers, t_column_index, t_part_pointers, t_part2Node)");
        t_rp = &(*transposed)[0]; t_ci = &(*transposed)[1]; t_pp = &(*transposed)[2]; t_p2n = &(*transposed)[3];
        gat_check_graph(Q, n_in, *t_rp, *t_ci, *t_pp, *t_p2n);
    }
    check_floats(lse, "lse");
    TORCH_CHECK(lse.dim() == 2 && lse.size(0) == n_out && lse.size(1) == heads && lse.device() == Q.device(),
                "lse must be [num_out_rows, heads] on Q's device");
    TORCH_CHECK(Y.device() == Q.device() && dY.device() == Q.device(), "Q, Y and dY must be on one device");
    gat_check_graph(Q, n_out, row_pointers, column_index, part_pointers, part2Node);
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(Q.device());
    auto dQ = fresh({n_out, width}, Q.options()), dK = fresh({n_in, width}, Q.options()), dV = fresh({n_in, width}, Q.options());
    check_rc(gnna_dot_attn_backward_f32(Q.data_ptr<float>(), ld_of(Q), K.data_ptr<float>(), ld_of(K), V.data_ptr<float>(), ld_of(V),
                                        lse.data_ptr<float>(), Y.data_ptr<float>(), ld_of(Y), dY.data_ptr<float>(), ld_of(dY),
                                        row_pointers.data_ptr<int32_t>(), column_index.data_ptr<int32_t>(),
                                        part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), part2Node.size(0),
                                        t_rp->data_ptr<int32_t>(), t_ci->data_ptr<int32_t>(), t_pp->data_ptr<int32_t>(),
                                        t_p2n->data_ptr<int32_t>(), t_p2n->size(0), (float)scale, (float)attn_drop, rng_seed,
                                        dQ.data_ptr<float>(), width, dK.data_ptr<float>(), width, dV.data_ptr<float>(), width, n_out,
                                        n_in, (int)heads, (int)(width / heads), partSize, 0u, current_stream()));
    return std::make_tuple(dQ, dK, dV);
}

// SDDMM (gnna_sddmm_ld_f32): edge_out[e] = <A[row(e)], B[column_index[e]]>; A and B may be row-strided views.
torch::Tensor sddmm(const torch::Tensor &A, const torch::Tensor &B, const torch::Tensor &column_index,
                    const torch::Tensor &part_pointers, const torch::Tensor &part2Node, int partSize)
{
    CHECK_CUDA(A); CHECK_CUDA(B); CHECK_F32(A); CHECK_F32(B);
    check_partition(column_index, part_pointers, part2Node);
    TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(1) == B.size(1), "A [rows, dim] and B [num_nodes, dim] expected");
    TORCH_CHECK(A.device() == B.device() && column_index.device() == A.device(), "A, B and column_index must be on one device");
    TORCH_CHECK(A.size(1) <= 1 || (A.stride(1) == 1 && B.stride(1) == 1), "the floats of a row must be contiguous (stride(1) == 1)");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(A.device());
    // (edges of rows without a neighbor-group -- none in a partition of the full CSR -- stay zero)
    auto out = torch::zeros({column_index.numel()}, A.options());
    check_rc(gnna_sddmm_ld_f32(A.data_ptr<float>(), ld_of(A), B.data_ptr<float>(), ld_of(B), column_index.data_ptr<int32_t>(),
                               part_pointers.data_ptr<int32_t>(), part2Node.data_ptr<int32_t>(), out.data_ptr<float>(),
                               A.size(0), B.size(0), (int)A.size(1), part2Node.size(0), partSize, current_stream()));
    return out;
}

}  // namespace

// ---- host launchers: reference names (GNNAdvisor_kernel.cu:110,267,422,559,696) -------------

// Weight gradient X^T G on the MFMA units (libgnna's tall-skinny kernel) in place of
// torch::mm(X.transpose(0,1), G) (.cu:473, :710): the BLAS library runs this shape -- reduction
// over the node dimension -- 5-14x off the memory bound.
torch::Tensor xtg(const torch::Tensor &X, const torch::Tensor &G)
{
    TORCH_CHECK(X.dim() == 2 && G.dim() == 2 && X.size(0) == G.size(0), "xtg: X [M, K] and G [M, N] expected");
    CHECK_F32(X);
    CHECK_F32(G);
    auto Xc = X.contiguous();
    auto Gc = G.contiguous();
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(X.device());
    auto dW = torch::empty({X.size(1), G.size(1)}, X.options());
    void *stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
    int rc = gnna_xtg_f32(Xc.data_ptr<float>(), Gc.data_ptr<float>(), dW.data_ptr<float>(), X.size(0),
                          (int)X.size(1), (int)G.size(1), stream);
    TORCH_CHECK(rc == GNNA_OK, "libgnna: ", gnna_last_error());
    return dW;
}

torch::Tensor SAG_cuda(torch::Tensor input, torch::Tensor row_pointers, torch::Tensor column_index,
                       torch::Tensor degrees, torch::Tensor part_pointers, torch::Tensor part2Node,
                       int partSize, int dimWorker, int warpPerBlock)
{
    return aggregate(AGG_SAG, input, row_pointers, column_index, &degrees, 1.f, part_pointers, part2Node,
                     partSize, dimWorker, warpPerBlock);
}

// update -> aggregate (.cu:280-282)
std::vector<torch::Tensor> spmm_forward_cuda(torch::Tensor input, torch::Tensor weight,
                                             torch::Tensor row_pointers, torch::Tensor column_index,
                                             torch::Tensor degrees, torch::Tensor part_pointers,
                                             torch::Tensor part2Node, int partSize, int dimWorker,
                                             int warpPerBlock)
{
    auto tmp = torch::mm(input, weight);
    auto output = aggregate(AGG_GCN, tmp, row_pointers, column_index, &degrees, 1.f, part_pointers,
                            part2Node, partSize, dimWorker, warpPerBlock);
    return {output};
}

// aggregate -> two GEMMs (.cu:436-473)
std::vector<torch::Tensor> spmm_backward_cuda(torch::Tensor d_output, torch::Tensor X, torch::Tensor W,
                                              torch::Tensor row_pointers, torch::Tensor column_index,
                                              torch::Tensor degrees, torch::Tensor part_pointers,
                                              torch::Tensor part2Node, int partSize, int dimWorker,
                                              int warpPerBlock)
{
    auto d_input_prime = aggregate(AGG_GCN, d_output, row_pointers, column_index, &degrees, 1.f,
                                   part_pointers, part2Node, partSize, dimWorker, warpPerBlock);
    auto d_input = torch::mm(d_input_prime, W.transpose(0, 1));
    auto d_weight = xtg(X, d_input_prime);
    return {d_input, d_weight};
}

// aggregate (x epsilon) -> update (.cu:575-616)
std::vector<torch::Tensor> spmm_forward_cuda_gin(torch::Tensor input, torch::Tensor weight,
                                                 torch::Tensor row_pointers, torch::Tensor column_index,
                                                 float epsilon, torch::Tensor part_pointers,
                                                 torch::Tensor part2Node, int partSize, int dimWorker,
                                                 int warpPerBlock)
{
    auto tmp = aggregate(AGG_GIN, input, row_pointers, column_index, nullptr, epsilon, part_pointers,
                         part2Node, partSize, dimWorker, warpPerBlock);
    auto output = torch::mm(tmp, weight);
    return {output, tmp};
}

// two GEMMs -> aggregate (x epsilon) (.cu:710-746)
std::vector<torch::Tensor> spmm_backward_cuda_gin(torch::Tensor d_output, torch::Tensor X, torch::Tensor W,
                                                  torch::Tensor row_pointers, torch::Tensor column_index,
                                                  float epsilon, torch::Tensor part_pointers,
                                                  torch::Tensor part2Node, int partSize, int dimWorker,
                                                  int warpPerBlock)
{
    auto d_weight = xtg(X, d_output);
    auto d_input_prime = torch::mm(d_output, W.transpose(0, 1));
    auto d_input = aggregate(AGG_GIN, d_input_prime, row_pointers, column_index, nullptr, epsilon,
                             part_pointers, part2Node, partSize, dimWorker, warpPerBlock);
    return {d_input, d_weight};
}

// ---- Python-visible wrappers (GNNAdvisor.cpp:75-207): input checks, then the launcher --------

torch::Tensor SAG(torch::Tensor input, torch::Tensor row_pointers, torch::Tensor column_index,
                  torch::Tensor degrees, torch::Tensor part_pointers, torch::Tensor part2Node,
                  int partSize, int dimWorker, int warpPerBlock)
{
    CHECK_INPUT(input);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(degrees);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    return SAG_cuda(input, row_pointers, column_index, degrees, part_pointers, part2Node, partSize,
                    dimWorker, warpPerBlock);
}

// Extension (not in the reference module): the epsilon-scaled aggregation of forward_gin /
// backward_gin on its own, eps * A * input -- lets the op layer run a GIN layer update-first.
torch::Tensor aggregate_gin(torch::Tensor input, torch::Tensor row_pointers, torch::Tensor column_index,
                            float epsilon, torch::Tensor part_pointers, torch::Tensor part2Node,
                            int partSize, int dimWorker, int warpPerBlock)
{
    CHECK_INPUT(input);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    return aggregate(AGG_GIN, input, row_pointers, column_index, nullptr, epsilon, part_pointers, part2Node,
                     partSize, dimWorker, warpPerBlock);
}

std::vector<torch::Tensor> spmm_forward(torch::Tensor input, torch::Tensor weight, torch::Tensor row_pointers,
                                        torch::Tensor column_index, torch::Tensor degrees,
                                        torch::Tensor part_pointers, torch::Tensor part2Node, int partSize,
                                        int dimWorker, int warpPerBlock)
{
    CHECK_INPUT(input);
    CHECK_INPUT(weight);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(degrees);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    return spmm_forward_cuda(input, weight, row_pointers, column_index, degrees, part_pointers, part2Node,
                             partSize, dimWorker, warpPerBlock);
}

std::vector<torch::Tensor> spmm_backward(torch::Tensor d_output, torch::Tensor X, torch::Tensor W,
                                         torch::Tensor row_pointers, torch::Tensor column_index,
                                         torch::Tensor degrees, torch::Tensor part_pointers,
                                         torch::Tensor part2Node, int partSize, int dimWorker,
                                         int warpPerBlock)
{
    CHECK_INPUT(d_output);
    CHECK_INPUT(X);
    CHECK_INPUT(W);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(degrees);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    return spmm_backward_cuda(d_output, X, W, row_pointers, column_index, degrees, part_pointers, part2Node,
                              partSize, dimWorker, warpPerBlock);
}

// Extension (not in the reference module): the weight gradient alone, for a first layer whose
// input needs no gradient -- skips the [N, Fout] x [Fout, Fin] GEMM and the N x Fin write of d_input.
std::vector<torch::Tensor> spmm_backward_weight(torch::Tensor d_output, torch::Tensor X,
                                                torch::Tensor row_pointers, torch::Tensor column_index,
                                                torch::Tensor degrees, torch::Tensor part_pointers,
                                                torch::Tensor part2Node, int partSize, int dimWorker,
                                                int warpPerBlock)
{
    CHECK_INPUT(d_output);
    CHECK_INPUT(X);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(degrees);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    auto d_input_prime = aggregate(AGG_GCN, d_output, row_pointers, column_index, &degrees, 1.f,
                                   part_pointers, part2Node, partSize, dimWorker, warpPerBlock);
    return {xtg(X, d_input_prime)};
}

std::vector<torch::Tensor> spmm_forward_gin(torch::Tensor input, torch::Tensor weight,
                                            torch::Tensor row_pointers, torch::Tensor column_index,
                                            float epsilon, torch::Tensor part_pointers,
                                            torch::Tensor part2Node, int partSize, int dimWorker,
                                            int warpPerBlock)
{
    CHECK_INPUT(input);
    CHECK_INPUT(weight);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    return spmm_forward_cuda_gin(input, weight, row_pointers, column_index, epsilon, part_pointers,
                                 part2Node, partSize, dimWorker, warpPerBlock);
}

std::vector<torch::Tensor> spmm_backward_gin(torch::Tensor d_output, torch::Tensor X, torch::Tensor W,
                                             torch::Tensor row_pointers, torch::Tensor column_index,
                                             float epsilon, torch::Tensor part_pointers,
                                             torch::Tensor part2Node, int partSize, int dimWorker,
                                             int warpPerBlock)
{
    CHECK_INPUT(d_output);
    CHECK_INPUT(X);
    CHECK_INPUT(W);
    CHECK_INPUT(row_pointers);
    CHECK_INPUT(column_index);
    CHECK_INPUT(part_pointers);
    CHECK_INPUT(part2Node);
    return spmm_backward_cuda_gin(d_output, X, W, row_pointers, column_index, epsilon, part_pointers,
                                  part2Node, partSize, dimWorker, warpPerBlock);
}

// CPU neighbor-group partitioner (GNNAdvisor.cpp:210-251): indptr is a CPU int32 tensor.
// float_compat = false (default): exact int32 tensors.  float_compat = true: float32 tensors like the
// reference returns (GNNAdvisor.cpp:229-230) for callers that depend on the dtype -- with the closing
// sentinel always written (reference bug A fixed), and refused with an error when an offset would not
// survive the float32 round trip (> 2^24 edges: reference bug B would silently misplace groups).
std::vector<torch::Tensor> build_part(int partSize, torch::Tensor indptr, bool float_compat)
{
    TORCH_CHECK(!indptr.is_cuda(), "indptr must be a CPU tensor");
    TORCH_CHECK(indptr.dim() == 1 && indptr.size(0) >= 1, "indptr must be 1-D with num_nodes + 1 entries");
    CHECK_I32(indptr);
    auto ip = indptr.contiguous();
    const int64_t num_nodes = ip.size(0) - 1;
    const int64_t num_parts = gnna_count_parts(partSize, ip.data_ptr<int32_t>(), num_nodes);
    TORCH_CHECK(num_parts >= 0, "GNNAdvisor (libgnna) error ", num_parts, ": ", gnna_last_error());
    auto opts = torch::TensorOptions().dtype(torch::kInt32).device(torch::kCPU);
    auto partPtr = torch::empty({num_parts + 1}, opts);
    auto part2Node = torch::empty({num_parts}, opts);
    int rc = gnna_build_part_i32(partSize, ip.data_ptr<int32_t>(), num_nodes, partPtr.data_ptr<int32_t>(),
                                 part2Node.data_ptr<int32_t>(), num_parts);
    TORCH_CHECK(rc == GNNA_OK, "GNNAdvisor (libgnna) error ", rc, ": ", gnna_last_error());
    if (float_compat) {
        const int64_t nnz = num_nodes > 0 ? (int64_t)ip.data_ptr<int32_t>()[num_nodes] : 0;
        TORCH_CHECK(nnz <= (int64_t(1) << 24) && num_nodes <= (int64_t(1) << 24),
                    "build_part(float_compat=True): ", nnz, " edges / ", num_nodes,
                    " nodes cannot be stored exactly in float32 tensors (limit 2^24); use the int32 result");
        return {partPtr.to(torch::kFloat32), part2Node.to(torch::kFloat32)};
    }
    return {partPtr, part2Node};
}

// ---- device builders of a directed graph's backward structure (gnna_transpose.hip) ----------------------------------------

static void check_device_ids(const torch::Tensor &t, const char *what)
{
    TORCH_CHECK(t.is_cuda(), what, " must be a CUDA tensor (the builder runs on the device)");
    TORCH_CHECK(t.is_contiguous() && t.dim() == 1, what, " must be a contiguous 1-D tensor");
    check_i32(t, what);
}

// (t_row_pointers [num_in_rows + 1], t_column_index [nnz], t_perm [nnz]) of A^T; t_perm is omitted with want_perm = false.
std::vector<torch::Tensor> transpose_csr(const torch::Tensor &row_pointers, const torch::Tensor &column_index,
                                         c10::optional<int64_t> num_in_rows, bool want_perm)
{
    check_device_ids(row_pointers, "row_pointers");
    check_device_ids(column_index, "column_index");
    TORCH_CHECK(row_pointers.numel() >= 1 && column_index.device() == row_pointers.device(),
                "row_pointers must be [num_out_rows + 1], on column_index's device");
    const int64_t n_out = row_pointers.numel() - 1, n_in = num_in_rows.value_or(n_out), nnz = column_index.numel();
    TORCH_CHECK(n_in >= 0, "num_in_rows must not be negative");
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(row_pointers.device());
    // (the library trusts row_pointers[num_out_rows] for the edge count: it must not exceed what column_index holds)
    if (n_out > 0) TORCH_CHECK(row_pointers[n_out].item<int32_t>() == nnz, "row_pointers[-1] must be column_index.numel()");
    auto t_rp = torch::empty({n_in + 1}, row_pointers.options());
    auto t_ci = torch::empty({nnz}, row_pointers.options());
    torch::Tensor t_perm;
    if (want_perm) t_perm = torch::empty({nnz}, row_pointers.options());
    check_rc(gnna_transpose_csr_i32(row_pointers.data_ptr<int32_t>(), nnz ? column_index.data_ptr<int32_t>() : nullptr, n_out, n_in,
                                    t_rp.data_ptr<int32_t>(), nnz ? t_ci.data_ptr<int32_t>() : nullptr,
                                    want_perm && nnz ? t_perm.data_ptr<int32_t>() : nullptr, current_stream()));
    if (want_perm) return {t_rp, t_ci, t_perm};
    return {t_rp, t_ci};
}

// build_part for device row pointers: (partPtr [P + 1], part2Node [P]) on the same device.
std::vector<torch::Tensor> build_part_device(int partSize, const torch::Tensor &indptr)
{
    check_device_ids(indptr, "indptr");
    TORCH_CHECK(indptr.numel() >= 1, "indptr must have num_nodes + 1 entries");
    const int64_t num_nodes = indptr.numel() - 1;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(indptr.device());
    void *stream = current_stream();
    const int64_t num_parts = gnna_count_parts_device_i32(partSize, indptr.data_ptr<int32_t>(), num_nodes, stream);
    TORCH_CHECK(num_parts >= 0, "GNNAdvisor (libgnna) error ", num_parts, ": ", gnna_last_error());
    auto partPtr = torch::empty({num_parts + 1}, indptr.options());
    auto part2Node = torch::empty({num_parts}, indptr.options());
    check_rc(gnna_build_part_device_i32(partSize, indptr.data_ptr<int32_t>(), num_nodes, partPtr.data_ptr<int32_t>(),
                                        num_parts ? part2Node.data_ptr<int32_t>() : nullptr, num_parts, stream));
    return {partPtr, part2Node};
}

// ---- hierarchical pooling on graph batches (gnna_topk.hip) ------------------------------------------------------------------

// Top-k selection per graph and the induced sub-batch (gnna_segment_topk_i32) -> (new_id [N], perm [N'], new_graph_pointers
// [G + 1], new_row_pointers [N' + 1], new_column_index [nnz'], edge_ids [nnz'], partPtr [P + 1], part2Node [P]); None for what was
// not asked for (the CSR without row_pointers / column_index, edge_ids without want_edge_ids, the partition with partSize = 0).
// ratio = 0 or k = 0 says which of the two is given.  The arrays are trimmed views of buffers of N rows and nnz edges.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
segment_topk(const torch::Tensor &score, const torch::Tensor &graph_pointers, double ratio, int64_t k,
             const c10::optional<torch::Tensor> &row_pointers, const c10::optional<torch::Tensor> &column_index, int64_t partSize,
             bool want_edge_ids)
{
    check_floats(score, "score");
    TORCH_CHECK(score.dim() == 1, "score must be 1-D [num_nodes]");
    check_device_ids(graph_pointers, "graph_pointers");
    TORCH_CHECK(graph_pointers.numel() >= 1 && graph_pointers.device() == score.device(),
                "graph_pointers must be [num_graphs + 1], on score's device");
    TORCH_CHECK(row_pointers.has_value() == column_index.has_value(), "row_pointers and column_index come together");
    TORCH_CHECK(partSize >= 0 && partSize <= std::numeric_limits<int>::max(), "partSize must not be negative");
    const bool csr = row_pointers.has_value(), parts = partSize > 0;
    TORCH_CHECK(csr || !parts, "a partition needs row_pointers and column_index");
    const int64_t n = score.numel(), g = graph_pointers.numel() - 1;
    int64_t nnz = 0;
    if (csr) {
        check_device_ids(*row_pointers, "row_pointers");
        check_device_ids(*column_index, "column_index");
        TORCH_CHECK(row_pointers->numel() == n + 1 && row_pointers->device() == score.device() && column_index->device() == score.device(),
                    "row_pointers must be [num_nodes + 1]; it and column_index live on score's device");
        nnz = column_index->numel();
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(score.device());
    const auto ids = graph_pointers.options();
    const torch::Tensor new_id = torch::empty({n}, ids), perm = torch::empty({n}, ids), new_gp = torch::empty({g + 1}, ids);
    torch::Tensor new_rp, new_ci, eid, pp, p2n;
    if (csr) { new_rp = torch::empty({n + 1}, ids); new_ci = torch::empty({nnz}, ids); }
    if (csr && want_edge_ids) eid = torch::empty({nnz}, ids);
    if (parts) { pp = torch::empty({nnz + 1}, ids); p2n = torch::empty({nnz}, ids); }
    auto ip = [](const torch::Tensor &t) { return t.defined() && t.numel() > 0 ? t.data_ptr<int32_t>() : nullptr; };
    int64_t counts[3] = {0, 0, 0};
    check_rc(gnna_segment_topk_i32(n > 0 ? score.data_ptr<float>() : nullptr, n, graph_pointers.data_ptr<int32_t>(), g, ratio, k,
                                   csr ? row_pointers->data_ptr<int32_t>() : nullptr, csr ? ip(*column_index) : nullptr, nnz, (int)partSize,
                                   ip(new_id), ip(perm), new_gp.data_ptr<int32_t>(), ip(new_rp), ip(new_ci), ip(eid), ip(pp), ip(p2n), n,
                                   nnz, parts ? nnz : 0, counts, current_stream()));
    auto opt = [](const torch::Tensor &t, int64_t len) { return t.defined() ? c10::optional<torch::Tensor>(t.narrow(0, 0, len)) : c10::nullopt; };
    return std::make_tuple(new_id, perm.narrow(0, 0, counts[0]), new_gp, opt(new_rp, counts[0] + 1), opt(new_ci, counts[1]),
                           opt(eid, counts[1]), opt(pp, counts[2] + 1), opt(p2n, counts[2]));
}

// ---- subgraph sampling (gnna_walk.hip) ---------------------------------------------------------------------------------------

// what both entries check of the graph and of their id list
static void walk_check(const torch::Tensor &row_pointers, const torch::Tensor &column_index, const torch::Tensor &ids, const char *ids_name)
{
    check_device_ids(row_pointers, "row_pointers");
    check_device_ids(column_index, "column_index");
    check_device_ids(ids, ids_name);
    TORCH_CHECK(row_pointers.numel() >= 1 && column_index.device() == row_pointers.device() && ids.device() == row_pointers.device(),
                "row_pointers must be [num_nodes + 1]; column_index and ", ids_name, " live on its device");
}

// Uniform random walks (gnna_random_walk_i32) -> (walks [R, walk_length + 1], edge_ids [R, walk_length] or None).
std::tuple<torch::Tensor, c10::optional<torch::Tensor>>
random_walk(const torch::Tensor &row_pointers, const torch::Tensor &column_index, const torch::Tensor &roots, int64_t walk_length,
            uint64_t rng_seed, bool want_edge_ids)
{
    walk_check(row_pointers, column_index, roots, "roots");
    TORCH_CHECK(walk_length >= 0 && walk_length < std::numeric_limits<int>::max(), "walk_length must not be negative");
    const int64_t n = row_pointers.numel() - 1, nnz = column_index.numel(), r = roots.numel();
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(row_pointers.device());
    const auto ids = row_pointers.options();
    const torch::Tensor walks = torch::empty({r, walk_length + 1}, ids);
    torch::Tensor eid;
    if (want_edge_ids) eid = torch::empty({r, walk_length}, ids);
    auto ip = [](const torch::Tensor &t) { return t.defined() && t.numel() > 0 ? t.data_ptr<int32_t>() : nullptr; };
    check_rc(gnna_random_walk_i32(row_pointers.data_ptr<int32_t>(), ip(column_index), n, nnz, ip(roots), r, (int)walk_length, rng_seed,
                                  ip(walks), ip(eid), current_stream()));
    return std::make_tuple(walks, want_edge_ids ? c10::optional<torch::Tensor>(eid) : c10::nullopt);
}

// The subgraph a node list induces (gnna_induced_subgraph_i32) -> (row_pointers [n + 1], column_index [nnz'], edge_ids [nnz'],
// nodes [n], new_id [N], partPtr [P + 1], part2Node [P]); None for what was not asked for (partSize = 0: no partition).  The
// arrays are trimmed views of buffers of min(num_ids, N) nodes and min(nnz, the degree sum over the list) edges.
std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>, torch::Tensor, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
induced_subgraph(const torch::Tensor &row_pointers, const torch::Tensor &column_index, const torch::Tensor &nodes, int64_t partSize,
                 bool want_edge_ids, bool want_new_id)
{
    walk_check(row_pointers, column_index, nodes, "nodes");
    TORCH_CHECK(partSize >= 0 && partSize <= std::numeric_limits<int>::max(), "partSize must not be negative");
    const bool parts = partSize > 0;
    const int64_t n = row_pointers.numel() - 1, nnz = column_index.numel(), k = nodes.numel();
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(row_pointers.device());
    const auto ids = row_pointers.options();
    const int64_t node_cap = std::min(k, n);
    int64_t edge_cap = 0;
    if (k > 0 && n > 0) {
        // the degree sum over the list (ids outside the graph are the library's to report)
        const auto rows = nodes.to(at::kLong).clamp(0, n - 1);
        const auto rp = row_pointers.to(at::kLong);
        edge_cap = std::min(nnz, (rp.index_select(0, rows + 1) - rp.index_select(0, rows)).clamp_min(0).sum().item<int64_t>());
    }
    const torch::Tensor sub_nodes = torch::empty({node_cap}, ids), sub_rp = torch::empty({node_cap + 1}, ids),
                        sub_ci = torch::empty({edge_cap}, ids);
    torch::Tensor eid, new_id, pp, p2n;
    if (want_edge_ids) eid = torch::empty({edge_cap}, ids);
    if (want_new_id) new_id = torch::empty({n}, ids);
    if (parts) { pp = torch::empty({edge_cap + 1}, ids); p2n = torch::empty({edge_cap}, ids); }
    auto ip = [](const torch::Tensor &t) { return t.defined() && t.numel() > 0 ? t.data_ptr<int32_t>() : nullptr; };
    int64_t counts[3] = {0, 0, 0};
    check_rc(gnna_induced_subgraph_i32(row_pointers.data_ptr<int32_t>(), ip(column_index), n, nnz, ip(nodes), k, (int)partSize,
                                       ip(sub_nodes), ip(new_id), sub_rp.data_ptr<int32_t>(), ip(sub_ci), ip(eid), ip(pp), ip(p2n),
                                       node_cap, edge_cap, counts, current_stream()));
    auto opt = [](const torch::Tensor &t, int64_t len) { return t.defined() ? c10::optional<torch::Tensor>(t.narrow(0, 0, len)) : c10::nullopt; };
    return std::make_tuple(sub_rp.narrow(0, 0, counts[0] + 1), sub_ci.narrow(0, 0, counts[1]), opt(eid, counts[1]),
                           sub_nodes.narrow(0, 0, counts[0]), opt(new_id, n), opt(pp, counts[2] + 1), opt(p2n, counts[2]));
}

// ---- graph construction from coordinates (gnna_spatial.hip) --------------------------------------------------------------------

// The radius / k-nearest-neighbour graph of every point set of a batch (gnna_radius_graph_f32) -> (row_pointers [N + 1],
// column_index [nnz'], dist2 [nnz'], partPtr [P + 1], part2Node [P]); None for what was not asked for (partSize = 0: no partition,
// max_neighbors = 0: no cap).  The arrays are trimmed views of buffers of min(U, max(2^22, 64 N)) edges, U = sum_g n_g *
// min(n_g - 1 + loop, max_neighbors or n_g); when that is too small the call is repeated once at the size it reported.
std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
radius_graph(const torch::Tensor &pos, const torch::Tensor &graph_pointers, double radius, int64_t max_neighbors, bool loop,
             int64_t partSize, bool want_dist2)
{
    TORCH_CHECK(pos.is_cuda(), "pos must be a CUDA tensor (the builder runs on the device)");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) >= 1 && pos.size(1) <= GNNA_SPATIAL_MAX_DIM, "pos must be 2-D [N, dim] with 1 .. ",
                GNNA_SPATIAL_MAX_DIM, " columns");
    check_f32(pos, "pos");
    check_rows(pos, "pos");
    check_device_ids(graph_pointers, "graph_pointers");
    TORCH_CHECK(graph_pointers.numel() >= 1 && graph_pointers.device() == pos.device(),
                "graph_pointers must be [num_graphs + 1] on pos's device");
    TORCH_CHECK(radius >= 0.0, "radius must be >= 0 or inf");
    TORCH_CHECK(max_neighbors >= 0 && max_neighbors <= GNNA_SPATIAL_MAX_NEIGHBORS, "max_neighbors must be in [0, ",
                GNNA_SPATIAL_MAX_NEIGHBORS, "] (0: no cap)");
    TORCH_CHECK(partSize >= 0 && partSize <= std::numeric_limits<int>::max(), "partSize must not be negative");
    const bool parts = partSize > 0;
    const int64_t n = pos.size(0), g = graph_pointers.numel() - 1;
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(pos.device());
    const auto ids = graph_pointers.options();
    int64_t edge_cap = 0;
    {
        const auto sizes = graph_pointers.to(at::kCPU).to(at::kLong).clamp(0, n).diff().clamp_min(0);
        auto per_row = (sizes - 1 + (loop ? 1 : 0)).clamp_min(0);
        if (max_neighbors > 0) per_row = per_row.clamp_max(max_neighbors);
        edge_cap = std::min<int64_t>((sizes * per_row).sum().item<int64_t>(), std::max<int64_t>((int64_t)1 << 22, 64 * n));
    }
    const torch::Tensor rp = torch::empty({n + 1}, ids);
    auto ip = [](const torch::Tensor &t) { return t.defined() && t.numel() > 0 ? t.data_ptr<int32_t>() : nullptr; };
    torch::Tensor ci, d2, pp, p2n;
    int64_t counts[3] = {0, 0, 0};
    for (int attempt = 0;; attempt++) {
        ci = torch::empty({edge_cap}, ids);
        if (want_dist2) d2 = torch::empty({edge_cap}, pos.options());
        if (parts) { pp = torch::empty({edge_cap + 1}, ids); p2n = torch::empty({edge_cap}, ids); }
        const int rc = gnna_radius_graph_f32(n > 0 ? pos.data_ptr<float>() : nullptr, ld_of(pos), n, (int)pos.size(1),
                                             graph_pointers.data_ptr<int32_t>(), g, (float)radius, (int)max_neighbors, loop ? 1 : 0,
                                             (int)partSize, rp.data_ptr<int32_t>(), ip(ci),
                                             want_dist2 && edge_cap > 0 ? d2.data_ptr<float>() : nullptr, ip(pp), ip(p2n), edge_cap,
                                             counts, current_stream());
        if (rc != GNNA_OK && attempt == 0 && counts[1] > edge_cap && counts[1] < ((int64_t)1 << 31)) {
            edge_cap = counts[1];                                          // once, from what it reported
            continue;
        }
        check_rc(rc);
        break;
    }
    auto opt = [](const torch::Tensor &t, int64_t len) { return t.defined() ? c10::optional<torch::Tensor>(t.narrow(0, 0, len)) : c10::nullopt; };
    return std::make_tuple(rp, ci.narrow(0, 0, counts[1]), opt(d2, counts[1]), opt(pp, counts[2] + 1), opt(p2n, counts[2]));
}

// what both row gathers check of their features, row ids and scale
static void gather_rows_check(const torch::Tensor &rows, const char *rows_name, const torch::Tensor &ids, const char *ids_name,
                              const c10::optional<torch::Tensor> &scale, int64_t scale_len)
{
    TORCH_CHECK(rows.is_cuda(), rows_name, " must be a CUDA tensor");
    TORCH_CHECK(rows.dim() == 2 && rows.size(1) >= 1, rows_name, " must be 2-D [rows, dim] with at least one column");
    check_f32(rows, rows_name);
    check_rows(rows, rows_name);
    check_device_ids(ids, ids_name);
    TORCH_CHECK(ids.device() == rows.device(), rows_name, " and ", ids_name, " must be on one device");
    if (scale.has_value()) {
        check_floats(*scale, "scale");
        TORCH_CHECK(scale->dim() == 1 && scale->numel() == scale_len && scale->device() == rows.device(),
                    "scale must be [num_nodes = ", scale_len, "] on ", rows_name, "'s device");
    }
}

// Scaled gather of rows (gnna_gather_rows_scale_ld_f32) -> out [perm.numel(), dim]: out[i] = scale[perm[i]] * input[perm[i]]; a
// plain gather without scale; a perm[i] outside the rows of input gives zeros.  Strided input as aggregate_ld.
torch::Tensor gather_rows_scale(const torch::Tensor &input, const torch::Tensor &perm, const c10::optional<torch::Tensor> &scale)
{
    gather_rows_check(input, "input", perm, "perm", scale, input.dim() == 2 ? input.size(0) : 0);
    const int64_t n = input.size(0), dim = input.size(1), m = perm.numel();
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(input.device());
    const torch::Tensor out = fresh({m, dim}, input.options());
    if (m == 0) return out;
    check_rc(gnna_gather_rows_scale_ld_f32(n > 0 ? input.data_ptr<float>() : nullptr, ld_of(input), n, perm.data_ptr<int32_t>(),
                                           scale.has_value() && n > 0 ? scale->data_ptr<float>() : nullptr, out.data_ptr<float>(), dim, m,
                                           (int)dim, current_stream()));
    return out;
}

// Backward of gather_rows_scale (gnna_gather_rows_scale_backward_ld_f32) -> (d_input [num_nodes, dim], d_scale [num_nodes]), None
// for the one that is not needed: a kept row r (0 <= new_id[r] < rows of d_out) gets scale[r] * d_out[new_id[r]] and
// <d_out[new_id[r]], input[r]>, every other row 0.  Without scale and d_scale: the unpooling of the rows of d_out.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
gather_rows_scale_backward(const torch::Tensor &d_out, const torch::Tensor &new_id, const c10::optional<torch::Tensor> &input,
                           const c10::optional<torch::Tensor> &scale, bool need_input, bool need_scale)
{
    gather_rows_check(d_out, "d_out", new_id, "new_id", scale, new_id.numel());
    TORCH_CHECK(need_input || need_scale, "neither d_input nor d_scale asked for");
    TORCH_CHECK(!need_scale || input.has_value(), "d_scale needs input");
    const int64_t m = d_out.size(0), dim = d_out.size(1), n = new_id.numel();
    if (need_scale) {
        CHECK_CUDA((*input));
        CHECK_F32((*input));
        TORCH_CHECK(input->dim() == 2 && input->size(0) == n && input->size(1) == dim && input->device() == d_out.device(),
                    "input must be [num_nodes, dim] on d_out's device");
        check_rows(*input, "input");
    }
    at::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(d_out.device());
    c10::optional<torch::Tensor> d_input, d_scale;
    if (need_input) d_input = fresh({n, dim}, d_out.options());
    if (need_scale) d_scale = fresh({n}, d_out.options());
    if (n == 0) return std::make_tuple(d_input, d_scale);
    check_rc(gnna_gather_rows_scale_backward_ld_f32(m > 0 ? d_out.data_ptr<float>() : nullptr, ld_of(d_out), m, new_id.data_ptr<int32_t>(),
                                                    need_scale ? input->data_ptr<float>() : nullptr, need_scale ? ld_of(*input) : dim,
                                                    scale.has_value() ? scale->data_ptr<float>() : nullptr,
                                                    need_input ? d_input->data_ptr<float>() : nullptr, dim,
                                                    need_scale ? d_scale->data_ptr<float>() : nullptr, n, (int)dim, current_stream()));
    return std::make_tuple(d_input, d_scale);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.def("SAG", &SAG, "GNNAdvisor base Scatter-and-Gather Kernel (HIP, gfx950)");
    m.def("forward", &spmm_forward, "GNNAdvisor forward (HIP, gfx950)");
    m.def("backward", &spmm_backward, "GNNAdvisor backward (HIP, gfx950)");
    m.def("xtg", [](torch::Tensor X, torch::Tensor G) { CHECK_CUDA(X); CHECK_CUDA(G); return xtg(X, G); },
          "X^T G, the weight gradient of the dense update, on the MFMA units (extension)");
    m.def("aggregate_gin", &aggregate_gin, "eps * A * input (extension)");
    m.def("backward_weight", &spmm_backward_weight, "GNNAdvisor backward, d_weight only (extension)");
    m.def("forward_gin", &spmm_forward_gin, "GNNAdvisor forward GIN (HIP, gfx950)");
    m.def("backward_gin", &spmm_backward_gin, "GNNAdvisor backward GIN (HIP, gfx950)");
    m.def("aggregate_ld", &aggregate_general,
          "general aggregation (extension): mode 0 sag / 1 gcn / 2 gin; input and out may be row-strided views; "
          "accumulate adds into out; relu clamps the result at zero in the same call.  bfloat16 / float16 input is accumulated "
          "in fp32 (degrees stay float32) and returned as out_dtype: float32 or the input's dtype (the default)",
          pybind11::arg("mode"), pybind11::arg("input"), pybind11::arg("column_index"), pybind11::arg("degrees"),
          pybind11::arg("epsilon"), pybind11::arg("part_pointers"), pybind11::arg("part2Node"), pybind11::arg("partSize"),
          pybind11::arg("out") = pybind11::none(), pybind11::arg("accumulate") = false, pybind11::arg("relu") = false,
          pybind11::arg("out_dtype") = pybind11::none());
    m.def("aggregate_edge", &aggregate_edge,
          "edge-weighted aggregation (extension): out[i] (+)= sum_e edge_weight[e] * X[column_index[e]], edge_weight indexed like "
          "column_index; X and out may be row-strided views",
          pybind11::arg("X"), pybind11::arg("column_index"), pybind11::arg("edge_weight"), pybind11::arg("partPtr"),
          pybind11::arg("part2Node"), pybind11::arg("partSize"), pybind11::arg("out") = pybind11::none(),
          pybind11::arg("accumulate") = false, pybind11::arg("relu") = false);
    m.def("aggregate_reduce", &aggregate_reduce,
          "element-wise max (op 0) / min (op 1) over every row's neighbours (extension) -> (out, arg): arg[i, f] is the position in "
          "column_index that supplied out[i, f], the smallest one among ties; rows without edges give 0 and -1",
          pybind11::arg("op"), pybind11::arg("X"), pybind11::arg("column_index"), pybind11::arg("partPtr"),
          pybind11::arg("part2Node"), pybind11::arg("partSize"), pybind11::arg("out") = pybind11::none(),
          pybind11::arg("want_arg") = true, pybind11::arg("relu") = false);
    m.def("aggregate_stats", &aggregate_stats,
          "sum, sum of squares, max and min over every row's neighbours from one gather (extension) -> (sum, sumsq, max, argmax, min, "
          "argmin); None for what was not asked for; the extrema are aggregate_reduce's bits",
          pybind11::arg("X"), pybind11::arg("column_index"), pybind11::arg("partPtr"), pybind11::arg("part2Node"),
          pybind11::arg("partSize"), pybind11::arg("num_out_rows") = -1, pybind11::arg("want_sum") = true,
          pybind11::arg("want_sumsq") = true, pybind11::arg("want_max") = true, pybind11::arg("want_min") = true);
    m.def("aggregate_softmax", &aggregate_softmax,
          "softmax aggregation with a temperature, per channel, in one gather (extension) -> (out, lse, sq): over the edges i <- j of "
          "row i, lse[i, f] = logsumexp_j temp[f] * X[j, f], out = sum_j alpha X[j], sq = sum_j alpha X[j]^2 (None unless want_sq); "
          "temp has 1 or dim elements; rows without edges give 0",
          pybind11::arg("X"), pybind11::arg("temp"), pybind11::arg("row_pointers"), pybind11::arg("column_index"),
          pybind11::arg("want_sq") = false);
    m.def("aggregate_softmax_backward", &aggregate_softmax_backward,
          "backward of aggregate_softmax (extension): dX[j, f] = sum over the transposed edges j <- i of exp(temp[f] X[j, f] - lse[i, f]) "
          "dY[i, f] (1 + temp[f] (X[j, f] - Y[i, f]))",
          pybind11::arg("X"), pybind11::arg("temp"), pybind11::arg("lse"), pybind11::arg("Y"), pybind11::arg("dY"),
          pybind11::arg("t_row_pointers"), pybind11::arg("t_column_index"));
    m.def("aggregate_edge_feat", &aggregate_edge_feat,
          "message passing with a feature row per edge, in one gather (extension) -> out: out[i, f] = sum over the positions e of row i "
          "of act(X[column_index[e], f] (+ | *) E[e, f]); combine 0 add, 1 multiply; act 0 none, 1 relu; E is [nnz, dim], edge-major",
          pybind11::arg("X"), pybind11::arg("E"), pybind11::arg("row_pointers"), pybind11::arg("column_index"),
          pybind11::arg("combine") = 0, pybind11::arg("act") = 0);
    m.def("aggregate_edge_feat_backward", &aggregate_edge_feat_backward,
          "backward of aggregate_edge_feat (extension) -> (dX | None, dE | None); the relu mask is recomputed from X and E; dX runs over "
          "the transposed structure with t_edge_pos (transpose_csr's perm, or the reverse-edge map of a symmetric structure)",
          pybind11::arg("X"), pybind11::arg("E"), pybind11::arg("dY"), pybind11::arg("row_pointers"), pybind11::arg("column_index"),
          pybind11::arg("t_row_pointers") = pybind11::none(), pybind11::arg("t_column_index") = pybind11::none(),
          pybind11::arg("t_edge_pos") = pybind11::none(), pybind11::arg("combine") = 0, pybind11::arg("act") = 0,
          pybind11::arg("want_dx") = true, pybind11::arg("want_de") = true);
    m.def("segment_pool", &segment_pool,
          "graph-level readout (extension) -> (sum, max, argmax, min, argmin), each [num_graphs, dim]: over the rows "
          "[graph_pointers[g], graph_pointers[g + 1]) of X, from one read of X; argmax / argmin are the winning rows (-1 and the value 0 "
          "for a graph without rows); mean divides the sum by the rows of the graph; None for what was not asked for",
          pybind11::arg("X"), pybind11::arg("graph_pointers"), pybind11::arg("want_sum") = true, pybind11::arg("want_max") = false,
          pybind11::arg("want_min") = false, pybind11::arg("mean") = false);
    m.def("segment_pool_backward", &segment_pool_backward,
          "backward of segment_pool (extension): dX[r, f] = s d_sum[g, f] + (argmax[g, f] == r) d_max[g, f] + (argmin[g, f] == r) "
          "d_min[g, f] for the rows r of graph g, s = 1 or 1 / rows with mean; one pass that writes every row, 0 for a row of no graph",
          pybind11::arg("d_sum"), pybind11::arg("d_max"), pybind11::arg("argmax"), pybind11::arg("d_min"), pybind11::arg("argmin"),
          pybind11::arg("graph_pointers"), pybind11::arg("num_rows"), pybind11::arg("mean") = false);
    m.def("segment_attn_pool", &segment_attn_pool,
          "attention readout (extension) -> (out [num_graphs, dim], lse [num_graphs, gate_dim]): over the rows r in "
          "[graph_pointers[g], graph_pointers[g + 1]) of X, lse[g, c] = logsumexp_r gate[r, c] and out[g, f] = sum_r exp(gate[r, c] - "
          "lse[g, c]) X[r, f], from one read of X and gate; gate is [num_nodes, 1] (a score per row) or [num_nodes, dim] (a score per "
          "element) and may be X itself; a graph without rows gives 0",
          pybind11::arg("X"), pybind11::arg("gate"), pybind11::arg("graph_pointers"));
    m.def("segment_attn_pool_backward", &segment_attn_pool_backward,
          "backward of segment_attn_pool (extension) -> (d_input, d_gate), None for the one not needed: with alpha = exp(gate[r, c] - "
          "lse[g, c]), d_input[r, f] = alpha dY[g, f] and d_gate[r, c] = alpha dY[g, f] (X[r, f] - Y[g, f]), summed over f for a score "
          "per row; one pass that writes every row, 0 for a row of no graph",
          pybind11::arg("X"), pybind11::arg("gate"), pybind11::arg("lse"), pybind11::arg("Y"), pybind11::arg("dY"),
          pybind11::arg("graph_pointers"), pybind11::arg("need_input") = true, pybind11::arg("need_gate") = true);
    m.def("segment_moments", &segment_moments,
          "centred moments per graph (extension) -> (mean, m2), each [num_graphs, dim]: over the rows [graph_pointers[g], "
          "graph_pointers[g + 1]) of X, mean and sum (x - mean)^2 from one read of X, merged pairwise (never from sums of x^2); 0 for a "
          "graph without rows",
          pybind11::arg("X"), pybind11::arg("graph_pointers"));
    m.def("segment_norm", &segment_norm,
          "per-graph normalisation, GraphNorm (extension) -> (out like X, mean, rstd [num_graphs, dim]): out[r, f] = weight (x - alpha "
          "mean) rstd + bias with rstd = 1 / sqrt(m2 / n + (1 - alpha)^2 mean^2 + eps) over the rows of graph g; weight / bias / alpha "
          "[dim] or None for 1 / 0 / 1; 0 for a row of no graph",
          pybind11::arg("X"), pybind11::arg("graph_pointers"), pybind11::arg("weight") = pybind11::none(),
          pybind11::arg("bias") = pybind11::none(), pybind11::arg("alpha") = pybind11::none(), pybind11::arg("eps") = 1e-5);
    m.def("segment_norm_backward", &segment_norm_backward,
          "backward of segment_norm (extension) -> (d_input | None, seg_a, seg_b): seg_a = sum dY and seg_b = sum dY xhat over the rows of "
          "every graph, then d_input in one pass that writes every row, 0 for a row of no graph",
          pybind11::arg("dY"), pybind11::arg("X"), pybind11::arg("mean"), pybind11::arg("rstd"), pybind11::arg("graph_pointers"),
          pybind11::arg("weight") = pybind11::none(), pybind11::arg("alpha") = pybind11::none(), pybind11::arg("need_input") = true);
    m.def("segment_topk", &segment_topk,
          "top-k rows per graph of a batch and the induced sub-batch (extension) -> (new_id [N], perm [N'], new_graph_pointers [G + 1], "
          "new_row_pointers, new_column_index, edge_ids, partPtr, part2Node): every graph keeps its min(n, ceil(ratio * n)) -- or "
          "min(n, k) -- best-scoring rows in the library's total order, ties to the smaller row, in increasing row order; None for what "
          "was not asked for.  One stream synchronisation; not capturable",
          pybind11::arg("score"), pybind11::arg("graph_pointers"), pybind11::arg("ratio") = 0.0, pybind11::arg("k") = 0,
          pybind11::arg("row_pointers") = pybind11::none(), pybind11::arg("column_index") = pybind11::none(),
          pybind11::arg("partSize") = 0, pybind11::arg("want_edge_ids") = false);
    m.def("random_walk", &random_walk,
          "uniform first-order random walks on the device (extension) -> (walks [R, walk_length + 1], edge_ids [R, walk_length] | None): "
          "step t of walk w takes position lo + floor(key * d / 2^64) of its row, key = the splitmix64 key of w * walk_length + t "
          "under rng_seed; a row without positions or an edge out of the graph makes the walk stay (edge id -1).  No "
          "synchronisation; capturable",
          pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("roots"), pybind11::arg("walk_length"),
          pybind11::arg("rng_seed"), pybind11::arg("want_edge_ids") = false);
    m.def("induced_subgraph", &induced_subgraph,
          "the subgraph a node list induces (extension) -> (row_pointers, column_index, edge_ids, nodes, new_id, partPtr, part2Node): "
          "the kept nodes are the distinct ids of the list in increasing global id (-1 skipped), every row keeps the positions whose "
          "column is kept, in increasing position; None for what was not asked for.  One stream synchronisation; not capturable",
          pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("nodes"), pybind11::arg("partSize") = 0,
          pybind11::arg("want_edge_ids") = true, pybind11::arg("want_new_id") = false);
    m.def("radius_graph", &radius_graph,
          "the radius / k-nearest-neighbour graph of every point set of a batch (extension) -> (row_pointers, column_index, dist2, "
          "partPtr, part2Node): row i keeps the rows j of its set with sum_c (pos[j, c] - pos[i, c])^2 <= radius^2 in fp32, under "
          "max_neighbors > 0 the that many with the smallest (d2, j), in increasing j; None for what was not asked for.  One stream "
          "synchronisation; not capturable",
          pybind11::arg("pos"), pybind11::arg("graph_pointers"), pybind11::arg("radius"), pybind11::arg("max_neighbors") = 0,
          pybind11::arg("loop") = false, pybind11::arg("partSize") = 0, pybind11::arg("want_dist2") = true);
    m.def("gather_rows_scale", &gather_rows_scale,
          "out[i] = scale[perm[i]] * input[perm[i]] (extension) -> out [perm.numel(), dim]; a plain gather without scale; a perm[i] "
          "outside the rows of input gives a row of zeros",
          pybind11::arg("input"), pybind11::arg("perm"), pybind11::arg("scale") = pybind11::none());
    m.def("gather_rows_scale_backward", &gather_rows_scale_backward,
          "backward of gather_rows_scale (extension) -> (d_input, d_scale), None for the one not needed: a kept row r gets "
          "scale[r] * d_out[new_id[r]] and <d_out[new_id[r]], input[r]>, every other row 0; without scale and d_scale it is the "
          "unpooling of the rows of d_out",
          pybind11::arg("d_out"), pybind11::arg("new_id"), pybind11::arg("input") = pybind11::none(),
          pybind11::arg("scale") = pybind11::none(), pybind11::arg("need_input") = true, pybind11::arg("need_scale") = true);
    m.def("scatter_arg", &scatter_arg,
          "backward of aggregate_reduce (extension): grad_in[column_index[arg[i, f]], f] += grad_out[i, f] for arg >= 0",
          pybind11::arg("grad_out"), pybind11::arg("arg"), pybind11::arg("column_index"), pybind11::arg("num_in_rows"));
    m.def("edge_softmax", &edge_softmax, "softmax over every row's edges; scores [nnz] or [heads, nnz] (extension)",
          pybind11::arg("scores"), pybind11::arg("row_pointers"));
    m.def("edge_softmax_backward", &edge_softmax_backward, "gradient of edge_softmax: probs * (grad - sum_row probs * grad) (extension)",
          pybind11::arg("probs"), pybind11::arg("grad"), pybind11::arg("row_pointers"));
    m.def("gat_forward", &gat_forward,
          "fused multi-head GAT attention -> (Y, lse): Y[i, h] = sum_e exp(leaky_relu(el[i, h] + er[col(e), h]) - lse[i, h]) H[col(e), h] (extension).  "
          "Rectangular structures: H [num_in_rows, heads * dim], er [num_in_rows, heads], el [num_out_rows, heads], row_pointers [num_out_rows + 1]",
          pybind11::arg("H"), pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("row_pointers"), pybind11::arg("column_index"),
          pybind11::arg("part_pointers"), pybind11::arg("part2Node"), pybind11::arg("partSize"), pybind11::arg("negative_slope") = 0.2);
    m.def("gat_backward", &gat_backward,
          "gradient of gat_forward -> (dH, d_el, d_er); dH is the attention part only (extension).  The structure must be symmetric "
          "unless transposed = [t_row_pointers, t_column_index, t_part_pointers, t_part2Node] (transpose_csr, build_part_device) is given; "
          "a rectangular structure (el.size(0) != H.size(0)) always needs it: dH / d_er get num_in_rows rows, d_el num_out_rows",
          pybind11::arg("H"), pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("lse"), pybind11::arg("Y"), pybind11::arg("dY"),
          pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("part_pointers"), pybind11::arg("part2Node"),
          pybind11::arg("partSize"), pybind11::arg("negative_slope") = 0.2, pybind11::arg("transposed") = pybind11::none());
    m.def("gat_forward_drop", &gat_forward_drop,
          "gat_forward with attention dropout (extension; gnna_ext.h): every alpha is scaled by k(rng_seed, i, j, h) = 0 or "
          "1 / (1 - attn_drop), a function of the seed, the two row numbers and the head that every pass recomputes; lse is that of "
          "the undropped scores.  attn_drop in [0, 1)",
          pybind11::arg("H"), pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("row_pointers"), pybind11::arg("column_index"),
          pybind11::arg("part_pointers"), pybind11::arg("part2Node"), pybind11::arg("partSize"), pybind11::arg("negative_slope"),
          pybind11::arg("attn_drop"), pybind11::arg("rng_seed"));
    m.def("gat_backward_drop", &gat_backward_drop,
          "gradient of gat_forward_drop for the same attn_drop and rng_seed -> (dH, d_el, d_er) (extension; gnna_ext.h); `transposed` "
          "as for gat_backward",
          pybind11::arg("H"), pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("lse"), pybind11::arg("Y"), pybind11::arg("dY"),
          pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("part_pointers"), pybind11::arg("part2Node"),
          pybind11::arg("partSize"), pybind11::arg("negative_slope"), pybind11::arg("attn_drop"), pybind11::arg("rng_seed"),
          pybind11::arg("transposed") = pybind11::none());
    m.def("gat_edge_forward", &gat_edge_forward,
          "gat_forward_drop with a per-edge score term (extension; gnna_gat_edge.h): z = el[i, h] + er[col(e), h] + ee[e, h]; "
          "ee [num_edges, heads], edge-major, indexed like column_index -> (Y, lse)",
          pybind11::arg("H"), pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("ee"), pybind11::arg("row_pointers"),
          pybind11::arg("column_index"), pybind11::arg("part_pointers"), pybind11::arg("part2Node"), pybind11::arg("partSize"),
          pybind11::arg("negative_slope") = 0.2, pybind11::arg("attn_drop") = 0.0, pybind11::arg("rng_seed") = 0);
    m.def("gat_edge_backward", &gat_edge_backward,
          "gradient of gat_edge_forward for the same ee, attn_drop and rng_seed -> (dH, d_el, d_er, d_ee) (extension; gnna_gat_edge.h).  "
          "t_edge_pos [num_edges]: the forward position of every position of the transposed structure (transpose_csr's t_perm with "
          "`transposed`, the reverse-edge map of a symmetric graph without)",
          pybind11::arg("H"), pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("ee"), pybind11::arg("lse"), pybind11::arg("Y"),
          pybind11::arg("dY"), pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("part_pointers"),
          pybind11::arg("part2Node"), pybind11::arg("t_edge_pos"), pybind11::arg("partSize"), pybind11::arg("negative_slope") = 0.2,
          pybind11::arg("attn_drop") = 0.0, pybind11::arg("rng_seed") = 0, pybind11::arg("transposed") = pybind11::none());
    m.def("gat_alpha", &gat_alpha,
          "attention coefficients edge for edge (extension; gnna_gat_edge.h) -> alpha [num_edges, heads] = exp(leaky_relu(el[i, h] + "
          "er[col(e), h] + ee[e, h]) - lse[i, h]), undropped, 0 for a skipped edge; ee None: those of gat_forward",
          pybind11::arg("el"), pybind11::arg("er"), pybind11::arg("ee"), pybind11::arg("lse"), pybind11::arg("row_pointers"),
          pybind11::arg("column_index"), pybind11::arg("negative_slope") = 0.2);
    m.def("gatv2_forward", &gatv2_forward,
          "fused multi-head GATv2 attention -> (Y, lse) (extension; gnna_gatv2.h): z = sum_d att[h, d] * leaky_relu(Hs[col(e), h, d] + "
          "Hd[i, h, d]), Y[i, h] = sum_e exp(z - lse[i, h]) * k * Hs[col(e), h] with the dropout factor k of gat_forward_drop (1 at "
          "attn_drop = 0).  Hs [num_in_rows, heads * dim], Hd [num_out_rows, heads * dim], att [heads, dim], row_pointers [num_out_rows + 1]",
          pybind11::arg("Hs"), pybind11::arg("Hd"), pybind11::arg("att"), pybind11::arg("row_pointers"), pybind11::arg("column_index"),
          pybind11::arg("part_pointers"), pybind11::arg("part2Node"), pybind11::arg("partSize"), pybind11::arg("negative_slope") = 0.2,
          pybind11::arg("attn_drop") = 0.0, pybind11::arg("rng_seed") = 0);
    m.def("gatv2_backward", &gatv2_backward,
          "gradient of gatv2_forward for the same attn_drop and rng_seed -> (dHs, dHd, d_att) (extension; gnna_gatv2.h); `transposed` "
          "as for gat_backward",
          pybind11::arg("Hs"), pybind11::arg("Hd"), pybind11::arg("att"), pybind11::arg("lse"), pybind11::arg("Y"), pybind11::arg("dY"),
          pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("part_pointers"), pybind11::arg("part2Node"),
          pybind11::arg("partSize"), pybind11::arg("negative_slope") = 0.2, pybind11::arg("attn_drop") = 0.0, pybind11::arg("rng_seed") = 0,
          pybind11::arg("transposed") = pybind11::none());
    m.def("dot_attn_forward", &dot_attn_forward,
          "fused multi-head scaled dot-product graph attention -> (Y, lse) (extension; gnna_dotattn.h): z = scale * <Q[i, h], K[col(e), h]>, "
          "Y[i, h] = sum_e exp(z - lse[i, h]) * k * V[col(e), h] with the dropout factor k of gat_forward_drop (1 at attn_drop = 0).  "
          "Q [num_out_rows, heads * dim], K and V [num_in_rows, heads * dim] (row-strided views are passed as they are), "
          "row_pointers [num_out_rows + 1]",
          pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("heads"), pybind11::arg("row_pointers"),
          pybind11::arg("column_index"), pybind11::arg("part_pointers"), pybind11::arg("part2Node"), pybind11::arg("partSize"),
          pybind11::arg("scale"), pybind11::arg("attn_drop") = 0.0, pybind11::arg("rng_seed") = 0);
    m.def("dot_attn_backward", &dot_attn_backward,
          "gradient of dot_attn_forward for the same scale, attn_drop and rng_seed -> (dQ, dK, dV) (extension; gnna_dotattn.h); "
          "`transposed` as for gat_backward",
          pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("heads"), pybind11::arg("lse"), pybind11::arg("Y"),
          pybind11::arg("dY"), pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("part_pointers"),
          pybind11::arg("part2Node"), pybind11::arg("partSize"), pybind11::arg("scale"), pybind11::arg("attn_drop") = 0.0,
          pybind11::arg("rng_seed") = 0, pybind11::arg("transposed") = pybind11::none());
    m.def("transpose_csr", &transpose_csr,
          "device-built CSR of A^T (extension) -> [t_row_pointers, t_column_index, t_perm]: row j lists the rows i of the edges i <- j in "
          "increasing position e, t_perm[p] = e (a stable argsort of column_index); ids outside [0, num_in_rows) are dropped",
          pybind11::arg("row_pointers"), pybind11::arg("column_index"), pybind11::arg("num_in_rows") = pybind11::none(),
          pybind11::arg("want_perm") = true);
    m.def("build_part_device", &build_part_device, "neighbor-group partitioner for device row pointers (extension): what build_part "
          "returns, on the device", pybind11::arg("partSize"), pybind11::arg("indptr"));
    m.def("sddmm", &sddmm, "edge_out[e] = <A[row(e)], B[column_index[e]]> over the neighbor-group partition (extension)",
          pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("column_index"), pybind11::arg("partPtr"), pybind11::arg("part2Node"),
          pybind11::arg("partSize"));
    m.def("build_part", &build_part, "GNNAdvisor neighbor-group partitioner (CPU)", pybind11::arg("partSize"),
          pybind11::arg("indptr"), pybind11::arg("float_compat") = false);
#ifndef GNNA_SOURCE_HASH
#define GNNA_SOURCE_HASH "unhashed"
#endif
    m.def("forget_graph", &forget_graph,
          "forget every plan, packed id copy and hint kept for this column_index (extension): call it after writing into a graph's "
          "arrays in a way torch's version counter does not see (`t.data[...] = ...`, raw pointers)", pybind11::arg("column_index"));
    m.def("auto_prepared_graphs", []() { return (long long)g_auto_prepared.load(); },
          "how many (graph, width) pairs the module prepared by itself once they had stood still for three calls (extension; see note_graph)");
    m.def("build_id", []() { return std::string("module ") + GNNA_SOURCE_HASH + ", library " + gnna_build_id(); },
          "source hashes this module and the libgnna.so it loaded were built from (extension)");
}

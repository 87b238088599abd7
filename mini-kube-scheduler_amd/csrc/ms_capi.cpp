// ms_capi.cpp — C ABI of the scheduling-cycle engine (include/minisched_gpu.h):
// the context's life cycle, node deltas, info, single binds, and the guard
// every ordered device call goes through. The cycles are in ms_cycle.cpp,
// ms_seq_host.cpp and ms_hostarray.cpp, the NodeAffinity tables in ms_nam_tab.cpp.
//
// Owns one device's node table (a shard of global ordinals), the node-delta
// queue fed by informer callbacks, pinned staging for the cgo caller, and the
// stream everything is ordered on. It never aborts: every HIP failure becomes
// MS_E_HIP with the message kept for ms_last_error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "ms_ctx.h"

using namespace msgpu;

// What must happen in order before the members release themselves (ms_ctx.h).
ms_ctx::~ms_ctx() {
    (void)hipSetDevice(cfg.device);
    comm_free(this);
    if (stream) (void)hipStreamSynchronize(stream);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
}

namespace msgpu {

namespace {
thread_local std::string g_create_err;
}  // namespace

int fail(ms_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    else g_create_err = msg;
    return code;
}

// Every grow routine (here and in the cycle files) keeps its capacity at zero
// while its group of buffers is not whole, so a failed growth is retried by
// the next call.

// Delta staging for n records. No synchronise of its own: the runtime's free of
// the old blocks waits for the work that used them (flush_locked's comes after).
int ensure_delta_cap(ms_ctx *c, uint32_t n) {
    if (n <= c->delta_cap) return MS_OK;
    uint32_t cap = std::max<uint32_t>(n, std::max<uint32_t>(1024, c->delta_cap * 2));
    c->delta_cap = 0;
    if (!c->h_deltas.alloc(cap)) return fail(c, MS_E_OOM, "pinned delta staging");
    if (!c->d_deltas.alloc(cap)) return fail(c, MS_E_OOM, "device delta staging");
    c->delta_cap = cap;
    return MS_OK;
}

// The context stream waits for the node-sharded sweeps still reading the table
// (comm_fence_reads), before work that writes it: 1 if waits were inserted (the
// ordering class counts them: caller streams ordered earlier wait again), 0 if
// none were outstanding, < 0 on failure.
static int fence_ctx(ms_ctx *c) {
    const int fenced = comm_fence_reads(c, c->stream);
    if (fenced > 0) c->order.fenced();
    return fenced;
}

// Drains the delta queue onto the stream (caller holds sched_mu).
int flush_locked(ms_ctx *c) {
    std::vector<NodeDelta> batch;
    {
        std::lock_guard<std::mutex> g(c->delta_mu);
        batch.swap(c->pending);
        c->rows_dev = c->rows_used;
        c->present_dev = c->present_count;
    }
    if (batch.empty()) return MS_OK;
    // the deltas land on the context stream: after the sweeps still reading the
    // table on the communicator's streams
    const int fenced = fence_ctx(c);
    if (fenced < 0) return fenced;
    // later deltas to one row win: keep the last occurrence only
    std::unordered_map<uint32_t, uint32_t> last;
    last.reserve(batch.size() * 2);
    for (uint32_t i = 0; i < batch.size(); ++i) last[batch[i].local] = i;
    std::vector<NodeDelta> uniq;
    uniq.reserve(last.size());
    for (uint32_t i = 0; i < batch.size(); ++i)
        if (last[batch[i].local] == i) uniq.push_back(batch[i]);
    int rc = ensure_delta_cap(c, (uint32_t)uniq.size());
    if (rc) return rc;
    // the previous use of h_deltas must be complete before it is overwritten
    MS_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(c->h_deltas, uniq.data(), sizeof(NodeDelta) * uniq.size());
    MS_HIP(c, hipMemcpyAsync(c->d_deltas, c->h_deltas, sizeof(NodeDelta) * uniq.size(),
                             hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, launch_apply_deltas(c->t, c->d_deltas, (uint32_t)uniq.size(), c->stream));
    MS_HIP(c, launch_build_planes(c->t, c->d_cand, c->d_deltas, (uint32_t)uniq.size(), c->stream));
    c->order.wrote_ctx();
    return MS_OK;
}

hipStream_t pick_stream(ms_ctx *c, void *s) { return s ? (hipStream_t)s : c->stream; }

static int order_failed(ms_ctx *c) {
    return fail(c, MS_E_HIP, std::string("stream ordering: ") + hipGetErrorString(hipGetLastError()));
}

// The prologue of an ordered device call (ms_ctx.h); the lock is held until the
// guard dies, whatever the prologue's status.
OrderedCall::OrderedCall(ms_ctx *c, void *stream, bool flush) : c_(c), g_(c->sched_mu) {
    rc_ = [&]() -> int {
        MS_HIP(c, hipSetDevice(c->cfg.device));
        if (flush) {
            const int rc = flush_locked(c);
            if (rc) return rc;
        }
        s_ = pick_stream(c, stream);
        const int fenced = comm_fence_reads(c, c->stream);
        if (fenced < 0) return fenced;
        if (!c->order.enter(s_, fenced > 0)) return order_failed(c);
        if (s_ != c->stream) {
            MS_HIP(c, made(c->order.back_event().ensure()));
            back_ = c->order.back_event();
        }
        return MS_OK;
    }();
}

int OrderedCall::done(bool recorded) { return c_->order.leave(s_, recorded) ? MS_OK : order_failed(c_); }

// Plugin sets whose filters and scores read no mutable node state (NU, NN,
// NodeAffinity): a bind never changes a later pod's outcome, so chunks of a
// call, or the queue-order loop, equal one batched sweep.
bool plugins_stateless(const ms_ctx *c) { return c->cfg.plugin_set != MS_PLUGINS_NU_NRF_NN_LA; }

// Pod / result staging for at least n pods (grown on demand). No synchronise
// of its own: the runtime's free of the old device blocks waits for the
// device, so no in-flight call still uses them.
int ensure_stage(ms_ctx *c, uint32_t n) {
    if (n <= c->stage_cap) return MS_OK;
    c->stage_cap = 0;
    if (!c->d_pods.alloc(n) || !c->d_res.alloc(n)) return fail(c, MS_E_OOM, "pod staging");
    c->stage_cap = n;
    return MS_OK;
}

}  // namespace msgpu

extern "C" {

int ms_abi_version(void) { return MS_ABI_VERSION; }

int ms_device_count(int *out) {
    if (!out) return MS_E_INVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return MS_OK;
}

int ms_create(const ms_config *cfg, ms_ctx **out) {
    if (!cfg || !out) return fail(nullptr, MS_E_INVAL, "ms_create: null argument");
    *out = nullptr;
    if (cfg->plugin_set != MS_PLUGINS_NU_NN && cfg->plugin_set != MS_PLUGINS_NU_NRF_NN_LA &&
        cfg->plugin_set != MS_PLUGINS_NU_NN_NA && cfg->plugin_set != MS_PLUGINS_NU_TT_NN &&
        cfg->plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(nullptr, MS_E_INVAL, "ms_create: unknown plugin_set");
    const uint32_t w0 = cfg->score_weight[0] ? cfg->score_weight[0] : 1u;
    const uint32_t w1 = cfg->score_weight[1] ? cfg->score_weight[1] : 1u;
    if (cfg->plugin_set != MS_PLUGINS_NU_NN_NA && cfg->plugin_set != MS_PLUGINS_NU_NN_NAM && (w0 != 1 || w1 != 1))
        return fail(nullptr, MS_E_INVAL, "ms_create: score weights apply to MS_PLUGINS_NU_NN_NA / _NAM only");
    if (w0 * 10u + w1 * 100u >= 2048u)
        return fail(nullptr, MS_E_INVAL, "ms_create: weighted score must stay below 2048 (packed key)");
    if (cfg->max_nodes == 0 || (uint64_t)cfg->node_base + cfg->max_nodes > (uint64_t)MS_MAX_ORDINAL + 1)
        return fail(nullptr, MS_E_INVAL, "ms_create: node range must be non-empty and end at or below 0xFFFFF");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, MS_E_NODEV, "ms_create: no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MS_E_NODEV, "ms_create: device out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, MS_E_NODEV, "ms_create: hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MS_E_NODEV, std::string("ms_create: built for gfx950, device is ") + prop.gcnArchName);

    ms_ctx *c = new (std::nothrow) ms_ctx();
    if (!c) return fail(nullptr, MS_E_OOM, "ms_create: host allocation");
    c->cfg = *cfg;
    if (c->cfg.max_batch == 0) c->cfg.max_batch = 1u << 16;
    c->num_cus = prop.multiProcessorCount;
    c->w_nn = w0;
    c->w_na = w1;
    c->batch_cap = c->cfg.max_batch;
    c->present.assign(cfg->max_nodes, 0);

    auto bail = [&](int code, const char *what) {
        std::string m = std::string("ms_create: ") + what;
        delete c;
        return fail(nullptr, code, m);
    };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(MS_E_HIP, "hipSetDevice");
    if (!c->stream.ensure(hipStreamNonBlocking)) return bail(MS_E_HIP, "stream creation");
    c->order.attach(c->stream);
    const size_t n = cfg->max_nodes;
    NodeTable &t = c->t;
    t.cap = cfg->max_nodes;
    t.base = cfg->node_base;
    // Every column in one allocation, 2 MB-rounded: the validator's write-back
    // stores one scattered row per lane into five of them each step, and
    // separate allocations spread those rows over many more translation entries.
    void **cols[] = {(void **)&t.flags,     (void **)&t.digit,     (void **)&t.zone,    (void **)&t.label2,
                     (void **)&t.taints,    (void **)&t.allowed_pods, (void **)&t.pod_count, (void **)&t.alloc_cpu,
                     (void **)&t.alloc_mem, (void **)&t.req_cpu,   (void **)&t.req_mem, (void **)&t.nz_cpu,
                     (void **)&t.nz_mem};
    const size_t bytes[] = {n + kColumnPad, n + kColumnPad, n + kColumnPad, n + kColumnPad, n * 4, n * 4, n * 4,
                            n * 8,          n * 8,          n * 8,          n * 8,          n * 8, n * 8};
    static_assert(sizeof(cols) / sizeof(cols[0]) == sizeof(bytes) / sizeof(bytes[0]), "one size per column");
    size_t off[sizeof(bytes) / sizeof(bytes[0])], total = 0;
    for (size_t i = 0; i < sizeof(bytes) / sizeof(bytes[0]); ++i) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    total = (total + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    bool ok = c->d_table.alloc(total);
    if (ok)
        for (size_t i = 0; i < sizeof(bytes) / sizeof(bytes[0]); ++i)
            *cols[i] = static_cast<char *>(c->d_table.get()) + off[i];
    t.gcap = (uint32_t)((n + kGroupRows - 1) / kGroupRows);
    ok = ok && c->d_planes.alloc((size_t)kPlanes * t.gcap) && c->d_cand.alloc(cand_words(t.cap));
    if (!ok) return bail(MS_E_OOM, "node table allocation");
    t.planes = c->d_planes;
    const size_t b = c->batch_cap;
    ok = ensure_stage(c, c->batch_cap) == MS_OK && c->d_keys.alloc(b) && c->d_flags.alloc(b) && c->d_one.alloc(1) &&
         c->d_overflow.alloc(kStatsBytes / sizeof(uint32_t));
    if (!ok) return bail(MS_E_OOM, "staging allocation");
    if (launch_init_table(t, c->stream) != hipSuccess || launch_build_planes(t, c->d_cand, nullptr, 0, c->stream) != hipSuccess)
        return bail(MS_E_HIP, "table init launch");
    if (hipMemsetAsync(c->d_overflow, 0, kStatsBytes, c->stream) != hipSuccess) return bail(MS_E_HIP, "memset");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(MS_E_HIP, "table init");
    *out = c;
    return MS_OK;
}

int ms_destroy(ms_ctx *c) {
    if (!c) return MS_E_INVAL;
    seq_diag_readout(c);  // (the diagnostic builds; nothing in the product)
    delete c;
    return MS_OK;
}

const char *ms_last_error(const ms_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int ms_last_call_profile(const ms_ctx *c, ms_call_profile *out) {
    if (!c || !out) return MS_E_INVAL;
    // CallClock writes prof under sched_mu while a call runs: read it under the
    // same lock, so a concurrent reader never sees a torn profile
    std::lock_guard<std::mutex> g(const_cast<ms_ctx *>(c)->sched_mu);
    for (int i = 0; i < MS_CALL_PHASES; ++i) out->ns[i] = c->prof[i];
    return MS_OK;
}

int ms_get_info(const ms_ctx *c, ms_info *out) {
    if (!c || !out) return MS_E_INVAL;
    ms_ctx *m = const_cast<ms_ctx *>(c);
    std::lock_guard<std::mutex> g(m->delta_mu);
    out->max_nodes = c->cfg.max_nodes;
    out->node_base = c->cfg.node_base;
    out->present_nodes = c->present_count;
    out->pending_deltas = (uint32_t)c->pending.size();
    out->device = c->cfg.device;
    out->plugin_set = c->cfg.plugin_set;
    out->seed = c->cfg.seed;
    uint32_t st[4] = {0, 0, 0, 0};
    // counters are written on the (non-blocking) context stream
    if (hipSetDevice(c->cfg.device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(st, c->d_overflow, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(m, MS_E_HIP, "ms_get_info: counter read-back");
    out->seq_pods = st[3];
    out->seq_resweep_tiles = st[1];
    out->seq_recomputes = st[2];
    out->_pad = st[0];  // non-zero would mean a validator capacity violation
    comm_rank_world(c, &out->comm_rank, &out->comm_world);
    return MS_OK;
}

int ms_seq_counters(const ms_ctx *c, struct ms_seq_counters *out) {
    if (!c || !out) return MS_E_INVAL;
    ms_ctx *m = const_cast<ms_ctx *>(c);
    std::lock_guard<std::mutex> g(m->delta_mu);
    uint32_t st[7] = {0, 0, 0, 0, 0, 0, 0};
    // (as ms_get_info: the counters are written on the context stream)
    if (hipSetDevice(c->cfg.device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(st, c->d_overflow, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(m, MS_E_HIP, "ms_seq_counters: counter read-back");
    out->overflow = st[0];
    out->resweep_tiles = st[1];
    out->recomputes = st[2];
    out->pods = st[3];
    out->misses = st[4];
    out->slow_pods = st[5];
    out->list_scans = st[6];
    out->_pad = 0;
    return MS_OK;
}

int ms_nodes_upsert(ms_ctx *c, uint32_t n, const uint32_t *ord, const ms_node_rec *recs) {
    if (!c || (n && (!ord || !recs))) return MS_E_INVAL;
    std::lock_guard<std::mutex> g(c->delta_mu);
    for (uint32_t i = 0; i < n; ++i)
        if (ord[i] < c->cfg.node_base || ord[i] - c->cfg.node_base >= c->cfg.max_nodes)
            return fail(c, MS_E_CAPACITY, "ms_nodes_upsert: ordinal " + std::to_string(ord[i]) + " outside shard");
    for (uint32_t i = 0; i < n; ++i) {
        NodeDelta d;
        d.local = ord[i] - c->cfg.node_base;
        d.absent = 0;
        d.rec = recs[i];
        c->pending.push_back(d);
        if (!c->present[d.local]) {
            c->present[d.local] = 1;
            ++c->present_count;
        }
        c->rows_used = std::max(c->rows_used, d.local + 1);
    }
    return MS_OK;
}

int ms_nodes_delete(ms_ctx *c, uint32_t n, const uint32_t *ord) {
    if (!c || (n && !ord)) return MS_E_INVAL;
    std::lock_guard<std::mutex> g(c->delta_mu);
    for (uint32_t i = 0; i < n; ++i)
        if (ord[i] < c->cfg.node_base || ord[i] - c->cfg.node_base >= c->cfg.max_nodes)
            return fail(c, MS_E_CAPACITY, "ms_nodes_delete: ordinal " + std::to_string(ord[i]) + " outside shard");
    for (uint32_t i = 0; i < n; ++i) {
        NodeDelta d{};
        d.local = ord[i] - c->cfg.node_base;
        d.absent = 1;
        c->pending.push_back(d);
        if (c->present[d.local]) {
            c->present[d.local] = 0;
            --c->present_count;
        }
    }
    return MS_OK;
}

int ms_nodes_flush(ms_ctx *c) {
    if (!c) return MS_E_INVAL;
    std::lock_guard<std::mutex> g(c->sched_mu);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    int rc = flush_locked(c);
    if (rc) return rc;
    MS_HIP(c, hipStreamSynchronize(c->stream));
    return MS_OK;
}

int ms_nodes_read(ms_ctx *c, uint32_t first, uint32_t n, ms_node_rec *out) {
    if (!c || (n && !out)) return MS_E_INVAL;
    if (first < c->cfg.node_base || (uint64_t)first - c->cfg.node_base + n > c->cfg.max_nodes)
        return fail(c, MS_E_CAPACITY, "ms_nodes_read: range outside shard");
    if (n == 0) return MS_OK;
    std::lock_guard<std::mutex> g(c->sched_mu);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    int rc = flush_locked(c);
    if (rc) return rc;
    DevBuf<ms_node_rec> d;  // (released on return, after the synchronise below)
    MS_HIP(c, made(d.alloc(n)));
    hipError_t e = launch_read_rows(c->t, first - c->cfg.node_base, n, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(ms_node_rec) * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, MS_E_HIP, std::string("ms_nodes_read: ") + hipGetErrorString(e));
    return MS_OK;
}

static int bind_common(ms_ctx *c, uint32_t ordinal, const ms_pod_rec *pod, int sign) {
    if (!c || !pod) return MS_E_INVAL;
    if (ordinal < c->cfg.node_base || ordinal - c->cfg.node_base >= c->cfg.max_nodes)
        return fail(c, MS_E_CAPACITY, "bind: ordinal outside shard");
    std::lock_guard<std::mutex> g(c->sched_mu);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    int rc = flush_locked(c);
    if (rc) return rc;
    {
        // present[] counts queued deltas; a bind drains first, so it is the row's
        // state on the device unless a delta arrived since (then the newest word)
        std::lock_guard<std::mutex> d(c->delta_mu);
        if (!c->present[ordinal - c->cfg.node_base])
            return fail(c, MS_E_INVAL, "bind: node " + std::to_string(ordinal) + " is not present");
    }
    rc = fence_ctx(c);  // (the bind writes the table: after in-flight sharded sweeps)
    if (rc < 0) return rc;
    // the context stream already waits for earlier caller-stream work (OrderedCall::done)
    MS_HIP(c, hipMemcpyAsync(c->d_one, pod, sizeof(ms_pod_rec), hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, launch_bind_one(c->t, ordinal - c->cfg.node_base, c->d_one, sign, c->stream));
    c->order.wrote_ctx();
    MS_HIP(c, hipStreamSynchronize(c->stream));
    return MS_OK;
}

int ms_commit_bind(ms_ctx *c, uint32_t ordinal, const ms_pod_rec *pod) { return bind_common(c, ordinal, pod, +1); }
int ms_uncommit_bind(ms_ctx *c, uint32_t ordinal, const ms_pod_rec *pod) { return bind_common(c, ordinal, pod, -1); }

}  // extern "C"

// ms_ctx.h — the engine context behind the C ABI, shared by the host layer
// (ms_capi.cpp: one device's node shard, deltas, staging, streams; ms_cycle.cpp,
// ms_seq_host.cpp, ms_hostarray.cpp, ms_nam_tab.cpp: the cycles above it) and
// ms_comm.cpp (the RCCL communicator and node-sharded pipelines). Not part of
// the public boundary.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "ms_copy_pool.h"
#include "ms_internal.h"
#include "ms_order.h"
#include "ms_owned.h"

namespace msgpu {
struct CommState;

// The release policies of ms_owned.h: the only place that allocates or frees
// device and pinned memory and creates or destroys events and streams.
template <class T>  // (buffers count elements of T; a void buffer bytes)
constexpr size_t kElemBytes = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);

template <class T>
struct DevMem {
    using handle = T *;
    static T *acquire(size_t count) {
        void *p = nullptr;
        return hipMalloc(&p, count * kElemBytes<T>) == hipSuccess ? static_cast<T *>(p) : nullptr;
    }
    static void release(T *p) { (void)hipFree(p); }
};
template <class T>
struct PinnedMem {
    using handle = T *;
    static T *acquire(size_t count, unsigned flags = hipHostMallocDefault) {
        void *p = nullptr;
        return hipHostMalloc(&p, count * kElemBytes<T>, flags) == hipSuccess ? static_cast<T *>(p) : nullptr;
    }
    static void release(T *p) { (void)hipHostFree(p); }
};
struct EventRes {
    using handle = hipEvent_t;
    static hipEvent_t acquire() {
        hipEvent_t e = nullptr;
        return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? e : nullptr;
    }
    static void release(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct StreamRes {
    using handle = hipStream_t;
    static hipStream_t acquire(unsigned flags) {
        hipStream_t s = nullptr;
        return hipStreamCreateWithFlags(&s, flags) == hipSuccess ? s : nullptr;
    }
    static hipStream_t acquire(unsigned flags, int priority) {
        hipStream_t s = nullptr;
        return hipStreamCreateWithPriority(&s, flags, priority) == hipSuccess ? s : nullptr;
    }
    static void release(hipStream_t s) { (void)hipStreamDestroy(s); }
};
template <class T>
using DevBuf = Owned<DevMem<T>>;
template <class T>
using PinnedBuf = Owned<PinnedMem<T>>;
using Event = Owned<EventRes>;
using Stream = Owned<StreamRes>;

// For MS_HIP around an owner's alloc / ensure: the runtime's error behind a false.
inline hipError_t made(bool ok) { return ok ? hipSuccess : hipGetLastError(); }

// The runtime calls of ms_order.h; the events are created on first use.
struct HipOrder {
    using stream = hipStream_t;
    using event = Event;
    static bool record(Event &e, hipStream_t s) { return e.ensure() && hipEventRecord(e, s) == hipSuccess; }
    static bool wait(hipStream_t s, Event &e) { return hipStreamWaitEvent(s, e, 0) == hipSuccess; }
};
}  // namespace msgpu

using msgpu::DevBuf;
using msgpu::DRow;
using msgpu::Event;
using msgpu::NodeDelta;
using msgpu::NodeTable;
using msgpu::PinnedBuf;
using msgpu::Stream;

struct ms_ctx {
    ms_config cfg{};
    // Owners release themselves in reverse declaration order: the two streams
    // are declared first, so they outlive every event and buffer used on them.
    Stream stream;
    // ms_schedule_batch's chunked copies (schedule_chunked): H2D / D2H of host arrays beside the cycle
    Stream copy_stream;
    int num_cus = 0;
    NodeTable t{};  // raw views: its columns point into d_table, t.planes is d_planes
    DevBuf<void> d_table;  // the node table's columns, one allocation (ms_create)
    DevBuf<uint32_t> d_planes;
    DevBuf<uint32_t> d_cand;  // K1 pp's candidate lists S_d / U_d (ms_internal.h cand_words), rebuilt with the planes
    ~ms_ctx();  // device set, communicator freed, both streams drained; then the members (ms_capi.cpp)

    // helper threads for the host copies of single-shard host-array calls
    // (ms_copy_pool.h; created on the first large call, joined when the context is deleted)
    std::unique_ptr<msgpu::CopyPool> copy_pool;

    // node deltas (informer goroutines) — guarded by delta_mu
    std::mutex delta_mu;
    std::vector<NodeDelta> pending;
    std::vector<uint8_t> present;  // host mirror of presence, updated at enqueue
    uint32_t present_count = 0;
    uint32_t rows_used = 0;  // high-water mark of upserted rows (sweep extent)
    // what the device table holds after the last flush: snapshots of the two
    // counters above taken with the drained deltas (under delta_mu), read only
    // by sched_mu holders
    uint32_t rows_dev = 0, present_dev = 0;

    // one scheduling caller at a time (minisched.go:28-30 runs one goroutine)
    std::mutex sched_mu;

    // staging (d_pods / d_res hold stage_cap pods; the key and flag scratch
    // batch_cap; the compact records compact_cap)
    uint32_t batch_cap = 0, stage_cap = 0, compact_cap = 0;
    DevBuf<ms_pod_compact> d_podc;
    DevBuf<ms_result_compact> d_resc;
    DevBuf<ms_pod_rec> d_pods;
    DevBuf<ms_result> d_res;
    DevBuf<unsigned long long> d_keys;
    DevBuf<uint32_t> d_flags;     // per-pod filter flags (set 1) / NodeAffinity anchors (set 2)
    uint32_t w_nn = 1, w_na = 1;  // score weights (MS_PLUGINS_NU_NN_NA)
    PinnedBuf<NodeDelta> h_deltas;
    DevBuf<NodeDelta> d_deltas;
    uint32_t delta_cap = 0;
    DevBuf<ms_pod_rec> d_one;  // commit/uncommit staging

    // sequential engine scratch
    DevBuf<unsigned long long> d_tile_keys;
    DevBuf<uint32_t> d_tile_flags;
    DevBuf<unsigned long long> d_spec;     // per-pod speculative winner key (atomicMax target)
    DevBuf<uint32_t> d_spec_flags;         // per-pod flags of tiles with no feasible row (atomicOr target)
    DevBuf<unsigned long long> d_top4;     // per-pod global speculative top-4 keys
    DevBuf<int64_t> d_top4_rec;            // their batch-start node records (validator layout)
    DevBuf<unsigned long long> d_top_ext;  // ranks 4..7 per pod (the validator's slow pods)
    DevBuf<uint32_t> d_merge_tags;         // per pod of both merge-output sets: the in-step merge's tag
    uint32_t merge_tag = 0;                // last in-step merge tag issued
    DevBuf<unsigned long long> d_tl;       // MS_VSTAMPS: step timeline (MS_TIMELINE=<file> dumps it at ms_destroy)
    DevBuf<uint32_t> d_prev;               // {count, rows} of the nodes each batch bound (x2)
    DevBuf<int64_t> d_prev_rec;            // and their final records (x2)
    DevBuf<DRow> d_drow;                   // derived rows of the binary64 sweep (tile_cap * kFullWaveTile)
    // (every sequential-engine buffer above is double-buffered by batch parity)
    Event ev_copy[4], ev_cyc[4];  // per chunk of a host-array call (ensure_chunk_events)
    uint32_t tile_cap = 0;  // tiles allocated per pod
    DevBuf<uint32_t> d_overflow;
    PinnedBuf<ms_pod_compact> h_podz;     // pinned compact pods / results the compact cycle's
    PinnedBuf<ms_result_compact> h_resz;  // kernel reads and writes over PCIe (zero-copy)
    uint32_t z_cap = 0;
    // MS_PLUGINS_NU_TT_NN: segment summaries of the sweep (tt_bytes allocated)
    DevBuf<void> d_tt;
    size_t tt_bytes = 0;
    // d_tt is one scratch for every TT cycle of the context: a cycle on another
    // stream than the previous one waits for ev_tt, recorded after that one's
    // combine (node-sharded submits run on caller / sweep streams that are not
    // chained through the context stream)
    Event ev_tt;
    hipStream_t tt_stream = nullptr;  // (not owned: the context's, a caller's or the communicator's)
    // MS_PLUGINS_NU_NN_NAM: the registered term sets as lookup tables (NamTab) and the
    // per-class passes' scratch of a chunk (nam_bytes allocated)
    // n_terms counts the ids with a table: max(preferred sets, required sets). The
    // host keeps both registered tables (h_pref, h_req), since each is replaced
    // on its own and every id's NamTab holds its share of both.
    DevBuf<void> d_terms;
    uint32_t n_terms = 0, terms_cap = 0;
    std::vector<ms_nam_term_set_ext> h_pref;
    std::vector<ms_nam_required_set> h_req;
    DevBuf<void> d_nam;
    size_t nam_bytes = 0;
    // d_nam is one scratch for every NAM cycle of the context, as d_tt is: a
    // cycle on another stream than the previous one waits for ev_nam, recorded
    // after that one's last launch (two node-sharded submits on different sweep
    // streams do not follow each other through the context stream)
    Event ev_nam;
    hipStream_t nam_stream = nullptr;  // (not owned)
    // node-sharded sequential mode: merged candidate lists (ms_seq_validate_device)
    DevBuf<ms_seq_cand> d_merged;
    DevBuf<uint32_t> d_merged_flags;
    // explain (ms_explain_host.cpp): the three stages' scratch (explain_bytes
    // allocated; every explain call is an OrderedCall, so the context stream
    // orders its users), and ms_explain's device staging of pods and rows
    DevBuf<void> d_explain;
    size_t explain_bytes = 0;
    DevBuf<ms_pod_rec> d_ex_pods;  // MS_EXPLAIN_MAX_PODS records
    DevBuf<ms_explain_row> d_ex_rows;
    size_t ex_rows_cap = 0;

    // every access to the table or the scratch above, on whichever stream, is
    // ordered through the context stream (ms_order.h; OrderedCall below)
    msgpu::StreamOrder<msgpu::HipOrder> order;

    // RCCL communicator and the node-sharded pipelines (ms_comm.cpp); null
    // until ms_comm_init
    msgpu::CommState *comm = nullptr;

    // host phase times of the last ms_schedule_batch(_compact) call (ms_last_call_profile)
    uint64_t prof[MS_CALL_PHASES] = {};

    std::string err;
};

namespace msgpu {

// Records msg as the context's last error (or the thread's ms_create error).
int fail(ms_ctx *c, int code, const std::string &msg);

#define MS_HIP(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return ::msgpu::fail((c), MS_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// Host wall time of a host-array call split into MS_PH_* phases: lap(ph) adds
// the time since the previous lap to phase ph; the destructor records the
// call's total (every return path of the call).
class CallClock {
  public:
    using Clock = std::chrono::steady_clock;
    explicit CallClock(ms_ctx *c) : c_(c), t0_(Clock::now()), t_(t0_) {
        for (uint64_t &v : c_->prof) v = 0;
    }
    ~CallClock() { c_->prof[MS_PH_TOTAL] = ns(t0_, Clock::now()); }
    void lap(int ph) {
        const auto now = Clock::now();
        c_->prof[ph] += ns(t_, now);
        t_ = now;
    }
    void count(int ph, uint64_t k = 1) { c_->prof[ph] += k; }

  private:
    static uint64_t ns(Clock::time_point a, Clock::time_point b) {
        return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count();
    }
    ms_ctx *c_;
    Clock::time_point t0_, t_;
};

constexpr uint32_t kTopKCands = 4;  // ms_seq_cand entries per pod and shard (the validator's top-K)

// validator counters (d_overflow): u32[6] (overflow, re-swept tiles, recomputes, pods, speculation
// misses, list scans), then u64[4] phase cycles in the MS_VSTAMPS diagnostic build
constexpr size_t kStatsBytes = 256;

// ms_capi.cpp (callers hold sched_mu)
int flush_locked(ms_ctx *c);
hipStream_t pick_stream(ms_ctx *c, void *s);
int ensure_stage(ms_ctx *c, uint32_t n);
bool plugins_stateless(const ms_ctx *c);

// One ordered device call (ms_order.h): the whole prologue of an entry point
// whose work touches the node table or the context's scratch, and its
// epilogue. The constructor locks sched_mu, sets the device, drains the node
// deltas (flush; not for the calls that must leave them queued), picks the
// stream and orders it after the context stream; done() chains the call's
// work back. A call that fails returns its code without done().
//     OrderedCall call(c, stream);
//     if (call.rc()) return call.rc();
//     ... launches on call.stream() ...
//     return call.done();
class OrderedCall {
  public:
    OrderedCall(ms_ctx *c, void *stream, bool flush = true);
    int rc() const { return rc_; }
    hipStream_t stream() const { return s_; }
    // On a caller stream: the chain-back event, for a dispatch that records it
    // itself after the call's last launch (then done(true)); null on the context stream.
    hipEvent_t back_event() const { return back_; }
    int done(bool recorded = false);

  private:
    ms_ctx *c_;
    std::lock_guard<std::mutex> g_;
    hipStream_t s_ = nullptr;
    hipEvent_t back_ = nullptr;
    int rc_ = MS_OK;
};

// ms_cycle.cpp: the per-plugin-set cycle drivers
// done (optional): recorded on s after the sweep (by the K1 dispatch itself when it is one launch)
int sweep_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, unsigned long long *keys, uint32_t *flags,
                 hipStream_t s, hipEvent_t done = nullptr);
// done (optional): recorded on s after the call's last launch
int select_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, ms_result *d_res, hipStream_t s,
                  int commit = 0, hipEvent_t done = nullptr);
// MS_PLUGINS_NU_TT_NN: the batch's summaries merged into out (this shard's, MS_TT_SUMMARY_BYTES
// per pod), or with out null the single-shard cycle into results
int tt_cycle_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, void *out, ms_result *results, int commit,
                    hipStream_t s);
// MS_PLUGINS_NU_TT_NN scratch of at least `need` bytes (the two-pass bit-sliced
// cycle's, or the node shards' summaries).
int ensure_tt(ms_ctx *c, size_t need);
// d_tt is one scratch for every TT cycle of the context (ev_tt above): a cycle
// on s takes it before its first launch (s waits for the previous cycle's end
// when that ran on another stream) and releases it after its last.
int tt_take(ms_ctx *c, hipStream_t s);
int tt_release(ms_ctx *c, hipStream_t s);
// The same for d_nam (ev_nam), around every user of the NodeAffinity scratch.
int nam_take(ms_ctx *c, hipStream_t s);
int nam_release(ms_ctx *c, hipStream_t s);
// MS_PLUGINS_NU_NN_NAM over node shards inside the library (ms_comm.cpp): a batch
// swept whole under ms_nam_layout.h's whole-batch plan. nam_shard_classes: the
// class records a rank sends for a batch of n_pods (the same on every rank).
// nam_shard_begin: the scratch for the batch, taken on s. nam_shard_segment: this
// shard's class records into cls_mine. nam_shard_keys: from the n_shards gathered
// records, this shard's keys and filter words, resuming from the scratch the
// segment pass of the same batch left. The caller releases (nam_release) after.
uint32_t nam_shard_classes(const ms_ctx *c, uint32_t n_pods);
int nam_shard_begin(ms_ctx *c, uint32_t n_pods, hipStream_t s);
int nam_shard_segment(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, void *cls_mine, hipStream_t s);
int nam_shard_keys(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, const void *cls_all, uint32_t n_shards,
                   uint32_t shard_index, unsigned long long *keys, uint32_t *flags, hipStream_t s);

// ms_seq_host.cpp: the sequential engine's host side
int ensure_tiles(ms_ctx *c, uint32_t n_tiles);
int run_sequential(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, ms_result *d_res, hipStream_t s);
int seq_candidates_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, ms_seq_cand *cands_dev,
                          uint32_t *flags_dev, hipStream_t s);
// The diagnostic builds' read-out at ms_destroy (MS_VSTAMPS counters to stderr,
// the MS_TIMELINE file); nothing in the product build.
void seq_diag_readout(ms_ctx *c);

// ms_comm.cpp
void comm_free(ms_ctx *c);
// ms_schedule_batch / ms_schedule_sequential_device on a context joined to a
// communicator (callers hold sched_mu; deltas flushed)
int comm_schedule_host(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods, int32_t mode, ms_result *out,
                       CallClock *ck);
// the same on pods already staged in c->d_pods (comm_stage(n) first), results in c->d_res
int comm_stage(ms_ctx *c, uint32_t n_pods);
int comm_cycle_staged(ms_ctx *c, uint32_t n_pods, int32_t mode);
int comm_schedule_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, ms_result *results_dev,
                         hipStream_t s);
void comm_rank_world(const ms_ctx *c, int32_t *rank, int32_t *world);
// Makes `writer` wait for the node-sharded sweeps still reading the table on the
// communicator's internal streams; returns 1 if it inserted waits, 0 if none
// were outstanding (or no communicator), < 0 on failure.
int comm_fence_reads(ms_ctx *c, hipStream_t writer);
// The sharded pipeline drained onto s (everything pending decoded, s after the
// decode stream), as the collective cycles do before they use s for their own
// collectives (the caller holds sched_mu).
int comm_drain_to(ms_ctx *c, hipStream_t s);

}  // namespace msgpu

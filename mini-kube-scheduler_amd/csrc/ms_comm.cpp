// ms_comm.cpp — multi-GPU inside the C ABI (include/minisched_gpu.h, "multi-GPU
// inside the library"). A context joined to an RCCL communicator owns one node
// shard per rank and runs the node-sharded cycles with their collectives in the
// library, so the Go scheduleOne (/root/reference/minisched/minisched.go:32-85,
// called from one goroutine, :28-30) drives G GPUs through the same cgo calls
// it uses for one, with no RCCL binding of its own (SURVEY §8(b) Ownership).
//
// Batched cycle (config C; selectHost over the union of the shards,
// minisched.go:304-325): this shard's sweep of the batch (K1 pp, the
// NodeAffinity sweep or the resource sweep) -> ONE grouped ncclReduceScatter
// on the collective stream:
//   keys   uint64 MAX, G x per pods -> this rank's slice of per pods (the keys
//          embed the global ordinal, so MAX is the global argmax);
//          A pod with no feasible node on a shard has key 1 there when the
//          shard lists a node (kKeyListed), so the MAX also carries the NU+NN /
//          NodeAffinity FitError mask: F = 0 with a listed node means
//          NodeUnschedulable rejected every node;
//   flags  NodeResourcesFit set: uint8 MAX of the filter bytes (byte-wise OR =
//          FitError's UnschedulablePlugins over the cluster, :130-137);
//          NodeAffinity set: uint32 MAX of the normalise anchors;
//          multi-term NodeAffinity set: uint8 MAX of its filter bytes, after a
//          first pass whose class records (one rescale record per (term set,
//          toleration) class of the batch) were all-gathered and a second pass
//          that computed the keys under them (nam_sharded_sweep);
// -> the decode of the slice on the caller's stream. Pipelined: the decodes of
// batch k are enqueued once `depth` later batches were submitted, so batch k's
// collective overlaps their sweeps. The sweeps run on the caller's stream, the
// collectives on the collective stream and the decodes on a decode stream, so
// no sweep waits for a collective or a decode (one cross-queue wait per step:
// the collective on its sweep). The sweeps only read the node table; writers
// (deltas, binds) are fenced behind the in-flight ones (comm_fence_reads)
// instead of every sweep being chained into the context stream. When each of
// these may run is ms_shard_order.h's (ShardOrder, with the argument for every
// wait); this file says what to launch. MINISCHED_SHARD_STREAMS=2 alternates
// the sweeps over two internal streams instead (two independent streams on
// separate hardware queues overlap one sweep's ramp and tail with the next:
// 55.4 vs 42.9 us per 12.5k-row sweep, tools/probe_streams.py; but the
// library's streams share the process's hardware queues and the extra waits
// made the pipelined step slower: profiles/r03_step_streams_ab.json).
//
// Exact sequential cycle (config E): per window of W pods, every
// shard's speculative top-4 with records (ms_seq_candidates_device) -> one
// grouped ncclAllGather -> the replicated in-order validation on every rank,
// which commits the binds on its own nodes. The queue cursor lives on the
// device (k_seq_window_in / k_seq_window_out), so windows are issued without a
// host round trip; the host reads the cursor once per round of
// ceil(remaining / W) windows (every window decides at least one pod; one
// round suffices unless a window stops early).
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>

#include "ms_ctx.h"
#include "ms_shard_order.h"

// The RCCL entry points. `make comm-loopback` (tests only) builds this file with
// -DMS_COMM_LOOPBACK against an in-process rendezvous of G contexts on one GPU
// (ms_comm_loopback.h), so the world > 1 code below runs on a 1-GPU box; the
// product library calls RCCL itself.
#ifdef MS_COMM_LOOPBACK
#include "ms_comm_loopback.h"
#define CCL(fn) lb_##fn
#else
#define CCL(fn) fn
#endif

namespace msgpu {

namespace {

constexpr uint32_t kPipeMax = 8;  // batch buffer sets: pipeline depth + 1 <= kPipeMax
static_assert(kPipeMax <= kMaxSliceJobs, "a full drain is one slice-decode launch");
static_assert(sizeof(ncclUniqueId) == MS_COMM_ID_BYTES, "ms_comm_id holds an ncclUniqueId");

// One in-flight batch's combine buffers.
struct ShardSlot {
    DevBuf<unsigned long long> keys;       // G x cap: this shard's maxima, pod order
    DevBuf<unsigned long long> keys_mine;  // cap: the cluster's maxima of this rank's slice
    DevBuf<uint32_t> flags, flags_mine;
    // MS_PLUGINS_NU_TT_NN, the two-pass form: this shard's census (G x cap records, pod
    // order), every shard's after the all-gather (G x G x cap, shard-major,
    // stride = the batch), and the slice's plans for the final pass
    DevBuf<void> cen_mine, cen_all, plans;
    // MS_PLUGINS_NU_NN_NAM: this shard's class records (cls_cap records) and every
    // shard's after the all-gather (G x cls_cap, shard-major, stride = the batch's
    // class cap). They grow with the classes of a batch, not with the slice.
    DevBuf<void> cls_mine, cls_all;
    uint32_t cap = 0;       // pods per slice the buffers hold
    uint32_t cls_cap = 0;   // class records the NAM buffers hold
};

// A batch from its submission to its decode (its slot's buffers may be swept
// again by a later one before the decode is enqueued: the payload is not the slot's).
struct Batch {
    uint32_t slot = 0, n = 0, first = 0, count = 0;
    const ms_pod_rec *pods = nullptr;  // the batch (decode reads pods + first)
    ms_result *results = nullptr;      // this rank's slice
    hipStream_t X = nullptr;           // its sweep stream
};

using Order = ShardOrder<HipOrder>;
static_assert(kPipeMax == Order::kSlotsMax, "one buffer set per ordering slot");

}  // namespace

struct CommState {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    // (the streams first: members release in reverse order, so they outlive the
    // events and buffers used on them)
    Stream cs;     // collective stream
    Stream ss[2];  // sweep streams, alternating batch by batch
    Stream ds;     // decode stream (the drains; callers wait on it in ms_sharded_drain)
    // when each step of a batch may run: every event and counter of the
    // pipeline, the slots' state and the pending ring (ms_shard_order.h).
    // depth: batches in flight before the oldest are decoded; two_streams
    // (MINISCHED_SHARD_STREAMS=2): sweeps alternate over ss[0], ss[1] (A/B)
    Order order;
    ShardSlot slot[kPipeMax];
    std::deque<Batch> pending;  // after their collectives, oldest first (in step with order's ring)
    CommState(uint32_t depth, bool two_streams) : order(depth, two_streams) {}
    // node-sharded exact sequential
    uint32_t seq_w = 0;
    DevBuf<ms_pod_rec> win_pods;
    DevBuf<ms_result> win_res;
    DevBuf<uint32_t> ctl;       // {cursor, live, n_done, pad}
    PinnedBuf<uint32_t> h_ctl;  // pinned read-back of the cursor
    DevBuf<ms_seq_cand> cands, cands_all, merged;
    DevBuf<uint32_t> sflags, sflags_all, merged_flags;
    uint64_t seq_windows = 0, seq_rounds = 0;
    // coalesced submits: a NU+NN submission whose sweep waits to share the
    // next one's launch (while order.held())
    Batch stash;
    bool coalesce = true;
    // MINISCHED_HOST_PROF=1: host time of ms_sharded_submit's phases (ns), printed at ms_destroy
    bool host_prof = false;
    uint64_t hp[6] = {0, 0, 0, 0, 0, 0}, hp_calls = 0;

    // In this order: the host profile, every stream and the device idle, the
    // communicator gone; the members then release themselves.
    ~CommState() {
        if (host_prof && hp_calls)
            std::fprintf(stderr, "MS_HOST_PROF submits=%llu us/submit: order=%.2f sweep=%.2f events=%.2f rccl=%.2f tail=%.2f\n",
                         (unsigned long long)hp_calls, hp[0] * 1e-3 / hp_calls, hp[1] * 1e-3 / hp_calls,
                         hp[2] * 1e-3 / hp_calls, hp[3] * 1e-3 / hp_calls, hp[4] * 1e-3 / hp_calls);
        for (hipStream_t q : ss)
            if (q) (void)hipStreamSynchronize(q);
        if (cs) (void)hipStreamSynchronize(cs);
        if (ds) (void)hipStreamSynchronize(ds);
        (void)hipDeviceSynchronize();
        if (comm) (void)CCL(ncclCommDestroy)(comm);
    }
};

namespace {

#define MS_NCCL(c, call)                                                                          \
    do {                                                                                          \
        ncclResult_t r_ = (call);                                                                 \
        if (r_ != ncclSuccess)                                                                    \
            return fail((c), MS_E_RCCL, std::string(#call) + ": " + CCL(ncclGetErrorString)(r_));      \
    } while (0)

// A step of the ordering class (false: a record or a wait failed, or a step
// was taken while a submission was still held back).
#define MS_ORD(c, call)                                                                            \
    do {                                                                                           \
        if (!(call))                                                                               \
            return fail((c), MS_E_HIP, std::string("stream ordering (" #call "): ") +              \
                                           hipGetErrorString(hipGetLastError()));                  \
    } while (0)

int drain_locked(ms_ctx *c, size_t k);

// Buffers of slot si for slices of `per` pods, rounded up to 1024 (grown; the
// slot's previous batch has been drained). No synchronise of its own: the
// runtime's free of the old blocks waits for that batch's decode, so the slot
// starts over as unused.
// cls (MS_PLUGINS_NU_NN_NAM, else 0): the class records of the batch, rounded up
// to 64; either growth replaces all of the slot's buffers.
int slot_ensure(ms_ctx *c, uint32_t si, uint32_t per, uint32_t cls) {
    ShardSlot &sl = c->comm->slot[si];
    if (per <= sl.cap && cls <= sl.cls_cap) return MS_OK;
    const size_t G = (size_t)c->comm->world;
    const uint32_t cap = std::max(sl.cap, std::max<uint32_t>(1024u, cdiv(per, 1024u) * 1024u));
    const uint32_t cls_cap = std::max(sl.cls_cap, cdiv(cls, 64u) * 64u);
    // (a submission held back for a partner makes the slot come round one
    // step early, its batch not decoded yet: that decode reads these buffers)
    if (const size_t k = c->comm->order.pending_through(si)) {
        const int rc = drain_locked(c, k);
        if (rc) return rc;
    }
    sl.cap = sl.cls_cap = 0;
    MS_ORD(c, c->comm->order.regrown(si));
    if (!sl.keys.alloc(G * cap) || !sl.keys_mine.alloc(cap) || !sl.flags.alloc(G * cap) || !sl.flags_mine.alloc(cap) ||
        (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN &&
         (!sl.cen_mine.alloc(G * cap * MS_TT_CENSUS_BYTES) || !sl.cen_all.alloc(G * G * cap * MS_TT_CENSUS_BYTES) ||
          !sl.plans.alloc((size_t)cap * MS_TT_CENSUS_BYTES))) ||
        (cls_cap && (!sl.cls_mine.alloc((size_t)cls_cap * MS_NAM_SEG_BYTES) ||
                     !sl.cls_all.alloc(G * cls_cap * MS_NAM_SEG_BYTES))))
        return fail(c, MS_E_OOM, "sharded combine buffers");
    sl.cap = cap;
    sl.cls_cap = cls_cap;
    return MS_OK;
}

void slice_of(const CommState &m, uint32_t n, uint32_t &first, uint32_t &count) {
    const uint32_t per = cdiv(n, (uint32_t)m.world);
    first = std::min<uint32_t>(n, (uint32_t)m.rank * per);
    count = std::min<uint32_t>(n, first + per) - first;
}

// Decodes of the oldest k pending batches on the decode stream (after their
// combines). The caller's stream is not involved: a sweep stream that orders
// after the caller's stream would otherwise wait for these combines too.
int drain_locked(ms_ctx *c, size_t k) {
    CommState &m = *c->comm;
    const hipStream_t s = m.ds;
    MS_ORD(c, m.order.drain_begin(k));
    if (k == 0) return MS_OK;
    if (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN) {  // the slice's plans + the MAX of the picks
        for (size_t i = 0; i < k; ++i) {
            const Batch &p = m.pending[i];
            const ShardSlot &sl = m.slot[p.slot];
            MS_HIP(c, launch_tt2_final_shard(c->t, c->rows_dev, p.pods + p.first, p.count, seed32_of(c->cfg.seed),
                                             sl.plans, p.count, static_cast<const char *>(sl.cen_all.get()) +
                                                                    (size_t)p.first * MS_TT_CENSUS_BYTES,
                                             p.n, (uint32_t)m.world, sl.keys_mine, p.results, s));
        }
    } else if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NA) {
        for (size_t i = 0; i < k; ++i) {
            const Batch &p = m.pending[i];
            const ShardSlot &sl = m.slot[p.slot];
            MS_HIP(c, launch_decode_na(p.pods + p.first, p.count, sl.keys_mine, sl.flags_mine, 0, seed32_of(c->cfg.seed),
                                       c->w_nn, c->w_na, p.results, s));
        }
    } else {
        SliceJob jobs[kMaxSliceJobs];
        // filter bytes: the resource-aware set's (bytes 0, 1) and the multi-term NodeAffinity
        // set's (bytes 0, 2). No present flag for either: key 1 from any shard says a node is listed
        const bool filt = c->cfg.plugin_set == MS_PLUGINS_NU_NRF_NN_LA || c->cfg.plugin_set == MS_PLUGINS_NU_NN_NAM;
        for (size_t i = 0; i < k; ++i) {
            const Batch &p = m.pending[i];
            const ShardSlot &sl = m.slot[p.slot];
            jobs[i] = SliceJob{p.pods + p.first, sl.keys_mine, filt ? sl.flags_mine : nullptr, nullptr, p.results,
                               p.count, 0};
        }
        MS_HIP(c, launch_decode_slices(jobs, (uint32_t)k, s));
    }
    MS_ORD(c, m.order.drain_end(k));
    m.pending.erase(m.pending.begin(), m.pending.begin() + (long)k);
    return MS_OK;
}

int flush_stash(ms_ctx *c);

// Everything pending decoded; then `s` waits for the decode stream.
int drain_to(ms_ctx *c, hipStream_t s) {
    CommState &m = *c->comm;
    int rc = flush_stash(c);  // (a coalesced submission waiting for a partner)
    if (rc) return rc;
    rc = drain_locked(c, m.order.pending());
    if (rc) return rc;
    MS_ORD(c, m.order.drained_to(s));
    return MS_OK;
}

using HostClock = std::chrono::steady_clock;
inline void host_tick(CommState &m, int i, HostClock::time_point &t) {
    if (!m.host_prof) return;
    const auto now = HostClock::now();
    m.hp[i] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now - t).count();
    t = now;
}

// Submissions whose sweep can share a launch with the next one: NU+NN K1
// sweeps of a shard one workgroup holds, on one sweep stream.
bool coalescable(const ms_ctx *c) {
    const CommState &m = *c->comm;
    return m.coalesce && !m.order.two_streams() && c->cfg.plugin_set == MS_PLUGINS_NU_NN &&
           c->rows_dev <= kPpMaxFusedRows;
}

// The collective of batch b on the collective stream; then the batch is
// pending, and the oldest are decoded when the ordering says so.
int collective_locked(ms_ctx *c, const Batch &b, HostClock::time_point &tp) {
    CommState &m = *c->comm;
    ShardSlot &sl = m.slot[b.slot];
    const uint32_t G = (uint32_t)m.world, per = cdiv(b.n, G);
    const int ps = c->cfg.plugin_set;
    MS_ORD(c, m.order.before_collective(b.slot));
    host_tick(m, 2, tp);  // events to the collective stream
    ncclResult_t r = ncclSuccess;
    if (ps == MS_PLUGINS_NU_NN || ps == MS_PLUGINS_NU_TT_NN) {  // the keys alone: one call
        r = CCL(ncclReduceScatter)(sl.keys, sl.keys_mine, per, ncclUint64, ncclMax, m.comm, m.cs);
    } else {
        r = CCL(ncclGroupStart)();
        if (r == ncclSuccess) r = CCL(ncclReduceScatter)(sl.keys, sl.keys_mine, per, ncclUint64, ncclMax, m.comm, m.cs);
        // 0/1 bytes: uint8 MAX = OR (resource-aware: bytes 0, 1; multi-term NodeAffinity: bytes 0, 2)
        if (r == ncclSuccess && (ps == MS_PLUGINS_NU_NRF_NN_LA || ps == MS_PLUGINS_NU_NN_NAM))
            r = CCL(ncclReduceScatter)(sl.flags, sl.flags_mine, (size_t)per * 4, ncclUint8, ncclMax, m.comm, m.cs);
        if (r == ncclSuccess && ps == MS_PLUGINS_NU_NN_NA)  // anchors < 2^21: uint32 MAX
            r = CCL(ncclReduceScatter)(sl.flags, sl.flags_mine, per, ncclUint32, ncclMax, m.comm, m.cs);
        const ncclResult_t r2 = CCL(ncclGroupEnd)();
        if (r == ncclSuccess) r = r2;
    }
    if (r != ncclSuccess) return fail(c, MS_E_RCCL, std::string("sharded combine: ") + CCL(ncclGetErrorString)(r));
    host_tick(m, 3, tp);  // the grouped reduce-scatter
    size_t n_drain = 0;
    MS_ORD(c, m.order.after_collective(b.slot, n_drain));
    m.pending.push_back(b);
    const int rc = n_drain ? drain_locked(c, n_drain) : MS_OK;
    host_tick(m, 4, tp);  // bookkeeping + drains
    return rc;
}

// The stashed submission's sweep alone, then its collective.
int flush_stash(ms_ctx *c) {
    CommState &m = *c->comm;
    if (!m.order.held()) return MS_OK;
    const Batch b = m.stash;
    HostClock::time_point tp = m.host_prof ? HostClock::now() : HostClock::time_point();
    MS_HIP(c, made(m.order.sweep_event(b.slot).ensure()));
    int rc = sweep_locked(c, b.n, b.pods, m.slot[b.slot].keys, nullptr, b.X, m.order.sweep_event(b.slot));
    if (rc) return rc;
    MS_ORD(c, m.order.swept(b.slot, b.X, true));
    return collective_locked(c, b, tp);
}

// MS_PLUGINS_NU_TT_NN, two-pass: the census of this shard on X, the all-gather of
// every shard's on the collective stream, then the picks on X again (the table's
// readers stay on the sweep stream, behind the delta fence). The shared two-pass
// scratch (d_tt) passes from sweep stream to sweep stream (tt_take / tt_release).
int tt2_sharded_sweep(ms_ctx *c, const Batch &b) {
    CommState &m = *c->comm;
    ShardSlot &sl = m.slot[b.slot];
    const uint32_t si = b.slot, n = b.n, seed32 = seed32_of(c->cfg.seed);
    const hipStream_t X = b.X;
    int rc = ensure_tt(c, tt2_scratch_bytes(c->rows_dev, std::max(1u, n)));
    if (rc) return rc;
    rc = tt_take(c, X);
    if (rc) return rc;
    rc = [&]() -> int {
        MS_HIP(c, launch_tt2_planes(c->t, c->rows_dev, c->d_tt, X));
        MS_HIP(c, launch_tt2_census_shard(c->t, c->rows_dev, b.pods, n, seed32, c->d_tt, std::max(1u, n), sl.cen_mine, X));
        MS_ORD(c, m.order.census_done(si, X));
        const ncclResult_t r = CCL(ncclAllGather)(sl.cen_mine, sl.cen_all, (size_t)n * MS_TT_CENSUS_BYTES, ncclUint8,
                                                  m.comm, m.cs);
        if (r != ncclSuccess) return fail(c, MS_E_RCCL, std::string("TaintToleration census all-gather: ") +
                                                            CCL(ncclGetErrorString)(r));
        MS_ORD(c, m.order.gathered(si, X));
        MS_HIP(c, launch_tt2_pick_shard(c->t, c->rows_dev, b.pods, n, seed32, c->d_tt, std::max(1u, n), sl.cen_all, n,
                                        (uint32_t)m.world, (uint32_t)m.rank, sl.keys, X));
        return MS_OK;
    }();
    // (after a failure too: the next cycle on another stream follows what this one enqueued)
    const int released = tt_release(c, X);
    if (rc || released) return rc ? rc : released;
    MS_ORD(c, m.order.swept(si, X, false));  // (again: the fence and the reduce-scatter follow the picks)
    return MS_OK;
}

// MS_PLUGINS_NU_NN_NAM, the same two-pass shape: this shard's class records on X
// (one 104-byte rescale record per (term set, toleration) class of the batch;
// class ids are the same on every rank), the all-gather of every shard's on the
// collective stream, then on X again the keys and this shard's filter words,
// resuming from the class pass the first pass left in the scratch. The shared
// scratch (d_nam) passes from sweep stream to sweep stream (nam_take / nam_release).
// In the ordering class the steps are TaintToleration's: cls_mine is written on
// X after the collective that read the slot's previous contents (begin);
// cls_all is written by the all-gather and read only by the keys pass of the
// same batch, which the slot's next all-gather follows through census_done.
int nam_sharded_sweep(ms_ctx *c, const Batch &b) {
    CommState &m = *c->comm;
    ShardSlot &sl = m.slot[b.slot];
    const uint32_t si = b.slot, n = b.n, C = nam_shard_classes(c, n);
    const hipStream_t X = b.X;
    int rc = nam_shard_begin(c, n, X);
    if (rc) return rc;
    rc = [&]() -> int {
        const int seg = nam_shard_segment(c, n, b.pods, sl.cls_mine, X);
        if (seg) return seg;
        MS_ORD(c, m.order.census_done(si, X));
        const ncclResult_t r = CCL(ncclAllGather)(sl.cls_mine, sl.cls_all, (size_t)C * MS_NAM_SEG_BYTES, ncclUint8,
                                                  m.comm, m.cs);
        if (r != ncclSuccess) return fail(c, MS_E_RCCL, std::string("NodeAffinity class record all-gather: ") +
                                                            CCL(ncclGetErrorString)(r));
        MS_ORD(c, m.order.gathered(si, X));
        return nam_shard_keys(c, n, b.pods, sl.cls_all, (uint32_t)m.world, (uint32_t)m.rank, sl.keys, sl.flags, X);
    }();
    // (after a failure too: the next cycle on another stream follows what this one enqueued)
    const int released = nam_release(c, X);
    if (rc || released) return rc ? rc : released;
    MS_ORD(c, m.order.swept(si, X, false));  // (again: the fence and the reduce-scatter follow the keys pass)
    return MS_OK;
}

int submit_locked(ms_ctx *c, uint32_t n, const ms_pod_rec *pods, ms_result *results, hipStream_t s) {
    CommState &m = *c->comm;
    HostClock::time_point tp = m.host_prof ? HostClock::now() : HostClock::time_point();
    if (m.host_prof) ++m.hp_calls;
    const bool co = coalescable(c);
    if (!co) {
        int rc = flush_stash(c);
        if (rc) return rc;
    }
    // the slot (its buffers sized for n pods) and the sweep stream, ordered
    Batch b{m.order.next_slot(), n, 0, 0, pods, results, nullptr};
    slice_of(m, n, b.first, b.count);
    const uint32_t si = b.slot;
    const bool nam = c->cfg.plugin_set == MS_PLUGINS_NU_NN_NAM;
    int rc = slot_ensure(c, si, cdiv(n, (uint32_t)m.world), nam ? nam_shard_classes(c, n) : 0u);
    if (rc) return rc;
    MS_ORD(c, m.order.begin(s, c->order.seq(), co, b.X));
    const hipStream_t X = b.X;
    host_tick(m, 0, tp);  // ordering of the sweep stream
    if (co && (!m.order.held() || m.stash.X != X)) {
        // Coalesced submits (MINISCHED_SHARD_COALESCE=0 turns it off): this
        // batch's sweep waits for the next submission (or a drain / table
        // writer) and then shares ONE K1 launch with it, so the launch's ramp
        // and drain (~7.5 us at a 12.5k-row shard, tools/probe_fixed.py) are
        // paid once per two batches. Its collective starts after both sweeps.
        rc = flush_stash(c);
        if (rc) return rc;
        m.stash = b;
        m.order.hold(si);
        return MS_OK;
    }
    ShardSlot &sl = m.slot[si];
    const int ps = c->cfg.plugin_set;
    // (the sweep event is recorded by the sweep's own dispatch for K1: no
    // separate event packet between consecutive sweeps on X)
    if (ps != MS_PLUGINS_NU_TT_NN && !nam) MS_HIP(c, made(m.order.sweep_event(si).ensure()));
    if (co) {  // the stashed batch and this one in one launch
        const Batch b0 = m.stash;
        MS_HIP(c, launch_sweep_pp2(c->t, c->d_cand, c->rows_dev, b0.pods, b0.n, m.slot[b0.slot].keys, pods, n, sl.keys,
                                   seed32_of(c->cfg.seed), c->present_dev, c->num_cus, X, m.order.sweep_event(si)));
        host_tick(m, 1, tp);  // the sweep launch
        MS_ORD(c, m.order.swept_pair(b0.slot, si));
        rc = collective_locked(c, b0, tp);
        if (rc) return rc;
        return collective_locked(c, b, tp);
    }
    if (ps == MS_PLUGINS_NU_TT_NN) {
        // the two-pass form: this shard's census, every shard's by one all-gather,
        // then this shard's picks for every pod (keys, combined by the reduce-scatter)
        rc = tt2_sharded_sweep(c, b);
        if (rc) return rc;
    } else if (nam) {
        // the same shape with class records: this shard's rescale record per class, every
        // shard's by one all-gather, then this shard's keys and filter words for every pod
        rc = nam_sharded_sweep(c, b);
        if (rc) return rc;
    } else {
        rc = sweep_locked(c, n, pods, sl.keys, ps == MS_PLUGINS_NU_NN ? nullptr : sl.flags, X, m.order.sweep_event(si));
        if (rc) return rc;
        MS_ORD(c, m.order.swept(si, X, true));
    }
    host_tick(m, 1, tp);  // the sweep launch
    return collective_locked(c, b, tp);
}

// Sequential-window buffers for windows of w pods.
int seq_ensure(ms_ctx *c, uint32_t w) {
    CommState &m = *c->comm;
    if (w <= m.seq_w) return MS_OK;
    MS_HIP(c, hipDeviceSynchronize());
    m.seq_w = 0;
    const size_t G = (size_t)m.world, K = kTopKCands;
    if (!m.win_pods.alloc(w) || !m.win_res.alloc(w) || !m.ctl.alloc(4) || !m.h_ctl.alloc(4) || !m.cands.alloc(w * K) ||
        !m.cands_all.alloc(G * w * K) || !m.merged.alloc(w * K) || !m.sflags.alloc(w) || !m.sflags_all.alloc(G * w) ||
        !m.merged_flags.alloc(w))
        return fail(c, MS_E_OOM, "sharded sequential buffers");
    m.seq_w = w;
    return MS_OK;
}

// Pods per window of the node-sharded exact sequential cycle: each window costs
// one all-gather of its candidates (W x 4 x 72 B per rank) and one validator
// launch. MINISCHED_SHARD_SEQ_BATCH overrides (1..256).
uint32_t seq_window() {
    uint32_t w = 128;
    if (const char *e = getenv("MINISCHED_SHARD_SEQ_BATCH")) w = (uint32_t)std::max(1, atoi(e));
    return std::min<uint32_t>(w, MS_SEQ_SHARD_BATCH_MAX);
}

int seq_sharded_locked(ms_ctx *c, uint32_t n, const ms_pod_rec *pods, ms_result *results, hipStream_t s) {
    CommState &m = *c->comm;
    const uint32_t W = seq_window();
    int rc = seq_ensure(c, W);
    if (rc) return rc;
    const uint32_t seed32 = seed32_of(c->cfg.seed);
    MS_HIP(c, hipMemsetAsync(m.ctl, 0, 4 * sizeof(uint32_t), s));
    const size_t cand_bytes = (size_t)W * kTopKCands * sizeof(ms_seq_cand);
    uint32_t known = 0;
    while (known < n) {
        const uint32_t r = cdiv(n - known, W);  // windows that may finish the queue
        for (uint32_t i = 0; i < r; ++i) {
            MS_HIP(c, launch_seq_window_in(pods, n, m.ctl, m.win_pods, W, s));
            rc = seq_candidates_locked(c, W, m.win_pods, m.cands, m.sflags, s);
            if (rc) return rc;
            ncclResult_t e = CCL(ncclGroupStart)();
            if (e == ncclSuccess) e = CCL(ncclAllGather)(m.cands, m.cands_all, cand_bytes, ncclUint8, m.comm, s);
            if (e == ncclSuccess) e = CCL(ncclAllGather)(m.sflags, m.sflags_all, W, ncclUint32, m.comm, s);
            const ncclResult_t e2 = CCL(ncclGroupEnd)();
            if (e == ncclSuccess) e = e2;
            if (e != ncclSuccess) return fail(c, MS_E_RCCL, std::string("sequential all-gather: ") + CCL(ncclGetErrorString)(e));
            MS_HIP(c, launch_seq_validate_rep(c->t, W, m.win_pods, seed32, (uint32_t)m.world, m.cands_all, m.sflags_all,
                                              m.merged, m.merged_flags, m.win_res, m.ctl + 2, s, m.ctl + 1));
            MS_HIP(c, launch_seq_window_out(m.win_res, m.ctl, results, n, s));
            ++m.seq_windows;
        }
        MS_HIP(c, hipMemcpyAsync(m.h_ctl, m.ctl, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MS_HIP(c, hipStreamSynchronize(s));
        ++m.seq_rounds;
        const uint32_t now = m.h_ctl[0];
        if (now <= known || now > n) return fail(c, MS_E_HIP, "sharded sequential cycle made no progress");
        known = now;
    }
    return MS_OK;
}

// The batched cycle of all n pods with every result on every rank: submit +
// drain (this rank's slice into stage + first), one all-gather of the slices
// (in place: slices are contiguous in pod order), then this shard's binds.
int batched_all_locked(ms_ctx *c, uint32_t n, const ms_pod_rec *pods, ms_result *stage, hipStream_t s, bool commit) {
    CommState &m = *c->comm;
    uint32_t first = 0, count = 0;
    slice_of(m, n, first, count);
    const uint32_t per = cdiv(n, (uint32_t)m.world);
    int rc = submit_locked(c, n, pods, stage + first, s);
    if (rc) return rc;
    rc = drain_to(c, s);
    if (rc) return rc;
    // (a rank whose slice is short or empty sends entries past n: never read)
    const size_t bytes = (size_t)per * sizeof(ms_result);
    MS_NCCL(c, CCL(ncclAllGather)(reinterpret_cast<char *>(stage) + (size_t)m.rank * bytes, stage, bytes, ncclUint8, m.comm, s));
    if (commit) MS_HIP(c, launch_apply_binds(c->t, pods, n, stage, s));  // NodeInfo.AddPod on this shard's winners
    return MS_OK;
}

}  // namespace

void comm_rank_world(const ms_ctx *c, int32_t *rank, int32_t *world) {
    *rank = c->comm ? c->comm->rank : 0;
    *world = c->comm ? c->comm->world : 0;
}

int comm_fence_reads(ms_ctx *c, hipStream_t writer) {
    if (!c->comm) return 0;
    const int rc = flush_stash(c);  // the stashed batch's sweep reads the table before this writer
    if (rc) return rc;
    const int fenced = c->comm->order.fence(writer);
    if (fenced < 0) return fail(c, MS_E_HIP, std::string("stream ordering (fence): ") + hipGetErrorString(hipGetLastError()));
    return fenced;
}

int comm_drain_to(ms_ctx *c, hipStream_t s) { return drain_to(c, s); }

int comm_all_gather(ms_ctx *c, const void *send, void *recv, size_t bytes, hipStream_t s) {
    MS_NCCL(c, CCL(ncclAllGather)(send, recv, bytes, ncclUint8, c->comm->comm, s));
    return MS_OK;
}

void comm_free(ms_ctx *c) {
    delete c->comm;
    c->comm = nullptr;
}

int comm_cycle_staged(ms_ctx *c, uint32_t n, int32_t mode) {
    CommState &m = *c->comm;
    const hipStream_t s = c->stream;
    c->order.wrote_ctx();  // binds below write the table on the context stream
    if (mode == MS_MODE_SEQUENTIAL && !plugins_stateless(c)) return seq_sharded_locked(c, n, c->d_pods, c->d_res, s);
    (void)m;
    return batched_all_locked(c, n, c->d_pods, c->d_res, s, true);
}

int comm_stage(ms_ctx *c, uint32_t n) {
    CommState &m = *c->comm;
    int rc = drain_to(c, c->stream);  // device-resident batches in flight finish first
    if (rc) return rc;
    const uint32_t per = cdiv(n, (uint32_t)m.world);
    return ensure_stage(c, std::max<uint32_t>(n, per * (uint32_t)m.world));
}

int comm_schedule_host(ms_ctx *c, uint32_t n, const ms_pod_rec *pods, int32_t mode, ms_result *out, CallClock *ck) {
    const hipStream_t s = c->stream;
    int rc = comm_stage(c, n);
    if (rc) return rc;
    ck->lap(MS_PH_ALLOC);
    ck->count(MS_PH_CHUNKS);
    MS_HIP(c, hipMemcpyAsync(c->d_pods, pods, sizeof(ms_pod_rec) * n, hipMemcpyHostToDevice, s));
    ck->lap(MS_PH_STAGE_IN);
    rc = comm_cycle_staged(c, n, mode);
    if (rc) return rc;
    ck->lap(MS_PH_LAUNCH);
    MS_HIP(c, hipMemcpyAsync(out, c->d_res, sizeof(ms_result) * n, hipMemcpyDeviceToHost, s));
    ck->lap(MS_PH_STAGE_OUT);
    MS_HIP(c, hipStreamSynchronize(s));
    ck->lap(MS_PH_WAIT);
    return MS_OK;
}

int comm_schedule_device(ms_ctx *c, uint32_t n, const ms_pod_rec *pods_dev, ms_result *results_dev, hipStream_t s) {
    CommState &m = *c->comm;
    if (!plugins_stateless(c)) return seq_sharded_locked(c, n, pods_dev, results_dev, s);
    // NU+NN / NodeAffinity: the batched cycle with its binds (equal to the queue-order loop)
    const uint32_t per = cdiv(n, (uint32_t)m.world);
    int rc = drain_to(c, s);
    if (rc) return rc;
    rc = ensure_stage(c, per * (uint32_t)m.world);
    if (rc) return rc;
    rc = batched_all_locked(c, n, pods_dev, c->d_res, s, true);
    if (rc) return rc;
    MS_HIP(c, hipMemcpyAsync(results_dev, c->d_res, sizeof(ms_result) * n, hipMemcpyDeviceToDevice, s));
    return MS_OK;
}

namespace {

// The communicator's streams (the ordering class makes its events as it first
// records them), then the rendezvous of the ranks.
int comm_setup(ms_ctx *c, CommState &m, const ms_comm_id *id, int32_t rank, int32_t world) {
    // The collective and decode streams get the highest priority: high-priority
    // streams are served by hardware queues of their own, so the caller's
    // (sweep) stream can never share a queue with them and serialise a
    // reduce-scatter or a decode behind the next sweep; their short kernels are
    // dispatched ahead of the sweep's pending workgroups (profiles/r03zc_comm_prio_ab.txt).
    int lo = 0, hi = 0;
    MS_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    const int cprio = hi;
    MS_HIP(c, made(m.cs.ensure(hipStreamNonBlocking, cprio)));
    // (MINISCHED_SHARD_STREAMS=2 only) two sweep streams at normal priority (at the
    // highest, the collectives fell behind)
    if (m.order.two_streams())
        for (Stream &q : m.ss) MS_HIP(c, made(q.ensure(hipStreamNonBlocking, 0)));
    MS_HIP(c, made(m.ds.ensure(hipStreamNonBlocking, cprio)));
    m.order.attach(c->stream, m.cs, m.ds, m.ss[0], m.ss[1]);
    ncclUniqueId uid;
    std::memcpy(&uid, id->internal, sizeof(uid));
    const ncclResult_t r = CCL(ncclCommInitRank)(&m.comm, world, uid, rank);
    if (r != ncclSuccess) {
        m.comm = nullptr;
        return fail(c, MS_E_RCCL, std::string("ncclCommInitRank: ") + CCL(ncclGetErrorString)(r));
    }
    return MS_OK;
}

}  // namespace

}  // namespace msgpu

using namespace msgpu;

extern "C" {

int ms_comm_id_create(ms_comm_id *out) {
    if (!out) return MS_E_INVAL;
    ncclUniqueId id;
    const ncclResult_t r = CCL(ncclGetUniqueId)(&id);
    if (r != ncclSuccess) return fail(nullptr, MS_E_RCCL, std::string("ncclGetUniqueId: ") + CCL(ncclGetErrorString)(r));
    std::memcpy(out->internal, &id, sizeof(id));
    return MS_OK;
}

int ms_comm_plugin_set_supported(int32_t plugin_set) {
    return plugin_set >= MS_PLUGINS_NU_NN && plugin_set <= MS_PLUGINS_NU_NN_NAM ? 1 : 0;
}

int ms_comm_init(ms_ctx *c, const ms_comm_id *id, int32_t rank, int32_t world) {
    if (!c || !id || world < 1 || rank < 0 || rank >= world) return MS_E_INVAL;
    std::lock_guard<std::mutex> g(c->sched_mu);
    if (c->comm) return fail(c, MS_E_INVAL, "ms_comm_init: the context already has a communicator");
    MS_HIP(c, hipSetDevice(c->cfg.device));
    bool two_streams = false;
    if (const char *e = getenv("MINISCHED_SHARD_STREAMS")) two_streams = atoi(e) == 2;
    CommState *m = new (std::nothrow) CommState(4, two_streams);  // (depth + 1 <= kPipeMax buffer sets)
    if (!m) return fail(c, MS_E_OOM, "ms_comm_init: host allocation");
    m->rank = rank;
    m->world = world;
    if (const char *e = getenv("MINISCHED_HOST_PROF")) m->host_prof = atoi(e) == 1;
    if (const char *e = getenv("MINISCHED_SHARD_COALESCE")) m->coalesce = atoi(e) != 0;
    // Attached before the streams exist (MS_HIP reports through the context);
    // every failure below goes through comm_free, so a context is either joined
    // or left without a communicator, never half-built.
    c->comm = m;
    const int rc = comm_setup(c, *m, id, rank, world);
    if (rc != MS_OK) comm_free(c);
    return rc;
}

int ms_sharded_slice(const ms_ctx *c, uint32_t n, uint32_t *first, uint32_t *count) {
    if (!c || !first || !count) return MS_E_INVAL;
    if (!c->comm) {
        *first = 0;
        *count = n;
        return MS_OK;
    }
    slice_of(*c->comm, n, *first, *count);
    return MS_OK;
}

int ms_sharded_submit(ms_ctx *c, uint32_t n, const ms_pod_rec *pods_dev, ms_result *results_dev, void *stream) {
    if (!c || (n && !pods_dev)) return MS_E_INVAL;
    if (!c->comm) return fail(c, MS_E_INVAL, "ms_sharded_submit: the context has no communicator (ms_comm_init)");
    if (n == 0) return MS_OK;
    std::lock_guard<std::mutex> g(c->sched_mu);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    uint32_t first = 0, count = 0;
    slice_of(*c->comm, n, first, count);
    if (count && !results_dev) return fail(c, MS_E_INVAL, "ms_sharded_submit: results_dev is required");
    int rc = flush_locked(c);
    if (rc) return rc;
    return submit_locked(c, n, pods_dev, results_dev, pick_stream(c, stream));
}

int ms_sharded_drain(ms_ctx *c, void *stream) {
    if (!c) return MS_E_INVAL;
    if (!c->comm) return fail(c, MS_E_INVAL, "ms_sharded_drain: the context has no communicator (ms_comm_init)");
    std::lock_guard<std::mutex> g(c->sched_mu);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    return drain_to(c, pick_stream(c, stream));
}

}  // extern "C"

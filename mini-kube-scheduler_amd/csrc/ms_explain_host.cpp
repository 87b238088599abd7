// ms_explain_host.cpp — ms_explain_device / ms_explain (minisched_gpu.h): the
// argument checks, the scratch of the three stages (ms_explain.hip) and, for
// host arrays, the chunked staging. Both are ordered calls (ms_ctx.h
// OrderedCall): deltas drained, the caller's stream after the context stream,
// the call's work chained back.
// ms_explain_sharded_device / ms_explain_sharded: the same on contexts joined to
// a communicator, collective over the ranks: the sharded pipeline drained onto
// the call's stream, then the stages and two all-gathers (the per-shard records,
// the best keys; ms_comm.cpp comm_all_gather) on that one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ms_ctx.h"

namespace msgpu {

namespace {

constexpr size_t kExplainStageBytes = 64ull << 20;  // ms_explain's device staging of rows

// Explain scratch of at least `need` bytes: grown after a device synchronise
// (an earlier explain on a caller stream may still use the old block), the
// capacity zero while the buffer is not there.
int ensure_explain(ms_ctx *c, size_t need) {
    if (need <= c->explain_bytes) return MS_OK;
    if (c->d_explain) MS_HIP(c, hipDeviceSynchronize());
    c->explain_bytes = 0;
    if (!c->d_explain.alloc(need)) return fail(c, MS_E_OOM, "explain scratch");
    c->explain_bytes = need;
    return MS_OK;
}

int check_args(ms_ctx *c, const char *who, uint32_t n_pods, const void *pods, uint32_t first, uint32_t n_nodes,
               const void *rows, const void *sums) {
    if (!c) return MS_E_INVAL;
    const std::string w(who);
    if (n_pods > MS_EXPLAIN_MAX_PODS) return fail(c, MS_E_INVAL, w + ": at most MS_EXPLAIN_MAX_PODS pods per call");
    if (c->comm)
        return fail(c, MS_E_INVAL, w + ": single-shard call on a sharded context (a row's final scores need the "
                                       "other shards' LIST context)");
    if (!rows && !sums) return fail(c, MS_E_INVAL, w + ": rows and summaries are both NULL");
    if (n_pods && !pods) return fail(c, MS_E_INVAL, w + ": pods is NULL");
    if (rows && n_nodes &&
        (first < c->cfg.node_base || (uint64_t)first - c->cfg.node_base + n_nodes > c->cfg.max_nodes))
        return fail(c, MS_E_CAPACITY, w + ": window outside the context's node range");
    return MS_OK;
}

// What every explain launch of the context shares: the table, the set and its tables.
ExplainArgs args_of(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods) {
    ExplainArgs a;
    a.t = c->t;
    a.n_rows = c->rows_dev;
    a.plugin_set = c->cfg.plugin_set;
    a.pods = d_pods;
    a.n_pods = n_pods;
    a.seed32 = seed32_of(c->cfg.seed);
    a.w_nn = c->w_nn;
    a.w_na = c->w_na;
    a.sets = c->d_terms;
    a.n_sets = c->n_terms;
    return a;
}

// One explain of device-resident pods on s (the caller holds the ordered call):
// rows (device, n_pods x n_nodes, or null) and, with want_sums, the summaries
// left in the scratch (explain_summaries).
int explain_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, uint32_t first, uint32_t n_nodes,
                   ms_explain_row *d_rows, bool want_sums, hipStream_t s) {
    ExplainArgs a = args_of(c, n_pods, d_pods);
    a.rows = n_nodes ? d_rows : nullptr;
    a.win_lo = a.rows ? first - c->cfg.node_base : 0u;
    a.win_n = a.rows ? n_nodes : 0u;
    a.summaries = want_sums;
    if (!a.rows && !a.summaries) return MS_OK;  // (an empty window alone)
    const uint32_t extent = explain_extent(a.n_rows, a.win_lo, a.win_n, a.rows != nullptr);
    const int rc = ensure_explain(c, explain_scratch_bytes(a.plugin_set, extent, n_pods));
    if (rc) return rc;
    a.scratch = c->d_explain;
    MS_HIP(c, launch_explain(a, s));
    return MS_OK;
}

// ---- node shards: ms_explain_sharded_device / ms_explain_sharded -------------
// Every check of a collective call, before any collective is issued: a rank whose
// arguments fail issues none, so the ranks of one call pass arguments that fail
// or pass alike (a caller obligation, stated in the header).
int check_sharded(ms_ctx *c, const char *who, uint32_t n_pods, const void *pods, uint32_t first, uint32_t n_nodes,
                  const void *rows) {
    if (!c) return MS_E_INVAL;
    const std::string w(who);
    // (what the context is comes before what the call asks of it)
    if (!c->comm)
        return fail(c, MS_E_INVAL, w + ": the context has no communicator (ms_comm_init); a single-shard context "
                                       "is served by ms_explain / ms_explain_device");
    if (n_pods > MS_EXPLAIN_MAX_PODS) return fail(c, MS_E_INVAL, w + ": at most MS_EXPLAIN_MAX_PODS pods per call");
    if (rows && n_nodes &&
        (first < c->cfg.node_base || (uint64_t)first - c->cfg.node_base + n_nodes > c->cfg.max_nodes))
        return fail(c, MS_E_CAPACITY, w + ": window outside the context's node range");
    if (n_pods && !pods) return fail(c, MS_E_INVAL, w + ": pods is NULL");
    return MS_OK;
}

// The call's arguments for all n_pods device-resident pods; the window counts
// only when rows are asked for. The scratch is grown here, before any collective.
int sharded_args(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, uint32_t first, uint32_t n_nodes,
                 bool want_rows, ExplainArgs &a) {
    a = args_of(c, n_pods, d_pods);
    a.win_lo = want_rows ? first - c->cfg.node_base : 0u;
    a.win_n = want_rows ? n_nodes : 0u;
    int32_t rank = 0, world = 0;
    comm_rank_world(c, &rank, &world);
    a.n_shards = (uint32_t)world;
    a.shard = (uint32_t)rank;
    const int rc = ensure_explain(c, explain_shard_scratch_bytes(a));
    if (rc) return rc;
    a.scratch = c->d_explain;
    return MS_OK;
}

// Up to the rows: this shard's records of all pods, the first all-gather (in
// place, n_pods records per rank whatever the rank asked for), the seeded scan.
int sharded_scan(ms_ctx *c, const ExplainArgs &a, hipStream_t s) {
    MS_HIP(c, launch_explain_shard(a, kExShardRecords, 0, a.n_pods, s));
    const ExplainExchange x = explain_exchange(a);
    const size_t bytes = x.record_bytes * a.n_pods;
    const int rc = comm_all_gather(c, static_cast<const char *>(x.records) + a.shard * bytes, x.records, bytes, s);
    if (rc) return rc;
    MS_HIP(c, launch_explain_shard(a, kExShardScan, 0, a.n_pods, s));
    return MS_OK;
}

// After the rows of every pod: this shard's best keys, the second all-gather
// (n_pods keys per rank), the maximum over the shards into the summaries.
int sharded_best(ms_ctx *c, const ExplainArgs &a, hipStream_t s) {
    MS_HIP(c, launch_explain_shard(a, kExShardBest, 0, a.n_pods, s));
    const ExplainExchange x = explain_exchange(a);
    const int rc = comm_all_gather(c, x.best + (size_t)a.shard * a.n_pods, x.best, sizeof(*x.best) * a.n_pods, s);
    if (rc) return rc;
    MS_HIP(c, launch_explain_shard(a, kExShardMax, 0, a.n_pods, s));
    return MS_OK;
}

}  // namespace

}  // namespace msgpu

using namespace msgpu;

extern "C" {

int ms_explain_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t first, uint32_t n_nodes,
                      ms_explain_row *rows_dev, ms_explain_summary *summaries_dev, void *stream) {
    int rc = check_args(c, "ms_explain_device", n_pods, pods_dev, first, n_nodes, rows_dev, summaries_dev);
    if (rc) return rc;
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    rc = explain_locked(c, n_pods, pods_dev, first, n_nodes, rows_dev, summaries_dev != nullptr, s);
    if (rc) return rc;
    if (summaries_dev)
        MS_HIP(c, hipMemcpyAsync(summaries_dev, explain_summaries(c->d_explain), sizeof(ms_explain_summary) * n_pods,
                                 hipMemcpyDeviceToDevice, s));
    return call.done();
}

int ms_explain(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods, uint32_t first, uint32_t n_nodes,
               ms_explain_row *rows, ms_explain_summary *summaries) {
    int rc = check_args(c, "ms_explain", n_pods, pods, first, n_nodes, rows, summaries);
    if (rc) return rc;
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, nullptr);  // the context stream
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    const bool want_rows = rows && n_nodes;
    // pods per chunk: the chunk's rows stay within the staging budget
    uint32_t chunk = n_pods;
    if (want_rows)
        chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_pods, kExplainStageBytes / ((size_t)n_nodes * sizeof(ms_explain_row))));
    if (!c->d_ex_pods && !c->d_ex_pods.alloc(MS_EXPLAIN_MAX_PODS)) return fail(c, MS_E_OOM, "explain pod staging");
    const size_t need_rows = want_rows ? (size_t)chunk * n_nodes : 0;
    if (need_rows > c->ex_rows_cap) {
        if (c->d_ex_rows) MS_HIP(c, hipDeviceSynchronize());
        c->ex_rows_cap = 0;
        if (!c->d_ex_rows.alloc(need_rows)) return fail(c, MS_E_OOM, "explain row staging");
        c->ex_rows_cap = need_rows;
    }
    for (uint32_t p0 = 0; p0 < n_pods; p0 += chunk) {
        const uint32_t nb = std::min(chunk, n_pods - p0);
        MS_HIP(c, hipMemcpyAsync(c->d_ex_pods, pods + p0, sizeof(ms_pod_rec) * nb, hipMemcpyHostToDevice, s));
        rc = explain_locked(c, nb, c->d_ex_pods, first, n_nodes, want_rows ? c->d_ex_rows.get() : nullptr,
                            summaries != nullptr, s);
        if (rc) return rc;
        if (want_rows)
            MS_HIP(c, hipMemcpyAsync(rows + (size_t)p0 * n_nodes, c->d_ex_rows, sizeof(ms_explain_row) * nb * n_nodes,
                                     hipMemcpyDeviceToHost, s));
        if (summaries)
            MS_HIP(c, hipMemcpyAsync(summaries + p0, explain_summaries(c->d_explain), sizeof(ms_explain_summary) * nb,
                                     hipMemcpyDeviceToHost, s));
        // the staging buffers are reused by the next chunk, and the caller's arrays are complete on return
        MS_HIP(c, hipStreamSynchronize(s));
    }
    return call.done();
}

int ms_explain_sharded_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t first, uint32_t n_nodes,
                              ms_explain_row *rows_dev, ms_explain_summary *summaries_dev, void *stream) {
    int rc = check_sharded(c, "ms_explain_sharded_device", n_pods, pods_dev, first, n_nodes, rows_dev);
    if (rc) return rc;
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    rc = comm_drain_to(c, s);  // the stages and both collectives run on s, after the sharded pipeline
    if (rc) return rc;
    ExplainArgs a;
    rc = sharded_args(c, n_pods, pods_dev, first, n_nodes, rows_dev && n_nodes, a);
    if (rc) return rc;
    rc = sharded_scan(c, a, s);
    if (rc) return rc;
    a.rows = a.win_n ? rows_dev : nullptr;
    MS_HIP(c, launch_explain_shard(a, kExShardRows, 0, n_pods, s));
    rc = sharded_best(c, a, s);
    if (rc) return rc;
    if (summaries_dev)
        MS_HIP(c, hipMemcpyAsync(summaries_dev, explain_summaries(c->d_explain), sizeof(ms_explain_summary) * n_pods,
                                 hipMemcpyDeviceToDevice, s));
    return call.done();
}

int ms_explain_sharded(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods, uint32_t first, uint32_t n_nodes,
                       ms_explain_row *rows, ms_explain_summary *summaries) {
    int rc = check_sharded(c, "ms_explain_sharded", n_pods, pods, first, n_nodes, rows);
    if (rc) return rc;
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, nullptr);  // the context stream
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    rc = comm_drain_to(c, s);
    if (rc) return rc;
    const bool want_rows = rows && n_nodes;
    // The exchange and the scan run once for all pods; only the row stage and its
    // copies go in pod chunks under ms_explain's staging rule, so the chunking
    // never changes the number or size of the collectives (a rank's window is its own).
    uint32_t chunk = n_pods;
    if (want_rows)
        chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_pods, kExplainStageBytes / ((size_t)n_nodes * sizeof(ms_explain_row))));
    if (!c->d_ex_pods && !c->d_ex_pods.alloc(MS_EXPLAIN_MAX_PODS)) return fail(c, MS_E_OOM, "explain pod staging");
    const size_t need_rows = want_rows ? (size_t)chunk * n_nodes : 0;
    if (need_rows > c->ex_rows_cap) {
        if (c->d_ex_rows) MS_HIP(c, hipDeviceSynchronize());
        c->ex_rows_cap = 0;
        if (!c->d_ex_rows.alloc(need_rows)) return fail(c, MS_E_OOM, "explain row staging");
        c->ex_rows_cap = need_rows;
    }
    ExplainArgs a;
    rc = sharded_args(c, n_pods, c->d_ex_pods, first, n_nodes, want_rows, a);
    if (rc) return rc;
    MS_HIP(c, hipMemcpyAsync(c->d_ex_pods, pods, sizeof(ms_pod_rec) * n_pods, hipMemcpyHostToDevice, s));
    rc = sharded_scan(c, a, s);
    if (rc) return rc;
    a.rows = want_rows ? c->d_ex_rows.get() : nullptr;
    for (uint32_t p0 = 0; p0 < n_pods; p0 += chunk) {
        const uint32_t nb = std::min(chunk, n_pods - p0);
        MS_HIP(c, launch_explain_shard(a, kExShardRows, p0, nb, s));
        if (!want_rows) continue;
        MS_HIP(c, hipMemcpyAsync(rows + (size_t)p0 * n_nodes, c->d_ex_rows, sizeof(ms_explain_row) * nb * n_nodes,
                                 hipMemcpyDeviceToHost, s));
        if (p0 + nb < n_pods) MS_HIP(c, hipStreamSynchronize(s));  // the staging is reused by the next chunk
    }
    rc = sharded_best(c, a, s);
    if (rc) return rc;
    if (summaries)
        MS_HIP(c, hipMemcpyAsync(summaries, explain_summaries(c->d_explain), sizeof(ms_explain_summary) * n_pods,
                                 hipMemcpyDeviceToHost, s));
    MS_HIP(c, hipStreamSynchronize(s));  // the caller's arrays are complete on return
    return call.done();
}

}  // extern "C"

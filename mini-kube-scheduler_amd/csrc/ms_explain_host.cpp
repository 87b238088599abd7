// ms_explain_host.cpp — ms_explain_device / ms_explain (minisched_gpu.h): the
// argument checks, the scratch of the three stages (ms_explain.hip) and, for
// host arrays, the chunked staging. Both are ordered calls (ms_ctx.h
// OrderedCall): deltas drained, the caller's stream after the context stream,
// the call's work chained back.
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

// One explain of device-resident pods on s (the caller holds the ordered call):
// rows (device, n_pods x n_nodes, or null) and, with want_sums, the summaries
// left in the scratch (explain_summaries).
int explain_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, uint32_t first, uint32_t n_nodes,
                   ms_explain_row *d_rows, bool want_sums, hipStream_t s) {
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

}  // extern "C"

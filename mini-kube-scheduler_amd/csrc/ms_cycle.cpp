// ms_cycle.cpp — the per-plugin-set cycle drivers on device-resident pods
// (sweep, select, decode; the TaintToleration and multi-term NodeAffinity
// cycles with their scratch) and the device entry points over them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ms_ctx.h"
#include "ms_nam_layout.h"

namespace msgpu {

// MS_PLUGINS_NU_TT_NN scratch: `need` bytes (summaries or the two-pass cycle's).
// As every grow routine: the capacity stays zero while the buffer is not
// there, so a failed growth is retried by the next call.
int ensure_tt(ms_ctx *c, size_t need) {
    if (need <= c->tt_bytes) return MS_OK;
    // (growing: the previous scratch may still be read by work on the sweep,
    // collective or decode streams of a node-sharded cycle)
    if (c->d_tt) MS_HIP(c, hipDeviceSynchronize());
    c->tt_bytes = 0;
    if (!c->d_tt.alloc(need)) return fail(c, MS_E_OOM, "TaintToleration scratch");
    c->tt_bytes = need;
    return MS_OK;
}

// d_tt is one scratch for every TT cycle of the context (ms_ctx.h ev_tt): a
// cycle on another stream than the previous one waits for that one's end.
int tt_take(ms_ctx *c, hipStream_t s) {
    MS_HIP(c, made(c->ev_tt.ensure()));
    if (c->tt_stream && c->tt_stream != s) MS_HIP(c, hipStreamWaitEvent(s, c->ev_tt, 0));
    return MS_OK;
}

int tt_release(ms_ctx *c, hipStream_t s) {
    MS_HIP(c, hipEventRecord(c->ev_tt, s));
    c->tt_stream = s;
    return MS_OK;
}

// The batch's per-pod summaries of every row segment, merged in LIST order into
// out (this shard's summary), or finalised into results (the single-shard
// cycle; commit: the winners' NodeInfo.AddPod). Chunks of batch_cap pods.
// A single-shard cycle (results) runs the two-pass bit-sliced form (round 5,
// launch_tt2_cycle); the shard summaries (out, ms_tt_summaries_device) the
// per-pair summary sweep.
int tt_cycle_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, void *out, ms_result *results, int commit,
                    hipStream_t s) {
    const bool two_pass = !out;
    const uint32_t B = c->batch_cap, segs = tt_segments(c->rows_dev), cap = std::min(B, n_pods);
    int rc = ensure_tt(c, two_pass ? tt2_scratch_bytes(c->rows_dev, cap)
                                   : (size_t)segs * cap * MS_TT_SUMMARY_BYTES);
    if (rc) return rc;
    // the previous cycle's sweep/combine on another stream still owns d_tt
    rc = tt_take(c, s);
    if (rc) return rc;
    const uint32_t seed32 = seed32_of(c->cfg.seed);
    if (two_pass) MS_HIP(c, launch_tt2_planes(c->t, c->rows_dev, c->d_tt, s));
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        if (two_pass) {
            MS_HIP(c, launch_tt2_cycle(c->t, c->rows_dev, d_pods + s0, nb, seed32, c->d_tt, cap, results + s0, commit,
                                       s));
            continue;
        }
        MS_HIP(c, launch_tt_sweep(c->t, c->rows_dev, d_pods + s0, nb, seed32, c->d_tt, s));
        MS_HIP(c, launch_tt_combine(c->d_tt, nb, segs, d_pods + s0, nb, seed32,
                                    out ? static_cast<char *>(out) + (size_t)s0 * MS_TT_SUMMARY_BYTES : nullptr,
                                    out ? nullptr : results + s0, c->t, commit, s));
    }
    return tt_release(c, s);
}

// MS_PLUGINS_NU_NN_NAM: a call's plan (ms_nam_layout.h): pods per chunk, the ONE
// layout every chunk of the call is carved with, the node-shard inputs behind
// it, and the allocation. A short last chunk keeps the plan's layout: one of
// its own pod count can have more row segments and need more scratch than the
// context holds (tests/cpp/test_nam_layout.cpp, tests/test_gpu_chunks.py).
static NamPlan nam_plan_for(const ms_ctx *c, uint32_t n_pods) {
    return nam_plan(c->batch_cap, c->rows_dev, c->n_terms, n_pods);
}

// Scratch for the plan: its layout's arrays, plus one record (the later shards'
// table) and one byte (an earlier shard has a non-zero node) per pod of a
// chunk (per class under the whole-batch plan). One scratch serves every NAM
// call of the context; each takes it on its stream (nam_take / nam_release).
static int ensure_nam(ms_ctx *c, const NamPlan &plan) {
    const size_t need = plan.alloc;
    if (need <= c->nam_bytes) return MS_OK;
    // (growing: a NodeAffinity call on a caller stream may still read the tables; as ensure_tt)
    if (c->d_nam) MS_HIP(c, hipDeviceSynchronize());
    c->nam_bytes = 0;
    if (!c->d_nam.alloc(need)) return fail(c, MS_E_OOM, "NodeAffinity scratch");
    c->nam_bytes = need;
    return MS_OK;
}

// d_nam is one scratch for every NAM cycle of the context (ms_ctx.h ev_nam): a
// cycle on another stream than the previous one waits for that one's end.
int nam_take(ms_ctx *c, hipStream_t s) {
    MS_HIP(c, made(c->ev_nam.ensure()));
    if (c->nam_stream && c->nam_stream != s) MS_HIP(c, hipStreamWaitEvent(s, c->ev_nam, 0));
    return MS_OK;
}

int nam_release(ms_ctx *c, hipStream_t s) {
    MS_HIP(c, hipEventRecord(c->ev_nam, s));
    c->nam_stream = s;
    return MS_OK;
}

// The in-library node-sharded cycle (ms_comm.cpp nam_sharded_sweep): the batch
// as one chunk under the whole-batch plan, one record per class exchanged.
static NamPlan nam_shard_plan(const ms_ctx *c, uint32_t n_pods) {
    return nam_plan_whole(c->rows_dev, c->n_terms, n_pods);
}

uint32_t nam_shard_classes(const ms_ctx *c, uint32_t n_pods) { return nam_class_cap(std::max(1u, n_pods), c->n_terms); }

int nam_shard_begin(ms_ctx *c, uint32_t n_pods, hipStream_t s) {
    const int rc = ensure_nam(c, nam_shard_plan(c, n_pods));
    return rc ? rc : nam_take(c, s);
}

int nam_shard_segment(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, void *cls_mine, hipStream_t s) {
    const NamPlan plan = nam_shard_plan(c, n_pods);
    if (c->rows_dev == 0) {  // no rows: identity maps, no non-zero node, no filter bits
        MS_HIP(c, launch_nam_identity(cls_mine, plan.L.cls_max, s));
        return MS_OK;
    }
    MS_HIP(c, launch_nam_class_segment(c->t, c->rows_dev, d_pods, n_pods, c->d_terms, c->n_terms, plan.L, c->d_nam,
                                       cls_mine, s));
    return MS_OK;
}

int nam_shard_keys(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, const void *cls_all, uint32_t n_shards,
                   uint32_t shard_index, unsigned long long *keys, uint32_t *flags, hipStream_t s) {
    if (c->rows_dev == 0) {  // (as nam_keys_locked: key 0, no filter saw a row)
        MS_HIP(c, launch_fill_keys(keys, n_pods, 0ull, s));
        MS_HIP(c, hipMemsetAsync(flags, 0, sizeof(uint32_t) * n_pods, s));
        return MS_OK;
    }
    const NamPlan plan = nam_shard_plan(c, n_pods);
    char *base = static_cast<char *>(c->d_nam.get());
    MS_HIP(c, launch_nam_class_keys(c->t, c->rows_dev, d_pods, n_pods, c->d_terms, c->n_terms, seed32_of(c->cfg.seed),
                                    c->w_nn, c->w_na, cls_all, n_shards, shard_index, c->present_dev ? 1u : 0u, plan.L,
                                    c->d_nam, base + plan.after, reinterpret_cast<uint8_t *>(base + plan.m_in), keys,
                                    flags, s));
    return MS_OK;
}

// This shard's packed keys of a chunk of nb pods into keys, carved with the
// call's layout L (the one ensure_nam sized the scratch for): per class its
// rows' normalised scores under the later segments' and (after / m_in, node
// shards) the later shards' rescales, then per pod the best key. flags
// (optional): per pod which filters rejected a present row of this context, the
// word the decode takes (no rows: zero).
static int nam_keys_locked(ms_ctx *c, const NamLayout &L, uint32_t nb, const ms_pod_rec *d_pods, const void *after,
                           const uint8_t *m_in, unsigned long long *keys, uint32_t *flags, hipStream_t s) {
    if (c->rows_dev == 0) {
        MS_HIP(c, launch_fill_keys(keys, nb, 0ull, s));
        if (flags) MS_HIP(c, hipMemsetAsync(flags, 0, sizeof(uint32_t) * nb, s));
        return MS_OK;
    }
    MS_HIP(c, launch_nam_keys(c->t, c->rows_dev, d_pods, nb, c->d_terms, c->n_terms, seed32_of(c->cfg.seed), c->w_nn,
                              c->w_na, after, m_in, c->present_dev ? 1u : 0u, L, c->d_nam, keys, flags, s));
    return MS_OK;
}

// The single-shard NAM cycle: keys and filter flags per chunk, decode, and with
// commit each winner's NodeInfo.AddPod (stateless: no later pod reads it).
static int nam_cycle_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, ms_result *d_res, int commit,
                            hipStream_t s) {
    const NamPlan plan = nam_plan_for(c, n_pods);
    const uint32_t B = plan.chunk;
    int rc = ensure_nam(c, plan);
    if (rc) return rc;
    rc = nam_take(c, s);
    if (rc) return rc;
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        rc = nam_keys_locked(c, plan.L, nb, d_pods + s0, nullptr, nullptr, c->d_keys, c->d_flags, s);
        if (rc) return rc;
        MS_HIP(c, launch_decode(d_pods + s0, nb, c->d_keys, c->d_flags, c->present_dev, d_res + s0, s));
        if (commit) MS_HIP(c, launch_apply_binds(c->t, d_pods + s0, nb, d_res + s0, s));
    }
    return nam_release(c, s);
}

// This shard's keys (and filter flags for the resource-aware set) for a batch.
int sweep_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, unsigned long long *keys, uint32_t *flags,
                 hipStream_t s, hipEvent_t done) {
    const uint32_t seed32 = seed32_of(c->cfg.seed);
    if (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN)
        return fail(c, MS_E_INVAL, "TaintToleration shards combine by summaries (ms_tt_summaries_device), not keys");
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "multi-term NodeAffinity shards exchange rescale tables first "
                                   "(ms_nam_segment_device, ms_nam_keys_device)");
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN) {
        MS_HIP(c, launch_sweep_pp(c->t, c->d_cand, c->rows_dev, d_pods, n_pods, seed32, keys, nullptr, c->present_dev,
                                  c->num_cus, s, 0, done));
        return MS_OK;
    } else if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NA) {
        MS_HIP(c, launch_fill_keys(keys, n_pods, c->present_dev ? kKeyListed : 0ull, s));
        MS_HIP(c, hipMemsetAsync(flags, 0, sizeof(uint32_t) * n_pods, s));
        MS_HIP(c, launch_sweep_na(c->t, c->rows_dev, d_pods, n_pods, seed32, c->w_nn, c->w_na, keys, flags,
                                  c->num_cus, s));
    } else {
        MS_HIP(c, launch_fill_keys(keys, n_pods, c->present_dev ? kKeyListed : 0ull, s));
        if (flags) MS_HIP(c, hipMemsetAsync(flags, 0, sizeof(uint32_t) * n_pods, s));
        MS_HIP(c, launch_sweep_full(c->t, c->rows_dev, d_pods, n_pods, seed32, keys, flags, c->num_cus, s));
    }
    if (done) MS_HIP(c, hipEventRecord(done, s));
    return MS_OK;
}

// Combined keys (+ flags / anchors) -> ms_result for this context's plugin set.
static hipError_t decode_for(const ms_ctx *c, const ms_pod_rec *pods, uint32_t n, const unsigned long long *keys,
                             const uint32_t *flags, uint32_t present, ms_result *out, hipStream_t s) {
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NA)
        return launch_decode_na(pods, n, keys, flags, present, seed32_of(c->cfg.seed), c->w_nn, c->w_na, out, s);
    return launch_decode(pods, n, keys, flags, present, out, s);
}

// The stateless cycle of a batch on a single-shard context: filter + score +
// selectHost + decode into results; commit != 0 also commits every winner's
// bind (NodeInfo.AddPod). NU+NN with K1 pp is one fused launch for the whole
// batch, binds included (it needs key scratch only above kPpMaxFusedRows
// rows); otherwise batch_cap chunks are swept into the context's key/flag
// scratch, then decoded (and their binds applied).
// done (optional): recorded on s after the call's last launch (by the fused
// K1 dispatch itself when the cycle is that one launch).
int select_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, ms_result *d_res, hipStream_t s, int commit,
                  hipEvent_t done) {
    const uint32_t B = c->batch_cap;
    const bool fused = c->cfg.plugin_set == MS_PLUGINS_NU_NN;
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NAM) {
        int rc = nam_cycle_locked(c, n_pods, d_pods, d_res, commit, s);
        if (rc) return rc;
        if (done) MS_HIP(c, hipEventRecord(done, s));
        return MS_OK;
    }
    if (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN) {  // (stateless: binds in the combine launch)
        int rc = tt_cycle_locked(c, n_pods, d_pods, nullptr, d_res, commit, s);
        if (rc) return rc;
        if (done) MS_HIP(c, hipEventRecord(done, s));
        return MS_OK;
    }
    if (fused && c->rows_dev <= kPpMaxFusedRows) {
        MS_HIP(c, launch_sweep_pp(c->t, c->d_cand, c->rows_dev, d_pods, n_pods, seed32_of(c->cfg.seed), nullptr, d_res,
                                  c->present_dev, c->num_cus, s, commit, done));
        return MS_OK;
    }
    // The resource-aware set reads Requested / pod_count: every chunk must be
    // decided before any bind of the call lands (MS_MODE_BATCHED), so
    // its binds are committed after the last chunk's decode.
    const bool late_commit = commit && !plugins_stateless(c);
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        if (fused) {
            MS_HIP(c, launch_sweep_pp(c->t, c->d_cand, c->rows_dev, d_pods + s0, nb, seed32_of(c->cfg.seed), c->d_keys,
                                      d_res + s0, c->present_dev, c->num_cus, s, commit));
            continue;
        }
        const bool want_flags = c->cfg.plugin_set != MS_PLUGINS_NU_NN;
        int rc = sweep_locked(c, nb, d_pods + s0, c->d_keys, want_flags ? c->d_flags : nullptr, s);
        if (rc) return rc;
        MS_HIP(c, decode_for(c, d_pods + s0, nb, c->d_keys, want_flags ? c->d_flags : nullptr, c->present_dev,
                             d_res + s0, s));
        if (commit && !late_commit) MS_HIP(c, launch_apply_binds(c->t, d_pods + s0, nb, d_res + s0, s));
    }
    if (late_commit) MS_HIP(c, launch_apply_binds(c->t, d_pods, n_pods, d_res, s));
    if (done) MS_HIP(c, hipEventRecord(done, s));
    return MS_OK;
}

}  // namespace msgpu

using namespace msgpu;

extern "C" {

int ms_sweep_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint64_t *keys_dev, uint32_t *flags_dev,
                    void *stream) {
    if (!c || (n_pods && (!pods_dev || !keys_dev))) return MS_E_INVAL;
    if ((c->cfg.plugin_set == MS_PLUGINS_NU_NRF_NN_LA || c->cfg.plugin_set == MS_PLUGINS_NU_NN_NA) && n_pods &&
        !flags_dev)
        return fail(c, MS_E_INVAL, "ms_sweep_device: flags required for the resource-aware / NodeAffinity plugin sets");
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);  // (deltas were applied on the context stream)
    if (call.rc()) return call.rc();
    // on a caller stream the chain-back event is recorded by the sweep's own dispatch
    const hipEvent_t back = call.back_event();
    const int rc = sweep_locked(c, n_pods, pods_dev, reinterpret_cast<unsigned long long *>(keys_dev), flags_dev,
                                call.stream(), back);
    if (rc) return rc;
    return call.done(back != nullptr);
}

int ms_select_batch_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, ms_result *results_dev,
                           void *stream) {
    if (!c || (n_pods && (!pods_dev || !results_dev))) return MS_E_INVAL;
    if (c->comm)
        return fail(c, MS_E_INVAL, "ms_select_batch_device: single-shard call on a sharded context (ms_sharded_submit)");
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    // on a caller stream the chain-back event is recorded by the cycle's own dispatch
    const hipEvent_t back = call.back_event();
    const int rc = select_locked(c, n_pods, pods_dev, results_dev, call.stream(), 0, back);
    if (rc) return rc;
    return call.done(back != nullptr);
}

int ms_decode_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, const uint64_t *keys_dev,
                     const uint32_t *flags_dev, uint32_t present_nodes, ms_result *results_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !keys_dev || !results_dev))) return MS_E_INVAL;
    MS_HIP(c, hipSetDevice(c->cfg.device));
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NA && n_pods && !flags_dev)
        return fail(c, MS_E_INVAL, "ms_decode_device: the NodeAffinity anchors (flags) are required for this plugin set");
    if (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN)
        return fail(c, MS_E_INVAL, "ms_decode_device: TaintToleration shards decode summaries (ms_tt_decode_device)");
    MS_HIP(c, decode_for(c, pods_dev, n_pods, reinterpret_cast<const unsigned long long *>(keys_dev), flags_dev,
                         present_nodes, results_dev, pick_stream(c, stream)));
    return MS_OK;
}

int ms_decode_device_jobs(ms_ctx *c, uint32_t n_jobs, const ms_decode_job *jobs, uint32_t present_nodes,
                          void *stream) {
    if (!c || n_jobs > MS_DECODE_MAX_JOBS || (n_jobs && !jobs)) return MS_E_INVAL;
    if (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN)
        return fail(c, MS_E_INVAL, "ms_decode_device_jobs: TaintToleration shards decode summaries (ms_tt_decode_device)");
    for (uint32_t i = 0; i < n_jobs; ++i)
        if (jobs[i].n_pods && (!jobs[i].pods || !jobs[i].keys || !jobs[i].results)) return MS_E_INVAL;
    if (n_jobs == 0) return MS_OK;
    MS_HIP(c, hipSetDevice(c->cfg.device));
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN_NA) {  // one launch per job
        for (uint32_t i = 0; i < n_jobs; ++i) {
            if (jobs[i].n_pods && !jobs[i].flags) return fail(c, MS_E_INVAL, "ms_decode_device_jobs: anchors required");
            MS_HIP(c, decode_for(c, jobs[i].pods, jobs[i].n_pods, reinterpret_cast<const unsigned long long *>(jobs[i].keys),
                                 jobs[i].flags, present_nodes, jobs[i].results, pick_stream(c, stream)));
        }
        return MS_OK;
    }
    MS_HIP(c, launch_decode_jobs(jobs, n_jobs, present_nodes, pick_stream(c, stream)));
    return MS_OK;
}

int ms_apply_binds_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, const ms_result *results_dev,
                          void *stream) {
    if (!c || (n_pods && (!pods_dev || !results_dev))) return MS_E_INVAL;
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream, false);  // after earlier sweeps and deltas (none drained here)
    if (call.rc()) return call.rc();
    MS_HIP(c, launch_apply_binds(c->t, pods_dev, n_pods, results_dev, call.stream()));
    return call.done();
}

int ms_tt_summaries_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, void *summaries_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !summaries_dev))) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_TT_NN)
        return fail(c, MS_E_INVAL, "ms_tt_summaries_device: the TaintToleration plugin set only");
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    const int rc = tt_cycle_locked(c, n_pods, pods_dev, summaries_dev, nullptr, 0, call.stream());
    if (rc) return rc;
    return call.done();
}

int ms_tt_decode_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t n_shards,
                        const void *summaries_all_dev, ms_result *results_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !summaries_all_dev || !results_dev))) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_TT_NN)
        return fail(c, MS_E_INVAL, "ms_tt_decode_device: the TaintToleration plugin set only");
    if (n_shards == 0) return fail(c, MS_E_INVAL, "ms_tt_decode_device: no shards");
    if (n_pods == 0) return MS_OK;
    MS_HIP(c, hipSetDevice(c->cfg.device));
    MS_HIP(c, launch_tt_combine(summaries_all_dev, n_pods, n_shards, pods_dev, n_pods, seed32_of(c->cfg.seed), nullptr,
                                results_dev, c->t, 0, pick_stream(c, stream)));
    return MS_OK;
}

// The two-pass TaintToleration cycle over node shards (ms_taint.hip launch_tt2_*):
// chunks of batch_cap pods; each call rebuilds the row planes on its stream.
// After the ordered call's prologue: the scratch for the call, taken from the
// previous TT cycle (ev_tt), with the planes unless the pass reads none.
static int tt2_shard_begin(ms_ctx *c, uint32_t n_pods, hipStream_t s, bool planes = true) {
    int rc = ensure_tt(c, tt2_scratch_bytes(c->rows_dev, std::min(c->batch_cap, n_pods)));
    if (rc) return rc;
    rc = tt_take(c, s);
    if (rc) return rc;
    if (planes) MS_HIP(c, launch_tt2_planes(c->t, c->rows_dev, c->d_tt, s));
    return MS_OK;
}

static int tt_only(ms_ctx *c, const char *who) {
    if (c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN) return MS_OK;
    return fail(c, MS_E_INVAL, std::string(who) + ": the TaintToleration plugin set only");
}

int ms_tt_census_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, void *census_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !census_dev))) return MS_E_INVAL;
    if (n_pods == 0) return c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN ? MS_OK : MS_E_INVAL;
    int rc = tt_only(c, "ms_tt_census_device");
    if (rc) return rc;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    rc = tt2_shard_begin(c, n_pods, s);
    if (rc) return rc;
    const uint32_t B = c->batch_cap, cap = std::min(B, n_pods), seed32 = seed32_of(c->cfg.seed);
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        MS_HIP(c, launch_tt2_census_shard(c->t, c->rows_dev, pods_dev + s0, nb, seed32, c->d_tt, cap,
                                          static_cast<char *>(census_dev) + (size_t)s0 * MS_TT_CENSUS_BYTES, s));
    }
    rc = tt_release(c, s);
    if (rc) return rc;
    return call.done();
}

int ms_tt_pick_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t n_shards, uint32_t shard_index,
                      const void *census_all_dev, unsigned long long *keys_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !census_all_dev || !keys_dev))) return MS_E_INVAL;
    if (n_shards == 0 || shard_index >= n_shards)
        return fail(c, MS_E_INVAL, "ms_tt_pick_device: shard_index must be below n_shards");
    if (n_pods == 0) return c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN ? MS_OK : MS_E_INVAL;
    int rc = tt_only(c, "ms_tt_pick_device");
    if (rc) return rc;
    // mid-cycle: no deltas drained, the table stays the one step 1 saw (as ms_seq_validate_device)
    OrderedCall call(c, stream, false);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    rc = tt2_shard_begin(c, n_pods, s);
    if (rc) return rc;
    const uint32_t B = c->batch_cap, cap = std::min(B, n_pods), seed32 = seed32_of(c->cfg.seed);
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        MS_HIP(c, launch_tt2_pick_shard(c->t, c->rows_dev, pods_dev + s0, nb, seed32, c->d_tt, cap,
                                        static_cast<const char *>(census_all_dev) + (size_t)s0 * MS_TT_CENSUS_BYTES,
                                        n_pods, n_shards, shard_index, keys_dev + s0, s));
    }
    rc = tt_release(c, s);
    if (rc) return rc;
    return call.done();
}

int ms_tt_final_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t n_shards,
                       const void *census_all_dev, const unsigned long long *keys_max_dev, ms_result *results_dev,
                       void *stream) {
    if (!c || (n_pods && (!pods_dev || !census_all_dev || !keys_max_dev || !results_dev)))
        return MS_E_INVAL;
    if (n_shards == 0) return fail(c, MS_E_INVAL, "ms_tt_final_device: no shards");
    if (n_pods == 0) return c->cfg.plugin_set == MS_PLUGINS_NU_TT_NN ? MS_OK : MS_E_INVAL;
    int rc = tt_only(c, "ms_tt_final_device");
    if (rc) return rc;
    // mid-cycle: no deltas drained, the table stays the one step 1 saw (as ms_seq_validate_device)
    OrderedCall call(c, stream, false);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    rc = tt2_shard_begin(c, n_pods, s, false);  // (the final pass reads no planes)
    if (rc) return rc;
    const uint32_t B = c->batch_cap, cap = std::min(B, n_pods), seed32 = seed32_of(c->cfg.seed);
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        // (the scratch's plan records: ADVICE r5, its start holds the row planes)
        MS_HIP(c, launch_tt2_final_shard(c->t, c->rows_dev, pods_dev + s0, nb, seed32,
                                         tt2_plans(c->d_tt, c->rows_dev, cap), cap,
                                         static_cast<const char *>(census_all_dev) + (size_t)s0 * MS_TT_CENSUS_BYTES,
                                         n_pods, n_shards, keys_max_dev + s0, results_dev + s0, s));
    }
    rc = tt_release(c, s);
    if (rc) return rc;
    return call.done();
}

int ms_nam_segment_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, void *seg_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !seg_dev))) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "ms_nam_segment_device: the multi-term NodeAffinity plugin set only");
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    const NamPlan plan = nam_plan_for(c, n_pods);
    const uint32_t B = plan.chunk;
    int rc = ensure_nam(c, plan);
    if (rc) return rc;
    rc = nam_take(c, s);
    if (rc) return rc;
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        char *out = static_cast<char *>(seg_dev) + (size_t)s0 * MS_NAM_SEG_BYTES;
        if (c->rows_dev == 0) {  // no rows: the identity map, no non-zero node
            MS_HIP(c, launch_nam_identity(out, nb, s));
            continue;
        }
        MS_HIP(c, launch_nam_segment(c->t, c->rows_dev, pods_dev + s0, nb, c->d_terms, c->n_terms,
                                     plan.L, c->d_nam, out, s));
    }
    rc = nam_release(c, s);
    if (rc) return rc;
    return call.done();
}

int ms_nam_keys_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t n_shards, uint32_t shard_index,
                       const void *segs_all_dev, unsigned long long *keys_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !segs_all_dev || !keys_dev))) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "ms_nam_keys_device: the multi-term NodeAffinity plugin set only");
    if (n_shards == 0 || shard_index >= n_shards)
        return fail(c, MS_E_INVAL, "ms_nam_keys_device: shard_index must be below n_shards");
    if (n_pods == 0) return MS_OK;
    // mid-cycle: no deltas drained, the table stays the one step 1 saw (as ms_seq_validate_device)
    OrderedCall call(c, stream, false);
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    const NamPlan plan = nam_plan_for(c, n_pods);
    const uint32_t B = plan.chunk;
    int rc = ensure_nam(c, plan);
    if (rc) return rc;
    rc = nam_take(c, s);
    if (rc) return rc;
    // the per-pod shard inputs (B records, B bytes) behind the plan layout's scratch
    char *after = static_cast<char *>(c->d_nam.get()) + plan.after;
    uint8_t *m_in = reinterpret_cast<uint8_t *>(static_cast<char *>(c->d_nam.get()) + plan.m_in);
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        // the later shards' tables composed, and whether an earlier shard has a non-zero node
        MS_HIP(c, launch_nam_compose(static_cast<const char *>(segs_all_dev) + (size_t)s0 * MS_NAM_SEG_BYTES, n_pods,
                                     n_shards, nb, (int32_t)shard_index, after, m_in, s));
        rc = nam_keys_locked(c, plan.L, nb, pods_dev + s0, after, m_in, keys_dev + s0, nullptr, s);
        if (rc) return rc;
    }
    rc = nam_release(c, s);
    if (rc) return rc;
    return call.done();
}

int ms_nam_flags_device(ms_ctx *c, uint32_t n_pods, uint32_t n_shards, const void *segs_all_dev, uint32_t *flags_dev,
                        void *stream) {
    if (!c || (n_pods && (!segs_all_dev || !flags_dev))) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "ms_nam_flags_device: the multi-term NodeAffinity plugin set only");
    if (n_shards == 0) return fail(c, MS_E_INVAL, "ms_nam_flags_device: no shards");
    if (n_pods == 0) return MS_OK;
    // (reads the caller's gathered records only: no table, no scratch, so no ordering
    // against the context stream, like ms_decode_device)
    MS_HIP(c, hipSetDevice(c->cfg.device));
    MS_HIP(c, launch_nam_flags(segs_all_dev, n_pods, n_shards, n_pods, flags_dev, pick_stream(c, stream)));
    return MS_OK;
}

}  // extern "C"

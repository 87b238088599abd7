// ms_hostarray.cpp — the calls that take the pods from and return the results
// to host arrays (ms_schedule_batch, ms_schedule_batch_compact) and their two
// pipelines: chunked copies beside the cycle, and the zero-copy compact cycle.
// They run on the context stream and wait for it before they return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <type_traits>

#include "ms_ctx.h"

namespace msgpu {

// Chunks of ms_schedule_batch's host-array cycle (NU+NN / NA sets, pageable
// copies): chunk i+1's H2D (copy stream; the runtime stages pageable memory on
// the calling thread, which here overlaps chunk i's fused cycle) and chunk i-1's
// D2H overlap chunk i on the context stream; one cross-stream wait per chunk.
constexpr uint32_t kE2eMinChunk = 16384, kE2eChunks = 2;

static uint32_t e2e_chunks(uint32_t n) { return std::max(1u, std::min(kE2eChunks, n / kE2eMinChunk)); }

// The per-chunk events of the host-array paths, each created once whichever
// path (zero-copy or chunked copies) runs first (no leak when a
// context switches paths); copies: also the copy-stream events.
static int ensure_chunk_events(ms_ctx *c, bool copies) {
    for (int i = 0; i < 4; ++i) {
        MS_HIP(c, made(c->ev_cyc[i].ensure()));
        if (copies) MS_HIP(c, made(c->ev_copy[i].ensure()));
    }
    return MS_OK;
}

static int schedule_chunked(ms_ctx *c, const ms_pod_rec *pods, uint32_t n, ms_result *out, uint32_t parts,
                            CallClock &ck) {
    const hipStream_t s = c->stream;
    if (!c->copy_stream) {
        MS_HIP(c, made(c->copy_stream.ensure(hipStreamNonBlocking)));
        ck.lap(MS_PH_ALLOC);
    }
    int erc = ensure_chunk_events(c, true);
    if (erc) return erc;
    const hipStream_t cs = c->copy_stream;
    const uint32_t per = cdiv(n, parts);
    auto beg = [&](uint32_t i) { return std::min(n, i * per); };
    auto cnt = [&](uint32_t i) { return beg(i + 1) - beg(i); };
    ck.count(MS_PH_CHUNKS, parts);
    MS_HIP(c, hipMemcpyAsync(c->d_pods, pods, sizeof(ms_pod_rec) * cnt(0), hipMemcpyHostToDevice, s));
    ck.lap(MS_PH_STAGE_IN);
    for (uint32_t i = 0; i < parts; ++i) {
        if (i > 0) MS_HIP(c, hipStreamWaitEvent(s, c->ev_copy[i], 0));
        int rc = select_locked(c, cnt(i), c->d_pods + beg(i), c->d_res + beg(i), s, 1);
        if (rc) return rc;
        MS_HIP(c, hipEventRecord(c->ev_cyc[i], s));
        ck.lap(MS_PH_LAUNCH);
        if (i + 1 < parts) {
            MS_HIP(c, hipMemcpyAsync(c->d_pods + beg(i + 1), pods + beg(i + 1), sizeof(ms_pod_rec) * cnt(i + 1),
                                     hipMemcpyHostToDevice, cs));
            MS_HIP(c, hipEventRecord(c->ev_copy[i + 1], cs));
            ck.lap(MS_PH_STAGE_IN);
        }
        if (i > 0) {
            MS_HIP(c, hipStreamWaitEvent(cs, c->ev_cyc[i - 1], 0));
            MS_HIP(c, hipMemcpyAsync(out + beg(i - 1), c->d_res + beg(i - 1), sizeof(ms_result) * cnt(i - 1),
                                     hipMemcpyDeviceToHost, cs));
            ck.lap(MS_PH_STAGE_OUT);
        }
    }
    MS_HIP(c, hipMemcpyAsync(out + beg(parts - 1), c->d_res + beg(parts - 1), sizeof(ms_result) * cnt(parts - 1),
                             hipMemcpyDeviceToHost, s));
    ck.lap(MS_PH_STAGE_OUT);
    MS_HIP(c, hipStreamSynchronize(cs));
    MS_HIP(c, hipStreamSynchronize(s));
    ck.lap(MS_PH_WAIT);
    return MS_OK;
}

// Pinned coherent staging of compact records (the compact cycle's kernel reads
// the pods from and writes the results to it over PCIe), grown to n. No
// synchronise of its own: the runtime's free of the old blocks waits for the
// work that used them (schedule_zc's synchronise comes after).
static int ensure_zc(ms_ctx *c, uint32_t n) {
    if (n <= c->z_cap) return MS_OK;
    c->z_cap = 0;
    // coherent (fine-grained): the kernel's reads see this call's host copy and
    // its writes reach host memory with no cache maintenance between calls
    if (!c->h_podz.alloc(n, hipHostMallocCoherent) || !c->h_resz.alloc(n, hipHostMallocCoherent))
        return fail(c, MS_E_OOM, "compact pinned staging");
    c->z_cap = n;
    return MS_OK;
}

// The single-shard NU+NN cycle of a host-array call without runtime (pageable)
// copies: chunk by chunk, the host writes the 8-B compact records K1 reads into
// pinned coherent memory (narrowing 40-B ms_pod_rec, or copying compact ones),
// the compact cycle kernel (one launch per chunk, binds included) reads them
// and writes 8-B results there over PCIe, and the host moves chunk i-1's
// results into the caller's array (widening to ms_result, or copying) while
// chunk i runs. For ms_schedule_batch the pageable copies this replaces cost
// 0.59 ms at config C (the blocking D2H alone ~0.42 ms of host time) and once
// took 7.3 ms (BENCH_r03 e2e.runs[4]; the A/B rerun caught a 6.7 ms pageable
// H2D in the call's stage_in phase, profiles/r04b_e2e_zc_ab.txt).
// Chunks: one per 50k pods, at most 4. With the fixed-slot K1 (shorter kernels) config C's 100k pods in 2
// chunks overlap the host copies: 0.320 vs 0.328 ms compact, 0.362 vs 0.403 ms
// with 40/24-B records (profiles/r04zb_zc_parts.txt; 3 chunks 0.325 / 0.364;
// round 3, slot-search K1: 4 chunks of 25k cost as much kernel time as their
// overlap saved).
constexpr uint32_t kZcMinChunk = 50000;
constexpr uint32_t kZcParMin = 16384;  // pods per chunk from which the copies use the pool
template <typename PodIn, typename ResOut>
static int schedule_zc(ms_ctx *c, const PodIn *pods, uint32_t n, ResOut *out, CallClock &ck) {
    static_assert(sizeof(ms_pod_compact) <= sizeof(PodIn), "compact pod = the first 8 B of a pod record");
    const hipStream_t s = c->stream;
    int rc = ensure_zc(c, n);
    if (rc) return rc;
    rc = ensure_chunk_events(c, false);
    if (rc) return rc;
    ck.lap(MS_PH_ALLOC);
    MS_HIP(c, hipStreamSynchronize(s));  // (no earlier call still reads h_podz)
    ck.lap(MS_PH_WAIT);
    const uint32_t parts = std::max(1u, std::min(4u, n / kZcMinChunk));
    const uint32_t per = cdiv(n, parts);
    auto beg = [&](uint32_t i) { return std::min(n, i * per); };
    // Host copies split over the caller and the copy pool's 3 helpers (7 measured
    // no better, profiles/r05v_e2e_ab.txt): the first chunk's copy-in and the last
    // one's copy-out are on the call's critical path.
    constexpr unsigned helpers = 3;
    if (per >= kZcParMin && !c->copy_pool) {
        try {  // (no helper threads, e.g. none can be created: the caller copies alone)
            c->copy_pool.reset(new CopyPool(helpers));
        } catch (...) {
            c->copy_pool.reset();
        }
    }
    CopyPool *pool = per >= kZcParMin ? c->copy_pool.get() : nullptr;
    auto par = [&](uint32_t lo, uint32_t hi, const std::function<void(uint32_t, uint32_t)> &fn) {
        if (!pool) {
            fn(lo, hi);
            return;
        }
        pool->run_parts([&](unsigned p, unsigned P) {
            fn(lo + (uint32_t)((uint64_t)(hi - lo) * p / P), lo + (uint32_t)((uint64_t)(hi - lo) * (p + 1) / P));
        });
    };
    auto move_out = [&](uint32_t i) {
        const ms_result_compact *r = c->h_resz;
        par(beg(i), beg(i + 1), [&](uint32_t a, uint32_t b) {
            if constexpr (std::is_same<ResOut, ms_result_compact>::value) {
                std::memcpy(out + a, r + a, sizeof(ms_result_compact) * (b - a));
            } else {
                for (uint32_t j = a; j < b; ++j) {
                    const ms_result_compact x = r[j];
                    out[j] = ms_result{x.node, (int32_t)x.code, (int64_t)x.score, (uint32_t)x.plugin_mask, 0u};
                }
            }
        });
    };
    c->order.wrote_ctx();  // binds write the table on the context stream
    ck.count(MS_PH_CHUNKS, parts);
    for (uint32_t i = 0; i < parts; ++i) {
        ms_pod_compact *z = c->h_podz;
        par(beg(i), beg(i + 1), [&](uint32_t a, uint32_t b) {
            if constexpr (std::is_same<PodIn, ms_pod_compact>::value) {
                std::memcpy(z + a, pods + a, sizeof(ms_pod_compact) * (b - a));
            } else {
                for (uint32_t j = a; j < b; ++j) std::memcpy(&z[j], &pods[j], sizeof(ms_pod_compact));
            }
        });
        ck.lap(MS_PH_STAGE_IN);
        MS_HIP(c, launch_sweep_pp_compact(c->t, c->d_cand, c->rows_dev, c->h_podz + beg(i), beg(i + 1) - beg(i),
                                          seed32_of(c->cfg.seed), c->h_resz + beg(i), c->present_dev, c->num_cus, s));
        MS_HIP(c, hipEventRecord(c->ev_cyc[i], s));
        ck.lap(MS_PH_LAUNCH);
        if (i > 0) {
            MS_HIP(c, hipEventSynchronize(c->ev_cyc[i - 1]));
            ck.lap(MS_PH_WAIT);
            move_out(i - 1);
            ck.lap(MS_PH_STAGE_OUT);
        }
    }
    MS_HIP(c, hipEventSynchronize(c->ev_cyc[parts - 1]));
    ck.lap(MS_PH_WAIT);
    move_out(parts - 1);
    ck.lap(MS_PH_STAGE_OUT);
    return MS_OK;
}

}  // namespace msgpu

using namespace msgpu;

extern "C" {

int ms_schedule_batch(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods, int32_t mode, ms_result *out) {
    if (!c || (n_pods && (!pods || !out))) return MS_E_INVAL;
    if (mode != MS_MODE_BATCHED && mode != MS_MODE_SEQUENTIAL) return fail(c, MS_E_INVAL, "unknown mode");
    if (n_pods == 0) return MS_OK;
    std::lock_guard<std::mutex> g(c->sched_mu);
    CallClock ck(c);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    int rc = flush_locked(c);
    if (rc) return rc;
    ck.lap(MS_PH_LOCK_FLUSH);
    if (c->comm) return comm_schedule_host(c, n_pods, pods, mode, out, &ck);  // node-sharded over the communicator
    if (c->cfg.plugin_set == MS_PLUGINS_NU_NN && c->rows_dev <= kPpMaxFusedRows)
        return schedule_zc(c, pods, n_pods, out, ck);  // (NU+NN: both modes are the batched cycle + binds)
    const hipStream_t s = c->stream;
    c->order.wrote_ctx();  // binds below write the table on the context stream
    uint32_t B = c->batch_cap;
    if (mode == MS_MODE_BATCHED && !plugins_stateless(c)) {
        // every pod of the call is decided on the same node state before any of
        // its binds lands: one pass over the whole call (header contract)
        rc = ensure_stage(c, n_pods);
        if (rc) return rc;
        ck.lap(MS_PH_ALLOC);
        B = n_pods;
    }
    // Host arrays go straight to the device (the runtime's own pageable-copy
    // path, 0.56 ms for config C's 4 MB in + 2.4 MB out + cycle, against 0.72 ms
    // through a single-threaded memcpy into the pinned staging buffers;
    // profiles/r02u_e2e_ab.txt). The call waits for its copies before it
    // returns, so no caller (cgo) pointer outlives it.
    for (uint32_t s0 = 0; s0 < n_pods; s0 += B) {
        const uint32_t nb = std::min(B, n_pods - s0);
        // (the stream is already idle after the previous chunk's synchronise; kept
        // because it delimits the MS_PH_WAIT phase of the call profile)
        MS_HIP(c, hipStreamSynchronize(s));
        ck.lap(MS_PH_WAIT);
        const bool seq_full = (mode == MS_MODE_SEQUENTIAL && c->cfg.plugin_set == MS_PLUGINS_NU_NRF_NN_LA);
        const uint32_t parts = plugins_stateless(c) ? e2e_chunks(nb) : 1u;
        if (parts > 1) {  // (NU+NN / NA: binds never change a later pod's keys, so chunks equal one batch)
            rc = schedule_chunked(c, pods + s0, nb, out + s0, parts, ck);
            if (rc) return rc;
            continue;
        }
        MS_HIP(c, hipMemcpyAsync(c->d_pods, pods + s0, sizeof(ms_pod_rec) * nb, hipMemcpyHostToDevice, s));
        ck.count(MS_PH_CHUNKS);
        ck.lap(MS_PH_STAGE_IN);
        if (seq_full) {
            rc = run_sequential(c, nb, c->d_pods, c->d_res, s);
            if (rc) return rc;
        } else {
            // NU+NN keys never read mutable node state, so the queue-order
            // loop equals the batched sweep; binds are committed after it.
            rc = select_locked(c, nb, c->d_pods, c->d_res, s, 1);
            if (rc) return rc;
        }
        ck.lap(MS_PH_LAUNCH);
        MS_HIP(c, hipMemcpyAsync(out + s0, c->d_res, sizeof(ms_result) * nb, hipMemcpyDeviceToHost, s));
        ck.lap(MS_PH_STAGE_OUT);
        MS_HIP(c, hipStreamSynchronize(s));
        ck.lap(MS_PH_WAIT);
    }
    return MS_OK;
}

int ms_schedule_batch_compact(ms_ctx *c, uint32_t n, const ms_pod_compact *pods, int32_t mode, ms_result_compact *out) {
    if (!c || (n && (!pods || !out))) return MS_E_INVAL;
    if (mode != MS_MODE_BATCHED && mode != MS_MODE_SEQUENTIAL) return fail(c, MS_E_INVAL, "unknown mode");
    if (!plugins_stateless(c))
        return fail(c, MS_E_INVAL, "ms_schedule_batch_compact: the resource-aware set needs ms_schedule_batch");
    if (c->comm && c->cfg.plugin_set == MS_PLUGINS_NU_NN_NAM)  // (as before the in-library NAM cycle: the header's sets only)
        return fail(c, MS_E_INVAL, "ms_schedule_batch_compact: multi-term NodeAffinity node shards take ms_schedule_batch");
    if (n == 0) return MS_OK;
    std::lock_guard<std::mutex> g(c->sched_mu);
    CallClock ck(c);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    int rc = flush_locked(c);
    if (rc) return rc;
    ck.lap(MS_PH_LOCK_FLUSH);
    // Single-shard NU+NN: one launch reading the pods from and writing the
    // results to pinned host memory (8 B each way per pod over PCIe, no copy
    // commands, no widen / narrow passes); the host copies the caller's arrays
    // in and out (the staged path below: node shards, larger tables).
    if (!c->comm && c->cfg.plugin_set == MS_PLUGINS_NU_NN && c->rows_dev <= kPpMaxFusedRows)
        return schedule_zc(c, pods, n, out, ck);
    rc = c->comm ? comm_stage(c, n) : ensure_stage(c, n);
    if (rc) return rc;
    if (n > c->compact_cap) {  // (as ensure_stage: the runtime's free waits for the device)
        c->compact_cap = 0;
        if (!c->d_podc.alloc(n) || !c->d_resc.alloc(n)) return fail(c, MS_E_OOM, "compact staging");
        c->compact_cap = n;
    }
    ck.lap(MS_PH_ALLOC);
    const hipStream_t s = c->stream;
    // 8 B per pod in and out over PCIe; widened / narrowed on the device
    MS_HIP(c, hipMemcpyAsync(c->d_podc, pods, sizeof(ms_pod_compact) * n, hipMemcpyHostToDevice, s));
    ck.lap(MS_PH_STAGE_IN);
    MS_HIP(c, launch_pods_widen(c->d_podc, n, c->d_pods, s));
    if (c->comm) {
        rc = comm_cycle_staged(c, n, mode);
    } else {
        c->order.wrote_ctx();  // binds write the table on the context stream
        rc = select_locked(c, n, c->d_pods, c->d_res, s, 1);  // (stateless sets: sequential == batched)
    }
    if (rc) return rc;
    MS_HIP(c, launch_results_narrow(c->d_res, n, c->d_resc, s));
    ck.lap(MS_PH_LAUNCH);
    MS_HIP(c, hipMemcpyAsync(out, c->d_resc, sizeof(ms_result_compact) * n, hipMemcpyDeviceToHost, s));
    ck.lap(MS_PH_STAGE_OUT);
    MS_HIP(c, hipStreamSynchronize(s));
    ck.lap(MS_PH_WAIT);
    return MS_OK;
}

}  // extern "C"

// ms_seq_host.cpp — the host side of the exact sequential engine (ms_seq.hip):
// its scratch, the step loop, the node shards' candidate and validation calls,
// and the diagnostic builds' read-out (MS_VSTAMPS, MS_TIMELINE), so that those
// builds recompile this one host file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ms_ctx.h"

namespace msgpu {

constexpr int kSeqBufs = 3;  // sequential-engine batch buffer sets (pipeline depth <= 3)

// Sequential-engine scratch for n_tiles tiles, kSeqBufs batches deep (the
// single-stream steps use two sets; the node-sharded candidates up to three).
// As every grow routine: the capacity stays zero while the group of buffers is
// not whole, so a failed growth is retried by the next call.
int ensure_tiles(ms_ctx *c, uint32_t n_tiles) {
    if (n_tiles <= c->tile_cap) return MS_OK;
    MS_HIP(c, hipDeviceSynchronize());  // no batch still reads the old buffers
    c->tile_cap = 0;
    // (ms_seq_candidates_device uses the same buffers for up to kSeqBufs * B pods)
    const size_t B = seq_batch_limit(), NB = kSeqBufs * B, n = NB * n_tiles;
    if (!c->d_tile_keys.alloc(n * seq_topk()) || !c->d_tile_flags.alloc(n) || !c->d_spec.alloc(NB) ||
        !c->d_spec_flags.alloc(NB) || !c->d_top4.alloc(NB * seq_topk()) ||
        !c->d_top4_rec.alloc(NB * seq_topk() * seq_rec_fields()) || !c->d_prev.alloc(2 * (2 + seq_prev_cap())) ||
        !c->d_prev_rec.alloc(2 * seq_prev_cap() * seq_rec_fields()) ||
        !c->d_drow.alloc((size_t)n_tiles * kFullWaveTile) || !c->d_top_ext.alloc(NB * seq_topk()) ||
        !c->d_merge_tags.alloc(NB))
        return fail(c, MS_E_OOM, "sequential-engine scratch");
    MS_HIP(c, hipMemsetAsync(c->d_merge_tags, 0, NB * sizeof(uint32_t), c->stream));
    MS_HIP(c, hipMemsetAsync(c->d_spec, 0, NB * sizeof(unsigned long long), c->stream));
    MS_HIP(c, hipMemsetAsync(c->d_spec_flags, 0, NB * sizeof(uint32_t), c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    c->tile_cap = n_tiles;
    return MS_OK;
}

// Pods per speculative batch: fewer nodes touched per batch keeps the top-K
// lists valid; more pods amortise the two launches. MINISCHED_SEQ_BATCH
// overrides (tuning), clamped to the validator's LDS capacity.
static uint32_t seq_batch() {
    uint32_t b = seq_batch_limit();  // the build's batch (128: profiles/r01_e_batch_sweep.jsonl, r03o)
    if (const char *e = getenv("MINISCHED_SEQ_BATCH")) b = (uint32_t)std::max(1, atoi(e));
    return std::min(b, seq_batch_limit());
}

// Batch k+1's merge inside step k (default since round 5, kInStep): the sweep
// workgroups stamp every tile list they write with the step's tag, and one
// wave per pod polls the pod's lists (written through, read L2-bypassing
// across the XCDs) until all carry it, then merges them while the validator
// continues; a worker whose bounded wait runs out leaves its pods untagged
// and the next validation merges them itself.
// With the binary64 tile keys the sweep + merge path fits beside the
// validator: config E 44.4 -> 40.5 ms against the merge launch
// (profiles/r05c_e_ab.txt, r05f_e_sync_ab.txt). MINISCHED_SEQ_MERGE=launch
// (kLaunch): a k_topk_merge launch after each step (A/B); "fallback"
// (kFallback): the in-step workers skip (a test hook). Read per call (tests
// switch it), never kept across calls.
enum class SeqMerge { kInStep, kFallback, kLaunch };

static SeqMerge seq_merge_mode() {
    const char *e = getenv("MINISCHED_SEQ_MERGE");
    if (!e || !std::strcmp(e, "instep")) return SeqMerge::kInStep;
    return !std::strcmp(e, "fallback") ? SeqMerge::kFallback : SeqMerge::kLaunch;
}

// Exact sequential engine: speculative per-tile top-K sweep + in-order
// validation, batch after batch on one stream.
int run_sequential(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *d_pods, ms_result *d_res, hipStream_t s) {
    const uint32_t rows = c->rows_dev;
    const uint32_t seed32 = seed32_of(c->cfg.seed);
    if (rows == 0) {  // no node listed: every pod is a FitError with an empty mask
        for (uint32_t s0 = 0; s0 < n_pods; s0 += c->batch_cap) {
            const uint32_t nb = std::min(c->batch_cap, n_pods - s0);
            MS_HIP(c, hipMemsetAsync(c->d_keys, 0, sizeof(unsigned long long) * nb, s));
            MS_HIP(c, launch_decode(d_pods + s0, nb, c->d_keys, nullptr, 0, d_res + s0, s));
        }
        return MS_OK;
    }
    if (rows > seq_max_rows())
        return fail(c, MS_E_CAPACITY, "resource-aware sequential mode supports at most " +
                                          std::to_string(seq_max_rows()) + " rows per context (shard the nodes)");
    // Tiles of the speculative sweep: one per CU beside the validator's where the
    // table allows (rows per tile a multiple of 16, 64..256): at 50k nodes 241
    // tiles of 208 rows on 241 CUs instead of 196 of 256 on 196 (round 6).
    NodeTable tq = c->t;
    {
        const uint32_t room = (uint32_t)std::max(2, c->num_cus) - 1u;
        const uint32_t tr = (cdiv(rows, room) + 15u) / 16u * 16u;
        tq.tile_rows = std::min<uint32_t>((uint32_t)kFullWaveTile, std::max<uint32_t>(64u, tr));
    }
    const uint32_t n_tiles = cdiv(rows, tq.tile_rows);
    int rc = ensure_tiles(c, n_tiles);
    if (rc) return rc;
    // the engine's table copy carries the derived rows of the binary64 sweep,
    // rebuilt here (deltas and binds since the last run) and kept current by
    // the validator's write-back
    tq.drow = c->d_drow;
    MS_HIP(c, launch_build_drows(tq, rows, n_tiles * tq.tile_rows, s));
    // Step k = ONE launch (launch_seq_step): validation of batch k on workgroup
    // 0 while the other workgroups sweep batch k+1 and then merge its tile lists
    // (the in-step merge); batch k+1 treats batch k's binds as stale. No
    // cross-stream hand-off: each cost ~12 us per batch, and a validation launched
    // beside a sweep waited for a SIMD to drain (two-stream modes and a depth-2
    // step measured slower and removed in round 6: profiles/r02j_e_modes.txt,
    // r04w_e_fused2_ab.txt).
    const uint32_t B = seq_batch(), SB = seq_batch_limit();
    // ranks 4..7 of the merge for the validator's slow pods (profiles/r03v_e_rank8_ab.txt)
    unsigned long long *const top_ext = c->d_top_ext;
    const size_t prev_words = 2 + seq_prev_cap(), prev_fields = (size_t)seq_prev_cap() * seq_rec_fields();
    const size_t cells_per_set = (size_t)SB * n_tiles, recs_per_set = (size_t)SB * seq_topk() * seq_rec_fields();
    // Warm-up batches: the first 4,096 pods of the queue in batches of 64. On an
    // empty cluster every pod prefers the same emptiest nodes, so early batches
    // touch each other's speculative winners most (the slow-path burst of
    // batches 20-30); half-size batches there cut the re-sweeps to 0 and the
    // recomputes by 10 %: config E 39.7 -> 38.5 ms (profiles/r05l_e_ab.txt;
    // 4096:32 / 8192:32 / 16384:32 / 16384:64 / 32768:64 measured slower,
    // r05k_e_warm.txt). Round 6, with the validator's ranks 4..7 walk: none /
    // 4,096 / 8,192 pods 32.3 / 31.1 / 31.2 ms (profiles/r06j_e_warm_ab.txt).
    constexpr uint32_t kWarmPods = 4096, kWarmBatch = 64;
    auto batch_at = [&](uint32_t s0) { return s0 < kWarmPods ? std::min(kWarmBatch, B) : B; };
    const uint32_t nb0 = std::min(batch_at(0), n_pods);
    const SeqMerge merge_mode = seq_merge_mode();
    const bool want_instep = merge_mode != SeqMerge::kLaunch;
    if (want_instep) {
        // Tagged lists: no cell of either set may hold a tag from an earlier run
        // (or an earlier chunk of this call). Both sets, every pod slot: a
        // warm-up batch rewrites only its first pods, and a cell left from a
        // previous run whose 2-bit tag happened to match was taken as swept
        // (config E's second 65,536-pod chunk, pods 64..127 of its first
        // full-size batch: tests/test_gpu_fullsize.py, profiles/r05n_e_probe.txt).
        MS_HIP(c, hipMemsetAsync(c->d_tile_keys, 0,
                                 (size_t)kSeqBufs * cells_per_set * seq_topk() * sizeof(unsigned long long), s));
        MS_HIP(c, hipMemsetAsync(c->d_tile_flags, 0, (size_t)kSeqBufs * cells_per_set * sizeof(uint32_t), s));
    }
    MS_HIP(c, launch_sweep_full_tiles(tq, rows, d_pods, nb0, seed32, c->d_tile_keys, c->d_tile_flags, n_tiles, s));
    MS_HIP(c, launch_topk_merge(c->d_tile_keys, c->d_tile_flags, nb0, n_tiles, c->d_top4, c->d_spec,
                                c->d_spec_flags, tq, c->d_top4_rec, s, top_ext));
    // (the merge of batch k+1: seq_merge_mode above; the lists were cleared above)
    uint32_t k = 0, in_tag = 0;
    for (uint32_t s0 = 0, nb = 0; s0 < n_pods; s0 += nb, ++k) {
        nb = std::min(batch_at(s0), n_pods - s0);
        const uint32_t cur = k & 1u, nxt = cur ^ 1u;
        const uint32_t s1 = s0 + nb, nn = s1 < n_pods ? std::min(batch_at(s1), n_pods - s1) : 0u;
        const size_t top_per_set = (size_t)SB * seq_topk();
        SeqStep st;
        st.t = tq;
        st.n_rows = rows;
        st.n_tiles = n_tiles;
        st.seed32 = seed32;
        st.num_cus = c->num_cus;
        // batch k: validated
        st.pods = d_pods + s0;
        st.n_pods = nb;
        st.tile_keys = c->d_tile_keys + cells_per_set * seq_topk() * cur;
        st.tile_flags = c->d_tile_flags + cells_per_set * cur;
        st.spec = c->d_spec + SB * cur;
        st.spec_flags = c->d_spec_flags + SB * cur;
        st.top4 = c->d_top4 + top_per_set * cur;
        st.top4_recs = c->d_top4_rec + recs_per_set * cur;
        st.top_ext = top_ext + top_per_set * cur;
        st.prev_in = k ? c->d_prev + prev_words * nxt : nullptr;
        st.prev_recs_in = k ? c->d_prev_rec + prev_fields * nxt : nullptr;
        st.prev_out = c->d_prev + prev_words * cur;
        st.prev_recs_out = c->d_prev_rec + prev_fields * cur;
        st.results = d_res + s0;
        st.stats = c->d_overflow;
        // batch k+1: swept, and merged into the other buffer set (in the step, or by the launch below)
        st.next_pods = nn ? d_pods + s1 : nullptr;
        st.n_next = nn;
        st.next_tile_keys = c->d_tile_keys + cells_per_set * seq_topk() * nxt;
        st.next_tile_flags = c->d_tile_flags + cells_per_set * nxt;
        unsigned long long *const top1 = c->d_top4 + top_per_set * nxt, *const spec1 = c->d_spec + SB * nxt;
        unsigned long long *const ext1 = top_ext + top_per_set * nxt;
        uint32_t *const spec_flags1 = c->d_spec_flags + SB * nxt;
        int64_t *const recs1 = c->d_top4_rec + recs_per_set * nxt;
        SeqMergeIO &mio = st.merge;
#if defined(MS_VSTAMPS) || defined(MS_TIMELINE_ONLY)
        // diagnostic builds: timeline of steps 0 .. kTimelineSteps - 1 (MS_TIMELINE=<file>)
        static const bool want_tl = getenv("MS_TIMELINE") != nullptr;
        if (want_tl && !c->d_tl && c->d_tl.alloc((size_t)kTimelineSteps * kTimelineWgs * 8))
            MS_HIP(c, hipMemsetAsync(c->d_tl, 0, (size_t)kTimelineSteps * kTimelineWgs * 8 * 8, s));
#endif
        mio.tl = c->d_tl;
        mio.tl_step = k;
        mio.in_tags = c->d_merge_tags + SB * cur;
        mio.in_tag = in_tag;
        const bool in_step = want_instep && seq_step_merges(tq, n_tiles, nn);
        if (in_step) {
            if (++c->merge_tag == 0) ++c->merge_tag;  // (0: no tag)
            mio.top = top1;
            mio.spec = spec1;
            mio.spec_flags = spec_flags1;
            mio.recs = recs1;
            mio.ext = ext1;
            mio.tags = c->d_merge_tags + SB * nxt;
            mio.tag = c->merge_tag;
            mio.skip = merge_mode == SeqMerge::kFallback ? 1 : 0;
        }
        MS_HIP(c, launch_seq_step(st, s));
        in_tag = in_step ? mio.tag : 0u;
        if (nn && !in_step)
            MS_HIP(c, launch_topk_merge(st.next_tile_keys, st.next_tile_flags, nn, n_tiles, top1, spec1, spec_flags1,
                                        tq, recs1, s, ext1));
    }
    return MS_OK;
}

// This shard's speculative top-4 candidates with records, and its filter flags,
// for a batch of at most MS_SEQ_SHARD_BATCH_MAX pods (ms_seq_candidates_device;
// the in-library node-sharded sequential cycle).
int seq_candidates_locked(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, ms_seq_cand *cands_dev,
                          uint32_t *flags_dev, hipStream_t s) {
    const uint32_t rows = c->rows_dev;
    if (rows == 0) {  // no node listed: no candidates, no rejections
        MS_HIP(c, hipMemsetAsync(cands_dev, 0, sizeof(ms_seq_cand) * kTopKCands * n_pods, s));
        MS_HIP(c, hipMemsetAsync(flags_dev, 0, sizeof(uint32_t) * n_pods, s));
        return MS_OK;
    }
    if (rows > seq_max_rows())
        return fail(c, MS_E_CAPACITY, "ms_seq_candidates_device: at most " + std::to_string(seq_max_rows()) +
                                          " rows per context");
    const uint32_t n_tiles = cdiv(rows, kFullWaveTile);
    int rc = ensure_tiles(c, n_tiles);
    if (rc) return rc;
    const uint32_t seed32 = seed32_of(c->cfg.seed);
    MS_HIP(c, launch_sweep_full_tiles(c->t, rows, pods_dev, n_pods, seed32, c->d_tile_keys, c->d_tile_flags, n_tiles, s));
    MS_HIP(c, launch_topk_merge(c->d_tile_keys, c->d_tile_flags, n_pods, n_tiles, c->d_top4, c->d_spec,
                                c->d_spec_flags, c->t, nullptr, s));
    MS_HIP(c, launch_seq_pack_cands(c->t, c->d_top4, c->d_tile_flags, n_tiles, n_pods, cands_dev, flags_dev, s));
    return MS_OK;
}

void seq_diag_readout(ms_ctx *c) {
    (void)c;
#ifdef MS_VSTAMPS
    {
        uint32_t st[64] = {};
        (void)hipSetDevice(c->cfg.device);
        (void)hipStreamSynchronize(c->stream);
        if (hipMemcpy(st, c->d_overflow, kStatsBytes, hipMemcpyDeviceToHost) == hipSuccess) {
            const uint64_t *cy = reinterpret_cast<const uint64_t *>(st + 8);
            std::fprintf(stderr,
                         "MS_VSTAMPS pods=%u slow=%u tile_scans=%u misses=%u recomputes=%u resweeps=%u rounds=%u cycles: prologue=%llu "
                         "group=%llu prologue_loads=%llu slow=%llu rounds=%llu epilogue=%llu first_slow=%llu round_cand=%llu "
                         "round_claim=%llu | step waves (10 ns): validator=%llu sweep_sum=%llu sweep_waves=%llu | epilogue "
                         "parts: counters=%llu compaction=%llu writeback=%llu | in-step merge (10 ns, summed from each "
                         "workgroup's start): swept=%llu waited=%llu merged=%llu workers=%llu wg_counted=%llu\n",
                         st[3], st[5], st[6], st[4], st[2], st[1], st[7], (unsigned long long)cy[0], (unsigned long long)cy[1],
                         (unsigned long long)cy[2], (unsigned long long)cy[3], (unsigned long long)cy[4],
                         (unsigned long long)cy[5], (unsigned long long)cy[6], (unsigned long long)cy[7],
                         (unsigned long long)cy[8], (unsigned long long)cy[9], (unsigned long long)cy[10],
                         (unsigned long long)cy[11], (unsigned long long)cy[12], (unsigned long long)cy[13],
                         (unsigned long long)cy[14], (unsigned long long)cy[15], (unsigned long long)cy[16],
                         (unsigned long long)cy[17], (unsigned long long)cy[18], (unsigned long long)cy[19]);
        }
    }
#endif
#if defined(MS_VSTAMPS) || defined(MS_TIMELINE_ONLY)
    {
        const char *tlf = getenv("MS_TIMELINE");
        if (tlf && c->d_tl) {
            // (the last step kernels, on any stream, may still be writing the timeline)
            (void)hipDeviceSynchronize();
            std::vector<unsigned long long> tl((size_t)kTimelineSteps * kTimelineWgs * 8);
            if (hipMemcpy(tl.data(), c->d_tl, tl.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                if (FILE *f = std::fopen(tlf, "wb")) {
                    std::fwrite(tl.data(), 8, tl.size(), f);
                    std::fclose(f);
                }
            }
        }
    }
#endif
}

}  // namespace msgpu

using namespace msgpu;

extern "C" {

int ms_schedule_sequential_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, ms_result *results_dev,
                                  void *stream) {
    if (!c || (n_pods && (!pods_dev || !results_dev))) return MS_E_INVAL;
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);  // (deltas were applied on the context stream)
    if (call.rc()) return call.rc();
    const hipStream_t s = call.stream();
    int rc;
    if (c->comm) {
        rc = comm_schedule_device(c, n_pods, pods_dev, results_dev, s);  // node-sharded over the communicator
    } else if (c->cfg.plugin_set == MS_PLUGINS_NU_NRF_NN_LA) {
        rc = run_sequential(c, n_pods, pods_dev, results_dev, s);
    } else {
        // NU+NN: keys are independent of mutable state -> batched cycle + commit
        rc = select_locked(c, n_pods, pods_dev, results_dev, s, 1);
    }
    if (rc) return rc;
    return call.done();
}

int ms_seq_candidates_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, ms_seq_cand *cands_dev,
                             uint32_t *flags_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !cands_dev || !flags_dev))) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NRF_NN_LA)
        return fail(c, MS_E_INVAL, "ms_seq_candidates_device: the resource-aware plugin set only");
    if (n_pods > MS_SEQ_SHARD_BATCH_MAX) return fail(c, MS_E_INVAL, "ms_seq_candidates_device: batch too large");
    if (n_pods == 0) return MS_OK;
    OrderedCall call(c, stream);
    if (call.rc()) return call.rc();
    const int rc = seq_candidates_locked(c, n_pods, pods_dev, cands_dev, flags_dev, call.stream());
    if (rc) return rc;
    return call.done();
}

int ms_seq_validate_device(ms_ctx *c, uint32_t n_pods, const ms_pod_rec *pods_dev, uint32_t n_shards,
                           const ms_seq_cand *cands_all_dev, const uint32_t *flags_all_dev, ms_result *results_dev,
                           uint32_t *n_done_dev, void *stream) {
    if (!c || (n_pods && (!pods_dev || !cands_all_dev || !flags_all_dev || !results_dev || !n_done_dev)))
        return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NRF_NN_LA)
        return fail(c, MS_E_INVAL, "ms_seq_validate_device: the resource-aware plugin set only");
    if (n_pods > MS_SEQ_SHARD_BATCH_MAX || n_shards == 0 || n_shards > MS_SEQ_MAX_SHARDS)
        return fail(c, MS_E_INVAL, "ms_seq_validate_device: batch or shard count out of range");
    if (n_pods == 0) {  // (touches neither table nor scratch: unordered)
        std::lock_guard<std::mutex> g(c->sched_mu);
        MS_HIP(c, hipSetDevice(c->cfg.device));
        MS_HIP(c, hipMemsetAsync(n_done_dev, 0, sizeof(uint32_t), pick_stream(c, stream)));
        return MS_OK;
    }
    OrderedCall call(c, stream, false);  // (deltas are not drained here: the candidates' records must stay current)
    if (call.rc()) return call.rc();
    if (!c->d_merged_flags &&  // (the second of the pair: set only when both are)
        (!c->d_merged.alloc((size_t)kTopKCands * MS_SEQ_SHARD_BATCH_MAX) ||
         !c->d_merged_flags.alloc(MS_SEQ_SHARD_BATCH_MAX)))
        return fail(c, MS_E_OOM, "sharded validator scratch");
    MS_HIP(c, launch_seq_validate_rep(c->t, n_pods, pods_dev, seed32_of(c->cfg.seed), n_shards, cands_all_dev,
                                      flags_all_dev, c->d_merged, c->d_merged_flags, results_dev, n_done_dev,
                                      call.stream()));
    return call.done();
}

}  // extern "C"

// ms_explain.hip — the row view of a pod's cycle (minisched_gpu.h ms_explain_device,
// DESIGN.md §2 "Explain"): per (pod, node) the first failing filter plugin, the
// score plugins' raw scores, their final scores after RunScorePlugins' in-loop
// NormalizeScore hook (the reference's minisched/minisched.go:164-199) and the
// packed selectHost key; per pod the counts a FitError is rendered from. What
// scheduler/plugin/resultstore/store.go keeps per pod and node, for all five
// plugin sets.
//
// A final score under the in-loop hook depends on the pod's whole feasible list
// in LIST order (TaintToleration: the row's rank parity, F, the first three and
// the last feasible node; NodeAffinity: the anchor and the rescales of every
// later node), so the rows come out of three stages over tiles of kExplainTile
// rows, one row per thread:
//   k_ex_tiles  grid (tiles of the table, pods): the tile's present / feasible /
//               per-plugin reject counts (wave ballots), and what the set's hook
//               needs from a LIST-ordered segment: the first feasible row with a
//               non-zero NodeAffinity score (sets 2, 4), the TaintToleration
//               census record (set 3, ms_tt_closed.h) and the tile's composed
//               101-entry rescale table (set 4, ms_nam_device.h);
//   k_ex_scan   one wave per pod over its tiles: the exclusive prefix of the
//               feasible counts (a tile's rank base), the LIST's anchor, the
//               census merged in LIST order and the closed form's per-pod plan
//               (set 3), the reverse exclusive composition of the tiles' tables
//               ("every rescale after this tile", set 4), and the summary;
//   k_ex_rows   grid (tiles, pods): the pair's verdict and raw scores again, the
//               row's rank = tile base + in-tile ballot prefix, the closed forms
//               of DESIGN.md §2, the r3 key; the rows staged in LDS and stored as
//               one contiguous span per tile with 8-byte stores; the tile's best
//               key, which k_ex_best reduces per pod (no atomics: thousands of
//               waves on sixteen addresses serialise).
// Per pod the work is O(table + window): nothing walks a feasible list per row.
// The pair evaluation of the resource-aware set is the sweep's general form
// (ms_rows.h eval_full: int64 LeastAllocated with an exact compare), not the
// binary64 shortcut.
//
// On node shards (ms_explain_sharded_device) a shard is one more tile: k_ex_shard
// reduces a pod's tile records to one ExShard record, the records of all shards
// are all-gathered by the host layer, k_ex_scan_seeded is the scan started from
// them, k_ex_rows runs unchanged, and after a second all-gather of the shards'
// best keys k_ex_best_shards takes their maximum. No kernel waits on a value
// another rank wrote: all cross-rank ordering comes from the collectives.
#include <algorithm>
#include <cstddef>

#include "ms_device.h"
#include "ms_nam_device.h"
#include "ms_rows.h"
#include "ms_tt_closed.h"

namespace msgpu {

namespace {

constexpr uint32_t kExThreads = kExplainTile;
constexpr uint32_t kExWaves = kExThreads / 64u;
constexpr uint32_t kRowNone = 0xFFFFFFFFu;
constexpr uint32_t kRowWords = sizeof(ms_explain_row) / 4;
static_assert(sizeof(ms_explain_row) == 24 && sizeof(ms_explain_summary) == 32, "explain record layout");
static_assert(sizeof(NamSeg) == MS_NAM_SEG_BYTES && MS_NAM_SEG_BYTES % 4 == 0, "NamSeg is copied as words");
static_assert(kExThreads % 64u == 0 && kExThreads >= 64u, "whole waves");

struct ExTile {  // 32 B per (pod, tile)
    uint32_t present, feasible, rej[4];
    uint32_t anchor;  // sets 2, 4: the tile's first feasible row with a non-zero NodeAffinity score (local row)
    uint32_t _pad;
};
struct ExPlan {  // 32 B per pod
    uint32_t F;
    uint32_t anchor;         // sets 2, 4: the LIST's anchor (local row; kRowNone: none)
    int32_t m_last, c_last;  // set 3, F > 4: the last step's list maximum, the last node's raw count
    int32_t v[4];            // set 3: F <= 4 the final scores of ranks 0..3, else ranks 0..2 before the last step
};

struct ExPair {
    uint32_t status;  // 0, the MS_MASK_* bit of the first failing filter, MS_EXPLAIN_ABSENT
    uint32_t nn;      // NodeNumber matches
    uint32_t raw1;    // the second score plugin's Score()
};

// LDS written by one lane of a wave, read by another (one wave only).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A pod's term table of MS_PLUGINS_NU_NN_NAM (null: no terms, no requirement).
__device__ __forceinline__ const uint8_t *ex_tab(const ms_pod_rec &pod, const NamTab *sets, uint32_t n_sets) {
    const uint32_t sid = (uint32_t)pod.pref_zone | (uint32_t)pod.pref_weight << 8;
    return (sid == 0u || sid > n_sets) ? nullptr : reinterpret_cast<const uint8_t *>(sets + (sid - 1u));
}

// One (pod, node) pair: filters in plugin order, the first failure wins
// (minisched.go:130-137), then the raw scores of a node that passed.
template <int kSet>
__device__ __forceinline__ ExPair ex_pair(const NodeTable &t, uint32_t r, uint32_t n_rows, const ms_pod_rec &pod,
                                          const PodFull &pf, const uint8_t *tab) {
    ExPair o = {MS_EXPLAIN_ABSENT, 0u, 0u};
    if (r >= n_rows) return o;
    const uint32_t fl = t.flags[r];
    if (fl & kNodeAbsent) return o;
    if ((fl & kNodeUnschedulable) && !pod.tolerates_unschedulable) {
        o.status = MS_MASK_NODE_UNSCHEDULABLE;
        return o;
    }
    const uint32_t dg = t.digit[r];
    o.nn = (dg <= 9u && (int)dg == (int)pod.name_digit) ? 1u : 0u;
    o.status = 0u;
    if (kSet == MS_PLUGINS_NU_NRF_NN_LA) {
        uint32_t nu = 0, nrf = 0;
        const u64 key = eval_full<true>(load_row(t, r, n_rows), t.base + r, pf, nu, nrf);
        if (nrf) o.status = MS_MASK_NODE_RESOURCES_FIT;
        else o.raw1 = (uint32_t)(key >> 52) - 10u * o.nn;
    } else if (kSet == MS_PLUGINS_NU_NN_NA) {
        o.raw1 = (pod.pref_zone != 0 && t.zone[r] == pod.pref_zone) ? pod.pref_weight : 0u;
    } else if (kSet == MS_PLUGINS_NU_TT_NN) {
        const uint32_t tn = t.taints[r];  // pref_zone / pref_weight: tol_hard / tol_soft (minisched_gpu.h)
        if (tn & 0xFFu & ~(uint32_t)pod.pref_zone) o.status = MS_MASK_TAINT_TOLERATION;
        else o.raw1 = (uint32_t)__popc((tn >> 8) & 0xFFu & ~(uint32_t)pod.pref_weight);
    } else if (kSet == MS_PLUGINS_NU_NN_NAM) {
        const uint32_t m = tab ? nam_terms(nam_row_word(t, r), tab) : kNamNoReqBit;
        if (m <= 15u) o.status = MS_MASK_NODE_AFFINITY;  // no required term matched
        else o.raw1 = tab ? nam_raw(m, tab) : 0u;
    }
    return o;
}

// Every thread's rank among the workgroup's threads with pred (thread order =
// LIST order), and their count. cnt: kExWaves words of LDS; two barriers.
__device__ __forceinline__ uint32_t block_rank(bool pred, uint32_t *cnt, uint32_t &total) {
    const uint64_t b = __ballot(pred);
    const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
    if (lane == 0) cnt[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kExWaves; ++w) {
        const uint32_t c = cnt[w];
        before += w < wv ? c : 0u;
        total += c;
    }
    __syncthreads();
    return before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

enum : uint32_t { kAccPresent = 0, kAccRej = 1, kAccAnchor = 5, kAccOcc = 6, kAccOcc1 = 7, kAccWords = 8 };

template <int kSet>
__global__ __launch_bounds__(kExThreads) void k_ex_tiles(NodeTable t, uint32_t n_rows, uint32_t n_tiles,
                                                         const ms_pod_rec *__restrict__ pods, uint32_t seed32,
                                                         const NamTab *__restrict__ sets, uint32_t n_sets,
                                                         ExTile *__restrict__ tiles, TtCensus *__restrict__ census,
                                                         NamSeg *__restrict__ segs) {
    __shared__ uint32_t cnt[kExWaves];
    __shared__ uint32_t acc[kAccWords];
    __shared__ uint32_t ent[4];  // the tile's feasible ranks 0..2 and its last (TtCensus entries)
    __shared__ uint32_t resc[kExThreads];  // the raw scores above 100 of the tile's feasible rows, in LIST order
    __shared__ __attribute__((aligned(16))) uint8_t tab[MS_NAM_SEG_BYTES];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const uint32_t tile = blockIdx.x, p = blockIdx.y, r = tile * kExThreads + tid;
    const size_t at = (size_t)p * n_tiles + tile;
    const ms_pod_rec pod = pods[p];
    PodFull pf = {};
    if (kSet == MS_PLUGINS_NU_NRF_NN_LA) pf = load_pod(pod, seed32);
    const uint8_t *nt = kSet == MS_PLUGINS_NU_NN_NAM ? ex_tab(pod, sets, n_sets) : nullptr;
    if (tid < kAccWords) acc[tid] = tid == kAccAnchor ? kRowNone : 0u;
    if (tid < 4u) ent[tid] = kEntNone;
    const ExPair x = ex_pair<kSet>(t, r, n_rows, pod, pf, nt);
    const bool feas = x.status == 0u;
    uint32_t F = 0;
    const uint32_t rank = block_rank(feas, cnt, F);  // (its barriers also publish acc and ent)
    const uint64_t b_pres = __ballot(x.status != MS_EXPLAIN_ABSENT);
    if (lane == 0 && b_pres) atomicAdd(&acc[kAccPresent], (uint32_t)__popcll(b_pres));
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint64_t b = __ballot(x.status == (1u << i));
        if (lane == 0 && b) atomicAdd(&acc[kAccRej + i], (uint32_t)__popcll(b));
    }
    if (kSet == MS_PLUGINS_NU_NN_NA || kSet == MS_PLUGINS_NU_NN_NAM) {
        const uint64_t b = __ballot(feas && x.raw1 > 0u);
        if (lane == 0 && b) atomicMin(&acc[kAccAnchor], tile * kExThreads + wv * 64u + (uint32_t)__builtin_ctzll(b));
    }
    if (kSet == MS_PLUGINS_NU_TT_NN && feas) {
        const uint32_t e = ent_pack(t.base + r, x.raw1, x.nn);
        if (rank < 3u) ent[rank] = e;
        if (rank + 1u == F) ent[3] = e;
        if (rank >= 3u && rank + 1u < F) {  // a middle row: its class by the in-tile rank parity
            const uint32_t k = 1u << (2u * x.raw1 + (rank & 1u));
            atomicOr(&acc[kAccOcc], k);
            if (x.nn) atomicOr(&acc[kAccOcc1], k);
        }
    }
    uint32_t n_resc = 0;
    if (kSet == MS_PLUGINS_NU_NN_NAM) {
        const bool rs = feas && x.raw1 > 100u;
        const uint32_t pos = block_rank(rs, cnt, n_resc);
        if (rs) resc[pos] = x.raw1;
    }
    __syncthreads();
    if (kSet == MS_PLUGINS_NU_NN_NAM && wv == 0u) {
        // the tile's rescales composed forward, T <- f_r o T (k_nam_seg's table of a segment)
        if (lane == 0) table_identity(tab);
        wave_lds_sync();
        for (uint32_t k = 0; k < n_resc && tab[100] != 0; ++k) {  // (all 0 stays all 0)
            table_post(tab, resc[k], lane);
            wave_lds_sync();
        }
        if (lane == 0) {
            tab[101] = acc[kAccAnchor] != kRowNone ? 1 : 0;
            tab[102] = acc[kAccRej + 0] ? 1 : 0;
            tab[103] = acc[kAccRej + 3] ? 1 : 0;
        }
        wave_lds_sync();
        if (lane < MS_NAM_SEG_BYTES / 4u)
            reinterpret_cast<uint32_t *>(segs + at)[lane] = reinterpret_cast<const uint32_t *>(tab)[lane];
    }
    if (tid == 0) {
        ExTile o;
        o.present = acc[kAccPresent];
        o.feasible = F;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) o.rej[i] = acc[kAccRej + i];
        o.anchor = acc[kAccAnchor];
        o._pad = 0;
        tiles[at] = o;
        if (kSet == MS_PLUGINS_NU_TT_NN) {
            TtCensus c;
            c.n = F;
            c.flags = (o.rej[0] ? (uint32_t)MS_MASK_NODE_UNSCHEDULABLE : 0u) |
                      (o.rej[2] ? (uint32_t)MS_MASK_TAINT_TOLERATION : 0u);
            c.occ = acc[kAccOcc];
            c.occ1 = acc[kAccOcc1];
            c.first[0] = ent[0];
            c.first[1] = ent[1];
            c.first[2] = ent[2];
            c.last = ent[3];
            census[at] = c;
        }
    }
}

// The per-pod values of TaintToleration's closed form that a ROW's final score
// needs (oracle/ms_oracle.c tt_closed; k_tt2_plan derives the winning classes
// from the same steps): with F <= 4 the loop itself over the explicit entries,
// else entries 0..2 through their three steps and the F - 4 flips, and the last
// step's list maximum.
__device__ __forceinline__ void ex_tt_plan(const TtCensus &r, ExPlan &plan) {
    const uint32_t F = r.n;
    if (F == 0u) return;
    if (F <= 4u) {
        const uint32_t e[4] = {r.first[0], r.first[1], r.first[2], r.last};
        int32_t s[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < F; ++k) {
            s[k] = (int32_t)ent_cc(e[k]);
            int32_t m = 0;
            for (uint32_t i = 0; i < F; ++i) m = max(m, s[i]);
            for (uint32_t i = 0; i < F; ++i) s[i] = tt_map(m, s[i]);
        }
        for (int k = 0; k < 4; ++k) plan.v[k] = s[k];
        return;
    }
    int32_t s[3], u = 0;  // entries 0..2 and the unscored entries after step 2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = (int32_t)ent_cc(r.first[k]);
        int32_t m = u;
        for (int i = 0; i <= k; ++i) m = max(m, s[i]);
        for (int i = 0; i <= k; ++i) s[i] = tt_map(m, s[i]);
        u = tt_map(m, u);
    }
    const bool nf_odd = ((F - 4u) & 1u) != 0u;  // flips of steps 3 .. F-2
    const int32_t c_last = (int32_t)ent_cc(r.last);
    int32_t m_last = c_last;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        plan.v[k] = nf_odd ? 100 - s[k] : s[k];
        m_last = max(m_last, plan.v[k]);
    }
    for (uint32_t k = 0; k < 18u; ++k)
        if ((r.occ >> k) & 1u) {  // class (c, rank parity): flipped F-2-j times after its own step
            const int32_t c = (int32_t)(k >> 1);
            m_last = max(m_last, ((k & 1u) == (F & 1u)) ? 100 - c : c);
        }
    plan.v[3] = 0;
    plan.m_last = m_last;
    plan.c_last = c_last;
}

// A row's final TaintToleration score from the plan, its global rank and raw count.
__device__ __forceinline__ uint32_t ex_tt_final(const ExPlan &plan, uint32_t rank, uint32_t c) {
    const uint32_t F = plan.F;
    if (F <= 4u) return (uint32_t)plan.v[rank & 3u];
    int32_t v;
    if (rank < 3u) v = plan.v[rank];
    else if (rank + 1u == F) v = plan.c_last;
    else v = ((rank & 1u) == (F & 1u)) ? 100 - (int32_t)c : (int32_t)c;
    return (uint32_t)tt_map(plan.m_last, v);
}

// One wave per pod.
template <int kSet>
__global__ __launch_bounds__(64) void k_ex_scan(uint32_t n_tiles, const ExTile *__restrict__ tiles,
                                                const TtCensus *__restrict__ census,
                                                const NamSeg *__restrict__ segs, uint32_t *__restrict__ base,
                                                NamSeg *__restrict__ after, ExPlan *__restrict__ plans,
                                                ms_explain_summary *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[MS_NAM_SEG_BYTES];
    __shared__ TtCensus cs[64];
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const size_t at0 = (size_t)p * n_tiles;
    uint32_t present = 0, rej[4] = {0, 0, 0, 0}, run = 0, anchor_inv = 0;
    TtCensus merged = {};
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += 64u) {
        const uint32_t i = b0 + lane;
        ExTile x = {};
        x.anchor = kRowNone;
        if (i < n_tiles) x = tiles[at0 + i];
        present += x.present;
#pragma unroll
        for (int k = 0; k < 4; ++k) rej[k] += x.rej[k];
        anchor_inv = max(anchor_inv, ~x.anchor);
        uint32_t inc = x.feasible;  // inclusive scan over the lanes
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inc, off, 64);
            if (lane >= off) inc += v;
        }
        if (i < n_tiles) base[at0 + i] = run + inc - x.feasible;
        run += (uint32_t)__shfl((int)inc, 63, 64);
        if (kSet == MS_PLUGINS_NU_TT_NN) {  // 64 census records staged, merged in LIST order by one lane
            if (i < n_tiles) cs[lane] = census[at0 + i];
            wave_lds_sync();
            if (lane == 0) {
                const uint32_t n = min(64u, n_tiles - b0);
                for (uint32_t k = 0; k < n; ++k) {
                    if (b0 + k == 0u) merged = cs[0];
                    else tt2_merge(merged, cs[k]);
                }
            }
            wave_lds_sync();
        }
    }
    present = wave_sum_u32_dpp(present);
#pragma unroll
    for (int k = 0; k < 4; ++k) rej[k] = wave_sum_u32_dpp(rej[k]);
    const uint32_t anchor = ~wave_max_u32_dpp(anchor_inv);  // the least row: the first in LIST order
    if (kSet == MS_PLUGINS_NU_NN_NAM) {
        // after[tile] = the rescales of every LATER tile composed: U <- U o T_tile, tiles descending
        if (lane == 0) table_identity(tab);
        wave_lds_sync();
        for (uint32_t tile = n_tiles; tile-- > 0u;) {
            if (lane < MS_NAM_SEG_BYTES / 4u)
                reinterpret_cast<uint32_t *>(after + at0 + tile)[lane] = reinterpret_cast<const uint32_t *>(tab)[lane];
            const NamSeg *T = segs + at0 + tile;
            // (a tile without a rescale is the identity: every f_r takes 100 below 100; all 0 stays all 0)
            if (T->T[100] == 100 || tab[100] == 0) continue;
            const uint32_t v0 = lane, v1 = lane + 64u;
            const uint8_t a = tab[T->T[v0]];
            const uint8_t b = v1 <= 100u ? tab[T->T[v1]] : 0;
            wave_lds_sync();
            tab[v0] = a;
            if (v1 <= 100u) tab[v1] = b;
            wave_lds_sync();
        }
    }
    if (lane != 0) return;
    ExPlan plan = {};
    plan.F = run;
    plan.anchor = anchor;
    if (kSet == MS_PLUGINS_NU_TT_NN) ex_tt_plan(merged, plan);
    plans[p] = plan;
    ms_explain_summary o;
    o.present = present;
    o.feasible = run;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.rejected[k] = rej[k];
    o.best_key = 0;
    sums[p] = o;
}

// grid (tiles from tile0, pods). tile_best (optional): the tile's best key per
// (pod, tile). rows (optional): the window [win_lo, win_lo + win_n) of local
// rows, pod-major.
template <int kSet>
__global__ __launch_bounds__(kExThreads) void k_ex_rows(NodeTable t, uint32_t n_rows, uint32_t n_tiles, uint32_t tile0,
                                                        const ms_pod_rec *__restrict__ pods, uint32_t seed32,
                                                        uint32_t w_nn, uint32_t w_na, const NamTab *__restrict__ sets,
                                                        uint32_t n_sets, const uint32_t *__restrict__ base,
                                                        const NamSeg *__restrict__ after,
                                                        const ExPlan *__restrict__ plans,
                                                        u64 *__restrict__ tile_best,
                                                        ms_explain_row *__restrict__ rows, uint32_t win_lo,
                                                        uint32_t win_n) {
    __shared__ uint32_t cnt[kExWaves];
    __shared__ u64 wbest[kExWaves];
    __shared__ uint32_t magic[kExThreads];  // div_magic of the tile's rescaling rows, in LIST order
    __shared__ __attribute__((aligned(16))) uint32_t stage[kExThreads * kRowWords];
    constexpr bool kHook = kSet == MS_PLUGINS_NU_NN_NA || kSet == MS_PLUGINS_NU_TT_NN || kSet == MS_PLUGINS_NU_NN_NAM;
    constexpr bool kWeights = kSet == MS_PLUGINS_NU_NN_NA || kSet == MS_PLUGINS_NU_NN_NAM;
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t tile = tile0 + blockIdx.x, p = blockIdx.y, r = tile * kExThreads + tid;
    const size_t at = (size_t)p * n_tiles + tile;
    const ms_pod_rec pod = pods[p];
    PodFull pf = {};
    if (kSet == MS_PLUGINS_NU_NRF_NN_LA) pf = load_pod(pod, seed32);
    const uint8_t *nt = kSet == MS_PLUGINS_NU_NN_NAM ? ex_tab(pod, sets, n_sets) : nullptr;
    const ExPair x = ex_pair<kSet>(t, r, n_rows, pod, pf, nt);
    const bool feas = x.status == 0u;
    ExPlan plan = {};
    if (kHook) plan = plans[p];
    uint32_t fin = x.raw1;  // the second plugin's score after the hook (sets 0, 1: no ScoreExtensions)
    if (kSet == MS_PLUGINS_NU_NN_NA) fin = r == plan.anchor ? 100u : x.raw1;
    if (kSet == MS_PLUGINS_NU_TT_NN) {
        uint32_t F_tile = 0;
        const uint32_t rank = base[at] + block_rank(feas, cnt, F_tile);
        fin = feas ? ex_tt_final(plan, rank, x.raw1) : 0u;
    }
    if (kSet == MS_PLUGINS_NU_NN_NAM) {
        // T_{>j}(v_j): the tile's later rescales one by one, then every later tile's table
        const bool rs = feas && x.raw1 > 100u;
        uint32_t n_resc = 0;
        const uint32_t pos = block_rank(rs, cnt, n_resc);
        if (rs) magic[pos] = div_magic(x.raw1);
        __syncthreads();
        uint32_t v = (r == plan.anchor || x.raw1 > 100u) ? 100u : x.raw1;
        if (feas) {
            for (uint32_t k = pos + (rs ? 1u : 0u); k < n_resc; ++k) v = f_r(v, magic[k]);
            v = after[at].T[v];
        }
        fin = feas ? v : 0u;
    }
    const bool scored = feas && pod.name_digit >= 0;  // a non-digit pod's Score fails on the first node
    const uint32_t ord = t.base + r;
    const uint32_t raw0 = 10u * x.nn;
    const uint32_t w0 = raw0 * (kWeights ? w_nn : 1u), w1 = fin * (kWeights ? w_na : 1u);
    const u64 key = scored ? make_key(w0 + w1, tb_hash(tb_pod(seed32, pod.ordinal), ord), ord) : 0ull;
    if (tile_best) {  // the tile's best key: the waves' maxima combined in LDS (k_ex_best reduces the tiles)
        const u64 m = wave_max_u64(key);
        if (lane == 0) wbest[tid >> 6] = m;
    }
    uint32_t *mine = stage + tid * kRowWords;
    mine[0] = (uint32_t)key;
    mine[1] = (uint32_t)(key >> 32);
    mine[2] = scored ? (raw0 | x.raw1 << 16) : 0u;
    mine[3] = scored ? (w0 | w1 << 16) : 0u;
    mine[4] = x.status;
    mine[5] = 0u;
    __syncthreads();
    if (tile_best && tid == 0) {
        u64 m = wbest[0];
#pragma unroll
        for (uint32_t w = 1; w < kExWaves; ++w) m = umax64(m, wbest[w]);
        tile_best[at] = m;
    }
    if (!rows) return;  // (uniform)
    // the tile's rows inside the window: one contiguous span, 8-byte stores
    const uint32_t t_lo = tile * kExThreads;
    const uint32_t lo = max(win_lo, t_lo), hi = min(win_lo + win_n, t_lo + kExThreads);
    if (lo >= hi) return;
    const uint2 *src = reinterpret_cast<const uint2 *>(stage + (size_t)(lo - t_lo) * kRowWords);
    uint2 *dst = reinterpret_cast<uint2 *>(rows + (size_t)p * win_n + (lo - win_lo));
    const uint32_t n2 = (hi - lo) * (kRowWords / 2u);
    for (uint32_t i = tid; i < n2; i += kExThreads) dst[i] = src[i];
}

// One wave per pod: best_key = the maximum of its tiles' best keys (selectHost).
__global__ __launch_bounds__(64) void k_ex_best(uint32_t n_tiles, const u64 *__restrict__ tile_best,
                                                ms_explain_summary *__restrict__ sums) {
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    u64 m = 0;
    for (uint32_t i = lane; i < n_tiles; i += 64u) m = umax64(m, tile_best[(size_t)p * n_tiles + i]);
    m = wave_max_u64(m);
    if (lane == 0) sums[p].best_key = m;
}

// ---- node shards (minisched_gpu.h ms_explain_sharded_device) ---------------
// A shard is one more tile: per pod it hands the other shards one record of what
// its tiles hand k_ex_scan, each part associative and in LIST order (the shards
// in rank order). The records of all G shards are gathered shard-major
// (all[s * n_pods + p]); k_ex_scan_seeded is k_ex_scan started from them. The
// layout is internal: the host layer moves the records as bytes.
struct ExShard {  // 168 B per (shard, pod), the same for every set
    uint32_t present, feasible, rej[4];
    uint32_t anchor;  // sets 2, 4: the shard's anchor as a GLOBAL ordinal (kRowNone: none)
    uint32_t _pad;
    TtCensus census;  // set 3: the shard's tiles merged (tt2_merge; its entries hold global ordinals)
    NamSeg seg;       // set 4: the shard's composed rescale table, its "any" and filter bits
};
static_assert(sizeof(ExShard) == 168 && sizeof(ExShard) % 8 == 0 && offsetof(ExShard, seg) % 4 == 0,
              "ExShard is gathered as bytes and its table copied as words");

// U <- U o T on the wave's LDS table (k_ex_scan's step): entries lane, lane + 64.
__device__ __forceinline__ void table_compose(uint8_t *tab, const uint8_t *T, uint32_t lane) {
    const uint32_t v0 = lane, v1 = lane + 64u;
    const uint8_t a = tab[T[v0]];
    const uint8_t b = v1 <= 100u ? tab[T[v1]] : 0;
    wave_lds_sync();
    tab[v0] = a;
    if (v1 <= 100u) tab[v1] = b;
    wave_lds_sync();
}

// One wave per pod: the shard's record from its tiles' records (mine[p]).
template <int kSet>
__global__ __launch_bounds__(64) void k_ex_shard(uint32_t n_tiles, uint32_t node_base,
                                                 const ExTile *__restrict__ tiles,
                                                 const TtCensus *__restrict__ census,
                                                 const NamSeg *__restrict__ segs, ExShard *__restrict__ mine) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[MS_NAM_SEG_BYTES];
    __shared__ TtCensus cs[64];
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const size_t at0 = (size_t)p * n_tiles;
    uint32_t present = 0, feasible = 0, rej[4] = {0, 0, 0, 0}, anchor_inv = 0, bits = 0;
    TtCensus merged = {};
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += 64u) {
        const uint32_t i = b0 + lane;
        ExTile x = {};
        x.anchor = kRowNone;
        if (i < n_tiles) x = tiles[at0 + i];
        present += x.present;
        feasible += x.feasible;
#pragma unroll
        for (int k = 0; k < 4; ++k) rej[k] += x.rej[k];
        anchor_inv = max(anchor_inv, ~x.anchor);
        if (kSet == MS_PLUGINS_NU_NN_NAM && i < n_tiles) {
            const NamSeg *T = segs + at0 + i;
            bits |= (T->any ? 1u : 0u) | (T->_pad[0] ? 2u : 0u) | (T->_pad[1] ? 4u : 0u);
        }
        if (kSet == MS_PLUGINS_NU_TT_NN) {  // as k_ex_scan: 64 records staged, merged in LIST order by one lane
            if (i < n_tiles) cs[lane] = census[at0 + i];
            wave_lds_sync();
            if (lane == 0) {
                const uint32_t n = min(64u, n_tiles - b0);
                for (uint32_t k = 0; k < n; ++k) {
                    if (b0 + k == 0u) merged = cs[0];
                    else tt2_merge(merged, cs[k]);
                }
            }
            wave_lds_sync();
        }
    }
    present = wave_sum_u32_dpp(present);
    feasible = wave_sum_u32_dpp(feasible);
#pragma unroll
    for (int k = 0; k < 4; ++k) rej[k] = wave_sum_u32_dpp(rej[k]);
    const uint32_t anchor = ~wave_max_u32_dpp(anchor_inv);
    uint32_t *seg_out = reinterpret_cast<uint32_t *>(&mine[p].seg);
    if (kSet == MS_PLUGINS_NU_NN_NAM) {
        // k_ex_scan's descending composition taken one step further, through tile 0. The "any" and
        // filter bits are carried so that the record is a whole NamSeg of the shard, as a tile's is
        // of the tile; the seeded scan and the rows read T[0..100] only.
        const bool any = __ballot(bits & 1u) != 0ull, f_nu = __ballot(bits & 2u) != 0ull,
                   f_na = __ballot(bits & 4u) != 0ull;
        if (lane == 0) table_identity(tab);
        wave_lds_sync();
        for (uint32_t tile = n_tiles; tile-- > 0u;) {
            const NamSeg *T = segs + at0 + tile;
            if (T->T[100] == 100 || tab[100] == 0) continue;  // (the identity; all 0 stays all 0)
            table_compose(tab, T->T, lane);
        }
        if (lane == 0) {
            tab[101] = any ? 1 : 0;
            tab[102] = f_nu ? 1 : 0;
            tab[103] = f_na ? 1 : 0;
        }
        wave_lds_sync();
        if (lane < MS_NAM_SEG_BYTES / 4u) seg_out[lane] = reinterpret_cast<const uint32_t *>(tab)[lane];
    } else if (lane < MS_NAM_SEG_BYTES / 4u) {
        seg_out[lane] = 0u;  // (no table in this set: the record's bytes stay defined)
    }
    if (lane != 0) return;
    ExShard &o = mine[p];
    o.present = present;
    o.feasible = feasible;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.rej[k] = rej[k];
    o.anchor = anchor == kRowNone ? kRowNone : node_base + anchor;
    o._pad = 0;
    o.census = merged;  // (all zero outside set 3)
}

// k_ex_scan for one shard of G (`shard`), started from the G gathered records
// instead of from nothing: a tile's rank base begins at the feasible count of the
// earlier shards, the plan comes from every shard's census merged in rank order
// (the same on every rank), the anchor is the cluster's least anchor ordinal (a
// local row only on the shard that holds it), after[] begins at the later
// shards' tables composed (ranks descending), and the summary counts are the
// sums over the shards. best_key is left 0 (k_ex_best_shards).
template <int kSet>
__global__ __launch_bounds__(64) void k_ex_scan_seeded(uint32_t n_tiles, uint32_t n_pods, uint32_t n_shards,
                                                       uint32_t shard, uint32_t node_base, uint32_t n_local,
                                                       const ExShard *__restrict__ all,
                                                       const ExTile *__restrict__ tiles,
                                                       const NamSeg *__restrict__ segs, uint32_t *__restrict__ base,
                                                       NamSeg *__restrict__ after, ExPlan *__restrict__ plans,
                                                       ms_explain_summary *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[MS_NAM_SEG_BYTES];
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const size_t at0 = (size_t)p * n_tiles;
    // the shards' counts: one shard per lane and round
    uint32_t present = 0, feasible = 0, before = 0, rej[4] = {0, 0, 0, 0}, anchor_min = kRowNone;
    for (uint32_t s0 = 0; s0 < n_shards; s0 += 64u) {
        const uint32_t s = s0 + lane;
        if (s >= n_shards) continue;
        const ExShard &x = all[(size_t)s * n_pods + p];
        present += x.present;
        feasible += x.feasible;
        before += s < shard ? x.feasible : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) rej[k] += x.rej[k];
        anchor_min = min(anchor_min, x.anchor);
    }
    present = wave_sum_u32_dpp(present);
    feasible = wave_sum_u32_dpp(feasible);
    before = wave_sum_u32_dpp(before);
#pragma unroll
    for (int k = 0; k < 4; ++k) rej[k] = wave_sum_u32_dpp(rej[k]);
    anchor_min = ~wave_max_u32_dpp(~anchor_min);  // the least ordinal: the first in LIST order
    // the rank base of this shard's tiles: the earlier shards' feasible rows, then the in-shard prefix
    uint32_t run = before;
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += 64u) {
        const uint32_t i = b0 + lane;
        const uint32_t f = i < n_tiles ? tiles[at0 + i].feasible : 0u;
        uint32_t inc = f;  // inclusive scan over the lanes
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inc, off, 64);
            if (lane >= off) inc += v;
        }
        if (i < n_tiles) base[at0 + i] = run + inc - f;
        run += (uint32_t)__shfl((int)inc, 63, 64);
    }
    if (kSet == MS_PLUGINS_NU_NN_NAM) {
        // after[tile] = the rescales of every LATER tile and shard composed: the later shards'
        // tables first (ranks descending to shard + 1), then this shard's tiles descending
        if (lane == 0) table_identity(tab);
        wave_lds_sync();
        for (uint32_t s = n_shards; s-- > shard + 1u;) {
            const NamSeg *T = &all[(size_t)s * n_pods + p].seg;
            if (T->T[100] == 100 || tab[100] == 0) continue;
            table_compose(tab, T->T, lane);
        }
        for (uint32_t tile = n_tiles; tile-- > 0u;) {
            if (lane < MS_NAM_SEG_BYTES / 4u)
                reinterpret_cast<uint32_t *>(after + at0 + tile)[lane] = reinterpret_cast<const uint32_t *>(tab)[lane];
            const NamSeg *T = segs + at0 + tile;
            if (T->T[100] == 100 || tab[100] == 0) continue;
            table_compose(tab, T->T, lane);
        }
    }
    if (lane != 0) return;
    ExPlan plan = {};
    plan.F = feasible;
    const uint32_t a = anchor_min - node_base;  // (wraps past n_local below this shard's range)
    plan.anchor = (anchor_min != kRowNone && anchor_min >= node_base && a < n_local) ? a : kRowNone;
    if (kSet == MS_PLUGINS_NU_TT_NN) {
        TtCensus merged = all[p].census;
        for (uint32_t s = 1; s < n_shards; ++s) tt2_merge(merged, all[(size_t)s * n_pods + p].census);
        ex_tt_plan(merged, plan);
    }
    plans[p] = plan;
    ms_explain_summary o;
    o.present = present;
    o.feasible = feasible;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.rejected[k] = rej[k];
    o.best_key = 0;
    sums[p] = o;
}

// One wave per pod: this shard's best key (k_ex_best's maximum) into best[p].
__global__ __launch_bounds__(64) void k_ex_best_shard(uint32_t n_tiles, const u64 *__restrict__ tile_best,
                                                      u64 *__restrict__ best) {
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    u64 m = 0;
    for (uint32_t i = lane; i < n_tiles; i += 64u) m = umax64(m, tile_best[(size_t)p * n_tiles + i]);
    m = wave_max_u64(m);
    if (lane == 0) best[p] = m;
}

// One thread per pod: best_key = the maximum of the G gathered shard maxima
// (the keys embed the global ordinal: selectHost over the union of the shards).
__global__ __launch_bounds__(256) void k_ex_best_shards(uint32_t n_pods, uint32_t n_shards,
                                                        const u64 *__restrict__ best_all,
                                                        ms_explain_summary *__restrict__ sums) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pods) return;
    u64 m = 0;
    for (uint32_t s = 0; s < n_shards; ++s) m = umax64(m, best_all[(size_t)s * n_pods + p]);
    sums[p].best_key = m;
}

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct ExScratch {
    ms_explain_summary *sums;
    ExPlan *plans;
    ExTile *tiles;
    uint32_t *base;
    u64 *tile_best;
    TtCensus *census;
    NamSeg *segs, *after;
    // node shards (n_shards > 0): the G gathered records and best keys, shard-major
    ExShard *shard_all;
    u64 *best_all;
    size_t bytes;
};

ExScratch ex_layout(void *scratch, int32_t plugin_set, uint32_t extent, uint32_t n_pods, uint32_t n_shards = 0) {
    const size_t cells = (size_t)cdiv(std::max(extent, 1u), kExThreads) * std::max(n_pods, 1u);
    char *b = static_cast<char *>(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char *at = b + o;
        o += align256(bytes);
        return at;
    };
    ExScratch x;
    x.sums = reinterpret_cast<ms_explain_summary *>(take((size_t)MS_EXPLAIN_MAX_PODS * sizeof(ms_explain_summary)));
    x.plans = reinterpret_cast<ExPlan *>(take((size_t)MS_EXPLAIN_MAX_PODS * sizeof(ExPlan)));
    x.tiles = reinterpret_cast<ExTile *>(take(cells * sizeof(ExTile)));
    x.base = reinterpret_cast<uint32_t *>(take(cells * 4));
    x.tile_best = reinterpret_cast<u64 *>(take(cells * 8));
    x.census = reinterpret_cast<TtCensus *>(take(plugin_set == MS_PLUGINS_NU_TT_NN ? cells * sizeof(TtCensus) : 0));
    x.segs = reinterpret_cast<NamSeg *>(take(plugin_set == MS_PLUGINS_NU_NN_NAM ? cells * sizeof(NamSeg) : 0));
    x.after = reinterpret_cast<NamSeg *>(take(plugin_set == MS_PLUGINS_NU_NN_NAM ? cells * sizeof(NamSeg) : 0));
    // (after everything else: the single-context layout is the prefix)
    const size_t gathered = (size_t)n_shards * std::max(n_pods, 1u);
    x.shard_all = reinterpret_cast<ExShard *>(take(gathered * sizeof(ExShard)));
    x.best_all = reinterpret_cast<u64 *>(take(gathered * 8));
    x.bytes = o;
    return x;
}

template <int kSet>
hipError_t launch_set(const ExplainArgs &a, hipStream_t s) {
    const uint32_t extent = explain_extent(a.n_rows, a.win_lo, a.win_n, a.rows != nullptr);
    const uint32_t n_tiles = cdiv(extent, kExThreads);
    const ExScratch x = ex_layout(a.scratch, kSet, extent, a.n_pods);
    const NamTab *sets = static_cast<const NamTab *>(a.sets);
    constexpr bool kHook = kSet == MS_PLUGINS_NU_NN_NA || kSet == MS_PLUGINS_NU_TT_NN || kSet == MS_PLUGINS_NU_NN_NAM;
    if (a.summaries || kHook) {  // (sets 0 and 1: a row needs nothing of the rest of the LIST)
        hipLaunchKernelGGL(k_ex_tiles<kSet>, dim3(n_tiles, a.n_pods), dim3(kExThreads), 0, s, a.t, a.n_rows, n_tiles,
                           a.pods, a.seed32, sets, a.n_sets, x.tiles, x.census, x.segs);
        hipLaunchKernelGGL(k_ex_scan<kSet>, dim3(a.n_pods), dim3(64), 0, s, n_tiles, x.tiles, x.census, x.segs, x.base,
                           x.after, x.plans, x.sums);
    }
    // the rows' tiles: the whole table for the best keys, else the window's
    uint32_t t0 = 0, t1 = n_tiles;
    if (!a.summaries) {
        t0 = a.win_lo / kExThreads;
        t1 = a.win_n ? cdiv(a.win_lo + a.win_n, kExThreads) : t0;
    }
    if (t1 > t0)
        hipLaunchKernelGGL(k_ex_rows<kSet>, dim3(t1 - t0, a.n_pods), dim3(kExThreads), 0, s, a.t, a.n_rows, n_tiles, t0,
                           a.pods, a.seed32, a.w_nn, a.w_na, sets, a.n_sets, x.base, x.after, x.plans,
                           a.summaries ? x.tile_best : nullptr, a.win_n ? a.rows : nullptr, a.win_lo, a.win_n);
    if (a.summaries)
        hipLaunchKernelGGL(k_ex_best, dim3(a.n_pods), dim3(64), 0, s, n_tiles, x.tile_best, x.sums);
    return hipGetLastError();
}

// The tiles a sharded call covers: the whole table always (the best keys), and the window.
inline uint32_t shard_extent(const ExplainArgs &a) { return explain_extent(a.n_rows, a.win_lo, a.win_n, true); }

template <int kSet>
hipError_t launch_shard_set(const ExplainArgs &a, ExplainShardStage stage, uint32_t p0, uint32_t nb, hipStream_t s) {
    const uint32_t extent = shard_extent(a);
    const uint32_t n_tiles = cdiv(extent, kExThreads);
    const ExScratch x = ex_layout(a.scratch, kSet, extent, a.n_pods, a.n_shards);
    const NamTab *sets = static_cast<const NamTab *>(a.sets);
    ExShard *mine = x.shard_all + (size_t)a.shard * a.n_pods;
    u64 *best_mine = x.best_all + (size_t)a.shard * a.n_pods;
    switch (stage) {
        case kExShardRecords:
            hipLaunchKernelGGL(k_ex_tiles<kSet>, dim3(n_tiles, a.n_pods), dim3(kExThreads), 0, s, a.t, a.n_rows, n_tiles,
                               a.pods, a.seed32, sets, a.n_sets, x.tiles, x.census, x.segs);
            hipLaunchKernelGGL(k_ex_shard<kSet>, dim3(a.n_pods), dim3(64), 0, s, n_tiles, a.t.base, x.tiles, x.census,
                               x.segs, mine);
            break;
        case kExShardScan:
            hipLaunchKernelGGL(k_ex_scan_seeded<kSet>, dim3(a.n_pods), dim3(64), 0, s, n_tiles, a.n_pods, a.n_shards,
                               a.shard, a.t.base, a.n_rows, x.shard_all, x.tiles, x.segs, x.base, x.after, x.plans,
                               x.sums);
            break;
        case kExShardRows: {  // pods [p0, p0 + nb): every tile (the best keys), the window's rows into a.rows
            const size_t c0 = (size_t)p0 * n_tiles;
            hipLaunchKernelGGL(k_ex_rows<kSet>, dim3(n_tiles, nb), dim3(kExThreads), 0, s, a.t, a.n_rows, n_tiles, 0u,
                               a.pods + p0, a.seed32, a.w_nn, a.w_na, sets, a.n_sets, x.base + c0, x.after + c0,
                               x.plans + p0, x.tile_best + c0, a.win_n ? a.rows : nullptr, a.win_lo, a.win_n);
            break;
        }
        case kExShardBest:
            hipLaunchKernelGGL(k_ex_best_shard, dim3(a.n_pods), dim3(64), 0, s, n_tiles, x.tile_best, best_mine);
            break;
        case kExShardMax:
            hipLaunchKernelGGL(k_ex_best_shards, dim3(cdiv(a.n_pods, 256u)), dim3(256), 0, s, a.n_pods, a.n_shards,
                               x.best_all, x.sums);
            break;
    }
    return hipGetLastError();
}

}  // namespace

uint32_t explain_extent(uint32_t n_rows, uint32_t win_lo, uint32_t win_n, bool rows) {
    return std::max(1u, std::max(n_rows, rows ? win_lo + win_n : 0u));
}

size_t explain_scratch_bytes(int32_t plugin_set, uint32_t extent, uint32_t n_pods) {
    return ex_layout(nullptr, plugin_set, extent, n_pods).bytes;
}

ms_explain_summary *explain_summaries(void *scratch) { return ex_layout(scratch, 0, 1, 1).sums; }

size_t explain_shard_scratch_bytes(const ExplainArgs &a) {
    return ex_layout(nullptr, a.plugin_set, shard_extent(a), a.n_pods, a.n_shards).bytes;
}

ExplainExchange explain_exchange(const ExplainArgs &a) {
    const ExScratch x = ex_layout(a.scratch, a.plugin_set, shard_extent(a), a.n_pods, a.n_shards);
    return ExplainExchange{x.shard_all, sizeof(ExShard), x.best_all};
}

hipError_t launch_explain_shard(const ExplainArgs &a, ExplainShardStage stage, uint32_t p0, uint32_t nb, hipStream_t s) {
    if (a.n_pods == 0 || a.n_pods > MS_EXPLAIN_MAX_PODS || !a.scratch || a.n_shards == 0 || a.shard >= a.n_shards ||
        p0 + nb > a.n_pods)
        return hipErrorInvalidValue;
    switch (a.plugin_set) {
        case MS_PLUGINS_NU_NN: return launch_shard_set<MS_PLUGINS_NU_NN>(a, stage, p0, nb, s);
        case MS_PLUGINS_NU_NRF_NN_LA: return launch_shard_set<MS_PLUGINS_NU_NRF_NN_LA>(a, stage, p0, nb, s);
        case MS_PLUGINS_NU_NN_NA: return launch_shard_set<MS_PLUGINS_NU_NN_NA>(a, stage, p0, nb, s);
        case MS_PLUGINS_NU_TT_NN: return launch_shard_set<MS_PLUGINS_NU_TT_NN>(a, stage, p0, nb, s);
        case MS_PLUGINS_NU_NN_NAM: return launch_shard_set<MS_PLUGINS_NU_NN_NAM>(a, stage, p0, nb, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_explain(const ExplainArgs &a, hipStream_t s) {
    if (a.n_pods == 0) return hipSuccess;
    if (a.n_pods > MS_EXPLAIN_MAX_PODS || !a.scratch || (!a.rows && !a.summaries)) return hipErrorInvalidValue;
    switch (a.plugin_set) {
        case MS_PLUGINS_NU_NN: return launch_set<MS_PLUGINS_NU_NN>(a, s);
        case MS_PLUGINS_NU_NRF_NN_LA: return launch_set<MS_PLUGINS_NU_NRF_NN_LA>(a, s);
        case MS_PLUGINS_NU_NN_NA: return launch_set<MS_PLUGINS_NU_NN_NA>(a, s);
        case MS_PLUGINS_NU_TT_NN: return launch_set<MS_PLUGINS_NU_TT_NN>(a, s);
        case MS_PLUGINS_NU_NN_NAM: return launch_set<MS_PLUGINS_NU_NN_NAM>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace msgpu

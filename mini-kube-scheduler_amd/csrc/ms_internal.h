// ms_internal.h — shared between the HIP kernels and the C-ABI host library.
// Not part of the public boundary (that is include/minisched_gpu.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minisched_gpu.h"

namespace msgpu {

// Node flag byte (device column `flags`).
constexpr uint8_t kNodeUnschedulable = 0x01;  // node.Spec.Unschedulable
constexpr uint8_t kNodeAbsent = 0x80;         // tombstone / never added: not in Nodes().List

// NodeAffinity sweep geometry: one node per lane-slot, 16 slots per lane.
constexpr int kNunnThreads = 256;
constexpr int kNunnSlots = 16;
constexpr int kNunnTile = kNunnThreads * kNunnSlots;  // nodes per block

// K3 (resource-aware sweep) geometry.
constexpr int kFullThreads = 256;
constexpr int kFullSlots = 4;
constexpr int kFullWaveTile = 64 * kFullSlots;            // nodes per wave  (validator tile; the most rows a tile holds)
constexpr int kFullTile = kFullThreads * kFullSlots;      // nodes per block

constexpr uint32_t kGolden32 = 0x9E3779B1u;  // LDS map hashing in the validator

// Bytes of padding after the flags/digit/zone columns (vector loads of a
// lane's rows may run past the last row).
constexpr uint32_t kColumnPad = 64;

// Device-resident node table, structure of arrays, indexed by LOCAL ordinal.
struct NodeTable {
    uint8_t *flags;
    uint8_t *digit;
    uint8_t *zone;  // zone label value id (MS_PLUGINS_NU_NN_NA), 0 = none
    uint8_t *label2;  // second label value id (MS_PLUGINS_NU_NN_NAM term key 1), 0 = none
    uint32_t *taints;  // taint ids (MS_PLUGINS_NU_TT_NN): bits 0-7 NoSchedule/NoExecute, 8-15 PreferNoSchedule
    int32_t *allowed_pods;
    int32_t *pod_count;
    int64_t *alloc_cpu, *alloc_mem;
    int64_t *req_cpu, *req_mem;
    int64_t *nz_cpu, *nz_mem;
    uint32_t cap;   // rows allocated
    uint32_t base;  // global ordinal of row 0
    // K1 "pp" bit planes, derived from flags/digit (k_build_planes after every
    // delta batch): planes[p * gcap + g], p = kPlane*, one u32 per group g of
    // kGroupRows consecutive rows (bit s = row g*kGroupRows + s).
    uint32_t *planes;
    uint32_t gcap;  // groups allocated = cdiv(cap, kGroupRows)
    // Rows per tile of the config-E sweep (the engine's table copy; 0 = kFullWaveTile).
    // run_sequential sizes tiles so that every CU beside the validator's gets one
    // (a multiple of 16, 64..256): 208 rows at 50k nodes = 241 tiles, not 196 x 256.
    // (In the 4 bytes of padding before drow: the structure's size is unchanged.)
    uint32_t tile_rows;
    // Derived rows of the config-E sweep's binary64 form (DRow), set only in the
    // table copy the sequential engine passes to its launches: rebuilt at the
    // start of each run (k_build_drows) and kept current by the validator's
    // write-back of the rows it binds. nullptr everywhere else.
    struct DRow *drow;
};

__host__ __device__ inline uint32_t tile_rows_of(const NodeTable &t) {
    return t.tile_rows ? t.tile_rows : (uint32_t)kFullWaveTile;
}

// One node as the config-E sweep's binary64 LeastAllocated form reads it
// (ms_rows.h make_drow; 64 B, one row per lane and load).
struct DRow {
    int64_t fr_cpu, fr_mem;  // Allocatable - Requested (NodeResourcesFit)
    double r_cpu, r_mem;     // RN(100 / Allocatable), 0 when Allocatable <= 0
    double a_cpu, a_mem;     // RN(RN((Allocatable - NonZeroRequested) * r) + 2^-43)
    int32_t room;            // AllowedPodNumber - len(Pods)
    uint32_t fd;             // flags | digit << 8
    uint32_t digit;          // name digit (0xFF: none)
    uint32_t rbits;          // kRb* below: the row's static filter outcomes, precomputed
};
static_assert(sizeof(DRow) == 64, "DRow layout");
// DRow::rbits. kRbUnsched and kRbNoRoom are set for present rows only.
constexpr uint32_t kRbAbsent = 1u;   // not in Nodes().List
constexpr uint32_t kRbUnsched = 2u;  // Spec.Unschedulable (NodeUnschedulable rejects unless tolerated)
constexpr uint32_t kRbNoRoom = 4u;   // AllowedPodNumber - len(Pods) < 1 (NodeResourcesFit rejects every pod)
constexpr uint32_t kRbSlow = 8u;     // the binary64 LeastAllocated form is not exact for this row
constexpr uint32_t kRbBlocked = 16u; // absent or unschedulable: no pod that does not tolerate it may bind here

constexpr uint32_t kGroupRows = 30;
enum : uint32_t {
    kPlaneD0 = 0,   // name digit bit 0 (15 = no digit)
    kPlaneD1,
    kPlaneD2,
    kPlaneD3,
    kPlaneSched,    // present && !Spec.Unschedulable
    kPlanePresent,  // present (not tombstoned)
    kPlaneOver,     // bit 0: the group holds more than 3 present rows of one digit (K1 pp's scan path);
                    // bit 1: some present row's digit is not its ordinal mod 10 (no fixed-slot path)
    kPlaneDigitPres,   // present && the name ends in a digit
    kPlaneDigitSched,  // present && !Spec.Unschedulable && the name ends in a digit
    kPlanes
};

// K1 "pp" candidate lists, derived from the planes (k_build_cand after every
// k_build_planes): two lists per name digit d of the hash bases (base + row) *
// kG24 of the present rows whose name ends in d, in row order: S_d (list d) the
// schedulable ones, U_d (list 10 + d) the unschedulable (cordoned) ones. A pod
// of digit d that does not tolerate node.kubernetes.io/unschedulable can win
// exactly the rows of S_d, one that tolerates it those of S_d and U_d. The two
// lists of a digit lie next to each other, S_d's tiles then U_d's, so a sweep
// loads them as one run of tiles and stops short of U_d for the pods that do
// not tolerate. One u32 buffer (the context's d_cand):
//   [d], d <= 10     first entry of S_d; [d + 1] - [d] is the padded length of
//                    S_d and U_d together (0: no present row ends in d)
//   [11 + d]         tiles of S_d (0: S_d is empty); U_d's follow them
//   [21 + c]         real length of list c (c = d: S_d, c = 10 + d: U_d)
//   [kCandHeader ..] the entries; every list padded to a multiple of kCandTile
//                    with copies of its own first entry (a duplicate candidate
//                    leaves every pod's maximum unchanged)
// A row is in at most one list and a list's padding is less than a tile, so
// cand_words(cap) words hold any table.
constexpr uint32_t kCandClasses = 20;
constexpr uint32_t kCandDigits = kCandClasses / 2u;
constexpr uint32_t kCandTile = 192;   // entries per tile: 3 per lane of a wave
constexpr uint32_t kCandHeader = 64;  // words before the entries
__host__ __device__ inline size_t cand_words(uint32_t cap) {
    return (size_t)kCandHeader + (size_t)cap + kCandClasses * kCandTile;
}

// One queued node delta (upsert or delete) as it travels to the device.
struct NodeDelta {
    uint32_t local;   // local row
    uint32_t absent;  // 1 = delete (tombstone)
    ms_node_rec rec;
};
static_assert(sizeof(ms_node_rec) == 64, "ms_node_rec layout");
static_assert(sizeof(ms_pod_rec) == 40, "ms_pod_rec layout");
static_assert(sizeof(ms_result) == 24, "ms_result layout");
static_assert(sizeof(ms_pod_compact) == 8, "ms_pod_compact layout");
static_assert(sizeof(ms_result_compact) == 8, "ms_result_compact layout");

// A shard's key for a pod with no feasible node on it: 1 when the shard lists at
// least one node, else 0 (real keys are >= 2: ordinals stop at MS_MAX_ORDINAL =
// 0xFFFFD, so the ordinal field 0xFFFFF - ordinal is >= 2). The element-wise MAX
// over shards then also tells the decode whether the cluster lists any node.
constexpr unsigned long long kKeyListed = 1ull;

__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
__host__ __device__ inline uint32_t seed32_of(uint64_t seed) { return (uint32_t)(seed ^ (seed >> 32)); }

// Tie-break hash (minisched_gpu.h, rule "r3"; oracle/ms_oracle.c msor_tb_hash):
//   A = fmix32(seed32 ^ pod_ordinal); h = mix32(A + node_ordinal * kG24)
// mix32(x): x ^= x>>16; x *= 0x85ebca6b; x ^= x>>16; x *= 0xc2b2ae35 (both
// xor-shifts by 16, one SDWA v_xor each). node_ordinal < 2^20, so the
// product is one v_mad_u32_u24. For a fixed pod h is a bijection of the
// ordinal (odd multipliers, xor-shifts by 16 are involutions), so no two nodes
// of one pod share a hash and tb_unhash recovers the ordinal from h alone: the
// sweep reduces bare 32-bit hashes and never carries the row along.
constexpr uint32_t kG24 = 0x9E3779u;  // odd, 24-bit
constexpr uint32_t kG24Inv = 0xF2B382C9u;  // kG24^-1 mod 2^32
__host__ __device__ inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 16;
    x *= 0xc2b2ae35u;
    return x;
}
__host__ __device__ inline uint32_t unmix32(uint32_t h) {
    h *= 0x7ED1B41Du;  // 0xc2b2ae35^-1
    h ^= h >> 16;
    h *= 0xA5CB9243u;  // 0x85ebca6b^-1
    h ^= h >> 16;
    return h;
}
__host__ __device__ inline uint32_t tb_pod(uint32_t seed32, uint32_t pod_ordinal) {
    return fmix32(seed32 ^ pod_ordinal);
}
__host__ __device__ inline uint32_t tb_hash(uint32_t A, uint32_t node_ordinal) {
    return mix32(A + node_ordinal * kG24);
}
// The node ordinal whose tb_hash under pod half A is h.
__host__ __device__ inline uint32_t tb_unhash(uint32_t A, uint32_t h) { return (unmix32(h) - A) * kG24Inv; }

// ---- MS_PLUGINS_NU_NN_NAM launchers (ms_affinity.hip) ----------------------
// A term set as the device reads it (built on the host from ms_nam_term_set(_ext)):
// z[v] / l[v] bit t = term t (weight > 0) holds zone / label2 value id v; wsum[m]
// = the weight sum of the terms in 4-bit mask m. raw = wsum[z[zone] & l[label2]].
// The high nibble is the id's required set (ms_nam_required_sets): bit 4 + k =
// required term k holds the value id; a node passes NodeAffinity's Filter when
// (z[zone] & l[label2]) >> 4 is non-zero. An id without a requirement has
// kNamNoReqBit on every value id of both keys, so the device needs no flag.
struct NamTab {
    uint8_t z[256];
    uint8_t l[256];
    uint16_t wsum[16];
};
constexpr uint32_t kNamNoReqBit = 0x10u;
// NamLayout (row segments and scratch shape), the carve offsets and a call's
// NamPlan: ms_nam_layout.h (host-only arithmetic). Every chunk of a call is
// launched with the call's plan layout L, never one of its own pod count.
struct NamLayout;
// Node shards, step 1: per pod this context's composed rescale record (out:
// MS_NAM_SEG_BYTES per pod), computed per class.
hipError_t launch_nam_segment(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                              const void *sets, uint32_t n_sets, const NamLayout &L, void *scratch, void *out,
                              hipStream_t s);
// n identity records (a shard without rows).
hipError_t launch_nam_identity(void *out, uint32_t n, hipStream_t s);
// Per pod the composition of n records in[s * stride + p] (s ascending); skip_to >= 0:
// only the records after skip_to, and m_in[p] = the OR of "any" of those before it.
hipError_t launch_nam_compose(const void *in, uint32_t stride, uint32_t n, uint32_t n_pods, int32_t skip_to,
                              void *out, uint8_t *m_in, hipStream_t s);
// Per pod the best packed key over this context's rows (keys[p] written; listed:
// the context lists a row, so a pod with none feasible gets kKeyListed); after /
// m_in: launch_nam_compose's outputs for these pods (node shards), or null.
// flags (optional): per pod this context's filter word for the decode (byte 0
// NodeUnschedulable, byte 2 NodeAffinity rejected a present row).
hipError_t launch_nam_keys(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                           const void *sets, uint32_t n_sets, uint32_t seed32, uint32_t w_nn, uint32_t w_na,
                           const void *after, const uint8_t *m_in, uint32_t listed, const NamLayout &L,
                           void *scratch, unsigned long long *keys, uint32_t *flags, hipStream_t s);
// Node shards: flags[p] = that word from the OR of the filter bits of the n
// gathered records in[s * stride + p].
hipError_t launch_nam_flags(const void *in, uint32_t stride, uint32_t n, uint32_t n_pods, uint32_t *flags,
                            hipStream_t s);
// The in-library node-sharded cycle (ms_comm.cpp), a batch as ONE chunk under a
// whole-batch plan (nam_plan_whole), exchanging one record per CLASS: class ids
// are dense in key order from the pods and n_sets alone, so class c is the same
// class on every shard of a batch.
// First pass: the class pass (classes, row segments), then this shard's composed
// record of every class into cls_out (L.cls_max records of MS_NAM_SEG_BYTES;
// those past the class count are identity records with no bits).
hipError_t launch_nam_class_segment(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                                    const void *sets, uint32_t n_sets, const NamLayout &L, void *scratch,
                                    void *cls_out, hipStream_t s);
// Second pass, RESUMING from the scratch the first pass of the same batch left
// (same pods, L and scratch; the class pass is not run again): cls_all holds the
// n_shards gathered class records [shard][L.cls_max]; after (L.cls_max records)
// and m_in (L.cls_max bytes) receive, per class, the later shards' composed table
// and "an earlier shard has a non-zero node"; then keys and flags as launch_nam_keys
// (flags: this shard's own rows' filter word per pod).
hipError_t launch_nam_class_keys(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                                 const void *sets, uint32_t n_sets, uint32_t seed32, uint32_t w_nn, uint32_t w_na,
                                 const void *cls_all, uint32_t n_shards, uint32_t shard_index, uint32_t listed,
                                 const NamLayout &L, void *scratch, void *after, uint8_t *m_in,
                                 unsigned long long *keys, uint32_t *flags, hipStream_t s);

// ---- launchers (ms_kernels.hip) -------------------------------------------
// All return hipError_t of the launch; none synchronises.
hipError_t launch_apply_deltas(const NodeTable &t, const NodeDelta *d_deltas, uint32_t n, hipStream_t s);
hipError_t launch_init_table(const NodeTable &t, hipStream_t s);
// K1 "pp" (ms_sweep_pp.hip): every (pod, node) pair through NU + NN + selectHost.
// results != nullptr: decoded ms_result per pod (single-shard cycle; keys is
// scratch, needed only above 122,880 rows), and with commit != 0 each winner's
// NodeInfo.AddPod in the same launch; else keys[i] = this shard's max packed
// key (0 = none), overwritten. present: global present-node count (decode).
// cand: the table's candidate lists (above), which class-sorted chunks of a
// one-workgroup-per-chunk launch sweep instead of the planes.
hipError_t launch_sweep_pp(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                           uint32_t seed32, unsigned long long *keys, ms_result *results, uint32_t present,
                           int num_cus, hipStream_t s, int commit = 0, hipEvent_t done = nullptr);
// Two shard sweeps (keys only, rows <= kPpMaxFusedRows) in ONE launch: the
// per-launch ramp and drain are paid once for both batches (ms_sharded_submit
// coalesces consecutive submits). done: recorded after both.
hipError_t launch_sweep_pp2(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_rec *pods1, uint32_t n1,
                            unsigned long long *keys1, const ms_pod_rec *pods2, uint32_t n2, unsigned long long *keys2,
                            uint32_t seed32, uint32_t present, int num_cus, hipStream_t s, hipEvent_t done);
// The compact host-array cycle (ms_schedule_batch_compact) in one launch, rows
// <= kPpMaxFusedRows: pods are ms_pod_compact records and results
// ms_result_compact, both in pinned host memory the kernel reads and writes
// over PCIe (no copy launches, no widen / narrow passes); binds committed.
hipError_t launch_sweep_pp_compact(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_compact *pods, uint32_t n_pods,
                                   uint32_t seed32, ms_result_compact *results, uint32_t present, int num_cus,
                                   hipStream_t s);
// (done, optional: recorded after the sweep, by its own dispatch when it is
// one launch: no separate event packet on s)
// Rows one K1 pp workgroup holds (16 waves x 64 lanes x 4 groups of 30):
// up to here the single-shard cycle is one launch with no key scratch.
constexpr uint32_t kPpMaxFusedRows = 16u * 64u * 4u * kGroupRows;
// Rebuilds the bit planes of the groups touched by deltas (or all groups when d_deltas
// is null), then every candidate list (cand: cand_words(t.cap) words) from the planes.
hipError_t launch_build_planes(const NodeTable &t, uint32_t *cand, const NodeDelta *d_deltas, uint32_t n,
                               hipStream_t s);
// keys[0, n) = v (the atomicMax targets of the NodeAffinity / resource sweeps
// start at kKeyListed when the shard lists a node, else 0)
hipError_t launch_fill_keys(unsigned long long *keys, uint32_t n, unsigned long long v, hipStream_t s);
// MS_PLUGINS_NU_NN_NA sweep (one pair per lane-slot): keys[i] = max packed key
// with raw NodeAffinity scores, fkeys[i] = max over this shard's feasible nodes
// with a non-zero raw NodeAffinity score of ((0xFFFFF - ordinal) << 1 | NN
// match) + 1, i.e. the normalise hook's anchor (the first such node in LIST
// order); both atomicMax targets, zeroed by the caller. w: score weights.
hipError_t launch_sweep_na(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                           uint32_t seed32, uint32_t w_nn, uint32_t w_na, unsigned long long *keys, uint32_t *fkeys,
                           int num_cus, hipStream_t s);
// decode of the NU+NN+NA set: the anchor's score becomes w_na * 100
hipError_t launch_decode_na(const ms_pod_rec *pods, uint32_t n_pods, const unsigned long long *keys,
                            const uint32_t *fkeys, uint32_t present_nodes, uint32_t seed32, uint32_t w_nn,
                            uint32_t w_na, ms_result *out, hipStream_t s, const uint32_t *present_dev = nullptr);
hipError_t launch_sweep_full(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                             uint32_t seed32, unsigned long long *keys, uint32_t *flags, int num_cus,
                             hipStream_t s);
// Derived rows [0, n_total) of the sequential engine's table copy (t.drow): rows
// at or past n_rows are absent.
hipError_t launch_build_drows(const NodeTable &t, uint32_t n_rows, uint32_t n_total, hipStream_t s);
// present_dev (optional): read the present count from the device (node-sharded combine)
hipError_t launch_decode(const ms_pod_rec *pods, uint32_t n_pods, const unsigned long long *keys,
                         const uint32_t *flags, uint32_t present_nodes, ms_result *out, hipStream_t s,
                         const uint32_t *present_dev = nullptr);

// ---- the exact sequential engine's launchers (ms_seq.hip) ------------------
// Largest speculative batch the sequential validator accepts.
uint32_t seq_batch_limit();
// i64 fields per validator node record; stale nodes per prev list.
uint32_t seq_rec_fields();
uint32_t seq_prev_cap();
// Entries per (pod, tile) speculative list: tile_keys has n_pods * n_tiles * seq_topk() u64.
uint32_t seq_topk();
// Rows the sequential engine's validator supports (tile lists held in registers).
uint32_t seq_max_rows();
// Per-(pod, wave tile) speculative sweep for the sequential engine: the
// tile's top-K keys at tile_keys[(p * n_tiles + t) * K + j], 0-terminated,
// and its filter flags at tile_flags[p * n_tiles + t].
// spec[p] accumulates (atomicMax) pod p's speculative global winner key and
// spec_flags[p] the filter flags of tiles without a feasible row; both must be
// zero on entry (the validator zeroes the entries it consumed).
hipError_t launch_sweep_full_tiles(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods,
                                   uint32_t n_pods, uint32_t seed32, unsigned long long *tile_keys,
                                   uint32_t *tile_flags, uint32_t n_tiles, hipStream_t s);
// Per pod: global speculative top-4 from the tile lists (top[p*4 + r]), the
// speculative winner (rank 0) and the filters of tiles with no feasible row;
// recs (optional, n_pods * 4 * seq_rec_fields() i64) gets the four entries'
// batch-start node records for the in-order validator; ext (optional, n_pods * 4)
// ranks 4..7 for its slow pods, with the certified rank count in spec_flags
// bits 28-31 (the validators pass it as top_ext).
hipError_t launch_topk_merge(const unsigned long long *tile_keys, const uint32_t *tile_flags, uint32_t n_pods,
                             uint32_t n_tiles, unsigned long long *top, unsigned long long *spec, uint32_t *spec_flags,
                             const NodeTable &t, int64_t *recs, hipStream_t s, unsigned long long *ext = nullptr);
// Batch k+1's merge inside step k at depth 1 (MINISCHED_SEQ_MERGE=instep):
// the step's sweep workgroups write batch k+1's tile lists through, each list
// stamped with the step's 2-bit tag (derived from `tag`), and their waves poll
// the lists until every one carries it, then merge the batch's pods into these
// buffers (launch_topk_merge's outputs), tagging each merged pod with `tag`.
// The lists must hold no tag of an earlier run (zeroed at the run's start).
// The wait is bounded: a worker that gives up leaves its pods untagged and
// validation k+1 merges them itself, so a grid that is not co-resident costs
// time, never correctness. top == nullptr: no in-step merge.
// in_tags / in_tag: batch k's tags (in_tag 0: batch k was merged by a launch).
// skip: the workers leave every pod to the fallback (a test hook).
struct SeqMergeIO {
    const uint32_t *in_tags = nullptr;
    uint32_t in_tag = 0;
    unsigned long long *top = nullptr, *spec = nullptr, *ext = nullptr;
    uint32_t *spec_flags = nullptr, *tags = nullptr;
    int64_t *recs = nullptr;
    uint32_t tag = 0;
    int skip = 0;
    // MS_VSTAMPS diagnostic build: per-workgroup timestamps of steps
    // tl_step < kTimelineSteps (u64 [step][workgroup][8], s_memrealtime)
    unsigned long long *tl = nullptr;
    uint32_t tl_step = ~0u;
};
constexpr uint32_t kTimelineSteps = 2048, kTimelineWgs = 256;  // (a config E run: 1627 steps)
// Whether launch_seq_step can merge n_next pods in-step (else launch_topk_merge follows).
bool seq_step_merges(const NodeTable &t, uint32_t n_tiles, uint32_t n_next);
// One single-stream step: in-order validation of batch k (n_pods, workgroup 0;
// writes results and commits binds to the table) while sweeping the next batch
// (n_next pods: tile lists, and with merge.top their in-step merge; else
// launch_topk_merge follows the step). Either count may be 0.
struct SeqStep {
    NodeTable t;
    uint32_t n_rows = 0, n_tiles = 0, seed32 = 0;
    int num_cus = 0;
    // batch k, validated: its pods, tile lists and launch_topk_merge's outputs
    // (top_ext: ranks 4..7, optional)
    const ms_pod_rec *pods = nullptr;
    uint32_t n_pods = 0;
    const unsigned long long *tile_keys = nullptr;
    const uint32_t *tile_flags = nullptr;
    const unsigned long long *spec = nullptr;
    const uint32_t *spec_flags = nullptr;
    const unsigned long long *top4 = nullptr;
    const int64_t *top4_recs = nullptr;
    const unsigned long long *top_ext = nullptr;
    // prev_in / prev_recs_in: the stale nodes (bound by the previous batch) with
    // their final records ({n_own, n_carried, rows} of 2 + seq_prev_cap() words;
    // seq_prev_cap() * seq_rec_fields() i64), written by the previous validation
    // into its prev_out / prev_recs_out. prev_in null: the sweep saw every earlier bind.
    const uint32_t *prev_in = nullptr;
    const int64_t *prev_recs_in = nullptr;
    uint32_t *prev_out = nullptr;
    int64_t *prev_recs_out = nullptr;
    ms_result *results = nullptr;
    // u32[6] = overflow flags, re-swept tiles, recomputed entries, pods,
    // speculation misses, pods whose speculative winner was touched
    uint32_t *stats = nullptr;
    // batch k+1, swept: its pods and the tile lists written
    const ms_pod_rec *next_pods = nullptr;
    uint32_t n_next = 0;
    unsigned long long *next_tile_keys = nullptr;
    uint32_t *next_tile_flags = nullptr;
    SeqMergeIO merge;
};
hipError_t launch_seq_step(const SeqStep &a, hipStream_t s);
// Node-sharded sequential mode (minisched_gpu.h ms_seq_*): this shard's top-4
// candidates with records + all-tile filter flags per pod, from the top-4 merge
// output; and the replicated validation over the shards' gathered lists
// (merged / merged_flags: n_pods * 4 / n_pods scratch).
hipError_t launch_seq_pack_cands(const NodeTable &t, const unsigned long long *top4, const uint32_t *tile_flags,
                                 uint32_t n_tiles, uint32_t n_pods, ms_seq_cand *cands, uint32_t *flags, hipStream_t s);
// live (optional): validate only the first min(n_pods, *live) pods (a cursor window)
hipError_t launch_seq_validate_rep(const NodeTable &t, uint32_t n_pods, const ms_pod_rec *pods, uint32_t seed32,
                                   uint32_t n_shards, const ms_seq_cand *cands_all, const uint32_t *flags_all,
                                   ms_seq_cand *merged, uint32_t *merged_flags, ms_result *results, uint32_t *n_done,
                                   hipStream_t s, const uint32_t *live = nullptr);
// Device cursor of the in-library node-sharded sequential cycle: ctl = {cursor,
// live, n_done}; window_in stages pods [cursor, cursor + live) of n into win (w
// entries), window_out copies ctl[2] decided results to res[cursor ..] and
// advances the cursor.
hipError_t launch_seq_window_in(const ms_pod_rec *pods, uint32_t n, uint32_t *ctl, ms_pod_rec *win, uint32_t w,
                                hipStream_t s);
hipError_t launch_seq_window_out(const ms_result *win_res, uint32_t *ctl, ms_result *res, uint32_t n, hipStream_t s);

// ---- MS_PLUGINS_NU_TT_NN launchers (ms_taint.hip) --------------------------
// MS_PLUGINS_NU_TT_NN (ms_taint.hip): per-pod summaries of LIST-ordered row
// segments (tt_segments(n_rows) of them, segment s at summaries[s * n_pods + p],
// MS_TT_SUMMARY_BYTES each), and their merge: n_segs summaries per pod (segment
// s at in[s * stride + p]) into out[p] (merged summary) or, with out null,
// results[p] (commit: NodeInfo.AddPod on winners this table owns).
uint32_t tt_segments(uint32_t n_rows, uint32_t *seg_rows = nullptr);
hipError_t launch_tt_sweep(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                           uint32_t seed32, void *summaries, hipStream_t s);
// The two-pass bit-sliced TaintToleration cycle of one context (ms_taint.hip
// k_tt2_*): row planes once per cycle (launch_tt2_planes), then per chunk of up
// to max_pods pods census -> plan -> pick -> final into results (commit: binds).
uint32_t tt2_words(uint32_t n_rows);
size_t tt2_scratch_bytes(uint32_t n_rows, uint32_t max_pods);
hipError_t launch_tt2_planes(const NodeTable &t, uint32_t n_rows, void *scratch, hipStream_t s);
hipError_t launch_tt2_cycle(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                            uint32_t seed32, void *scratch, uint32_t max_pods, ms_result *results, int commit,
                            hipStream_t s);
// Node shards of the two-pass cycle: a shard's census (one MS_TT_CENSUS_BYTES
// record per pod, its segments merged, ordinals global); its pick under the plan
// of every shard's census (census_all[s * stride + p], shards in LIST order) ->
// one key per pod for the cross-shard uint64 MAX; the results from the census of
// every shard and the MAX of the keys.
hipError_t launch_tt2_census_shard(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                                   uint32_t seed32, void *scratch, uint32_t max_pods, void *census_out,
                                   hipStream_t s);
hipError_t launch_tt2_pick_shard(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                                 uint32_t seed32, void *scratch, uint32_t max_pods, const void *census_all,
                                 uint32_t stride, uint32_t n_shards, uint32_t shard, unsigned long long *keys_out,
                                 hipStream_t s);
// The plan records inside a two-pass scratch (tt2_scratch_bytes) for max_pods pods.
void *tt2_plans(void *scratch, uint32_t n_rows, uint32_t max_pods);
hipError_t launch_tt2_final_shard(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                                  uint32_t seed32, void *plans_buf, uint32_t max_pods, const void *census_all,
                                  uint32_t stride, uint32_t n_shards, const unsigned long long *keys_max,
                                  ms_result *results, hipStream_t s);
hipError_t launch_tt_combine(const void *in, uint32_t stride, uint32_t n_segs, const ms_pod_rec *pods, uint32_t n_pods,
                             uint32_t seed32, void *out, ms_result *results, const NodeTable &t, int commit,
                             hipStream_t s);

// ---- explain (ms_explain.hip): per-node verdicts and scores ---------------
// Rows per tile of the explain kernels (one row per thread of a workgroup).
constexpr uint32_t kExplainTile = 256;
struct ExplainArgs {
    NodeTable t;
    uint32_t n_rows = 0;   // sweep extent of the table (rows past it are absent)
    int32_t plugin_set = 0;
    const ms_pod_rec *pods = nullptr;
    uint32_t n_pods = 0;
    uint32_t seed32 = 0, w_nn = 1, w_na = 1;
    const void *sets = nullptr;  // MS_PLUGINS_NU_NN_NAM: the NamTab of every registered id
    uint32_t n_sets = 0;
    uint32_t win_lo = 0, win_n = 0;  // the window in local rows (rows != nullptr)
    ms_explain_row *rows = nullptr;  // n_pods x win_n, or null
    bool summaries = false;          // whole-table summaries (with best_key) into explain_summaries(scratch)
    void *scratch = nullptr;         // explain_scratch_bytes
    // node shards (launch_explain_shard only): the communicator's world and this
    // context's rank; n_pods is then the whole call's, rows a chunk's staging
    uint32_t n_shards = 0, shard = 0;
};
// Local rows the call's tiles cover and the scratch they need.
uint32_t explain_extent(uint32_t n_rows, uint32_t win_lo, uint32_t win_n, bool rows);
size_t explain_scratch_bytes(int32_t plugin_set, uint32_t extent, uint32_t n_pods);
// Where the n_pods summaries of a call lie inside its scratch.
ms_explain_summary *explain_summaries(void *scratch);
// Tile summaries, the per-pod scan over the tiles, then the rows (and the best keys).
hipError_t launch_explain(const ExplainArgs &a, hipStream_t s);
// Explain on node shards (ms_explain_sharded_device): a shard is one
// more tile. The stages of one call, in this order on one stream, between them
// the two all-gathers of explain_exchange's buffers (in place: this rank's block
// is block `shard`); none waits on a value another rank wrote.
enum ExplainShardStage {
    kExShardRecords,  // the tiles' records of all n_pods pods, then this shard's record per pod
    kExShardScan,     // after the records' all-gather: the scan started from the G shards' records
    kExShardRows,     // pods [p0, p0 + nb): every tile's best key, the window's rows into a.rows (nb x win_n)
    kExShardBest,     // this shard's best key per pod, from every chunk's tiles
    kExShardMax,      // after the keys' all-gather: the summaries' best_key = the maximum over the shards
};
// The window counts whether or not rows are asked for (win_n = 0: no rows).
size_t explain_shard_scratch_bytes(const ExplainArgs &a);
struct ExplainExchange {
    void *records;        // n_shards x n_pods opaque records of record_bytes, shard-major
    size_t record_bytes;
    unsigned long long *best;  // n_shards x n_pods keys, shard-major
};
ExplainExchange explain_exchange(const ExplainArgs &a);
hipError_t launch_explain_shard(const ExplainArgs &a, ExplainShardStage stage, uint32_t p0, uint32_t nb,
                                hipStream_t s);

// ---- node-shard exchange (ms_comm.cpp) -------------------------------------
// One all-gather over the context's communicator on s: `bytes` bytes from send
// into block `rank` of every rank's recv (send may be that block of recv). The
// callers outside ms_comm.cpp name no RCCL entry point. MS_OK or MS_E_RCCL.
int comm_all_gather(ms_ctx *c, const void *send, void *recv, size_t bytes, hipStream_t s);

// ---- launchers (ms_kernels.hip), continued: decodes, binds, read-back ------
// One launch decoding several batches' pod slices, each with a device-side present flag.
constexpr uint32_t kMaxSliceJobs = 8;
struct SliceJob {
    const ms_pod_rec *pods;
    const unsigned long long *keys;
    const uint32_t *flags;    // NodeResourcesFit set: combined filter bytes; else nullptr
    const uint32_t *present;  // device present count, or nullptr: from the key (kKeyListed)
    ms_result *results;
    uint32_t n_pods, _pad;
};
hipError_t launch_decode_slices(const SliceJob *jobs, uint32_t n_jobs, hipStream_t s);
// n_jobs in [1, MS_DECODE_MAX_JOBS] (checked by the caller)
hipError_t launch_decode_jobs(const ms_decode_job *jobs, uint32_t n_jobs, uint32_t present_nodes, hipStream_t s);
hipError_t launch_apply_binds(const NodeTable &t, const ms_pod_rec *pods, uint32_t n_pods,
                              const ms_result *res, hipStream_t s);
hipError_t launch_bind_one(const NodeTable &t, uint32_t local, const ms_pod_rec *pod_dev, int sign,
                           hipStream_t s);
hipError_t launch_read_rows(const NodeTable &t, uint32_t first, uint32_t n, ms_node_rec *out, hipStream_t s);
// Compact records (ms_schedule_batch_compact): pods widened to ms_pod_rec (zero
// requests), results narrowed to ms_result_compact, on the device.
hipError_t launch_pods_widen(const ms_pod_compact *in, uint32_t n, ms_pod_rec *out, hipStream_t s);
hipError_t launch_results_narrow(const ms_result *in, uint32_t n, ms_result_compact *out, hipStream_t s);

}  // namespace msgpu

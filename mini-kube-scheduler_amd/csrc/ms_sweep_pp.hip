// ms_sweep_pp.hip — K1 "pp", the production NU+NN sweep: for every (pod, node)
// pair it evaluates NodeUnschedulable and NodeNumber, and selectHost's argmax
// with the deterministic tie-break.
//
// Reference path (/root/reference/minisched/minisched.go):
//   RunFilterPlugins :115-151 -> NodeUnschedulable.Filter (k8s@v1.22.0, restated)
//   RunScorePlugins  :164-199 -> NodeNumber.Score (plugins/score/nodenumber/nodenumber.go:73-95)
//   unweighted sum   :187-196
//   selectHost       :304-325 (rand.Intn tie-break -> rule r3, minisched_gpu.h)
//
// Bit-sliced evaluation. The node table keeps, per group of 30 consecutive
// rows, bit planes (ms_internal.h kPlane*): the four bits of each row's
// name digit (15 = no digit), "present and schedulable" and "present" (and
// both restricted to digit names, plus a per-group flag word). A lane
// holds up to kPpWords groups in registers. For one pod and one group:
//   F = tolerates ? present : schedulable                     (NodeUnschedulable, 30 rows)
//   m = F & XNOR(d0, pod bit 0) & .. & XNOR(d3, pod bit 3)    (NodeNumber's 10, 30 rows)
// five v_bitop3 in all, each computing one boolean term for each of the 30
// (pod, row) pairs of the group: every pair's filter and score comes from its
// own row's bits and the pod's own bits. The rows set in m are the pairs that
// pass the filter with score 10; their tie-break hashes (mix32 of A + ordinal *
// kG24, rule r3) are the candidates of selectHost's max. A group of 30
// consecutive names holds at most 3 rows of one digit when the digits cycle, so
// three v_ffbl slots cover it with no lane-divergent loop; a tile where some
// lane has more (the wave-uniform `gen` flag, computed when the tile is
// loaded) takes a bit-scan loop instead. Rows scoring 0 matter only when no
// feasible row of the wave scores 10: the wave's maximum is then 0 and the pod
// is redone by the exact slow path (every feasible row hashed, explicit
// found flags), which also covers non-digit pods.
// Fixed-slot form (word_fix): where every present digit-named row of a
// wave's groups has digit == ordinal mod 10 (the digit-aligned allocator's
// layout, and the synthetic clusters'), the pod's digit can only sit at three
// known slots, so the per-pod mask is one v_bitop3 and the slots need no
// search: 24 VALU per pod and group instead of 31, same keys bit for bit.
// Class runs (run_setup): the mask and the candidate rows depend only on the
// pod's class (fixed slot, tolerates), so a workgroup sorts its pods by class
// and a wave finds a class's candidates once per run; a pod of the run then
// costs one add and one mix32 per candidate, 17 VALU per pod and group.
// Candidate lists (sweep_lists): the candidate rows of a class depend only on
// the node table, so k_build_cand lists them once per flush, beside the planes
// (ms_internal.h kCand*): per name digit d the present schedulable rows (S_d)
// and, right after them, the present cordoned rows (U_d). A pod of digit d that
// does not tolerate node.kubernetes.io/unschedulable can win exactly the rows
// of S_d, one that tolerates it those of S_d and U_d, so a row is listed once.
// Where one workgroup holds every row (grid.y == 1) a sorted chunk's pods lie
// digit by digit, the tolerating ones last, and a wave loads its tiles of a
// digit (192 entries to a wave and tile) in one round, whatever the rows'
// layout, sweeps the pods that do not tolerate through its S tiles and the
// others through all of them; the planes then serve only pods without a digit
// and pods with no candidate. What a wave needs to know of the chunk's 21
// classes it gathers once, a class to a lane (class_lanes), so that moving on
// to the next digit waits for nothing but the tiles.
//
// Grid: a workgroup holds ALL of the context's rows (up to 16 waves x 64 lanes
// x kPpWords groups = 122,880 rows; more rows split over grid.y and combine
// with atomicMax) and sweeps a chunk of pods through them, 8 pods at a time.
// From the planes, the 8 lane maxima are reduced by one transposed butterfly
// (reduce8) and the waves combine in LDS (ds_max_u64 of level<<32 | hash): a
// wave needs its own maximum there, to redo a pod whose maximum is 0. The list
// form needs no such thing, so where LDS allows (lane_table_fits) it combines
// the other way round: every wave puts its lane maxima into the pod's row of a
// lane table, lane by lane (ds_max_u32, no cross-lane instruction in the
// sweep), and after the sweep's barrier the workgroup reduces each row once
// into the pod's slot; where the table does not fit, the list form reduces per
// wave like the planes. After one more barrier the workgroup unhashes each
// pod's winner (tb_unhash) and writes either the packed key (ms_sweep_device:
// one plain store per pod, no zeroing, no atomics) or the decoded ms_result
// directly (the fused single-shard cycle).
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#ifdef MS_PP_TIMELINE
#include <cstdio>
#include <vector>
#endif

#include "ms_device.h"

namespace msgpu {

namespace {

// Diagnostic build (`make pp-timeline`, -DMS_PP_TIMELINE): a wave timeline of
// k_sweep_nunn_pp. Lane 0 of every wave writes s_memtime at the points below
// into tl[workgroup][wave][stamp] (plain vector stores; a kernel argument that
// exists in this build only), and one pair of s_memrealtime (100 MHz) for the
// clock. sweep_pp_impl allocates the buffer, and appends it after a synchronise
// to the file named by MS_PP_TIMELINE (read out by tools/pp_wg_timeline.py).
// Without the macro every MS_TL* below expands to nothing.
#ifdef MS_PP_TIMELINE
constexpr uint32_t kTlStamps = 48;  // u64 per wave
enum : uint32_t {
    kTlEntry = 0,      // kernel entry
    kTlBar1 = 1,       // after the sort's barriers 1 .. 3 (0: an unsorted chunk has none)
    kTlBar2 = 2,
    kTlBar3 = 3,
    kTlPlanes = 4,     // the plane loads landed (0: the workgroup loads none)
    kTlBar4 = 5,       // after the barrier in front of the sweep
    kTlSweepEnd = 6,   // the wave's sweep done
    kTlSweepBar = 7,   // after the sweep's barrier
    kTlFinal = 8,      // after the lane table's final pass and its barrier
    kTlEnd = 9,        // the wave's end
    kTlReal0 = 10,     // s_memrealtime at entry and at the end
    kTlReal1 = 11,
    kTlDigit0 = 12,    // per sort slot s / 2, three each: its (last pass's) tile loads issued,
                       // the tiles landed (first hash can issue), the digit done
    kTlHashes = 42,    // candidate hashes per lane of the wave: sum of pods x tiles x 3
};
#define MS_TL_KPARAM , u64 *__restrict__ tl
#define MS_TL_PARAM , u64 *tlw
#define MS_TL_PASS , tlw
#define MS_TL_NONE , (u64 *)nullptr
#define MS_TL_BUF , tl_dev
#define MS_TL_INIT                                                                                      \
    u64 *tlw = tl ? tl + ((size_t)blockIdx.x * kPpMaxWaves + wv) * kTlStamps : nullptr;                   \
    MS_TL(kTlEntry);                                                                                    \
    MS_TL_PUT(kTlReal0, __builtin_amdgcn_s_memrealtime())
#define MS_TL_PUT(i, v)                  \
    do {                                 \
        const u64 tl_v_ = (v);           \
        if (tlw && lane == 0u) tlw[i] = tl_v_; \
    } while (0)
#define MS_TL(i) MS_TL_PUT(i, __builtin_amdgcn_s_memtime())
#define MS_TL_LANDED __builtin_amdgcn_s_waitcnt(0x0F70)  // s_waitcnt vmcnt(0)
#define MS_TL_COUNT_DECL u64 tl_hashes = 0
#define MS_TL_COUNT(n) tl_hashes += (n)
#define MS_TL_COUNT_PUT MS_TL_PUT(kTlHashes, tl_hashes)
#else
#define MS_TL_KPARAM
#define MS_TL_PARAM
#define MS_TL_PASS
#define MS_TL_NONE
#define MS_TL_BUF
#define MS_TL_INIT
#define MS_TL_PUT(i, v)
#define MS_TL(i)
#define MS_TL_LANDED
#define MS_TL_COUNT_DECL
#define MS_TL_COUNT(n)
#define MS_TL_COUNT_PUT
#endif

template <typename F>
constexpr uint32_t truth3(F f) {  // v_bitop3 table, S0 the most significant index bit
    uint32_t t = 0;
    for (int i = 0; i < 8; ++i)
        if (f((i >> 2) & 1, (i >> 1) & 1, i & 1)) t |= 1u << i;
    return t;
}
constexpr uint32_t kXnorAnd = truth3([](int a, int b, int c) { return c && a == b; });  // c & ~(a ^ b)
constexpr uint32_t kSelect = truth3([](int a, int b, int c) { return c ? a : b; });     // c ? a : b

constexpr uint32_t kTailShare = 4;  // waves sharing the packed last word (tail_pods)

constexpr int kPpWords = 4;      // 30-row groups per lane (KW, shards above kPpSmallGroups)
constexpr int kPpWordsSmall = 8; // KW for small shards: one wave holds every row
constexpr int kPpMaxWaves = 16;  // 1024-thread workgroups
constexpr uint32_t kPpSmallGroups = 64u * kPpWordsSmall;  // 15,360 rows

struct Word {
    uint32_t d0, d1, d2, d3;  // digit bit planes
    uint32_t sched, pres;     // present & schedulable, present
    uint32_t dsched, dpres;   // the same restricted to rows whose name ends in a digit
    uint32_t hb;              // (ordinal of the group's row 0) * kG24
};

// One pod as the wave sees it (all wave-uniform, SGPRs).
struct Pod {
    uint32_t A;               // tb_pod(seed32, ordinal)
    uint32_t s0, s1, s2, s3;  // digit bit i as 0 / ~0 (non-digit pods: 14, which no node has)
    uint32_t tol;             // tolerates node.kubernetes.io/unschedulable: 0 / ~0
    // fixed-slot form (groups whose rows' digits equal their ordinals mod 10):
    // the three slots of the pod's digit, p0 = (digit - node_base) mod 10, p0 + 10,
    // p0 + 20 (non-digit pods: 30, a bit no group sets), and A + p_j * kG24
    uint32_t p0, p1, p2;
    uint32_t A0, A1, A2;
};

#define MS_BITOP3(a, b, c, imm) __builtin_amdgcn_bitop3_b32((a), (b), (c), (imm))

__device__ __forceinline__ uint32_t feasible(const Word &w, const Pod &q) {
    return MS_BITOP3(w.pres, w.sched, q.tol, kSelect);
}

// Rows of the group that pass NodeUnschedulable and score NodeNumber's 10.
__device__ __forceinline__ uint32_t match10(const Word &w, const Pod &q) {
    uint32_t m = MS_BITOP3(w.d0, q.s0, feasible(w, q), kXnorAnd);
    m = MS_BITOP3(w.d1, q.s1, m, kXnorAnd);
    m = MS_BITOP3(w.d2, q.s2, m, kXnorAnd);
    return MS_BITOP3(w.d3, q.s3, m, kXnorAnd);
}

// Leading zeros (v_ffbh_u32; 0xFFFFFFFF for an empty mask).
__device__ __forceinline__ uint32_t last_lz(uint32_t m) {
    uint32_t s;
    asm("v_ffbh_u32 %0, %1" : "=v"(s) : "v"(m));
    return s;
}

__device__ __forceinline__ uint32_t hash_slot(uint32_t slot, uint32_t hbA) {
    return mix32(__umul24(slot, kG24) + hbA);  // A + (row0 + slot) * kG24, rule r3
}

// Lane maximum hash over the group's score-10 rows, at most 3 of them (the
// tile's `gen` flag is clear): the lowest (v_ffbl), the highest (v_ffbh) and
// the lowest of the rest, which falls back to the lowest when fewer than 3
// (a duplicate leaves the max unchanged); an empty mask gives 0.
__device__ __forceinline__ uint32_t word_fast(const Word &w, const Pod &q) {
    const uint32_t m = match10(w, q);
    const uint32_t hbA = w.hb + q.A;
    const int i0 = (int)first_slot(m);
    const int i2 = 31 - (int)last_lz(m);
    const int i1 = max((int)first_slot(m & (m - 1u)), i0);
    const uint32_t h = max(max(hash_slot((uint32_t)i0, hbA), hash_slot((uint32_t)i1, hbA)),
                           hash_slot((uint32_t)i2, hbA));
    return m ? h : 0u;
}

// Any number of score-10 rows per lane: a bit-scan loop (lane-divergent trip count).
__device__ __forceinline__ uint32_t word_scan(uint32_t m, uint32_t hbA) {
    uint32_t h = 0;
    while (m) {
        const uint32_t s = first_slot(m);
        m &= m - 1u;
        h = max(h, hash_slot(s, hbA));
    }
    return h;
}

// info: the pod entry's class bits (pod_entry), the fixed slot p0 in bits 16-20.
__device__ __forceinline__ Pod pod_bits(uint32_t A, uint32_t info) {
    Pod q;
    q.A = A;
    q.s0 = (info & 1u) ? ~0u : 0u;
    q.s1 = (info & 2u) ? ~0u : 0u;
    q.s2 = (info & 4u) ? ~0u : 0u;
    q.s3 = (info & 8u) ? ~0u : 0u;
    q.tol = (info & 16u) ? ~0u : 0u;
    q.p0 = (info >> 16) & 31u;  // (30 for a non-digit pod: p1 = p2 = 30 too)
    const uint32_t step = q.p0 < 10u ? 10u : 0u;
    q.p1 = q.p0 + step;
    q.p2 = q.p1 + step;
    q.A0 = A + q.p0 * kG24;
    q.A1 = q.A0 + 10u * kG24;
    q.A2 = q.A0 + 20u * kG24;
    return q;
}

// Fixed-slot form: in a group where every present row's name digit is its
// ordinal mod 10 (the digit-aligned allocator's layout, ms_nodes_upsert docs),
// the rows of the pod's digit can only sit at slots p0, p0 + 10, p0 + 20, and
// such a row scores NodeNumber's 10 exactly when its name ends in a digit. So
// the filter-and-score mask of the group is ONE v_bitop3 over the digit-name
// planes (NodeUnschedulable with the toleration, as feasible()), and the
// three candidates need no slot search: each hash input is hb + A_j, zeroed by
// its slot's bit (v_bfe_i32 gives 0 / ~0; mix32(0) = 0, the empty value).
__device__ __forceinline__ uint32_t match_fix(const Word &w, const Pod &q) {
    return MS_BITOP3(w.dpres, w.dsched, q.tol, kSelect);
}

__device__ __forceinline__ uint32_t word_fix(const Word &w, const Pod &q) {
    const uint32_t m = match_fix(w, q);
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_sbfe((int)m, (int)q.p0, 1);
    const uint32_t k1 = (uint32_t)__builtin_amdgcn_sbfe((int)m, (int)q.p1, 1);
    const uint32_t k2 = (uint32_t)__builtin_amdgcn_sbfe((int)m, (int)q.p2, 1);
    uint32_t x0 = (w.hb + q.A0) & k0, x1 = (w.hb + q.A1) & k1, x2 = (w.hb + q.A2) & k2;
    // (opaque: left visible, the compiler folds the AND into a v_bitop3 with the
    // first xor-shift and pays a separate shift for it, one VALU more per slot)
    asm("" : "+v"(x0), "+v"(x1), "+v"(x2));
    return max(max(mix32(x0), mix32(x1)), mix32(x2));
}

// Exact evaluation of one pod over the wave's NW groups, with explicit found
// flags: level 11 (score 10 + 1) over the score-10 rows, else level 1 over
// every feasible row (all score 0). Returns level<<32 | max hash (wave-uniform),
// 0 when no row of the wave is feasible.
// tail: the wave's packed last word (below) is evaluated here like a full one:
// its groups repeat in every lane segment, and repeats leave the max unchanged.
// FIX: the wave's words are digit-aligned (word_fix): the score-10 rows are
// the fixed slots' digit-name rows.
template <int KW, int NW, bool FIX>
__device__ __forceinline__ u64 pod_slow(const Word (&W)[KW], const Word &Wt, bool tail, const Pod &q) {
    uint32_t h = 0;
    bool found = false;
    const uint32_t cmask = (1u << q.p0) | (1u << q.p1) | (1u << q.p2);  // (non-digit pods: bit 30, never set)
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t m = FIX ? match_fix(W[k], q) & cmask : match10(W[k], q);
        found = found || m != 0;
        h = max(h, word_scan(m, W[k].hb + q.A));
    }
    if (tail) {
        const uint32_t m = match10(Wt, q);
        found = found || m != 0;
        h = max(h, word_scan(m, Wt.hb + q.A));
    }
    if (__ballot(found) != 0) return (11ull << 32) | wave_max_u32_dpp(h);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t m = feasible(W[k], q);
        found = found || m != 0;
        h = max(h, word_scan(m, W[k].hb + q.A));
    }
    if (tail) {
        const uint32_t m = feasible(Wt, q);
        found = found || m != 0;
        h = max(h, word_scan(m, Wt.hb + q.A));
    }
    if (__ballot(found) != 0) return (1ull << 32) | wave_max_u32_dpp(h);
    return 0;
}

// Pod p of a workgroup's chunk as the prologue leaves it in LDS: x = A =
// tb_pod(seed32, ordinal), y = class bits (digit, 14 for a non-digit name, |
// tolerates << 4) | name digit byte << 8 | the fixed slot p0 << 16 ((digit -
// node_base) mod 10, 30 for a non-digit name: word_fix). Bits 21-31 of y are
// free here: the prologue puts the pod's index in the chunk there.
// pstride: bytes per pod record (sizeof(ms_pod_rec), or 8 for ms_pod_compact,
// its first 8 bytes).
__device__ __forceinline__ uint2 pod_entry(const ms_pod_rec *__restrict__ pods, uint32_t p, uint32_t seed32,
                                           uint32_t pstride, uint32_t base10) {
    const uint2 pr = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(pods) + (size_t)p * pstride);
    const int dig = (int)(int8_t)(pr.y & 0xFFu);
    const bool isd = (uint32_t)dig <= 9u;
    const uint32_t info = (isd ? (uint32_t)dig : 14u) | (((pr.y >> 8) & 0xFFu) ? 16u : 0u);
    const uint32_t p0 = isd ? ((uint32_t)dig + 10u - base10) % 10u : 30u;
    return make_uint2(tb_pod(seed32, pr.x), info | ((pr.y & 0xFFu) << 8) | (p0 << 16));
}

// Class runs. A pod's class is (fixed slot p0, tolerates): 20 digit classes,
// key 2 * p0 + tolerates (slot-major: the pods of one slot, which is one name
// digit, are contiguous, those that do not tolerate first, as the list form
// sweeps them), and one "other" class (non-digit names). The match
// mask of a word and the three candidate rows depend on the class alone, so
// the prologue counting-sorts the chunk's entries by class and the sweep
// hoists that work out of the pod loop for runs of one class (run_setup).
// Sorted order: the whole 8-pod blocks of every digit class first, class by
// class (region A; class c holds positions rb[c] .. rb[c + 1]), then what is
// left of every class and the other class (region B, rb[20] .. rb[21] = np).
// A chunk swept in the list form has no rests: region A holds every digit
// class whole, at any length, and region B the other class alone.
// Bits 21-31 of an entry's y carry its index in the chunk (np <= kPpMaxChunk
// = 2048), which the epilogue writes by.
constexpr uint32_t kPpClasses = 20;
// LDS words after pinfo: counts, rb, region B cursors, the candidate lists' header (11 first
// entries and 10 tile counts) (24 each)
constexpr uint32_t kPpSortWords = 96;
// Chunks below this are swept in arrival order (no sort, one region B): their
// runs are too short for the run form (20 classes), and the small shards'
// 2-wave workgroups of 49-56 pods keep their prologue.
constexpr uint32_t kPpSortMin = 80;

__device__ __forceinline__ uint32_t pod_class(uint32_t info) {
    const uint32_t p0 = (info >> 16) & 31u;
    return p0 < 10u ? 2u * p0 + ((info >> 4) & 1u) : kPpClasses;
}

// Candidate bases of one class for a wave whose NW words hold at most 3 rows
// of a digit each (not kModeGen): B[3k .. 3k+2] = hb + slot * kG24 for the
// score-10 rows of word k (match10, which on digit-aligned words is match_fix
// at the class's slots), fewer than 3 filled by a duplicate as in word_fast.
// A word with no such row takes a base of another word of the lane, a lane with
// none the base of the wave's first lane that has one: duplicates of real
// candidates, which leave every pod's maximum unchanged. Then a pod of the class
// costs one add and one mix32 per slot and needs no mask. False (wave-uniform)
// when no row of the wave scores 10 for the class: its pods take the per-pod
// path, get u == 0 there and are redone by pod_slow.
template <int KW, int NW>
__device__ __forceinline__ bool run_setup(const Word (&W)[KW], uint32_t info, uint32_t (&B)[NW * 3]) {
    const Pod qc = pod_bits(0u, info);
    uint32_t m[NW], fb = 0;
    bool has = false;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        m[k] = match10(W[k], qc);
        const int i0 = (int)first_slot(m[k]);
        const int i2 = 31 - (int)last_lz(m[k]);
        const int i1 = max((int)first_slot(m[k] & (m[k] - 1u)), i0);
        B[3 * k + 0] = __umul24((uint32_t)i0, kG24) + W[k].hb;
        B[3 * k + 1] = __umul24((uint32_t)i1, kG24) + W[k].hb;
        B[3 * k + 2] = __umul24((uint32_t)i2, kG24) + W[k].hb;
        if (m[k] != 0u && !has) fb = B[3 * k];
        has = has || m[k] != 0u;
    }
    const u64 any = __ballot(has);
    if (any == 0ull) return false;
    const uint32_t fbw = (uint32_t)__builtin_amdgcn_readlane((int)fb, (int)__builtin_ctzll(any));
    if (!has) fb = fbw;
#pragma unroll
    for (int k = 0; k < NW; ++k)
        if (m[k] == 0u) B[3 * k + 0] = B[3 * k + 1] = B[3 * k + 2] = fb;
    return true;
}

// One wave sweeps the chunk's pods [beg, end) (beg a multiple of 8) through its
// NW words into lds[p]. form (wave-uniform): the range is a run of one class
// whose candidate bases are B (run_setup); else every pod is evaluated by its
// own bits.
// tpt != 0: the wave also holds the workgroup's packed last word Wt, whose
// T <= 64 / tpt groups repeat in tpt lane segments of 64 / tpt lanes: segment
// i evaluates pod i of a group of tpt pods (its bits from the lanes' block
// entries by ds_bpermute), so a partial word costs 8 / tpt evaluations per 8
// pods instead of 8; and up to 4 waves (on different SIMDs) hold it, wave
// tidx of tshare taking the 8-pod blocks b with b mod tshare == tidx. (A
// partial word holding the full cost on one SIMD was 6 % of config C:
// 100,000 rows 323 us, 99,840 rows 303 us, profiles/r03zd_tail.json.)
// MODE: kModeFast (three slots found by bit scans, word_fast), kModeGen (some
// group of the wave holds more than 3 rows of a digit: the bit-scan loop),
// kModeFix (every group of the wave is digit-aligned: word_fix).
constexpr int kModeFast = 0, kModeGen = 1, kModeFix = 2;

template <int KW, int NW, int MODE, bool TAIL, int NB>
__device__ __forceinline__ void sweep_pods(const Word (&W)[KW], const Word &Wt, uint32_t tpt, uint32_t tshare,
                                           uint32_t tidx, const uint2 *pinfo, uint32_t beg, uint32_t end, bool form,
                                           const uint32_t (&B)[NB], uint32_t lane, u64 *lds) {
    constexpr bool GEN = MODE == kModeGen;
    constexpr bool RUN = NB > 1;  // the run form is compiled in (NB = 3 * NW)
    const uint32_t seg_shift = tpt == 8u ? 3u : tpt == 4u ? 4u : 5u;  // log2(64 / tpt)
    for (uint32_t pb = beg; pb < end; pb += 64) {
        const uint32_t nblk = min(64u, end - pb);
        // the block's pods, one per lane: A and digit | tolerates << 4
        uint32_t a_l = 0, info_l = 14u | (30u << 16);  // (lanes past the block: no row matches)
        if (lane < nblk) {
            const uint2 e = pinfo[pb + lane];
            a_l = e.x;
            info_l = e.y;
        }
        for (uint32_t j = 0; j < nblk; j += 8) {
            uint32_t r[8];
            if (RUN && form) {
                // a whole block of one class: every slot holds a candidate
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const uint32_t A = (uint32_t)__builtin_amdgcn_readlane((int)a_l, (int)(j + t));
                    uint32_t h = 0;
#pragma unroll
                    for (int i = 0; i < NB; ++i) h = max(h, mix32(B[i] + A));
                    r[t] = h;
                }
            } else {
                Pod q[8];
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    q[t] = pod_bits((uint32_t)__builtin_amdgcn_readlane((int)a_l, (int)(j + t)),
                                    (uint32_t)__builtin_amdgcn_readlane((int)info_l, (int)(j + t)));
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    uint32_t h = 0;
#pragma unroll
                    for (int k = 0; k < NW; ++k)
                        h = max(h, MODE == kModeGen ? word_scan(match10(W[k], q[t]), W[k].hb + q[t].A)
                                   : MODE == kModeFix ? word_fix(W[k], q[t])
                                                      : word_fast(W[k], q[t]));
                    r[t] = h;
                }
            }
            if (TAIL && ((pb + j) >> 3) % tshare == tidx) {  // wave-uniform
                const uint32_t seg = lane >> seg_shift;
                for (uint32_t e = 0; e < 8u; e += tpt) {
                    // lanes of segment seg: pod j + e + seg of the block (past nblk: A 0 and
                    // class 14, which no row matches, so h stays 0)
                    const int src = (int)(j + e + seg) << 2;
                    const Pod qt = pod_bits((uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a_l),
                                            (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)info_l));
                    const uint32_t h = GEN ? word_scan(match10(Wt, qt), Wt.hb + qt.A) : word_fast(Wt, qt);
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if ((uint32_t)t >= e && (uint32_t)t < e + tpt) r[t] = max(r[t], seg == (uint32_t)t - e ? h : 0u);
                }
            }
            const uint32_t u = reduce8(r, lane);
            const uint32_t pi = j + rev3(lane >> 3);  // lanes 8k: pod pi of the block
            const bool mine = (lane & 7u) == 0u && pi < nblk;
            if (mine && u != 0u) atomicMax(&lds[pb + pi], (11ull << 32) | u);
            // a zero maximum: no score-10 row in this wave (or one whose hash is 0);
            // redo those pods exactly
            u64 redo = __ballot(mine && u == 0u);
            while (redo) {
                const uint32_t l = (uint32_t)__builtin_ctzll(redo);
                redo &= redo - 1ull;
                const uint32_t t = rev3(l >> 3);
                const Pod qs = pod_bits((uint32_t)__builtin_amdgcn_readlane((int)a_l, (int)(j + t)),
                                        (uint32_t)__builtin_amdgcn_readlane((int)info_l, (int)(j + t)));
                const u64 v = pod_slow<KW, NW, MODE == kModeFix>(W, Wt, TAIL && ((pb + j) >> 3) % tshare == tidx, qs);
                if (lane == 0 && v) atomicMax(&lds[pb + j + t], v);
            }
        }
    }
}

// The list form. The lists of name digit d as tiles of kCandTile entries, 3 per
// lane: S_d's ns tiles from entry off, then U_d's, nt tiles in all
// (ms_internal.h kCand*). hdr: the buffer's header (in LDS).
struct DigitLists {
    uint32_t off, ns, nt;
};

__device__ __forceinline__ DigitLists digit_lists(const uint32_t *hdr, uint32_t d) {
    DigitLists L;
    L.off = hdr[d];
    L.nt = (hdr[d + 1] - L.off) / kCandTile;
    L.ns = hdr[kCandDigits + 1u + d];
    return L;
}

// Who is swept over what, for sweep_lists and sweep_range alike: the leading
// tiles of its digit's lists that hold the candidates of a digit pod, S_d's for
// a pod that does not tolerate, all of them for one that does. 0: the list form
// has nothing for the pod and sweep_range takes it through the planes per pod:
// a pod that does not tolerate when S_d is empty, one that does when S_d and
// U_d both are (and the pods of the other class, which have no lists).
__device__ __forceinline__ uint32_t list_tiles(const DigitLists &L, bool tolerates) {
    return tolerates ? L.nt : L.ns;
}

// A list-form chunk's classes, class c in lane c (c <= kPpClasses; the lanes
// above repeat the other class): its pods [beg, end) and the lists of its
// digit, which is its sort slot c / 2 moved back by the table's base (pod_entry).
// A wave gathers them twice, at the start of sweep_range and of sweep_lists,
// every LDS read independent of the others, and takes a class's values by
// v_readlane: read from LDS class by class, bounds, then an entry's digit, then
// the header, they were three dependent round trips at each of 21 classes
// before a wave hashed anything, and again at every digit of sweep_lists.
// planes (wave-uniform): the classes with pods that sweep_range takes per pod,
// one bit per class (the ballot counts lanes 0 .. kPpClasses only: the lanes
// above hold copies of the other class, which must be swept once).
struct ClassLanes {
    uint32_t beg, end;
    DigitLists L;
    u64 planes;
};

// (pods: the lane's class holds a pod)
__device__ __forceinline__ u64 plane_classes(const DigitLists &L, uint32_t lane, bool pods) {
    const uint32_t c = min(lane, kPpClasses);
    return __ballot(lane <= kPpClasses && pods && (c == kPpClasses || list_tiles(L, (c & 1u) != 0u) == 0u));
}

__device__ __forceinline__ ClassLanes class_lanes(const uint32_t *hdr, const uint32_t *rb, uint32_t base10,
                                                  uint32_t lane) {
    const uint32_t c = min(lane, kPpClasses);
    ClassLanes C;
    C.beg = rb[c];
    C.end = rb[c + 1];
    C.L = digit_lists(hdr, ((c >> 1) + base10) % kCandDigits);
    C.planes = plane_classes(C.L, lane, C.beg < C.end);
    return C;
}

// class_lanes' planes from the sort's class counts (cnt, final after its second
// barrier), before the bounds exist. Every wave reads the same words, so the answer
// is workgroup-uniform. Empty (config C: every class has tiles and every pod a
// digit): nothing of this workgroup is taken from the planes.
__device__ __forceinline__ u64 plane_classes_ahead(const uint32_t *hdr, const uint32_t *cnt, uint32_t base10,
                                                   uint32_t lane) {
    const uint32_t c = min(lane, kPpClasses);
    return plane_classes(digit_lists(hdr, ((c >> 1) + base10) % kCandDigits), lane, cnt[c] != 0u);
}

// A pod of class c (pod_class) of a list-form chunk is swept by sweep_lists: the
// complement of class_lanes' planes for the classes that hold a pod, asked per pod
// (the lane table's final pass).
__device__ __forceinline__ bool list_covered(const uint32_t *hdr, uint32_t c, uint32_t base10) {
    return c < kPpClasses && list_tiles(digit_lists(hdr, ((c >> 1) + base10) % kCandDigits), (c & 1u) != 0u) != 0u;
}

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}

// The lane table (LT = 64 words per pod position, a word to a lane; after the sort
// words in LDS, zeroed by the prologue). In the list form a pod's candidates are spread
// over all the waves' lanes, and every lane's maximum is a candidate's hash, so
// the lane maxima need no reduction in the wave: a wave puts them into the
// pod's row of the table by ds_max_u32, lane by lane, and the workgroup reduces
// each row once after the sweep (table_rowmax, the kernel's final pass). A wave
// held 9 to 12 entries per lane at config C and paid the 8-pod butterfly for
// every 50 to 66 hash instructions per pod; this way it pays one LDS
// instruction per pod and no cross-lane one. (32 words per pod, reduce8's first
// stage in front of 4 ds_max_u32 per block, gained half as much at config C:
// profiles/r15a_lane_table_ab.txt.)
// row: the block's first row plus the lane (table + (first pod) * LT + lane), so
// consecutive lanes hit consecutive banks and the pods differ by the
// instruction's offset field alone. n: the pods present in the block
// (wave-uniform); the absent ones write nothing.
__device__ __forceinline__ void lds_max_u32(uint32_t *p, uint32_t v) {
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (no return value: ds_max_u32)
}

template <int LT>
__device__ __forceinline__ void table_put(uint32_t *row, const uint32_t (&r)[8], uint32_t n) {
    static_assert(LT == 64, "a word to a lane");
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if ((uint32_t)t < n) lds_max_u32(row + t * LT, r[t]);
}

// One wave sweeps the pods [beg, end) of one class through NT tiles of the
// lists of the class's digit, B[3k .. 3k+2] the lane's entries of tile k: one
// add and one mix32 per pod and entry. Every entry is a candidate of every pod
// of the range (or a copy of one), so the maximum stands as it is, also when it is 0:
// that is the hash of a real candidate then, and no redo is needed.
// The range may start anywhere and its last block hold fewer than 8 pods,
// whose absent pods are not hashed (wave-uniform tests).
// LT != 0: the lane maxima go to the lane table (tabl: the table plus the lane);
// else they are reduced here (reduce8) and combined in the pods' slots.
template <int NT, int LT>
__device__ __forceinline__ void sweep_list_pods(const uint32_t (&B)[3 * kPpWords], const uint2 *pinfo, uint32_t beg,
                                                uint32_t end, uint32_t lane, u64 *lds, uint32_t *tabl) {
    for (uint32_t pb = beg; pb < end; pb += 64) {
        const uint32_t nblk = min(64u, end - pb);
        const uint32_t a_l = lane < nblk ? pinfo[pb + lane].x : 0u;
        for (uint32_t j = 0; j < nblk; j += 8) {
            uint32_t r[8];
            if (nblk - j >= 8u) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const uint32_t A = (uint32_t)__builtin_amdgcn_readlane((int)a_l, (int)(j + t));
                    uint32_t h = 0;
#pragma unroll
                    for (int i = 0; i < 3 * NT; ++i) h = max(h, mix32(B[i] + A));
                    r[t] = h;
                }
                if constexpr (LT != 0) table_put<LT>(tabl + (pb + j) * LT, r, 8u);
            } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    r[t] = 0;
                    if (j + (uint32_t)t < nblk) {
                        const uint32_t A = (uint32_t)__builtin_amdgcn_readlane((int)a_l, (int)(j + t));
#pragma unroll
                        for (int i = 0; i < 3 * NT; ++i) r[t] = max(r[t], mix32(B[i] + A));
                    }
                }
                if constexpr (LT != 0) table_put<LT>(tabl + (pb + j) * LT, r, nblk - j);
            }
            if constexpr (LT == 0) {
                const uint32_t u = reduce8(r, lane);
                const uint32_t pi = j + rev3(lane >> 3);  // lanes 8k: pod pi of the block
                if ((lane & 7u) == 0u && pi < nblk) atomicMax(&lds[pb + pi], (11ull << 32) | u);
            }
        }
    }
}

// (sweep_list_pods over the first n of the lane's tiles)
template <int LT>
__device__ __forceinline__ void sweep_list_tiles(uint32_t n, const uint32_t (&B)[3 * kPpWords], const uint2 *pinfo,
                                                 uint32_t beg, uint32_t end, uint32_t lane, u64 *lds, uint32_t *tabl) {
    switch (n) {  // wave-uniform
        case 1: sweep_list_pods<1, LT>(B, pinfo, beg, end, lane, lds, tabl); break;
        case 2: sweep_list_pods<2, LT>(B, pinfo, beg, end, lane, lds, tabl); break;
        case 3: sweep_list_pods<3, LT>(B, pinfo, beg, end, lane, lds, tabl); break;
        default: sweep_list_pods<4, LT>(B, pinfo, beg, end, lane, lds, tabl); break;
    }
}

// The maximum of row i of the lane table, in the last of the LT / 4 = 16
// consecutive lanes (a DPP row) that read it, 4 words each (one ds_read_b128; the
// other lanes hold partial maxima). Every lane of the wave takes part.
template <int LT>
__device__ __forceinline__ uint32_t table_rowmax(const uint32_t *tab, uint32_t i, uint32_t sub) {
    const uint4 q = *reinterpret_cast<const uint4 *>(tab + i * LT + sub * 4u);
    uint32_t m = max(max(q.x, q.y), max(q.z, q.w));
    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x111, 0xF, 0xF, false));  // row_shr:1
    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x112, 0xF, 0xF, false));  // row_shr:2
    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x114, 0xF, 0xF, false));  // row_shr:4
    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x118, 0xF, 0xF, false));  // row_shr:8
    return m;
}

// The wave's tiles t0, t0 + waves, .. of a pass, nt of them, 3 entries per lane
// and tile. Every load is issued whatever nt is, a tile past the wave's last
// reading its first again (no sweep uses it): loads under a test of nt came out
// as one branch and one wait per tile, four dependent round trips where this is one.
__device__ __forceinline__ void load_list_tiles(const uint32_t *__restrict__ cand, uint32_t off, uint32_t t0,
                                                uint32_t nt, uint32_t waves, uint32_t lane,
                                                uint32_t (&B)[3 * kPpWords]) {
#pragma unroll
    for (int k = 0; k < kPpWords; ++k) {
        const uint32_t tile = t0 + ((uint32_t)k < nt ? (uint32_t)k * waves : 0u);
        const uint32_t *e = cand + kCandHeader + off + tile * kCandTile + lane;
#pragma unroll
        for (int i = 0; i < 3; ++i) B[3 * k + i] = e[i * 64];
    }
}

// One wave's share of a class-sorted chunk in the list form. The pods of a
// digit (a slot of the sort) are contiguous, [b0, b1) those that do not
// tolerate and [b1, b2) those that do, and so are the digit's lists, S_d's tiles
// then U_d's. Wave wv takes tiles wv, wv + waves, .. of the digit, up to
// kPpWords of them per pass (more than kPpWords * waves tiles take further
// passes; the waves combine by atomicMax on LDS either way), in ONE load round
// for both tolerations: the S tiles come first, so the first ns of the wave's
// nt tiles are S_d's (both counts wave-uniform), the pods that do not tolerate
// are swept through those and the pods that do through all nt, out of the same
// registers. A pass that holds U tiles only skips the former; a digit none of
// whose pods tolerates stops at S_d's tiles. A wave with no tile of a digit
// skips it.
template <int LT>
__device__ __forceinline__ void sweep_lists(const uint32_t *__restrict__ cand, const ClassLanes &C,
                                            const uint2 *pinfo, uint32_t wv, uint32_t waves, uint32_t lane,
                                            u64 *lds, uint32_t *tabl MS_TL_PARAM) {
    MS_TL_COUNT_DECL;
    for (uint32_t s = 0; s < kPpClasses; s += 2) {
        const uint32_t b0 = lane_value(C.beg, s), b1 = lane_value(C.end, s), b2 = lane_value(C.end, s + 1u);
        if (b0 >= b2) continue;
        const DigitLists L = {lane_value(C.L.off, s), lane_value(C.L.ns, s), lane_value(C.L.nt, s)};
        const uint32_t ntile = list_tiles(L, b1 < b2);  // (no pod tolerates: S_d's tiles)
        for (uint32_t t0 = wv; t0 < ntile; t0 += kPpWords * waves) {
            const uint32_t nt = min((uint32_t)kPpWords, (ntile - t0 + waves - 1u) / waves);  // >= 1
            const uint32_t ns = t0 < L.ns ? min((uint32_t)kPpWords, (L.ns - t0 + waves - 1u) / waves) : 0u;
            uint32_t B[3 * kPpWords];
            load_list_tiles(cand, L.off, t0, nt, waves, lane, B);
            MS_TL(kTlDigit0 + 3u * (s >> 1));
            MS_TL_LANDED;
            MS_TL(kTlDigit0 + 3u * (s >> 1) + 1u);
            MS_TL_COUNT(3u * ((b0 < b1 ? ns * (b1 - b0) : 0u) + nt * (b2 - b1)));
            if (ns != 0u && b0 < b1) sweep_list_tiles<LT>(ns, B, pinfo, b0, b1, lane, lds, tabl);
            if (b1 < b2) sweep_list_tiles<LT>(nt, B, pinfo, b1, b2, lane, lds, tabl);
        }
        MS_TL(kTlDigit0 + 3u * (s >> 1) + 2u);
    }
    MS_TL_COUNT_PUT;
}

// One wave sweeps the chunk's pods [0, np). runs: the entries are class-sorted
// (rb: the 22 bounds); kModeFix and kModeFast waves then take region A's class
// runs one by one, in the run form where run_setup finds a candidate, and
// region B per pod. Every bound but np is a multiple of 8, so every wave cuts
// the same 8-pod blocks (the packed last word's sharing counts them). Without
// runs, and for kModeGen waves, the chunk is one per-pod range.
// lists: the chunk is swept in the list form (sweep_lists takes every digit
// class for which list_tiles gives a tile): what is left here, for waves of
// every mode, are the classes of class_lanes' planes, the digit classes it gives
// none and the other class, per pod. Their ranges start anywhere; the packed last
// word's sharing only needs every wave to cut the same blocks, which they do
// (the same beg for all).
// (Padding every run to whole blocks instead of sweeping the rests per pod
// measured 0.5 % slower at config C, profiles/r07a_class_runs_ab.txt.)
template <int KW, int NW, int MODE, bool TAIL>
__device__ __forceinline__ void sweep_range(const Word (&W)[KW], const Word &Wt, uint32_t tpt, uint32_t tshare,
                                            uint32_t tidx, const uint2 *pinfo, const uint32_t *rb, bool runs,
                                            bool lists, const uint32_t *hdr, uint32_t base10, uint32_t np,
                                            uint32_t lane, u64 *lds) {
    // (not in the 8-word form: with 24 bases more it needs over 128 VGPRs)
    constexpr bool RUN = MODE != kModeGen && NW > 0 && KW == kPpWords;
    const bool cut = lists || (RUN && runs);
    // the classes to take here: those the list form leaves (their bounds a class to a
    // lane), every class, or the chunk as one range
    u64 todo = cut ? (2ull << kPpClasses) - 1ull : 1ull << kPpClasses;
    uint32_t cbeg = 0, cend = 0;
    if (lists) {
        const ClassLanes C = class_lanes(hdr, rb, base10, lane);
        cbeg = C.beg, cend = C.end, todo = C.planes;
    }
    for (; todo; todo &= todo - 1ull) {
        const uint32_t c = (uint32_t)__builtin_ctzll(todo);
        const uint32_t beg = lists ? lane_value(cbeg, c)
                             : cut ? (uint32_t)__builtin_amdgcn_readfirstlane((int)rb[c]) : 0u;
        const uint32_t end = lists ? lane_value(cend, c)
                             : cut ? (uint32_t)__builtin_amdgcn_readfirstlane((int)rb[c + 1]) : np;
        if (beg >= end) continue;
        uint32_t B[RUN ? NW * 3 : 1] = {};
        bool form = false;
        if constexpr (RUN)
            if (!lists && c < kPpClasses)
                form = run_setup<KW, NW>(W, (uint32_t)__builtin_amdgcn_readfirstlane((int)pinfo[beg].y), B);
        sweep_pods<KW, NW, MODE, TAIL>(W, Wt, tpt, tshare, tidx, pinfo, beg, end, form, B, lane, lds);
    }
}

// KW words per lane: 4 (workgroups of up to 16 waves split the rows) or 8 for
// shards of at most kPpSmallGroups groups, where ONE wave holds every row: then
// every wave does the same work whatever SIMD it lands on (with 4 words a
// 12.5k-row shard dealt over 4 waves gave them 2, 2, 2 and 1 words, and the
// SIMD that hosts the short waves idled), and the per-pod reduction is paid
// once per 7 words instead of once per 2.
// Pods per evaluation of a workgroup's packed last word (sweep_range): 8 for a
// last word of <= 8 groups, 0 when it stays a full word (sweep_range also
// takes 4 and 2: 16 and 32 groups). ng
// groups over `waves` waves. Packed only where that lowers the busiest SIMD's
// load (waves w and w + 4 of a workgroup share a SIMD): words per SIMD, in
// sixteenths, with and without it (100,000 rows over 16 waves: 14 -> 13.06;
// 50,010 over 8: 7 either way, and packing cost 1 %).
__host__ __device__ inline uint32_t tail_pods(uint32_t ng, uint32_t waves) {
    if (ng == 0) return 0u;
    const uint32_t wlast = (ng + 63u) / 64u - 1u, tail_n = ng - wlast * 64u;
    // (8 pods per evaluation only: 2 per evaluation, 17 groups left over a
    // 6,250-row wave, cost more than the full word, profiles/r03zk_tail_pack_ab.txt)
    const uint32_t tpt = tail_n <= 8u ? 8u : 0u;
    if (!tpt) return 0u;
    // up to 4 waves: several workgroups share a CU and the hardware rotates
    // their waves over the SIMDs (profiles/r03z_hwid_placement.txt), so every
    // word saved is saved on every SIMD
    if (waves <= 4u) return tpt;
    const uint32_t wv_t = wlast % waves;
    const uint32_t tshare = kTailShare < waves - wv_t ? kTailShare : waves - wv_t;
    uint32_t L[4] = {0, 0, 0, 0};
    for (uint32_t w = 0; w < waves && w <= wlast; ++w) L[w & 3u] += 16u * ((wlast - w) / waves + 1u);
    auto mx = [&] {
        const uint32_t a = L[0] > L[1] ? L[0] : L[1], b = L[2] > L[3] ? L[2] : L[3];
        return a > b ? a : b;
    };
    const uint32_t m0 = mx();
    L[wv_t & 3u] -= 16u;
    const uint32_t eps = ((tpt == 8u ? 4u : tpt == 4u ? 8u : 12u) + tshare - 1u) / tshare;
    for (uint32_t i = 0; i < tshare; ++i) L[(wv_t + i) & 3u] += eps;
    return mx() < m0 ? tpt : 0u;
}

// A second batch swept by the same launch (shard sweeps with key output only:
// ms_sharded_submit coalesces two consecutive submits into one launch, paying
// the per-launch ramp and drain once). Workgroups nblk1.. take its chunks.
struct PpJob2 {
    const ms_pod_rec *pods;  // nullptr: one batch
    u64 *keys;
    uint32_t n_pods, nblk1;
};

// TP: the packed-last-word path is compiled in (launch_sweep_pp picks it only
// for shapes tail_pods packs; the others run the plain form).
// LT: words per pod of the lane table (0: none; launch_sweep_pp picks it for
// list-form chunks whose table fits, lane_table_fits).
template <int KW, bool TP, int LT>
__global__ __launch_bounds__(64 * kPpMaxWaves) void k_sweep_nunn_pp(
    const uint32_t *__restrict__ planes, uint32_t gstride, uint32_t n_groups, uint32_t node_base,
    const ms_pod_rec *__restrict__ pods1, uint32_t n_pods1, uint32_t chunk, uint32_t seed32, u64 *__restrict__ keys1,
    int atomic_keys, ms_result *__restrict__ results, uint32_t present, NodeTable tab, int commit,
    uint32_t pstride, ms_result_compact *__restrict__ resc, PpJob2 j2, int fix_ok, uint32_t xtra,
    const uint32_t *__restrict__ cand MS_TL_KPARAM) {
    // LDS: one combine slot per pod of the chunk, then the chunk's pod entries,
    // then the kPpSortWords words of the class sort, then (LT != 0) the lane
    // table: LT words per pod position
    // (xtra: workgroups 0 .. xtra-1 take chunk + 8 pods, the balanced split)
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    uint2 *pinfo = reinterpret_cast<uint2 *>(lds + chunk + (xtra ? 8u : 0u));
    const uint32_t lane = lane_id();
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    MS_TL_INIT;
    const bool second = j2.pods && blockIdx.x >= j2.nblk1;  // (workgroup-uniform)
    const ms_pod_rec *__restrict__ pods = second ? j2.pods : pods1;
    const uint32_t n_pods = second ? j2.n_pods : n_pods1;
    u64 *__restrict__ keys = second ? j2.keys : keys1;
    const uint32_t bi = second ? blockIdx.x - j2.nblk1 : blockIdx.x;
    const uint32_t pbeg = bi * chunk + min(bi, xtra) * 8u;
    const uint32_t pend = min(n_pods, pbeg + chunk + (bi < xtra ? 8u : 0u));
    const uint32_t np = pend > pbeg ? pend - pbeg : 0u;
    // after the entries: class counts, the sweep's bounds rb, region B's class starts
    uint32_t *cnt = reinterpret_cast<uint32_t *>(pinfo + chunk + (xtra ? 8u : 0u));
    uint32_t *rb = cnt + 24, *sb = cnt + 48, *hdr = cnt + 72;
    const bool runs = KW == kPpWords && chunk >= kPpSortMin;  // (kernel-uniform; KW = 8: no run form)
    // the list form: this workgroup holds every row (else the workgroups of a chunk
    // would each sweep the whole list)
    const bool lists = runs && cand != nullptr && gridDim.y == 1u;
    uint32_t *ltab = hdr + 24;
    if constexpr (LT != 0) {
        // (16-byte stores; the sort's barriers come before the sweep)
        uint4 *z = reinterpret_cast<uint4 *>(ltab);
        for (uint32_t i = threadIdx.x; i < np * (LT / 4); i += blockDim.x) z[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    // a list-form workgroup with no class to take from the planes (plane_classes_ahead)
    // clears this: it loads no plane and runs no sweep_range
    bool use_planes = true;
    if (!runs) {
        for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) {
            lds[i] = 0;
            uint2 e = pod_entry(pods, pbeg + i, seed32, pstride, node_base % 10u);
            e.y |= i << 21;
            pinfo[i] = e;
        }
    } else {
        // counting sort by class: the unsorted entries wait in the combine slots
        // (8 bytes each) with their rank in the class, taken with the count
        if (threadIdx.x < 24u) cnt[threadIdx.x] = 0u;
        if (lists)
            for (uint32_t i = threadIdx.x; i <= kCandClasses; i += blockDim.x) hdr[i] = cand[i];
        __syncthreads();
        MS_TL(kTlBar1);
        for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) {
            uint2 e = pod_entry(pods, pbeg + i, seed32, pstride, node_base % 10u);
            e.y |= atomicAdd(&cnt[pod_class(e.y)], 1u) << 21;
            reinterpret_cast<uint2 *>(lds)[i] = e;
        }
        __syncthreads();
        MS_TL(kTlBar2);
        if constexpr (KW == kPpWords)
            if (lists) use_planes = plane_classes_ahead(hdr, cnt, node_base % 10u, lane) != 0ull;
        if (threadIdx.x <= kPpClasses) {
            // region A: the whole 8-pod blocks of the digit classes (the list form: all
            // their pods); region B: the rest
            uint32_t a = 0, b = 0, na = 0, nb = 0;
            for (uint32_t c = 0; c < kPpClasses; ++c) {
                const uint32_t n = cnt[c], full = lists ? n : n & ~7u;
                if (c == threadIdx.x) a = na, b = nb;
                na += full;
                nb += n - full;
            }
            if (threadIdx.x == kPpClasses) {
                a = na, b = nb;
                rb[kPpClasses + 1] = np;
            }
            rb[threadIdx.x] = a;
            sb[threadIdx.x] = na + b;
        }
        __syncthreads();
        MS_TL(kTlBar3);
        for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) {
            const uint2 e = reinterpret_cast<const uint2 *>(lds)[i];
            const uint32_t c = pod_class(e.y), rank = e.y >> 21;
            const uint32_t full = c < kPpClasses ? rb[c + 1] - rb[c] : 0u;
            const uint32_t pos = rank < full ? rb[c] + rank : sb[c] + (rank - full);
            pinfo[pos] = make_uint2(e.x, (e.y & 0x1FFFFFu) | (i << 21));
            lds[i] = 0;
        }
    }

    const uint32_t waves = blockDim.x >> 6;
    // The planes, for everything but a list-form workgroup none of whose classes is
    // taken from them. Such a workgroup works out no word's share (tail_pods, a loop of
    // divisions, stood between every workgroup's sort and its first hash), loads no
    // plane and no packed last word, detects no mode and has no sweep_range to run:
    // it goes from the scatter's barrier straight to sweep_lists. (The test is
    // workgroup-uniform, so every wave meets the same barrier.)
    if (use_planes) {
        // the wave's groups, dealt round-robin over the workgroup's waves so their
        // word counts differ by at most one: word k of lane l is group
        // g0 + (k * waves + wv) * 64 + l. The workgroup's last word, when it holds
        // T <= 32 groups, is packed instead (sweep_range): its wave loads group
        // (lane mod 64/tpt) of it into Wt.
        const uint32_t g0 = blockIdx.y * waves * 64u * KW;
        const uint32_t ng = min(n_groups - g0, waves * 64u * KW);  // (blockIdx.y < gy: g0 < n_groups)
        const uint32_t wlast = (ng + 63u) / 64u - 1u, tail_n = ng - wlast * 64u;
        uint32_t tpt = TP ? tail_pods(ng, waves) : 0u;
        const uint32_t wv_t = wlast % waves, tshare = min(kTailShare, waves - wv_t);  // its waves
        const bool owner = wv == wv_t;     // it is this wave's last word in the dealing
        if (wv < wv_t || wv >= wv_t + tshare) tpt = 0u;  // wave-uniform
        Word W[KW], Wt;
        int nw = 0;
        bool over = false, misaligned = false;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const uint32_t wi = k * waves + wv;
            const uint32_t gw = g0 + wi * 64u;
            const uint32_t g = gw + lane;
            const bool in = g < n_groups && !(tpt && owner && wi == wlast);
            if (gw < n_groups && !(tpt && owner && wi == wlast)) nw = k + 1;  // wave-uniform
            W[k].d0 = in ? planes[kPlaneD0 * gstride + g] : 0u;
            W[k].d1 = in ? planes[kPlaneD1 * gstride + g] : 0u;
            W[k].d2 = in ? planes[kPlaneD2 * gstride + g] : 0u;
            W[k].d3 = in ? planes[kPlaneD3 * gstride + g] : 0u;
            W[k].sched = in ? planes[kPlaneSched * gstride + g] : 0u;
            W[k].pres = in ? planes[kPlanePresent * gstride + g] : 0u;
            W[k].dsched = in ? planes[kPlaneDigitSched * gstride + g] : 0u;
            W[k].dpres = in ? planes[kPlaneDigitPres * gstride + g] : 0u;
            W[k].hb = (node_base + g * kGroupRows) * kG24;
            const uint32_t ov = in ? planes[kPlaneOver * gstride + g] : 0u;
            // more than 3 present rows of one digit in a group: the fast slots cannot hold them
            over = over || (ov & 1u) != 0u;
            misaligned = misaligned || (ov & 2u) != 0u;
        }
        {
            const uint32_t gi = tpt ? lane & ((64u / tpt) - 1u) : 0u;
            const uint32_t g = g0 + wlast * 64u + gi;
            const bool in = tpt && gi < tail_n;
            Wt.d0 = in ? planes[kPlaneD0 * gstride + g] : 0u;
            Wt.d1 = in ? planes[kPlaneD1 * gstride + g] : 0u;
            Wt.d2 = in ? planes[kPlaneD2 * gstride + g] : 0u;
            Wt.d3 = in ? planes[kPlaneD3 * gstride + g] : 0u;
            Wt.sched = in ? planes[kPlaneSched * gstride + g] : 0u;
            Wt.pres = in ? planes[kPlanePresent * gstride + g] : 0u;
            Wt.hb = (node_base + g * kGroupRows) * kG24;
            Wt.dsched = Wt.dpres = 0u;  // (the packed word always takes word_fast / word_scan)
            over = over || (in && (planes[kPlaneOver * gstride + g] & 1u) != 0u);
        }
        const bool gen = __ballot(over) != 0;
        // every word of the wave digit-aligned
        const int mode = gen ? kModeGen : (fix_ok && __ballot(misaligned) == 0) ? kModeFix : kModeFast;
        MS_TL_LANDED;
        MS_TL(kTlPlanes);
        __syncthreads();
        MS_TL(kTlBar4);
        if (np && (nw || tpt)) {
            switch (nw * 6 + mode * 2 + (tpt ? 1 : 0)) {  // wave-uniform
#define MS_PP_CASE1(N, M, T)                                                                                     \
        case 6 * N + 2 * M + T:                                                                                      \
            if constexpr (N <= KW && (N > 0 || T))                                                                   \
                sweep_range<KW, (N <= KW ? N : KW), M, T>(W, Wt, tpt, tshare, wv - wv_t, pinfo, rb, runs, lists, hdr,   \
                                                          node_base % 10u, np, lane, lds);                          \
            break;
#define MS_PP_CASE(N)        \
        MS_PP_CASE1(N, 0, false) \
        MS_PP_CASE1(N, 0, true)  \
        MS_PP_CASE1(N, 1, false) \
        MS_PP_CASE1(N, 1, true)  \
        MS_PP_CASE1(N, 2, false) \
        MS_PP_CASE1(N, 2, true)
                MS_PP_CASE(0)
                MS_PP_CASE(1)
                MS_PP_CASE(2)
                MS_PP_CASE(3)
                MS_PP_CASE(4)
                MS_PP_CASE(5)
                MS_PP_CASE(6)
                MS_PP_CASE(7)
                MS_PP_CASE(8)
#undef MS_PP_CASE
#undef MS_PP_CASE1
                default:
                    break;  // no groups in this wave
            }
        }
    } else {
        __syncthreads();
        MS_TL(kTlBar4);
    }
    if constexpr (KW == kPpWords)
        if (np && lists)
            sweep_lists<LT>(cand, class_lanes(hdr, rb, node_base % 10u, lane), pinfo, wv, waves, lane, lds,
                            ltab + lane MS_TL_PASS);
    MS_TL(kTlSweepEnd);
    __syncthreads();
    MS_TL(kTlSweepBar);
    if constexpr (LT != 0) {
        // The lane table's final pass, once per pod: LT / 4 lanes to a row. A list-form
        // maximum is level 11 whatever its value (0 is a real candidate's hash), so what
        // says that a row holds one is the pod's class (list_covered). The pod's slot may
        // hold the planes path's value; an uncovered pod keeps it alone.
        if (np && lists) {  // (workgroup-uniform)
            constexpr uint32_t G = LT / 4;
            const uint32_t sub = threadIdx.x % G;
            for (uint32_t i0 = 0; i0 < np; i0 += blockDim.x / G) {
                const uint32_t i = i0 + threadIdx.x / G;
                const uint32_t m = table_rowmax<LT>(ltab, min(i, np - 1u), sub);
                if (sub == G - 1u && i < np) {
                    if (list_covered(hdr, pod_class(pinfo[i].y), node_base % 10u))
                        lds[i] = umax64(lds[i], (11ull << 32) | m);
                }
            }
        }
        __syncthreads();
        MS_TL(kTlFinal);
    }
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) {
        const u64 v = lds[i];
        const uint2 pe = pinfo[i];
        const uint32_t po = pbeg + (pe.y >> 21);  // the pod at (sorted) position i
        u64 key = present ? kKeyListed : 0ull;  // no feasible row: listed or not (decode_key)
        if (v) {
            const uint32_t h = (uint32_t)v;
            key = make_key((uint32_t)(v >> 32) - 1u, h, tb_unhash(pe.x, h));
        }
        if (keys) {
            if (!atomic_keys) keys[po] = key;
            else if (key) atomicMax(&keys[po], key);
        }
        if (results || resc) {
            const ms_result r = decode_key(key, (int8_t)(pe.y >> 8), nullptr, 0, present);
            if (results) {
                results[po] = r;
            } else {  // the compact record, straight into the caller's (pinned host) array
                ms_result_compact rc;
                rc.node = r.node;
                rc.score = (uint16_t)r.score;
                rc.code = (uint8_t)r.code;
                rc.plugin_mask = (uint8_t)r.plugin_mask;
                resc[po] = rc;
            }
            // assume-on-select in the same launch (ms_schedule_batch / the sequential
            // NU+NN cycle): NodeInfo.AddPod on the winner, which this context owns
            // (one workgroup holds all its rows); a compact pod requests nothing
            if (commit && r.code == MS_CODE_SUCCESS) {
                if (resc) {
                    const ms_pod_rec z = {};
                    add_pod(tab, (uint32_t)r.node - tab.base, z, +1);
                } else {
                    add_pod(tab, (uint32_t)r.node - tab.base, pods[po], +1);
                }
            }
        }
    }
    MS_TL(kTlEnd);
    MS_TL_PUT(kTlReal1, __builtin_amdgcn_s_memrealtime());
}

__host__ __device__ inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// Bit planes of one 30-row group from the SoA columns (flags, digit).
__device__ __forceinline__ void build_group(const NodeTable &t, uint32_t g) {
    uint32_t d[4] = {0, 0, 0, 0}, sched = 0, pres = 0, isdig = 0, misal = 0;
    for (uint32_t s = 0; s < kGroupRows; ++s) {
        const uint32_t r = g * kGroupRows + s;
        if (r >= t.cap) break;
        const uint32_t f = t.flags[r], dg = t.digit[r];
        const uint32_t v = dg <= 9u ? dg : 15u;
#pragma unroll
        for (int b = 0; b < 4; ++b) d[b] |= ((v >> b) & 1u) << s;
        if (!(f & kNodeAbsent)) {
            pres |= 1u << s;
            if (!(f & kNodeUnschedulable)) sched |= 1u << s;
            if (v <= 9u) {
                isdig |= 1u << s;
                if (v != (t.base + r) % 10u) misal = 2u;  // digit != ordinal mod 10
            }
        }
    }
    uint32_t over = misal;
#pragma unroll
    for (int v = 0; v < 10; ++v) {
        const uint32_t m = pres & ((v & 1) ? d[0] : ~d[0]) & ((v & 2) ? d[1] : ~d[1]) & ((v & 4) ? d[2] : ~d[2]) &
                           ((v & 8) ? d[3] : ~d[3]);
        over |= __popc(m) > 3 ? 1u : 0u;
    }
    const uint32_t st = t.gcap;
    t.planes[kPlaneDigitPres * st + g] = pres & isdig;
    t.planes[kPlaneDigitSched * st + g] = sched & isdig;
    t.planes[kPlaneOver * st + g] = over;
    t.planes[kPlaneD0 * st + g] = d[0];
    t.planes[kPlaneD1 * st + g] = d[1];
    t.planes[kPlaneD2 * st + g] = d[2];
    t.planes[kPlaneD3 * st + g] = d[3];
    t.planes[kPlaneSched * st + g] = sched;
    t.planes[kPlanePresent * st + g] = pres;
}

// deltas != nullptr: the groups of the applied deltas (a group rebuilt twice gets the
// same bits: the deltas' column writes finished in the previous launch); else all groups.
__global__ void k_build_planes(NodeTable t, const NodeDelta *__restrict__ deltas, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = deltas ? deltas[i].local / kGroupRows : i;
    if (g < t.gcap) build_group(t, g);
}

// The rows of group g in list c (ms_internal.h kCand*): the present rows of name digit
// c mod 10, the schedulable ones for c < 10 (S_d), the unschedulable ones above (U_d).
__device__ __forceinline__ uint32_t cand_mask(const NodeTable &t, uint32_t g, uint32_t c) {
    const uint32_t st = t.gcap, v = c % kCandDigits;
    const uint32_t d0 = t.planes[kPlaneD0 * st + g], d1 = t.planes[kPlaneD1 * st + g];
    const uint32_t d2 = t.planes[kPlaneD2 * st + g], d3 = t.planes[kPlaneD3 * st + g];
    const uint32_t sched = t.planes[kPlaneSched * st + g];
    const uint32_t f = c < kCandDigits ? sched : t.planes[kPlanePresent * st + g] & ~sched;
    return f & ((v & 1u) ? d0 : ~d0) & ((v & 2u) ? d1 : ~d1) & ((v & 4u) ? d2 : ~d2) & ((v & 8u) ? d3 : ~d3);
}

// The candidate lists (ms_internal.h kCand*) from the planes: block c builds
// list c. Every block first counts all 20 lists (its list starts after the
// padded lengths of those before it: the lists of the lower digits, and for
// U_d also S_d), then writes its entries in row order: 1024 groups at a time,
// each thread one group, placed by a block-wide prefix sum of the groups'
// candidate counts.
constexpr uint32_t kCandThreads = 1024;

__global__ __launch_bounds__(kCandThreads) void k_build_cand(NodeTable t, uint32_t *__restrict__ cand) {
    __shared__ uint32_t cnt[kCandClasses], wsum[kCandThreads / 64], first;
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid < kCandClasses) cnt[tid] = 0u;
    __syncthreads();
    uint32_t n[kCandClasses] = {};
    for (uint32_t g = tid; g < t.gcap; g += kCandThreads) {
#pragma unroll
        for (uint32_t k = 0; k < kCandClasses; ++k) n[k] += (uint32_t)__popc(cand_mask(t, g, k));
    }
#pragma unroll
    for (uint32_t k = 0; k < kCandClasses; ++k) {
        const uint32_t sum = wave_sum_u32_dpp(n[k]);
        if (lane == 0u && sum) atomicAdd(&cnt[k], sum);
    }
    __syncthreads();
    const uint32_t dg = c % kCandDigits;
    uint32_t off = 0;
    for (uint32_t k = 0; k < dg; ++k)
        off += (cdiv(cnt[k], kCandTile) + cdiv(cnt[kCandDigits + k], kCandTile)) * kCandTile;
    if (c >= kCandDigits) off += cdiv(cnt[dg], kCandTile) * kCandTile;
    const uint32_t len = cnt[c], padded = cdiv(len, kCandTile) * kCandTile;
    if (tid == 0u) {
        if (c < kCandDigits) {
            cand[dg] = off;
            cand[kCandDigits + 1u + dg] = padded / kCandTile;
        }
        cand[kCandClasses + 1u + c] = len;
        if (c + 1u == kCandClasses) cand[kCandDigits] = off + padded;
    }
    uint32_t *ent = cand + kCandHeader + off;
    uint32_t done = 0;  // entries written by the groups before g0
    for (uint32_t g0 = 0; g0 < t.gcap; g0 += kCandThreads) {
        const uint32_t g = g0 + tid;
        uint32_t m = g < t.gcap ? cand_mask(t, g, c) : 0u;
        const uint32_t k = (uint32_t)__popc(m);
        uint32_t incl = k;  // inclusive prefix sum over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) wsum[wv] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kCandThreads / 64; ++w) {
            if (w < wv) before += wsum[w];
            total += wsum[w];
        }
        uint32_t pos = done + before + incl - k;
        while (m) {
            const uint32_t slot = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            const uint32_t e = (t.base + g * kGroupRows + slot) * kG24;
            if (pos == 0u) first = e;
            if (pos < len) ent[pos] = e;  // (always: the counts come from the same planes)
            ++pos;
        }
        done += total;
        __syncthreads();
    }
    for (uint32_t i = len + tid; i < padded; i += kCandThreads) ent[i] = first;
}

}  // namespace

hipError_t launch_build_planes(const NodeTable &t, uint32_t *cand, const NodeDelta *d_deltas, uint32_t n,
                               hipStream_t s) {
    if (!t.planes) return hipSuccess;
    if (!d_deltas) n = t.gcap;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_build_planes, dim3(cdiv(n, 256)), dim3(256), 0, s, t, d_deltas, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !cand) return e;
    hipLaunchKernelGGL(k_build_cand, dim3(kCandClasses), dim3(kCandThreads), 0, s, t, cand);
    return hipGetLastError();
}

// Geometry: W waves (<= 16) of up to 256 groups each hold the rows (more
// rows: grid.y workgroups per chunk); pods per workgroup sized for one
// round of resident workgroups (16 waves per CU while chunks stay <= 1024
// pods, else 32) in multiples of 8, at most kPpMaxChunk (LDS).
constexpr uint32_t kPpMaxChunk = 2048;

// LDS of one workgroup whose largest chunk holds cap pods: slots, entries and sort
// words, and with lt != 0 a lane table of lt words per pod (k_sweep_nunn_pp).
constexpr uint32_t kPpLdsPerCu = 160u * 1024u;
constexpr int kPpLaneWords = 64;

__host__ inline uint32_t pp_lds_bytes(uint32_t cap, uint32_t lt) {
    return cap * (uint32_t)(sizeof(u64) + sizeof(uint2)) + kPpSortWords * (uint32_t)sizeof(uint32_t) +
           cap * lt * (uint32_t)sizeof(uint32_t);
}

// Where the list sweep combines through the lane table: the chunk is sorted (so
// that, with lists and one workgroup per chunk, it is swept in the list form), and
// with the table per_cu workgroups, the number the geometry sized the chunk for,
// still fit a CU's LDS together (each rounded up to 2 KiB, no finer than the
// allocation granule). Else the sweep reduces per wave as before: a table that
// cost residency would cost more than the reductions it saves.
__host__ inline bool lane_table_fits(uint32_t chunk, uint32_t xtra, uint32_t W, uint32_t per_cu) {
    if (chunk < kPpSortMin || W > (uint32_t)kPpMaxWaves) return false;
    const uint32_t wg = (pp_lds_bytes(chunk + (xtra ? 8u : 0u), (uint32_t)kPpLaneWords) + 2047u) / 2048u * 2048u;
    return wg * per_cu <= kPpLdsPerCu;
}

namespace {
// hipFuncAttributeMaxDynamicSharedMemorySize of one instantiation (the flags are
// per kernel, not per kernel type), a CU's whole LDS, set once per device (two
// threads setting it at once set the same value).
template <auto kernel>
hipError_t allow_lds() {
    static std::atomic<bool> set[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !set[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kPpLdsPerCu);
        if (e == hipSuccess && dev >= 0 && dev < 64) set[dev].store(true, std::memory_order_release);
    }
    return e;
}

hipError_t sweep_pp_impl(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                         uint32_t seed32, unsigned long long *keys, ms_result *results, uint32_t present, int num_cus,
                         hipStream_t s, int commit, hipEvent_t done, uint32_t pstride, ms_result_compact *resc,
                         const ms_pod_rec *pods2 = nullptr, uint32_t n_pods2 = 0, unsigned long long *keys2 = nullptr) {
    if (n_pods == 0 && n_pods2 == 0) return done ? hipEventRecord(done, s) : hipSuccess;
    // (two batches: shard sweeps into keys, one workgroup holding every row)
    const uint32_t n_all = n_pods + (pods2 ? n_pods2 : 0u);
    if (!t.planes) return hipErrorInvalidValue;
    const uint32_t n_groups = cdiv(n_rows, kGroupRows);
    // small shards with many pods: KW = 8, one single-wave workgroup per pod
    // chunk holds every row. It needs enough pods per wave to balance whole
    // waves over the SIMDs: 12.5k rows x 800k pods 347 vs 412 us, but x 100k
    // pods 58.8 vs 52.7 us (profiles/r03_pp_words_ab.txt): a line through the
    // two crosses near 160k pods, and a coalesced pair of 100k-pod batches
    // (200k) still ran faster at KW = 4 (53.5 vs 54.5 us per batch,
    // profiles/r04f_coalesce_probe.txt), so the form switches at 1024 pods per
    // CU. MINISCHED_PP_WORDS = 4 / 8 forces a form (A/B).
    const char *wenv = getenv("MINISCHED_PP_WORDS");
    const uint32_t cus_ = (uint32_t)(num_cus > 0 ? num_cus : 256);
    bool small = n_groups <= kPpSmallGroups && n_all >= 1024u * cus_ && !getenv("MINISCHED_PP_WAVES");
    if (wenv) small = n_groups <= kPpSmallGroups && atoi(wenv) == 8;
    const uint32_t KW = small ? (uint32_t)kPpWordsSmall : (uint32_t)kPpWords;
    const uint32_t waves_needed = std::max(1u, cdiv(n_groups, 64u * KW));
    // W a power of two (32 / W workgroups per CU fill all 8 wave slots per
    // SIMD; W = 7 leaves one idle and was 9% slower at 50k rows): large shards
    // 16-wave workgroups (the groups are dealt round-robin, so every wave holds
    // 3 or 4 words), shards of 257..2048 groups at least 4 waves
    // (profiles/r02c_ab.json, r02j_ab_shard_waves.jsonl)
    // Shards needing exactly 2 waves (257..512 groups) keep 2: with the fixed-slot
    // form's shorter words the 4-wave split (2, 2, 2, 1 words at 12.5k rows) paid the
    // per-8-pod reduction twice as often; the pipelined G = 8 step went 46.1 -> 43.9 us
    // (profiles/r04t_g8_w2.txt; the slot-search form was 53.7 -> 53.0, r04f).
    uint32_t W = 1;
    if (waves_needed == 2) W = 2;
    else if (waves_needed > 1)
        while (W < std::max(4u, waves_needed) && W < (uint32_t)kPpMaxWaves) W *= 2;
    if (const char *w = getenv("MINISCHED_PP_WAVES")) W = (uint32_t)std::min(16, std::max(1, atoi(w)));
    if (!keys) W = std::max(W, std::min<uint32_t>(kPpMaxWaves, waves_needed));  // no scratch: one workgroup per chunk
    const uint32_t gy = std::max(1u, cdiv(n_groups, W * 64u * KW));
    const uint32_t cus = (uint32_t)(num_cus > 0 ? num_cus : 256);
    // (multiples of 8: a wave takes pods 8 at a time, and a part-filled 8 costs
    // a full one -- exact chunks ran 11% slower at 25k rows, r02k_ab_chunk.txt)
    auto chunk_for = [&](uint32_t per_cu) {
        const uint32_t resident = std::max(1u, per_cu * cus / gy);
        return cdiv(cdiv(n_all, resident), 8) * 8;
    };
    uint32_t per_cu = std::max(1u, 32u / W);  // workgroups per CU the chunk is sized for
    uint32_t chunk = chunk_for(per_cu);       // one round at 32 waves per CU
    // Half as many workgroups (16 waves per CU, 4 per SIMD still saturate VALU
    // issue) while chunks stay modest: each workgroup's fixed costs (plane
    // loads, pod prologue, two barriers, epilogue) are paid half as often.
    // Config C 334 -> 324 us and 350 -> 341 us on two boxes; at 1M pods (chunks
    // near 2k) it was 1.3% slower, at 12.5k rows x 800k pods (784) 1.6% faster
    // (profiles/r02zb_ab_chunk_half.jsonl).
    if (32u / W > 1u && chunk_for(std::max(1u, 16u / W)) <= 1024u) {
        per_cu = std::max(1u, 16u / W);
        chunk = chunk_for(per_cu);
    }
    // (Chunks of <= 56 pods for <= 8-wave workgroups sped the shard sweep alone up,
    // 12.5k rows 44.3 -> 43.7 us, 25k 73.3 -> 71.0, 50k 133.0 -> 127.0, but slowed the
    // pipelined sharded step, whose collective and decode kernels then interleave with
    // a multi-round sweep: 74.6 -> 77.7 us at 25k, 136.3 -> 140 at 50k;
    // profiles/r04n_shard_shapes.txt, r04p_chunk56_probe.json. Not kept.)
    chunk = std::min(std::max(chunk, 8u), kPpMaxChunk);
    uint32_t nblk1 = cdiv(n_pods, chunk), xtra = 0;
    // Balanced split of a one-batch shard sweep (2- and 4-wave workgroups, one
    // round of 16 waves per CU): chunks rounded up to 8 leave some SIMDs a wave
    // short of others (12.5k rows x 100k pods: 1,786 workgroups of 56 pods over
    // 2,048 slots, 3.5 waves per SIMD, the busiest 4 x 56 pods). Instead every
    // slot gets a workgroup: `chunk` pods each, 8 more for the first `xtra`
    // (4 x 48.8 pods on the busiest SIMD): the shard sweep alone 42.0 -> 38.7 us
    // at G = 8, 71.5 -> 67.5 at G = 4 (profiles/r05r_balance_ab.txt).
    // A coalesced pair of equal batches splits the slots in halves, each balanced alike.
    if ((!pods2 || n_pods2 == n_pods) && gy == 1 && W <= 4u) {
        const uint32_t slots = (16u / W) * cus / (pods2 ? 2u : 1u);
        const uint32_t cb = (n_pods / slots) / 8u * 8u;
        if (cb >= 8u && cb + 8u <= kPpMaxChunk && n_pods > cb * slots) {
            const uint32_t nx = cdiv(n_pods - cb * slots, 8u);
            if (nx <= slots) {
                chunk = cb;
                xtra = nx;
                nblk1 = slots;
                per_cu = 16u / W;
            }
        }
    }
    const dim3 grid(nblk1 + (pods2 ? (xtra ? nblk1 : cdiv(n_pods2, chunk)) : 0u), gy);
    // the fixed-slot form for digit-aligned waves (profiles/r04j_fix_ab.txt)
    constexpr int fix_ok = 1;
    const PpJob2 j2 = {pods2, reinterpret_cast<u64 *>(keys2), n_pods2, nblk1};
    if (pods2 && (gy > 1 || results || resc || !keys || !keys2)) return hipErrorInvalidValue;
    if (gy > 1) {
        // several workgroups per chunk: combine keys with atomicMax, then decode
        // (done: an event record after the last of these launches)
        if (!keys || resc) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(keys, 0, sizeof(unsigned long long) * n_pods, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_sweep_nunn_pp<kPpWords, false, 0>), grid, dim3(64 * W),
                           chunk * (sizeof(u64) + sizeof(uint2)) + kPpSortWords * sizeof(uint32_t), s, t.planes,
                           t.gcap, n_groups, t.base, pods, n_pods, chunk, seed32, keys, 1, (ms_result *)nullptr, present,
                           t, 0, (uint32_t)sizeof(ms_pod_rec), (ms_result_compact *)nullptr, PpJob2{}, fix_ok, 0u,
                           (const uint32_t *)nullptr MS_TL_NONE);
        e = hipGetLastError();
        if (e == hipSuccess && results) e = launch_decode(pods, n_pods, keys, nullptr, present, results, s);
        if (e == hipSuccess && results && commit) e = launch_apply_binds(t, pods, n_pods, results, s);
        if (e == hipSuccess && done) e = hipEventRecord(done, s);
        return e;
    }
    // done: recorded by the dispatch itself (hipExtLaunchKernel's stop event: no
    // separate event packet between this sweep and the next launch on s)
    // the list form (as the kernel decides it) through the lane table where that fits
    const bool table = KW == (uint32_t)kPpWords && cand != nullptr && lane_table_fits(chunk, xtra, W, per_cu);
    const uint32_t lds = pp_lds_bytes(chunk + (xtra ? 8u : 0u), table ? (uint32_t)kPpLaneWords : 0u);
    unsigned long long *kk = (results || resc) ? nullptr : keys;
    const int cm = (results || resc) ? commit : 0;
    // (gy == 1: the workgroup holds every group; the 8-word form stays unpacked: its
    // packed instantiation needs 117 VGPRs, half the waves per SIMD it sizes for)
    const bool tp = KW == (uint32_t)kPpWords && tail_pods(n_groups, W) != 0u;
#ifdef MS_PP_TIMELINE
    // (diagnostic build, one launching thread: the buffer is kept between launches)
    static u64 *tl_dev = nullptr;
    static size_t tl_cap = 0;
    const size_t tl_n = (size_t)grid.x * kPpMaxWaves * kTlStamps;
    if (tl_n > tl_cap) {
        if (tl_dev) (void)hipFree(tl_dev);
        tl_dev = nullptr, tl_cap = 0;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&tl_dev), tl_n * sizeof(u64));
        if (e != hipSuccess) return e;
        tl_cap = tl_n;
    }
    {
        const hipError_t e = hipMemsetAsync(tl_dev, 0, tl_n * sizeof(u64), s);
        if (e != hipSuccess) return e;
    }
#endif
#define MS_PP_LAUNCH(KWV, TPV, LTV)                                                                                 \
    hipExtLaunchKernelGGL((k_sweep_nunn_pp<KWV, TPV, LTV>), grid, dim3(64 * W), lds, s, nullptr, done, 0, t.planes,   \
                          t.gcap, n_groups, t.base, pods, n_pods, chunk, seed32, kk, 0, results, present, t, cm, pstride, \
                          resc, j2, fix_ok, xtra, cand MS_TL_BUF)
    if (KW == (uint32_t)kPpWordsSmall) {
        MS_PP_LAUNCH(kPpWordsSmall, false, 0);
    } else if (table) {
        // (a table may pass the 64 KiB a kernel gets of dynamic LDS unasked)
        const hipError_t e = tp ? allow_lds<k_sweep_nunn_pp<kPpWords, true, kPpLaneWords>>()
                                : allow_lds<k_sweep_nunn_pp<kPpWords, false, kPpLaneWords>>();
        if (e != hipSuccess) return e;
        if (tp) MS_PP_LAUNCH(kPpWords, true, kPpLaneWords);
        else MS_PP_LAUNCH(kPpWords, false, kPpLaneWords);
    } else {
        if (tp) MS_PP_LAUNCH(kPpWords, true, 0);
        else MS_PP_LAUNCH(kPpWords, false, 0);
    }
#undef MS_PP_LAUNCH
#ifdef MS_PP_TIMELINE
    if (const char *path = getenv("MS_PP_TIMELINE")) {
        // one record per launch, appended: 8 header words, then grid.x x 16 x kTlStamps u64
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        std::vector<u64> host(tl_n);
        e = hipMemcpy(host.data(), tl_dev, tl_n * sizeof(u64), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        if (FILE *f = fopen(path, "ab")) {
            const uint32_t hdr[8] = {0x4C545050u /* "PPTL" */, 1u, grid.x, W, kTlStamps, chunk, n_pods, (uint32_t)kPpMaxWaves};
            fwrite(hdr, sizeof(hdr), 1, f);
            fwrite(host.data(), sizeof(u64), tl_n, f);
            fclose(f);
        }
    }
#endif
    return hipGetLastError();
}
}  // namespace

hipError_t launch_sweep_pp(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                           uint32_t seed32, unsigned long long *keys, ms_result *results, uint32_t present,
                           int num_cus, hipStream_t s, int commit, hipEvent_t done) {
    return sweep_pp_impl(t, cand, n_rows, pods, n_pods, seed32, keys, results, present, num_cus, s, commit, done,
                         (uint32_t)sizeof(ms_pod_rec), nullptr);
}

hipError_t launch_sweep_pp2(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_rec *pods1, uint32_t n1,
                            unsigned long long *keys1, const ms_pod_rec *pods2, uint32_t n2, unsigned long long *keys2,
                            uint32_t seed32, uint32_t present, int num_cus, hipStream_t s, hipEvent_t done) {
    if (n_rows > kPpMaxFusedRows) return hipErrorInvalidValue;
    return sweep_pp_impl(t, cand, n_rows, pods1, n1, seed32, keys1, nullptr, present, num_cus, s, 0, done,
                         (uint32_t)sizeof(ms_pod_rec), nullptr, pods2, n2, keys2);
}

hipError_t launch_sweep_pp_compact(const NodeTable &t, const uint32_t *cand, uint32_t n_rows, const ms_pod_compact *pods, uint32_t n_pods,
                                   uint32_t seed32, ms_result_compact *results, uint32_t present, int num_cus,
                                   hipStream_t s) {
    static_assert(sizeof(ms_pod_compact) == 8 && sizeof(ms_result_compact) == 8, "compact records");
    if (n_rows > kPpMaxFusedRows || !results) return hipErrorInvalidValue;
    return sweep_pp_impl(t, cand, n_rows, reinterpret_cast<const ms_pod_rec *>(pods), n_pods, seed32, nullptr, nullptr,
                         present, num_cus, s, 1, nullptr, (uint32_t)sizeof(ms_pod_compact), results);
}

}  // namespace msgpu

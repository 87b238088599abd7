// MS_PLUGINS_NU_NN_NAM scratch arithmetic: how a call is cut into chunks, the
// row segments of the per-class passes, where each scratch array starts, how
// much the context allocates, and where the node-shard inputs (after / m_in)
// sit. Host only, plain integers, no HIP: ms_affinity.hip and ms_cycle.cpp use
// this one copy, and tests/cpp/test_nam_layout.cpp sweeps it on the CPU.
//
// The rule the rest depends on: ONE NamPlan per call. The allocation is sized
// for the plan's layout, after / m_in are placed behind it, and every chunk of
// the call, the short last one included, is carved with that same layout.
// nam_layout is not monotone in cls_max (fewer classes give more, shorter row
// segments: segs = max(8, cdiv(128, cdiv(cls_max, 64))), seg_rows rounded to
// 64), so a layout of the chunk's own pod count can need MORE scratch than the
// full chunk's.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace msgpu {

constexpr uint32_t kNamSegBytes = 104;    // one rescale record (MS_NAM_SEG_BYTES, asserted in ms_affinity.hip)
constexpr uint32_t kNamDigits = 11;       // node name digit 0..9, 10 = none
constexpr uint32_t kNamSortCap = 65536;   // (class, digit) buckets the class sort takes (else batch order)
constexpr size_t kNamAlign = 256;         // every carved array starts on a multiple of this
// The per-class scores F take classes x rows bytes: chunks shrink so F stays
// within this (only with very many term sets; 64 sets at 50k rows: 130 classes, 6.5 MB).
constexpr size_t kNamFBudget = 512ull << 20;

inline uint32_t nam_cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
inline size_t nam_align(size_t bytes) { return (bytes + (kNamAlign - 1)) & ~(kNamAlign - 1); }

// Row segments and scratch shape of one call's per-class passes (cls_max = the
// most classes a chunk can hold: min(pods, 2 (n_sets + 1))).
struct NamLayout {
    uint32_t segs = 1, seg_rows = 64, fpitch = 64, cls_max = 1;
};

// Row segments for the per-class passes: enough (segment, class-block) waves to
// spread over the chip, 64-row multiples (F is written four rows per word and
// read sixteen per load; a segment never writes its neighbour's rows).
inline NamLayout nam_layout(uint32_t n_rows, uint32_t cls_max) {
    NamLayout L;
    const uint32_t blocks = std::max(1u, nam_cdiv(cls_max, 64u));
    // (per class and segment: rows / segs row steps, and up to segs compositions of
    // the later segments' 101-entry tables, so a few tens of segments)
    const uint32_t segs = std::min(32u, std::max(8u, nam_cdiv(128u, blocks)));
    L.seg_rows = std::max(64u, nam_cdiv(nam_cdiv(std::max(n_rows, 1u), segs), 64u) * 64u);
    L.segs = std::max(1u, nam_cdiv(std::max(n_rows, 1u), L.seg_rows));
    L.fpitch = nam_cdiv(std::max(n_rows, 1u), 64u) * 64u;
    L.cls_max = cls_max;
    return L;
}

// Byte offsets of a chunk's scratch arrays (n_pods pods under layout L), in
// carve order; end = the first byte past the last one.
struct NamCarve {
    size_t local, comp, F, dmask, fmax, used, ctl, cls_key, rep, pcls, perm, bcnt, bstart, end;
};

inline NamCarve nam_carve_offsets(const NamLayout &L, uint32_t n_pods, uint32_t n_sets) {
    NamCarve x;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += nam_align(bytes);
        return at;
    };
    x.local = take((size_t)L.segs * L.cls_max * kNamSegBytes);
    x.comp = take((size_t)L.cls_max * kNamSegBytes);
    x.F = take((size_t)L.cls_max * L.fpitch);
    x.dmask = take((size_t)kNamDigits * L.fpitch);
    x.fmax = take((size_t)L.cls_max * kNamDigits * 4);
    x.used = take(2ull * (n_sets + 1u) * 4);
    x.ctl = take(16 * 4);
    x.cls_key = take((size_t)L.cls_max * 4);
    x.rep = take((size_t)L.cls_max * 4);
    x.pcls = take((size_t)n_pods * 4);
    x.perm = take((size_t)n_pods * 4);
    const size_t nb = std::min<size_t>((size_t)L.cls_max * kNamDigits, kNamSortCap);
    x.bcnt = take(nb * 4);
    x.bstart = take(nb * 4);
    x.end = o;
    return x;
}

inline size_t nam_scratch_bytes(const NamLayout &L, uint32_t n_pods, uint32_t n_sets) {
    return nam_carve_offsets(L, n_pods, n_sets).end;
}

// Pods per chunk of a call of n_pods on a context of n_rows rows and n_sets
// term sets whose max_batch is batch_cap.
inline uint32_t nam_chunk_pods(uint32_t batch_cap, uint32_t n_rows, uint32_t n_sets, uint32_t n_pods) {
    uint32_t nb = std::min(batch_cap, n_pods);
    const size_t rows = std::max<uint32_t>(64u, n_rows);
    const uint32_t cls_sets = 2u * (n_sets + 1u);
    if ((size_t)std::min(nb, cls_sets) * rows > kNamFBudget)
        nb = std::max<uint32_t>(256u, (uint32_t)std::min<size_t>(nb, kNamFBudget / rows));
    return std::max(1u, nb);
}

// The most classes nb pods can fall into: (term set or none) x toleration.
inline uint32_t nam_class_cap(uint32_t nb, uint32_t n_sets) {
    return std::max(1u, std::min(nb, 2u * (n_sets + 1u)));
}

// Whether n_pods pods may be launched under L (launch_nam_segment / launch_nam_keys).
inline bool nam_launch_ok(const NamLayout &L, uint32_t n_pods, uint32_t n_sets) {
    return n_pods <= L.cls_max || L.cls_max >= 2u * (n_sets + 1u);
}

// One call's plan: chunks of `chunk` pods, ALL carved with L; behind L's scratch
// one record (the later shards' table) and one byte (an earlier shard has a
// non-zero node) per pod of a chunk; alloc = what the context must hold.
struct NamPlan {
    uint32_t chunk = 1;
    NamLayout L;
    size_t after = 0, m_in = 0, alloc = 0;
};

inline NamPlan nam_plan(uint32_t batch_cap, uint32_t n_rows, uint32_t n_sets, uint32_t n_pods) {
    NamPlan p;
    p.chunk = nam_chunk_pods(batch_cap, n_rows, n_sets, n_pods);
    p.L = nam_layout(n_rows, nam_class_cap(p.chunk, n_sets));
    const size_t scratch = nam_scratch_bytes(p.L, p.chunk, n_sets);
    p.after = nam_align(scratch);
    p.m_in = p.after + (size_t)p.chunk * kNamSegBytes;
    p.alloc = scratch + (size_t)p.chunk * (kNamSegBytes + 1) + 512;
    return p;
}

// The plan of a batch swept WHOLE, as ONE chunk (the in-library node-sharded
// cycle, ms_comm.cpp): chunk = n_pods and no kNamFBudget shrink, so how a batch
// is cut never depends on a rank's row count (an allocation too large fails as
// MS_E_OOM, like any other buffer). The shard inputs behind the scratch are per
// CLASS: C = nam_class_cap(n_pods, n_sets) records (after) and C bytes (m_in).
// C = L.cls_max is a function of (n_pods, n_sets) alone: every rank of a
// communicator computes the same C for a batch, which sizes its all-gather.
inline NamPlan nam_plan_whole(uint32_t n_rows, uint32_t n_sets, uint32_t n_pods) {
    NamPlan p;
    p.chunk = std::max(1u, n_pods);
    const uint32_t C = nam_class_cap(p.chunk, n_sets);
    p.L = nam_layout(n_rows, C);
    const size_t scratch = nam_scratch_bytes(p.L, p.chunk, n_sets);
    p.after = nam_align(scratch);
    p.m_in = p.after + (size_t)C * kNamSegBytes;
    p.alloc = p.m_in + C + 512;
    return p;
}

}  // namespace msgpu

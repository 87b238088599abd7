// ms_nam_device.h -- device-only: the pieces of MS_PLUGINS_NU_NN_NAM that more
// than one translation unit needs (ms_affinity.hip's per-class passes and
// ms_explain.hip's row view): the rescale record of a LIST-ordered row segment,
// a row's staged word, the term-table lookups for Score and Filter, and the
// 101-entry rescale tables with their exact multiply-high.
#pragma once

#include "ms_device.h"

namespace msgpu {

struct NamSeg {
    uint8_t T[101];  // the composed rescale map on 0..100
    uint8_t any;     // a feasible node of the segment has a non-zero raw score
    // the segment's filter bits (the FitError mask): [0] a present row failed
    // NodeUnschedulable, [1] a present row passed it and failed NodeAffinity
    uint8_t _pad[2];
};

// Row word staged in LDS: bit 0 absent, bit 1 unschedulable, zone << 8,
// label2 << 16, digit << 24 (15 = none).
__device__ __forceinline__ uint32_t nam_row_word(const NodeTable &t, uint32_t r) {
    const uint8_t f = t.flags[r];
    const uint32_t d = t.digit[r];
    return ((f & kNodeAbsent) ? 1u : 0u) | ((f & kNodeUnschedulable) ? 2u : 0u) | ((uint32_t)t.zone[r] << 8) |
           ((uint32_t)t.label2[r] << 16) | ((d <= 9u ? d : 15u) << 24);
}

// The row-word bits that rule a row out for a class under NodeUnschedulable:
// absent, and unschedulable unless the class tolerates it.
__device__ __forceinline__ uint32_t nam_nu_bits(uint32_t tol) { return tol ? 1u : 3u; }

// NodeAffinity of a row word under a term table in LDS, one lookup for Score and
// Filter: the terms whose two id sets hold the row's zone and label2 ids, bits 0-3
// the preferred terms, bits 4-7 the required ones (a set without a requirement
// has bit 4 on every value id; a lane without a class has an all-zero table).
__device__ __forceinline__ uint32_t nam_terms(uint32_t w, const uint8_t *tab) {
    return tab[(w >> 8) & 0xFFu] & tab[256u + ((w >> 16) & 0xFFu)];
}
// NodeAffinity.Score: the weight sum of the matching preferred terms.
__device__ __forceinline__ uint32_t nam_raw(uint32_t m, const uint8_t *tab) {
    return reinterpret_cast<const uint16_t *>(tab + 512)[m & 15u];
}
// Both filters in one compare: feasible = no NodeUnschedulable bit of the row
// under nu (nam_nu_bits) and a required term matched (m > 15). m < 256, so any
// bit of w & nu lifts the bound past it. The key orders the rows the same way:
// below 16 exactly for a row that passes NodeUnschedulable and fails NodeAffinity.
__device__ __forceinline__ uint32_t nam_filter_key(uint32_t w, uint32_t nu, uint32_t m) { return ((w & nu) << 8) | m; }
__device__ __forceinline__ bool nam_feasible(uint32_t w, uint32_t nu, uint32_t m) { return m > (((w & nu) << 8) | 15u); }

// The identity map in a lane's LDS table.
__device__ __forceinline__ void table_identity(uint8_t *row) {
    for (uint32_t v = 0; v <= 100u; v += 4u) {
        const uint32_t x = v | (v + 1u) << 8 | (v + 2u) << 16 | (v + 3u) << 24;
        *reinterpret_cast<uint32_t *>(row + v) = x;
    }
}

// floor(100 v / r) for v <= 100 (r > 100) as a multiply-high by m = floor((2^32 - 1) / r) + 1
// (one division per rescale, not per entry): m exceeds 2^32 / r by at most 1, so the
// product overshoots 100 v / r by at most 10^4 / 2^32 < 1 / r, less than the gap from any
// fraction k / r (k < r) to the next integer: the floor is exact.
__device__ __forceinline__ uint32_t div_magic(uint32_t r) { return 0xFFFFFFFFu / r + 1u; }
__device__ __forceinline__ uint32_t f_r(uint32_t v, uint32_t m) { return __umulhi(100u * v, m); }

// f_r o T on table `row` (every lane of the wave: entries lane, lane + 64).
__device__ __forceinline__ void table_post(uint8_t *row, uint32_t r, uint32_t lane) {
    const uint32_t m = div_magic(r);
    for (uint32_t v = lane; v <= 100u; v += 64u) row[v] = (uint8_t)f_r(row[v], m);
}

}  // namespace msgpu

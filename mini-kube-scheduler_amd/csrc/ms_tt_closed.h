// ms_tt_closed.h -- device-only: the pieces of MS_PLUGINS_NU_TT_NN's closed form
// that more than one translation unit needs (ms_taint.hip's two-pass cycle and
// ms_explain.hip's row view): one step of the in-loop reverse normalise, the
// census record of a LIST-ordered row segment and its associative merge.
#pragma once

#include "ms_device.h"

namespace msgpu {

__device__ __forceinline__ int32_t tt_map(int32_t m, int32_t v) { return m == 0 ? 100 : 100 - (100 * v) / m; }

constexpr uint32_t kEntNone = 0xFFFFFFFFu;

struct TtCensus {  // 32 B per (segment, pod)
    uint32_t n, flags;
    uint32_t occ, occ1;  // bit 2c + q: a middle row of class (c, q) / one matching NodeNumber
    uint32_t first[3], last;  // entries: ordinal | nn << 21 | c << 24 (kEntNone: none)
};
static_assert(sizeof(TtCensus) == MS_TT_CENSUS_BYTES, "TtCensus layout (ms_tt_census_device)");

__device__ __forceinline__ uint32_t ent_pack(uint32_t row, uint32_t c, uint32_t nn) { return row | nn << 21 | c << 24; }
__device__ __forceinline__ uint32_t ent_row(uint32_t e) { return e & 0x1FFFFFu; }
__device__ __forceinline__ uint32_t ent_nn(uint32_t e) { return (e >> 21) & 1u; }
__device__ __forceinline__ uint32_t ent_cc(uint32_t e) { return (e >> 24) & 0xFu; }

__device__ __forceinline__ uint32_t swap_parity(uint32_t occ) {  // 18 class bits: 2c <-> 2c + 1
    return ((occ & 0x15555u) << 1) | ((occ >> 1) & 0x15555u);
}

// r <- r merged with b (b follows r in LIST order), occupancy form of tt_merge_into.
__device__ __forceinline__ void tt2_merge(TtCensus &r, const TtCensus &b) {
    const uint32_t an = r.n, alast = r.last;
    r.n = an + b.n;
    r.flags |= b.flags;
    const bool sh = (an & 1u) != 0;
    r.occ |= sh ? swap_parity(b.occ) : b.occ;
    r.occ1 |= sh ? swap_parity(b.occ1) : b.occ1;
    auto place = [&](uint32_t e, uint32_t g) {
        if (g == 0u) r.first[0] = e;
        if (g == 1u) r.first[1] = e;
        if (g == 2u) r.first[2] = e;
        if (g + 1u == r.n) r.last = e;
        if (g >= 3u && g + 1u < r.n) {
            const uint32_t k = 1u << (2u * ent_cc(e) + (g & 1u));
            r.occ |= k;
            if (ent_nn(e)) r.occ1 |= k;
        }
    };
    if (an > 3u) place(alast, an - 1u);
    if (b.n > 0u) place(b.first[0], an);
    if (b.n > 1u) place(b.first[1], an + 1u);
    if (b.n > 2u) place(b.first[2], an + 2u);
    if (b.n > 3u) place(b.last, an + b.n - 1u);
    if (b.n == 0u) r.last = alast;
}

}  // namespace msgpu

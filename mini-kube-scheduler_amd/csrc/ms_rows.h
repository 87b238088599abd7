// ms_rows.h -- device-only: one node row and one pod of MS_PLUGINS_NU_NRF_NN_LA as
// the resource-aware kernels evaluate them, shared by the batched sweep
// (ms_kernels.hip) and the exact sequential engine (ms_seq.hip): the general
// int64/f32 form (FullRow, PodFull, eval_full) and the binary64 fast form
// (DRow / FastRow, PodFast, eval_fast), each with its loaders.
#pragma once

#include "ms_device.h"

namespace msgpu {

// ----------------------------------------------------------------------------
// K3: NodeUnschedulable + NodeResourcesFit filters, NodeNumber + LeastAllocated
// scores (upstream v1.22 semantics restated in oracle/ms_oracle.c).
// ----------------------------------------------------------------------------
// LeastAllocated (k8s@v1.22.0 least_allocated.go leastRequestedScore) per
// resource: capacity 0 or requested > capacity -> 0, else
// floor((capacity - requested) * 100 / capacity), requested = NonZeroRequested
// + the pod's non-zero request n. With av = capacity - NonZeroRequested and
// d = av - n, the f32 estimate x = (f32(av) - f32(n)) * f32(100/capacity) is
// within 4e-5 of q = 100 d / capacity whenever 0 <= d (then n <= av <= capacity:
// every operand's rounding is relative to at most capacity). So with
// m = round(x), floor(q) is m or m - 1, and ONE exact int64 comparison
// 100 d >= m * capacity decides it. 100 d = a100 - n100 with a100 = 100 av per
// node and n100 = 100 min(n, 2^55) per pod; valid (d >= 0) <=> 100 d >= 0.
// Rows with capacity >= 2^53 (beyond any real allocatable) hold av in the a100
// field and take plain int64 arithmetic (kHuge, chosen per wave).
constexpr int64_t kHugeCap = 1ll << 53;

struct FullRow {
    int64_t fr_cpu, fr_mem;      // Allocatable - Requested          (NodeResourcesFit)
    int64_t a100_cpu, a100_mem;  // 100 (Allocatable - NonZeroRequested); av itself when huge
    int64_t cap_cpu, cap_mem;    // Allocatable
    float avf_cpu, avf_mem;      // f32(Allocatable - NonZeroRequested)
    float r_cpu, r_mem;          // f32(100 / Allocatable), 0 when Allocatable == 0
    int32_t room;                // AllowedPodNumber - len(Pods)
    uint32_t fd;                 // flags | digit << 8
};

__device__ __forceinline__ float r100(int64_t cap) { return cap > 0 ? 100.0f / (float)cap : 0.0f; }

__device__ __forceinline__ FullRow make_row(int64_t alloc_cpu, int64_t alloc_mem, int64_t req_cpu, int64_t req_mem,
                                            int64_t nz_cpu, int64_t nz_mem, int32_t room, uint32_t fd) {
    FullRow x;
    x.cap_cpu = alloc_cpu;
    x.cap_mem = alloc_mem;
    x.fr_cpu = alloc_cpu - req_cpu;
    x.fr_mem = alloc_mem - req_mem;
    const int64_t av_cpu = alloc_cpu - nz_cpu, av_mem = alloc_mem - nz_mem;
    x.a100_cpu = alloc_cpu >= kHugeCap ? av_cpu : av_cpu * 100;
    x.a100_mem = alloc_mem >= kHugeCap ? av_mem : av_mem * 100;
    x.avf_cpu = (float)av_cpu;
    x.avf_mem = (float)av_mem;
    x.r_cpu = r100(alloc_cpu);
    x.r_mem = r100(alloc_mem);
    x.room = room;
    x.fd = fd;
    return x;
}

__device__ __forceinline__ FullRow load_row(const NodeTable &t, uint32_t r, uint32_t n_rows) {
    if (r >= n_rows) return make_row(0, 0, 0, 0, 0, 0, 0, kNodeAbsent | (0xFFu << 8));
    return make_row(t.alloc_cpu[r], t.alloc_mem[r], t.req_cpu[r], t.req_mem[r], t.nz_cpu[r], t.nz_mem[r],
                    t.allowed_pods[r] - t.pod_count[r], (uint32_t)t.flags[r] | ((uint32_t)t.digit[r] << 8));
}

template <bool kHuge = true>
__device__ __forceinline__ int64_t least_requested(int64_t a100, float avf, int64_t cap, float r, int64_t n,
                                                   int64_t n100, float nf) {
    if (kHuge && cap >= kHugeCap) {  // a100 holds av
        const int64_t d = a100 - n;
        return (a100 < n) ? 0 : (int64_t)((uint64_t)d * 100u) / cap;
    }
    const uint32_t m = (uint32_t)__builtin_fmaf(avf - nf, r, 0.5f);  // round(x); x < 0 -> 0
    const int64_t d100 = a100 - n100;
    const uint32_t lo = (uint32_t)cap, hi = (uint32_t)((uint64_t)cap >> 32);
    const uint64_t mc = (uint64_t)m * lo + ((uint64_t)(m * hi) << 32);  // m * capacity (< 2^60)
    const uint32_t q = m - (d100 < (int64_t)mc ? 1u : 0u);
    return d100 >= 0 ? (int64_t)q : 0;
}

struct PodFull {
    int64_t rc, rm, nc, nm;   // requests (Fit) and non-zero requests (LeastAllocated)
    int64_t n100c, n100m;     // 100 min(nonzero, 2^55)
    float nfc, nfm;           // f32(nonzero)
    int dig;
    bool tol;
    bool zero_req;
    uint32_t A;
};

__device__ __forceinline__ PodFull load_pod(const ms_pod_rec &pr, uint32_t seed32) {
    PodFull q;
    q.rc = pr.req_milli_cpu;
    q.rm = pr.req_memory;
    q.nc = pr.nonzero_milli_cpu;
    q.nm = pr.nonzero_memory;
    // (both operands int64_t: min(long, long long) resolves to the mixed-type overload that
    // compares AND returns binary64, and the product then rounds to 53 bits once n > 2^53 / 100)
    constexpr int64_t kN100Max = (int64_t)1 << 55;
    q.n100c = (q.nc < kN100Max ? q.nc : kN100Max) * 100;
    q.n100m = (q.nm < kN100Max ? q.nm : kN100Max) * 100;
    q.nfc = (float)q.nc;
    q.nfm = (float)q.nm;
    q.dig = pr.name_digit;
    q.tol = pr.tolerates_unschedulable != 0;
    q.zero_req = (q.rc == 0 && q.rm == 0);
    q.A = tb_pod(seed32, pr.ordinal);
    return q;
}

__device__ __forceinline__ int64_t readlane_i64(int64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), (int)l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Sweeps hold up to 64 pods lane-resident (one parallel load, no per-pod
// memory round trip) and broadcast pod i with readlanes.
struct PodLanes {
    PodFull q;
};

__device__ __forceinline__ PodLanes stage_pods(const ms_pod_rec *__restrict__ pods, uint32_t g, uint32_t cnt,
                                               uint32_t lane, uint32_t seed32) {
    PodLanes m;
    ms_pod_rec z = {};
    m.q = load_pod(lane < cnt ? pods[g + lane] : z, seed32);
    return m;
}

__device__ __forceinline__ PodFull pod_of_lane(const PodLanes &m, uint32_t i) {
    PodFull q;
    q.rc = readlane_i64(m.q.rc, i);
    q.rm = readlane_i64(m.q.rm, i);
    q.nc = readlane_i64(m.q.nc, i);
    q.nm = readlane_i64(m.q.nm, i);
    q.n100c = readlane_i64(m.q.n100c, i);
    q.n100m = readlane_i64(m.q.n100m, i);
    q.nfc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m.q.nfc), (int)i));
    q.nfm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m.q.nfm), (int)i));
    q.A = (uint32_t)__builtin_amdgcn_readlane((int)m.q.A, (int)i);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane(
        (int)(((uint32_t)m.q.dig & 0xFFu) | (m.q.tol ? 0x100u : 0u) | (m.q.zero_req ? 0x200u : 0u)), (int)i);
    q.dig = (int)(int8_t)(b & 0xFFu);
    q.tol = (b & 0x100u) != 0;
    q.zero_req = (b & 0x200u) != 0;
    return q;
}

// Evaluates one (pod,node) pair: returns the packed key (0 when filtered out)
// and sets the first-failing filter plugin (minisched.go:130-137 breaks on
// the first failure, so a node rejected by NU is never charged to NRF).
template <bool kHuge = true>
__device__ __forceinline__ u64 eval_full(const FullRow &x, uint32_t ord, const PodFull &q,
                                         uint32_t &nu, uint32_t &nrf) {
    const uint32_t fl = x.fd & 0xFFu;
    const bool absent = (fl & kNodeAbsent) != 0;
    const bool f_nu = !absent && (fl & kNodeUnschedulable) != 0 && !q.tol;
    bool bad = x.room < 1;  // len(Pods)+1 > AllowedPodNumber
    if (!q.zero_req) bad = bad || (q.rc > x.fr_cpu) || (q.rm > x.fr_mem);
    const bool f_nrf = !absent && !f_nu && bad;
    nu = f_nu ? 1u : 0u;
    nrf = f_nrf ? 1u : 0u;
    const int64_t s_cpu = least_requested<kHuge>(x.a100_cpu, x.avf_cpu, x.cap_cpu, x.r_cpu, q.nc, q.n100c, q.nfc);
    const int64_t s_mem = least_requested<kHuge>(x.a100_mem, x.avf_mem, x.cap_mem, x.r_mem, q.nm, q.n100m, q.nfm);
    const uint32_t nn = ((int)(x.fd >> 8) == q.dig) ? 10u : 0u;
    const uint32_t la = (uint32_t)((s_cpu + s_mem) / 2);
    const u64 key = make_key(nn + la, tb_hash(q.A, ord), ord);
    return (absent || f_nu || bad) ? 0ull : key;
}

// Whether any of the wave's rows needs the int64 LeastAllocated path.
__device__ __forceinline__ bool rows_huge(const FullRow *x) {
    bool h = false;
#pragma unroll
    for (int s = 0; s < kFullSlots; ++s) h = h || x[s].cap_cpu >= kHugeCap || x[s].cap_mem >= kHugeCap;
    return __ballot(h) != 0;
}

// ---- binary64 LeastAllocated (the config-E sweep's fast form) --------------
// floor(100 (av - n) / cap) as ONE fma + a saturating conversion per resource:
//   r = RN(100 / cap), a = RN(RN(av * r) + 2^-43), x = RN(-n * r + a) (fma),
//   score = x <= 0 ? 0 : trunc(x)                               (v_cvt_u32_f64)
// |x - (X + 2^-43)| <= 402 u (u = 2^-53) for X = 100 (av - n) / cap <= 100, so
// trunc(x) = floor(X) whenever 2^-43 > 402 u and 2^-43 + 402 u < 1 / cap, i.e.
// for 0 < cap < 2^41 (cap <= 0: r = 0, score 0 as leastRequestedScore gives);
// negative X (requested > capacity) lands below 0 and saturates to 0.
// Exact by the bound and by tests/c/la_f64_exact.c (boundary cases around every
// k * cap / 100; the window of working epsilons is 2^-46 .. 2^-42). Needs
// NonZeroRequested >= 0 (av <= cap) and 0 <= pod non-zero request < 2^53; a
// wave whose rows or pods fall outside takes the general path (eval_full).
constexpr int64_t kFastCap = 1ll << 41;
constexpr int64_t kFastReq = 1ll << 53;
constexpr double kLaEps = 0x1p-43;

typedef DRow FastRow;  // (ms_internal.h)

__device__ __forceinline__ double la_r(int64_t cap) { return cap > 0 ? __ddiv_rn(100.0, (double)cap) : 0.0; }

__device__ __forceinline__ double la_a(int64_t cap, int64_t nz, double r) {
    const int64_t av = (int64_t)((uint64_t)cap - (uint64_t)nz);  // (wraps only where r == 0 or av < 0 anyway)
    return __dadd_rn(__dmul_rn((double)av, r), kLaEps);
}

__device__ __forceinline__ DRow make_drow(int64_t ac, int64_t am, int64_t rqc, int64_t rqm, int64_t zc, int64_t zm,
                                          int32_t room, uint32_t fd) {
    DRow x;
    x.fr_cpu = (int64_t)((uint64_t)ac - (uint64_t)rqc);
    x.fr_mem = (int64_t)((uint64_t)am - (uint64_t)rqm);
    x.r_cpu = la_r(ac);
    x.r_mem = la_r(am);
    x.a_cpu = la_a(ac, zc, x.r_cpu);
    x.a_mem = la_a(am, zm, x.r_mem);
    x.room = room;
    x.fd = fd;
    x.digit = fd >> 8;
    const bool absent = (fd & kNodeAbsent) != 0;
    const bool unsched = !absent && (fd & kNodeUnschedulable);
    x.rbits = (absent ? kRbAbsent : 0u) | (unsched ? kRbUnsched : 0u) | (absent || unsched ? kRbBlocked : 0u) |
              (!absent && room < 1 ? kRbNoRoom : 0u) |
              ((ac < kFastCap && am < kFastCap && zc >= 0 && zm >= 0) ? 0u : kRbSlow);
    return x;
}

__device__ __forceinline__ DRow absent_drow() {
    DRow x;
    x.fr_cpu = x.fr_mem = 0;
    x.r_cpu = x.r_mem = x.a_cpu = x.a_mem = 0.0;
    x.room = 0;
    x.fd = kNodeAbsent | (0xFFu << 8);
    x.digit = 0xFFu;
    x.rbits = kRbAbsent | kRbBlocked;
    return x;
}

__device__ __forceinline__ FastRow load_fast_row(const NodeTable &t, uint32_t r, uint32_t n_rows) {
    if (r >= n_rows) return absent_drow();
    return make_drow(t.alloc_cpu[r], t.alloc_mem[r], t.req_cpu[r], t.req_mem[r], t.nz_cpu[r], t.nz_mem[r],
                     t.allowed_pods[r] - t.pod_count[r], (uint32_t)t.flags[r] | ((uint32_t)t.digit[r] << 8));
}

struct PodFast {
    int64_t rc, rm;    // requests (Fit)
    double nnc, nnm;   // -(double) non-zero requests (LeastAllocated)
    uint32_t A;
    uint32_t bits;     // digit (9 bits, sign-extended) | kPfTol | kPfZero | kPfOk
    uint32_t rej;      // DRow::rbits that reject the pod statically: absent, no room, unschedulable unless tolerated
    uint32_t cand;     // DRow::rbits that exclude a rejection from NodeResourcesFit: absent, NU-rejected
};
constexpr uint32_t kPfTol = 0x200u, kPfZero = 0x400u, kPfOk = 0x800u;

__device__ __forceinline__ PodFast load_pod_fast(const ms_pod_rec &pr, uint32_t seed32) {
    PodFast q;
    q.rc = pr.req_milli_cpu;
    q.rm = pr.req_memory;
    q.nnc = -(double)pr.nonzero_milli_cpu;
    q.nnm = -(double)pr.nonzero_memory;
    q.A = tb_pod(seed32, pr.ordinal);
    const bool ok = pr.nonzero_milli_cpu >= 0 && pr.nonzero_milli_cpu < kFastReq && pr.nonzero_memory >= 0 &&
                    pr.nonzero_memory < kFastReq;
    // the digit as 9 bits: a negative (non-digit) name never equals a node's digit byte
    q.bits = ((uint32_t)(int32_t)pr.name_digit & 0x1FFu) | (pr.tolerates_unschedulable ? kPfTol : 0u) |
             ((pr.req_milli_cpu == 0 && pr.req_memory == 0) ? kPfZero : 0u) | (ok ? kPfOk : 0u);
    q.cand = kRbAbsent | (pr.tolerates_unschedulable ? 0u : kRbUnsched);
    q.rej = q.cand | kRbNoRoom;
    return q;
}

__device__ __forceinline__ double readlane_f64(double v, uint32_t l) {
    return __longlong_as_double(readlane_i64(__double_as_longlong(v), l));
}

__device__ __forceinline__ PodFast pod_fast_of_lane(const PodFast &m, uint32_t i) {
    PodFast q;
    q.rc = readlane_i64(m.rc, i);
    q.rm = readlane_i64(m.rm, i);
    q.nnc = readlane_f64(m.nnc, i);
    q.nnm = readlane_f64(m.nnm, i);
    q.A = (uint32_t)__builtin_amdgcn_readlane((int)m.A, (int)i);
    q.bits = (uint32_t)__builtin_amdgcn_readlane((int)m.bits, (int)i);
    q.rej = (uint32_t)__builtin_amdgcn_readlane((int)m.rej, (int)i);
    q.cand = (uint32_t)__builtin_amdgcn_readlane((int)m.cand, (int)i);
    return q;
}

__device__ __forceinline__ uint32_t cvt_u32_sat(double x) {  // negatives -> 0
    uint32_t q;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(q) : "v"(x));
    return q;
}

// eval_full's key and first-failure flags through the binary64 LeastAllocated.
__device__ __forceinline__ u64 eval_fast(const FastRow &x, uint32_t ord, const PodFast &q, uint32_t &nu,
                                         uint32_t &nrf) {
    const uint32_t rb = x.rbits;
    const bool absent = (rb & kRbAbsent) != 0;
    const bool f_nu = (rb & kRbUnsched) != 0 && !(q.bits & kPfTol);
    bool bad = (rb & kRbNoRoom) != 0;
    if (!(q.bits & kPfZero)) bad = bad || (q.rc > x.fr_cpu) || (q.rm > x.fr_mem);
    const bool f_nrf = !absent && !f_nu && bad;
    nu = f_nu ? 1u : 0u;
    nrf = f_nrf ? 1u : 0u;
    const uint32_t s_cpu = cvt_u32_sat(__builtin_fma(q.nnc, x.r_cpu, x.a_cpu));
    const uint32_t s_mem = cvt_u32_sat(__builtin_fma(q.nnm, x.r_mem, x.a_mem));
    const uint32_t nn = (x.digit == (q.bits & 0x1FFu)) ? 10u : 0u;
    const u64 key = make_key(nn + ((s_cpu + s_mem) >> 1), tb_hash(q.A, ord), ord);
    return (absent || f_nu || bad) ? 0ull : key;
}

}  // namespace msgpu

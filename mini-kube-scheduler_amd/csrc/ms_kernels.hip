// ms_kernels.hip -- gfx950 kernels of minisched's scheduling cycle outside the
// fused NU+NN cycle (ms_sweep_pp.hip), the TaintToleration and NodeAffinity
// term-set cycles (ms_taint.hip, ms_affinity.hip) and the exact sequential
// engine (ms_seq.hip): node table maintenance (init, deltas, binds, read-back),
// the batched resource-aware sweep (k_sweep_full), the NodeAffinity
// preferred-zone sweep (k_sweep_na), the decodes of packed keys into results,
// the compact record conversions and the derived rows of the sequential
// engine's table copy (k_build_drows).
//
// Reference path (all in minisched/minisched.go of the project this one follows):
//   RunFilterPlugins :115-151 -> NodeUnschedulable.Filter (k8s@v1.22.0, restated)
//   RunScorePlugins  :164-199 -> NodeNumber.Score (plugins/score/nodenumber/nodenumber.go:73-95)
//   unweighted sum   :187-196
//   selectHost       :304-325 (tie-break replaced by the packed key, see minisched_gpu.h)
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "ms_rows.h"

namespace msgpu {

namespace {

__global__ void k_build_drows(NodeTable t, uint32_t n_rows, uint32_t n_total) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_total) t.drow[r] = load_fast_row(t, r, n_rows);
}

// Batched resource-aware sweep: atomicMax into keys[P] / atomicOr into flags[P].
__global__ __launch_bounds__(kFullThreads) void k_sweep_full(NodeTable t, uint32_t n_rows,
                                                             const ms_pod_rec *__restrict__ pods, uint32_t n_pods,
                                                             uint32_t chunk, uint32_t seed32, u64 *__restrict__ keys,
                                                             uint32_t *__restrict__ pflags) {
    const uint32_t lane = lane_id();
    const uint32_t row0 = blockIdx.x * kFullTile + threadIdx.x * kFullSlots;
    FullRow x[kFullSlots];
#pragma unroll
    for (int s = 0; s < kFullSlots; ++s) x[s] = load_row(t, row0 + s, n_rows);
    const uint32_t ord0 = t.base + row0;
    const bool huge = rows_huge(x);
    const uint32_t pbeg = blockIdx.y * chunk;
    const uint32_t pend = min(n_pods, pbeg + chunk);
    for (uint32_t g = pbeg; g < pend; g += 64) {
        const uint32_t cnt = min(64u, pend - g);
        const PodLanes m = stage_pods(pods, g, cnt, lane, seed32);
        u64 mine = 0;
        uint32_t myflag = 0;
        for (uint32_t i = 0; i < cnt; ++i) {
            const PodFull q = pod_of_lane(m, i);
            u64 best = 0;
            uint32_t nu_any = 0, nrf_any = 0;
#pragma unroll
            for (int s = 0; s < kFullSlots; ++s) {
                uint32_t nu, nrf;
                best = umax64(best, huge ? eval_full<true>(x[s], ord0 + s, q, nu, nrf)
                                         : eval_full<false>(x[s], ord0 + s, q, nu, nrf));
                nu_any |= nu;
                nrf_any |= nrf;
            }
            best = wave_max_u64(best);
            const uint32_t f = (__ballot(nu_any != 0) ? 1u : 0u) | (__ballot(nrf_any != 0) ? 0x100u : 0u);
            if (lane == i) {
                mine = best;
                myflag = f;
            }
        }
        if (lane < cnt) {
            if (mine) atomicMax(&keys[g + lane], mine);
            if (myflag) atomicOr(&pflags[g + lane], myflag);
        }
    }
}

// ----------------------------------------------------------------------------
// decode / bind commit / deltas
// ----------------------------------------------------------------------------
__device__ __forceinline__ void decode_one(const ms_pod_rec *__restrict__ pods, const u64 *__restrict__ keys,
                                           const uint32_t *__restrict__ flags, uint32_t present,
                                           ms_result *__restrict__ out, uint32_t i) {
    out[i] = decode_key(keys[i], pods[i].name_digit, flags, i, present);
}

// present_dev (optional): the present count as the node-sharded combine left
// it on the device (non-zero iff some shard lists a node), instead of present.
__global__ void k_decode(const ms_pod_rec *__restrict__ pods, uint32_t n_pods, const u64 *__restrict__ keys,
                         const uint32_t *__restrict__ flags, uint32_t present, const uint32_t *__restrict__ present_dev,
                         ms_result *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pods) decode_one(pods, keys, flags, present_dev ? *present_dev : present, out, i);
}

// Several batches' decodes in one launch (grid.y = job): the grouped drain of
// the pipelined multi-GPU step decodes its batches together.
struct DecodeJobs {
    ms_decode_job j[MS_DECODE_MAX_JOBS];
};

__global__ void k_decode_jobs(DecodeJobs jobs, uint32_t present) {
    const ms_decode_job &jb = jobs.j[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < jb.n_pods)
        decode_one(jb.pods, reinterpret_cast<const u64 *>(jb.keys), jb.flags, present, jb.results, i);
}

// The in-library node-sharded drain: several batches' pod slices, each with
// its own device-side present flag (ms_comm.cpp).
struct SliceJobs {
    SliceJob j[kMaxSliceJobs];
};

__global__ void k_decode_slices(SliceJobs jobs) {
    const SliceJob &jb = jobs.j[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < jb.n_pods) decode_one(jb.pods, jb.keys, jb.flags, jb.present ? *jb.present : 0u, jb.results, i);
}

__global__ void k_fill_keys(u64 *__restrict__ keys, uint32_t n, u64 v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = v;
}

__global__ void k_pods_widen(const ms_pod_compact *__restrict__ in, uint32_t n, ms_pod_rec *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2 v = *reinterpret_cast<const uint2 *>(in + i);  // = the first 8 bytes of ms_pod_rec
    uint2 *o = reinterpret_cast<uint2 *>(out + i);
    o[0] = v;
    o[1] = o[2] = o[3] = o[4] = make_uint2(0u, 0u);
}

__global__ void k_results_narrow(const ms_result *__restrict__ in, uint32_t n, ms_result_compact *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ms_result r = in[i];
    ms_result_compact c;
    c.node = r.node;
    c.score = (uint16_t)r.score;
    c.code = (uint8_t)r.code;
    c.plugin_mask = (uint8_t)r.plugin_mask;
    out[i] = c;
}

__global__ void k_apply_binds(NodeTable t, const ms_pod_rec *__restrict__ pods, uint32_t n_pods,
                              const ms_result *__restrict__ res) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pods) return;
    const ms_result r = res[i];
    if (r.code != MS_CODE_SUCCESS || r.node < 0) return;
    const uint32_t node = (uint32_t)r.node;
    if (node < t.base || node - t.base >= t.cap) return;  // another shard owns it
    add_pod(t, node - t.base, pods[i], +1);
}

__global__ void k_bind_one(NodeTable t, uint32_t row, const ms_pod_rec *pod, int sign) {
    if (threadIdx.x == 0 && blockIdx.x == 0) add_pod(t, row, *pod, sign);
}

__global__ void k_apply_deltas(NodeTable t, const NodeDelta *__restrict__ d, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NodeDelta x = d[i];
    const uint32_t r = x.local;
    if (x.absent) {
        t.flags[r] = kNodeAbsent;
        t.digit[r] = 0xFF;
        t.zone[r] = 0;
        t.label2[r] = 0;
        t.taints[r] = 0;
        t.allowed_pods[r] = 0;
        t.pod_count[r] = 0;
        t.alloc_cpu[r] = t.alloc_mem[r] = 0;
        t.req_cpu[r] = t.req_mem[r] = 0;
        t.nz_cpu[r] = t.nz_mem[r] = 0;
        return;
    }
    t.flags[r] = x.rec.unschedulable ? kNodeUnschedulable : 0;
    t.digit[r] = x.rec.name_digit <= 9 ? x.rec.name_digit : 0xFF;
    t.zone[r] = x.rec.zone;
    t.label2[r] = x.rec.label2;
    t.taints[r] = x.rec.taints & 0xFFFFu;
    t.allowed_pods[r] = x.rec.allowed_pods;
    t.pod_count[r] = x.rec.pod_count;
    t.alloc_cpu[r] = x.rec.alloc_milli_cpu;
    t.alloc_mem[r] = x.rec.alloc_memory;
    t.req_cpu[r] = x.rec.req_milli_cpu;
    t.req_mem[r] = x.rec.req_memory;
    t.nz_cpu[r] = x.rec.nonzero_milli_cpu;
    t.nz_mem[r] = x.rec.nonzero_memory;
}

__global__ void k_init_table(NodeTable t) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= t.cap) return;
    t.flags[r] = kNodeAbsent;
    t.digit[r] = 0xFF;
    t.zone[r] = 0;
    t.label2[r] = 0;
    t.taints[r] = 0;
    t.allowed_pods[r] = 0;
    t.pod_count[r] = 0;
    t.alloc_cpu[r] = t.alloc_mem[r] = 0;
    t.req_cpu[r] = t.req_mem[r] = 0;
    t.nz_cpu[r] = t.nz_mem[r] = 0;
}

__global__ void k_read_rows(NodeTable t, uint32_t first, uint32_t n, ms_node_rec *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = first + i;
    ms_node_rec x = {};
    const uint8_t f = t.flags[r];
    x.unschedulable = (f & kNodeUnschedulable) ? 1 : 0;
    x.name_digit = t.digit[r];
    x.zone = t.zone[r];
    x.label2 = t.label2[r];
    x.taints = t.taints[r];
    x.allowed_pods = (f & kNodeAbsent) ? -1 : t.allowed_pods[r];
    x.pod_count = t.pod_count[r];
    x.alloc_milli_cpu = t.alloc_cpu[r];
    x.alloc_memory = t.alloc_mem[r];
    x.req_milli_cpu = t.req_cpu[r];
    x.req_memory = t.req_mem[r];
    x.nonzero_milli_cpu = t.nz_cpu[r];
    x.nonzero_memory = t.nz_mem[r];
    out[i] = x;
}

// ----------------------------------------------------------------------------
// MS_PLUGINS_NU_NN_NA: Filter[NU]; Score[NodeNumber, NodeAffinity preferred term]
// with NodeAffinity's DefaultNormalizeScore(100, reverse=false) run by
// RunScorePlugins after every node on the whole, partially filled list
// (minisched.go:164-185). For raw scores <= 100 that in-loop hook leaves every
// entry at its raw score except the first feasible node in LIST order with a
// non-zero raw score (the anchor), which ends at 100: after the first non-zero
// entry the list maximum is 100 and every later normalisation is the
// identity (oracle/ms_oracle.c msor_schedule_na checks the closed form against
// the loop as written). So per pod the sweep keeps (a) the max packed key with
// raw NodeAffinity scores and (b) the anchor as a min-ordinal reduction; the
// decode takes max(a, key of the anchor scored w_nn*NN + w_na*100). The
// anchor's raw key never beats its boosted key, so including it in (a) is
// harmless. One pair per lane-slot, plain per-pair evaluation.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(kNunnThreads) void k_sweep_na(
    const uint8_t *__restrict__ nflags, const uint8_t *__restrict__ ndigit, const uint8_t *__restrict__ nzone,
    uint32_t n_rows, uint32_t node_base, const ms_pod_rec *__restrict__ pods, uint32_t n_pods, uint32_t chunk,
    uint32_t seed32, uint32_t w_nn, uint32_t w_na, u64 *__restrict__ keys, uint32_t *__restrict__ fkeys) {
    const uint32_t row0 = blockIdx.x * kNunnTile + threadIdx.x * kNunnSlots;
    uint8_t fl[kNunnSlots], dg[kNunnSlots], zn[kNunnSlots];
#pragma unroll
    for (int i = 0; i < kNunnSlots; ++i) {
        const uint32_t r = row0 + i;
        fl[i] = r < n_rows ? nflags[r] : kNodeAbsent;
        dg[i] = r < n_rows ? ndigit[r] : 0xFF;
        zn[i] = r < n_rows ? nzone[r] : 0;
    }
    const uint32_t pbeg = blockIdx.y * chunk;
    const uint32_t pend = min(n_pods, pbeg + chunk);
    for (uint32_t p = pbeg; p < pend; ++p) {
        const ms_pod_rec pr = pods[p];  // wave-uniform
        const uint32_t A = tb_pod(seed32, pr.ordinal);
        u64 best = 0;
        uint32_t anchor = 0;
#pragma unroll
        for (int i = 0; i < kNunnSlots; ++i) {
            const bool feas = !(fl[i] & kNodeAbsent) && !((fl[i] & kNodeUnschedulable) && !pr.tolerates_unschedulable);
            const uint32_t ord = node_base + row0 + i;
            const uint32_t nn = ((int)dg[i] == (int)pr.name_digit) ? 1u : 0u;
            const uint32_t raw = (pr.pref_zone != 0 && zn[i] == pr.pref_zone) ? pr.pref_weight : 0u;
            const u64 key = make_key(w_nn * 10u * nn + w_na * raw, tb_hash(A, ord), ord);
            best = feas ? umax64(best, key) : best;
            const uint32_t a = (((0xFFFFFu - ord) << 1) | nn) + 1u;
            anchor = (feas && raw) ? max(anchor, a) : anchor;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            best = umax64(best, __shfl_xor(best, off, 64));
            anchor = max(anchor, (uint32_t)__shfl_xor(anchor, off, 64));
        }
        if ((threadIdx.x & 63u) == 0u) {
            if (best) atomicMax(&keys[p], best);
            if (anchor) atomicMax(&fkeys[p], anchor);
        }
    }
}

__global__ void k_decode_na(const ms_pod_rec *__restrict__ pods, uint32_t n_pods, const u64 *__restrict__ keys,
                            const uint32_t *__restrict__ fkeys, uint32_t present, const uint32_t *__restrict__ present_dev,
                            uint32_t seed32, uint32_t w_nn, uint32_t w_na, ms_result *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pods) return;
    u64 k = keys[i];
    const uint32_t a = fkeys[i];
    if (a) {  // the normalise anchor, scored w_nn * NN + w_na * 100
        const uint32_t ord = 0xFFFFFu - ((a - 1u) >> 1), nn = (a - 1u) & 1u;
        k = umax64(k, make_key(w_nn * 10u * nn + w_na * 100u, tb_hash(tb_pod(seed32, pods[i].ordinal), ord), ord));
    }
    out[i] = decode_key(k, pods[i].name_digit, nullptr, 0, present_dev ? *present_dev : present);
}

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// pods per chunk: enough blocks to fill the chip twice over, multiple of 64
inline uint32_t pod_chunk(uint32_t n_pods, uint32_t node_blocks, int num_cus) {
    const uint32_t target = (uint32_t)(num_cus > 0 ? num_cus : 256) * 8u * 2u;
    uint32_t chunks = cdiv(target, node_blocks > 0 ? node_blocks : 1);
    chunks = chunks < 1 ? 1 : chunks;
    const uint32_t max_chunks = cdiv(n_pods, 64);
    if (chunks > max_chunks) chunks = max_chunks;
    uint32_t c = cdiv(n_pods, chunks);
    return cdiv(c, 64) * 64;
}

}  // namespace


hipError_t launch_sweep_na(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                           uint32_t seed32, uint32_t w_nn, uint32_t w_na, unsigned long long *keys, uint32_t *fkeys,
                           int num_cus, hipStream_t s) {
    if (n_pods == 0 || n_rows == 0) return hipSuccess;
    const uint32_t gx = cdiv(n_rows, kNunnTile);
    const uint32_t chunk = pod_chunk(n_pods, gx, num_cus);
    hipLaunchKernelGGL(k_sweep_na, dim3(gx, cdiv(n_pods, chunk)), dim3(kNunnThreads), 0, s, t.flags, t.digit, t.zone,
                       n_rows, t.base, pods, n_pods, chunk, seed32, w_nn, w_na, keys, fkeys);
    return hipGetLastError();
}

hipError_t launch_decode_na(const ms_pod_rec *pods, uint32_t n_pods, const unsigned long long *keys,
                            const uint32_t *fkeys, uint32_t present_nodes, uint32_t seed32, uint32_t w_nn,
                            uint32_t w_na, ms_result *out, hipStream_t s, const uint32_t *present_dev) {
    if (n_pods == 0) return hipSuccess;
    hipLaunchKernelGGL(k_decode_na, dim3(cdiv(n_pods, 256)), dim3(256), 0, s, pods, n_pods, keys, fkeys,
                       present_nodes, present_dev, seed32, w_nn, w_na, out);
    return hipGetLastError();
}

hipError_t launch_sweep_full(const NodeTable &t, uint32_t n_rows, const ms_pod_rec *pods, uint32_t n_pods,
                             uint32_t seed32, unsigned long long *keys, uint32_t *flags, int num_cus,
                             hipStream_t s) {
    if (n_pods == 0 || n_rows == 0) return hipSuccess;
    const uint32_t gx = cdiv(n_rows, kFullTile);
    const uint32_t chunk = pod_chunk(n_pods, gx, num_cus);
    const dim3 grid(gx, cdiv(n_pods, chunk));
    hipLaunchKernelGGL(k_sweep_full, grid, dim3(kFullThreads), 0, s, t, n_rows, pods, n_pods, chunk, seed32, keys,
                       flags);
    return hipGetLastError();
}

hipError_t launch_build_drows(const NodeTable &t, uint32_t n_rows, uint32_t n_total, hipStream_t s) {
    if (!t.drow || n_total == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_build_drows, dim3(cdiv(n_total, 256)), dim3(256), 0, s, t, n_rows, n_total);
    return hipGetLastError();
}

hipError_t launch_decode(const ms_pod_rec *pods, uint32_t n_pods, const unsigned long long *keys,
                         const uint32_t *flags, uint32_t present_nodes, ms_result *out, hipStream_t s,
                         const uint32_t *present_dev) {
    if (n_pods == 0) return hipSuccess;
    hipLaunchKernelGGL(k_decode, dim3(cdiv(n_pods, 256)), dim3(256), 0, s, pods, n_pods, keys, flags,
                       present_nodes, present_dev, out);
    return hipGetLastError();
}

hipError_t launch_decode_slices(const SliceJob *jobs, uint32_t n_jobs, hipStream_t s) {
    if (n_jobs == 0 || n_jobs > kMaxSliceJobs) return n_jobs ? hipErrorInvalidValue : hipSuccess;
    SliceJobs sj = {};
    uint32_t most = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        sj.j[i] = jobs[i];
        most = std::max(most, jobs[i].n_pods);
    }
    if (most == 0) return hipSuccess;
    hipLaunchKernelGGL(k_decode_slices, dim3(cdiv(most, 256), n_jobs), dim3(256), 0, s, sj);
    return hipGetLastError();
}

hipError_t launch_decode_jobs(const ms_decode_job *jobs, uint32_t n_jobs, uint32_t present_nodes, hipStream_t s) {
    DecodeJobs dj = {};
    uint32_t most = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj.j[i] = jobs[i];
        most = std::max(most, jobs[i].n_pods);
    }
    if (most == 0) return hipSuccess;
    hipLaunchKernelGGL(k_decode_jobs, dim3(cdiv(most, 256), n_jobs), dim3(256), 0, s, dj, present_nodes);
    return hipGetLastError();
}

hipError_t launch_apply_binds(const NodeTable &t, const ms_pod_rec *pods, uint32_t n_pods, const ms_result *res,
                              hipStream_t s) {
    if (n_pods == 0) return hipSuccess;
    hipLaunchKernelGGL(k_apply_binds, dim3(cdiv(n_pods, 256)), dim3(256), 0, s, t, pods, n_pods, res);
    return hipGetLastError();
}

hipError_t launch_fill_keys(unsigned long long *keys, uint32_t n, unsigned long long v, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fill_keys, dim3(cdiv(n, 256)), dim3(256), 0, s, reinterpret_cast<u64 *>(keys), n, (u64)v);
    return hipGetLastError();
}

hipError_t launch_pods_widen(const ms_pod_compact *in, uint32_t n, ms_pod_rec *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pods_widen, dim3(cdiv(n, 256)), dim3(256), 0, s, in, n, out);
    return hipGetLastError();
}

hipError_t launch_results_narrow(const ms_result *in, uint32_t n, ms_result_compact *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_results_narrow, dim3(cdiv(n, 256)), dim3(256), 0, s, in, n, out);
    return hipGetLastError();
}

hipError_t launch_bind_one(const NodeTable &t, uint32_t local, const ms_pod_rec *pod_dev, int sign,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_bind_one, dim3(1), dim3(64), 0, s, t, local, pod_dev, sign);
    return hipGetLastError();
}

hipError_t launch_apply_deltas(const NodeTable &t, const NodeDelta *d_deltas, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_apply_deltas, dim3(cdiv(n, 256)), dim3(256), 0, s, t, d_deltas, n);
    return hipGetLastError();
}

hipError_t launch_init_table(const NodeTable &t, hipStream_t s) {
    if (t.cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_table, dim3(cdiv(t.cap, 256)), dim3(256), 0, s, t);
    return hipGetLastError();
}

hipError_t launch_read_rows(const NodeTable &t, uint32_t first, uint32_t n, ms_node_rec *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_read_rows, dim3(cdiv(n, 256)), dim3(256), 0, s, t, first, n, out);
    return hipGetLastError();
}

}  // namespace msgpu

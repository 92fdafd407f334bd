// fit_preempt_k.hip — which victims to evict so that a multi-node job fits: fit_preempt's question for
// a job that needs `need` distinct nodes at once (include/fitgpu.h fit_preempt_k; DESIGN.md §2m,
// §3.21).  State, eligibility, the counters and the key of a (job, node) pair are fit_preempt's
// (fit_pre_row.h); the picks are the `need` smallest keys.  gfx950.
//
// fit_preempt's launches in the query frame (fit_query.h), the minimum replaced by a selection:
//   k_prek_classify : per job, the partition-limit code, a zeroed row with its `need`, the job's
//                     component, out_node = -1 and out_victims = 0 in all kmax entries
//   k_prek_walk<K>  : k_pre_walk with a sorted list of the K smallest keys per lane in registers, K the
//                     power of two at or above kmax.  An offered key goes through a fully unrolled
//                     compare-exchange chain, and only when a ballot finds a lane whose offer is below
//                     its worst kept key: after the first rows almost none is.  The eight waves' lists
//                     are folded pairwise through LDS in three rounds (waves 4-7 into 0-3, 2-3 into
//                     0-1, 1 into 0), each a bitonic merge of two sorted lists that keeps the K
//                     smallest; the buffer holds four waves' lists, not eight, and first serves the
//                     counters' sums.  One list of kmax 16-byte keys per (job position, node slice),
//                     disjoint stores.
//   k_prek_final<K> : merges a job's slices the same way, then the row, out_node and out_victims.
// Integer sums and the K smallest of distinct keys do not depend on the order: exact and
// reproducible.  No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.  A batch
// above PRE_CHUNK jobs takes the walk and the final per chunk of positions, so the lists stay bounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "fit_device.h"
#include "fit_pre_row.h"
#include "fit_pre_top.h"
#include "fit_query.h"

namespace fitgpu {

// EvictKRow, the keys' order and PreTop<K> are fit_pre_top.h's: fit_preempt_tl_k's walk shares them.
// k_prek_walk's fold stays spelled out below: as a call of the header's prek_fold, which says the
// same, the compiler allocated this kernel's registers differently.

__global__ __launch_bounds__(256) void k_prek_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const uint16_t* __restrict__ jk,
    int32_t kmax, int32_t nj, const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np,
    int32_t ncomp, EvictKRow* __restrict__ out, int32_t* __restrict__ out_node, int32_t* __restrict__ out_vic,
    int8_t* __restrict__ jcomp, int32_t* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    int comp = lim.comp >= 0 && lim.comp < ncomp ? lim.comp : -1;
    if (c < 0 || m < 0 || g < 0 || w < 0 || max(jk ? (int32_t)jk[q] : 1, 1) > kmax) {  // the whole call fails
        comp = -1;
        atomicOr(bad, 1);
    }
    // a row without a component is final here: a limit code, or no node carries the partition's bit
    EvictKRow r;
    r.code = lim.code != LIM_NONE ? lim.code : (comp < 0 ? (int)PRE_NO_NODES : (int)PRE_FITS);
    r.need = tl_need(jk, q, kmax);
    r.evict_nodes = r.victims = r.top_prio = r.reserved = 0;
#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) r.cnt[i] = 0;
    out[q] = r;
    for (int i = 0; i < kmax; ++i) {
        out_node[(size_t)q * kmax + i] = -1;
        out_vic[(size_t)q * kmax + i] = 0;
    }
    jcomp[q] = (int8_t)comp;
}

// grid (job tiles of the chunk, node slices); jl / live: fit_query.h's job list.  The chunk is the
// positions [t0, t0 + nt); part: nt * gridDim.y lists of kmax keys, position-major.  K = 8 asks for
// six waves per SIMD: 80 VGPRs instead of 81, three workgroups per CU instead of two, no spill.
template <int K>
__global__ __launch_bounds__(PRE_WAVES * 64, K == 8 ? 6 : 1) void k_prek_walk(
    const NodeRec* __restrict__ rec, const int32_t* __restrict__ voff, const VicEnt* __restrict__ vent, ExplainComps C,
    const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t nj, int32_t t0, int32_t nt, int32_t kmax,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int32_t* __restrict__ jprio,
    const int8_t* __restrict__ jcomp, EvictKRow* __restrict__ out, PreKey* __restrict__ part) {
    // four waves' lists, [wave][key][hi, lo][lane]; before that the eight waves' counters
    constexpr int KEY_WORDS = (PRE_WAVES / 2) * K * 2 * PRE_JOBS;
    constexpr int CNT_WORDS = PRE_WAVES * PRE_NCNT * PRE_JOBS / 2;
    __shared__ uint64_t sm[KEY_WORDS > CNT_WORDS ? KEY_WORDS : CNT_WORDS];
    __shared__ int32_t qs[PRE_JOBS];
    const int nlive = min(query_live(jl, live, nj), t0 + nt);
    const int tb = t0 + (int)blockIdx.x * PRE_JOBS;
    if (tb >= nlive) return;  // block-uniform: k_prek_final reads no position at or behind nlive
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int q = query_job(tb + lane, nlive, jl, nj);
    const int comp = q >= 0 ? (int)jcomp[q] : -1;
    const bool on = comp >= 0 && comp < C.ncomp;
    PreJob j;
    j.cpu = on ? jcpu[q] : 0;
    j.mem = on ? jmem[q] : 0;
    j.gpu = on ? jgpu[q] : 0;
    j.wall = on ? jwall[q] : 0;
    j.prio = on ? jprio[q] : 0;
    const uint32_t pbit = on ? 1u << (jpart[q] & 31) : 0u;
    int32_t n[PRE_NCNT];
#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) n[i] = 0;
    PreTop<K> top;
    top.clear();

    QueryWalk w = query_walk(on);
    while (w.rem) {  // wave-uniform: one pass per distinct component
        const QueryRange r = query_next<PRE_WAVES>(w, C, comp, on, wave);
        const uint32_t pb = r.mine ? pbit : 0u;
        int x = r.n0;
        for (; x + 4 <= r.n1; x += 4) {  // four scalar row loads per wait, as k_scan
            NodeRec r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = rec[x + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) pre_row(r[u], x + u, pb, j, voff, vent, n, top);
        }
        for (; x < r.n1; ++x) pre_row(rec[x], x, pb, j, voff, vent, n, top);
    }

    // the counters: thread (i, l) sums counter i of job-lane l over the waves, one atomic per
    // workgroup, job and counter, none for a zero
    int32_t* red = reinterpret_cast<int32_t*>(sm);  // [wave][counter][lane]
#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) red[(wave * PRE_NCNT + i) * PRE_JOBS + lane] = n[i];
    if (wave == 0) qs[lane] = on ? q : -1;
    __syncthreads();
    if (threadIdx.x < PRE_NCNT * PRE_JOBS) {
        const int i = threadIdx.x / PRE_JOBS, l = threadIdx.x - i * PRE_JOBS;
        int32_t v = 0;
#pragma unroll
        for (int w = 0; w < PRE_WAVES; ++w) v += red[(w * PRE_NCNT + i) * PRE_JOBS + l];
        const int jq = qs[l];
        if (jq >= 0 && v != 0) atomicAdd(&out[jq].cnt[i], v);
    }
    // the lists: waves [h, 2h) hand theirs to waves [0, h), h = 4, 2, 1
#pragma unroll
    for (int h = PRE_WAVES / 2; h >= 1; h /= 2) {
        __syncthreads();  // the buffer's readers of the round before (the counters' the first time) are done
        if (wave >= h && wave < 2 * h) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                sm[(((wave - h) * K + i) * 2 + 0) * PRE_JOBS + lane] = top.k[i].hi;
                sm[(((wave - h) * K + i) * 2 + 1) * PRE_JOBS + lane] = top.k[i].lo;
            }
        }
        __syncthreads();
        if (wave < h) {
            PreKey b[K];
#pragma unroll
            for (int i = 0; i < K; ++i)
                b[i] = {sm[((wave * K + i) * 2 + 0) * PRE_JOBS + lane], sm[((wave * K + i) * 2 + 1) * PRE_JOBS + lane]};
            top.merge(b);
        }
    }
    // this slice's list: every position of the tile inside the chunk, live or not, so none is left
    // unwritten
    const int t = tb - t0 + lane;
    if (wave == 0 && t < nt) {
        PreKey* dst = part + ((size_t)t * gridDim.y + blockIdx.y) * kmax;
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (i < kmax) dst[i] = top.k[i];
    }
}

// One thread per position of the chunk: the job's slices merged, the row and its picks written.
template <int K>
__global__ __launch_bounds__(256) void k_prek_final(const int32_t* __restrict__ jl, const int32_t* __restrict__ live,
                                                    int32_t nj, int32_t t0, int32_t nt, int32_t ncomp, int slices,
                                                    int32_t kmax, const int8_t* __restrict__ jcomp,
                                                    const PreKey* __restrict__ part, EvictKRow* __restrict__ out,
                                                    int32_t* __restrict__ out_node, int32_t* __restrict__ out_vic) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int q = query_job(t0 + t, jl, live, nj);
    if (q < 0) return;
    const int comp = jcomp[q];
    if (comp < 0 || comp >= ncomp) return;  // final since k_prek_classify
    PreTop<K> top;
    top.clear();
    for (int s = 0; s < slices; ++s) {
        const PreKey* src = part + ((size_t)t * slices + s) * kmax;
        PreKey b[K];
        b[0] = src[0];
        // a slice's list is sorted: nothing of it enters when its first key does not
        if (!prek_less(b[0].hi, b[0].lo, top.k[K - 1].hi, top.k[K - 1].lo)) continue;
#pragma unroll
        for (int i = 1; i < K; ++i) b[i] = i < kmax ? src[i] : PreKey{PRE_NOKEY, PRE_NOKEY};
        top.merge(b);
    }
    EvictKRow r = out[q];
    const int members = r.cnt[0], fit = r.cnt[1], able = r.cnt[2], need = r.need;
    // fit + able <= members <= 2^29 rows: no overflow
    const bool pick = members > 0 && fit + able >= need;
    int32_t evn = 0, vic = 0, tp = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        if (pick && i < need) {
            const int32_t v = (int32_t)(uint32_t)top.k[i].hi;  // 0: the node fits now (hi == 0)
            out_node[(size_t)q * kmax + i] = (int32_t)(uint32_t)top.k[i].lo;
            out_vic[(size_t)q * kmax + i] = v;
            evn += v > 0;
            vic += v;
            // the keys ascend in top: the last evicting pick has the largest
            tp = v > 0 ? (int32_t)((uint32_t)(top.k[i].hi >> 32) ^ 0x80000000u) : tp;
        }
    }
    r.evict_nodes = evn;
    r.victims = vic;
    r.top_prio = tp;
    r.code = members == 0 ? PRE_NO_NODES : (fit >= need ? PRE_FITS : (fit + able >= need ? PRE_EVICT : PRE_NONE));
    out[q] = r;
}

// The rows on stream st in two calls, the caller ordering the jobs by component in between: `out` (nj
// rows of 40 B), out_node / out_vic (nj * kmax each) and *bad (1: a negative demand or nodes_k above
// kmax) are valid when the stream has drained.
hipError_t launch_preempt_k_classify(hipStream_t st, const int32_t* ptab, int32_t np, int ncomp, const int32_t* jcpu,
                                     const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                     const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t nj, void* out,
                                     int32_t* out_node, int32_t* out_vic, int8_t* jcomp, int32_t* bad) {
    if (kmax < 1 || kmax > FIT_KMAX) return hipErrorInvalidValue;
    return launch_per_job(st, nj, k_prek_classify, jcpu, jmem, jgpu, jwall, jpart, jk, kmax, nj, ptab, np,
                          (int32_t)ncomp, static_cast<EvictKRow*>(out), out_node, out_vic, jcomp, bad);
}

// The lists a batch of nj jobs needs (16-byte words of `part`): a chunk's positions x its slices
// (preempt_slices) x kmax.
size_t preempt_k_partials(int32_t nj, int slices, int32_t kmax) { return preempt_partials(nj, slices) * (size_t)kmax; }

namespace {
template <int K>
hipError_t launch_prek(hipStream_t st, const NodeRec* rec, const int32_t* voff, const VicEnt* vent,
                       const ExplainComps& C, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                       const int32_t* jwall, const uint16_t* jpart, const int32_t* jprio, int32_t kmax, int32_t nj,
                       const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, PreKey* p, EvictKRow* o,
                       int32_t* out_node, int32_t* out_vic) {
    for (int32_t t0 = 0; t0 < nj; t0 += PRE_CHUNK) {
        const int32_t nt = std::min<int32_t>(nj - t0, PRE_CHUNK);
        hipLaunchKernelGGL(k_prek_walk<K>, dim3((nt + PRE_JOBS - 1) / PRE_JOBS, slices), dim3(PRE_WAVES * 64), 0, st,
                           rec, voff, vent, C, jl, live, nj, t0, nt, kmax, jcpu, jmem, jgpu, jwall, jpart, jprio, jcomp,
                           o, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_prek_final<K>, dim3((nt + 255) / 256), dim3(256), 0, st, jl, live, nj, t0, nt,
                           (int32_t)C.ncomp, slices, kmax, jcomp, p, o, out_node, out_vic);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

// Walk and finalise, a chunk of PRE_CHUNK positions after the other; the stream orders their use of
// the one scratch.  jl / live as launch_explain's; slices: preempt_slices; part: preempt_k_partials.
hipError_t launch_preempt_k(hipStream_t st, const NodeRec* rec, const int32_t* voff, const VicEnt* vent,
                            const ExplainComps& C, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                            const int32_t* jwall, const uint16_t* jpart, const int32_t* jprio, int32_t kmax,
                            int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                            void* part, void* out, int32_t* out_node, int32_t* out_vic) {
    if (nj <= 0 || C.ncomp == 0) return hipSuccess;  // no component: every row is final since the classifier
    if (C.ncomp < 0 || C.ncomp > 32 || slices < 1 || slices > 65535 || kmax < 1 || kmax > FIT_KMAX)
        return hipErrorInvalidValue;
    EvictKRow* o = static_cast<EvictKRow*>(out);
    PreKey* p = static_cast<PreKey*>(part);
#define PREK_ARGS \
    st, rec, voff, vent, C, jcpu, jmem, jgpu, jwall, jpart, jprio, kmax, nj, jcomp, jl, live, slices, p, o, out_node, out_vic
    if (kmax == 1) return launch_prek<1>(PREK_ARGS);
    if (kmax == 2) return launch_prek<2>(PREK_ARGS);
    if (kmax <= 4) return launch_prek<4>(PREK_ARGS);
    return launch_prek<8>(PREK_ARGS);
#undef PREK_ARGS
}

namespace {
template <int K>
hipError_t launch_prek_final(hipStream_t st, const int32_t* jl, const int32_t* live, int32_t nj, int32_t t0, int32_t nt,
                             int ncomp, int slices, int32_t kmax, const int8_t* jcomp, const PreKey* p, EvictKRow* o,
                             int32_t* out_node, int32_t* out_vic) {
    hipLaunchKernelGGL(k_prek_final<K>, dim3((nt + 255) / 256), dim3(256), 0, st, jl, live, nj, t0, nt, (int32_t)ncomp,
                       slices, kmax, jcomp, p, o, out_node, out_vic);
    return hipGetLastError();
}
}  // namespace

// k_prek_final<K> for the positions [t0, t0 + nt) of a `_k` walk's lists (fit_preempt_tl_k.hip's walk
// ends in it too), K the power of two at or above kmax
hipError_t launch_preempt_k_final(hipStream_t st, const int32_t* jl, const int32_t* live, int32_t nj, int32_t t0,
                                  int32_t nt, int ncomp, int slices, int32_t kmax, const int8_t* jcomp,
                                  const void* part, void* out, int32_t* out_node, int32_t* out_vic) {
    if (nt <= 0) return hipSuccess;
    if (ncomp < 0 || ncomp > 32 || slices < 1 || kmax < 1 || kmax > FIT_KMAX) return hipErrorInvalidValue;
    const PreKey* p = static_cast<const PreKey*>(part);
    EvictKRow* o = static_cast<EvictKRow*>(out);
#define PREKF_ARGS st, jl, live, nj, t0, nt, ncomp, slices, kmax, jcomp, p, o, out_node, out_vic
    if (kmax == 1) return launch_prek_final<1>(PREKF_ARGS);
    if (kmax == 2) return launch_prek_final<2>(PREKF_ARGS);
    if (kmax <= 4) return launch_prek_final<4>(PREKF_ARGS);
    return launch_prek_final<8>(PREKF_ARGS);
#undef PREKF_ARGS
}

}  // namespace fitgpu

// fit_preempt.hip — which running jobs to evict so that a pending job fits: per job, the member
// nodes that fit now, those a prefix of lower-priority victims frees, those only jobs of equal or
// higher priority hold, and the node kube-scheduler's DefaultPreemption would pick (include/fitgpu.h
// fit_preempt).  gfx950.
//
// The victims (fit_load_victims) live in row order: row x of the NodeRec table owns the entries
// [voff[x], voff[x + 1]) of `vent`, in eviction order.  An entry is 16 bytes: the victim's priority
// and the INCLUSIVE prefix sums of the three amounts over the row's entries up to it, saturated at
// INT32_MAX.  free >= 0 and demand <= INT32_MAX make `free + min(S, INT32_MAX) >= demand` what the
// exact 64-bit sum gives, and min(free + S, INT32_MAX) is the same either way.
//
// fit_room's three bounded launches, in the query frame (fit_query.h):
//   k_pre_classify : per job, the partition-limit code, a zeroed row, the job's component
//   k_pre_walk     : every live job × every row of its component.  Lanes = jobs, rows wave-uniform
//                    (scalar loads of a NodeRec, four per wait), grid.y = explain_slices().  Only when
//                    a lane of the wave is eligible and short on a row whose whole list would free
//                    enough does the wave walk that row's entries (scalar 16-byte loads, four per
//                    wait); a lane stops at its first fit (able) or at the first entry it does not
//                    outrank (outranked), the loop when a ballot finds no lane looking.  The four
//                    counters are summed over the 8 waves through LDS: one integer atomicAdd per
//                    (workgroup, job, non-zero counter).  The 128-bit key (top, v, score, node id) has
//                    no atomic: the waves' minima are folded lexicographically in LDS and stored as
//                    one 16-byte partial per (job position, node slice) — disjoint stores.
//   k_pre_final    : folds a job's slices and sets node / victims / top_prio and the code.
// Integer sums and a lexicographic minimum do not depend on the order: exact and reproducible.  No
// cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.  A batch above PRE_CHUNK
// jobs takes the walk and the final per chunk of positions, so the partials stay bounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "fit_device.h"
#include "fit_pre_row.h"
#include "fit_query.h"

namespace fitgpu {

// fit_evict as the kernels see it (include/fitgpu.h)
struct alignas(32) EvictRow {
    int32_t code, node, victims, top_prio, cnt[PRE_NCNT];
};
static_assert(sizeof(EvictRow) == 32 && offsetof(EvictRow, cnt) == 16, "fit_evict is 32 bytes, its counters at 16");

// The walk's sink of offered keys (fit_pre_row.h): one lexicographic minimum per lane
struct PreMin {
    PreKey k;
    __device__ __forceinline__ void offer(bool has, uint64_t hi, uint64_t lo) { pre_min(k, has, hi, lo); }
};

// ---- fit_load_victims ---------------------------------------------------------------------------
// One thread per caller's node: its offsets, then — only when they lie in order inside [0, nvic], so
// a bad offset reads nothing out of bounds — its entries.  *bad |= 1 on any violation; nothing else
// is written.
__global__ __launch_bounds__(256) void k_vic_check(const int32_t* __restrict__ off, int32_t n, int64_t nvic,
                                                   const int32_t* __restrict__ prio, const int32_t* __restrict__ cpu,
                                                   const int32_t* __restrict__ mem, const int32_t* __restrict__ gpu,
                                                   int32_t* __restrict__ bad) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0) {
        if (x == 0 && (off[0] != 0 || nvic != 0)) atomicOr(bad, 1);
        return;
    }
    if (x >= n) return;
    const int64_t a = off[x], b = off[x + 1];
    bool err = a < 0 || b < a || b > nvic || (x == 0 && a != 0) || (x == n - 1 && b != nvic);
    if (!err)
        for (int64_t k = a; k < b; ++k) {
            err |= cpu[k] < 0 || mem[k] < 0 || gpu[k] < 0;
            err |= k > a && prio[k] < prio[k - 1];
        }
    if (err) atomicOr(bad, 1);
}

// One thread per row: the row's entries with their saturated prefix sums.  off: the caller's CSR
// (validated), voff: the row-ordered offsets (host-built from it).
__global__ __launch_bounds__(256) void k_vic_build(const int32_t* __restrict__ off, const int32_t* __restrict__ prio,
                                                   const int32_t* __restrict__ cpu, const int32_t* __restrict__ mem,
                                                   const int32_t* __restrict__ gpu, const int32_t* __restrict__ perm,
                                                   int32_t nn, const int32_t* __restrict__ voff,
                                                   VicEnt* __restrict__ vent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn) return;
    const int x = perm[i];
    const int a = off[x], len = off[x + 1] - a, d = voff[i];
    uint32_t sc = 0, sm = 0, sg = 0;
    for (int k = 0; k < len; ++k) {  // amounts are in [0, 2^31): a 32-bit sum of two saturated terms cannot wrap
        sc = min(sc + (uint32_t)cpu[a + k], PRE_SAT);
        sm = min(sm + (uint32_t)mem[a + k], PRE_SAT);
        sg = min(sg + (uint32_t)gpu[a + k], PRE_SAT);
        VicEnt e;
        e.prio = prio[a + k];
        e.cpu = (int32_t)sc;
        e.mem = (int32_t)sm;
        e.gpu = (int32_t)sg;
        vent[d + k] = e;
    }
}

hipError_t launch_vic_check(hipStream_t st, const int32_t* off, int32_t n, int64_t nvic, const int32_t* prio,
                            const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int32_t* bad) {
    hipLaunchKernelGGL(k_vic_check, dim3((std::max(n, 1) + 255) / 256), dim3(256), 0, st, off, n, nvic, prio, cpu, mem,
                       gpu, bad);
    return hipGetLastError();
}

hipError_t launch_vic_build(hipStream_t st, const int32_t* off, const int32_t* prio, const int32_t* cpu,
                            const int32_t* mem, const int32_t* gpu, const int32_t* perm, int32_t nn,
                            const int32_t* voff, VicEnt* vent) {
    if (nn <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_vic_build, dim3((nn + 255) / 256), dim3(256), 0, st, off, prio, cpu, mem, gpu, perm, nn, voff,
                       vent);
    return hipGetLastError();
}

// ---- fit_preempt --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pre_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, int32_t nj,
    const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np, int32_t ncomp,
    EvictRow* __restrict__ out, int8_t* __restrict__ jcomp, int32_t* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    int comp = lim.comp >= 0 && lim.comp < ncomp ? lim.comp : -1;
    if (c < 0 || m < 0 || g < 0 || w < 0) {  // the whole call fails (FIT_E_INVAL)
        comp = -1;
        atomicOr(bad, 1);
    }
    // a row without a component is final here: a limit code, or no node carries the partition's bit
    EvictRow r;
    r.code = lim.code != LIM_NONE ? lim.code : (comp < 0 ? (int)PRE_NO_NODES : (int)PRE_FITS);
    r.node = -1;
    r.victims = r.top_prio = 0;
#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) r.cnt[i] = 0;
    out[q] = r;
    jcomp[q] = (int8_t)comp;
}

// grid (job tiles of the chunk, node slices); jl / live: fit_query.h's job list.  The chunk is the
// positions [t0, t0 + nt); part: nt * gridDim.y partials, position-major.
__global__ __launch_bounds__(PRE_WAVES * 64) void k_pre_walk(
    const NodeRec* __restrict__ rec, const int32_t* __restrict__ voff, const VicEnt* __restrict__ vent, ExplainComps C,
    const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t nj, int32_t t0, int32_t nt,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int32_t* __restrict__ jprio,
    const int8_t* __restrict__ jcomp, EvictRow* __restrict__ out, PreKey* __restrict__ part) {
    __shared__ int32_t red[PRE_WAVES][PRE_NCNT][PRE_JOBS];
    __shared__ uint64_t redk[PRE_WAVES][2][PRE_JOBS];
    __shared__ int32_t qs[PRE_JOBS];
    const int nlive = min(query_live(jl, live, nj), t0 + nt);
    const int tb = t0 + (int)blockIdx.x * PRE_JOBS;
    if (tb >= nlive) return;  // block-uniform: k_pre_final reads no position at or behind nlive
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
    PreMin key = {{PRE_NOKEY, PRE_NOKEY}};

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
            for (int u = 0; u < 4; ++u) pre_row(r[u], x + u, pb, j, voff, vent, n, key);
        }
        for (; x < r.n1; ++x) pre_row(rec[x], x, pb, j, voff, vent, n, key);
    }

#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) red[wave][i][lane] = n[i];
    redk[wave][0][lane] = key.k.hi;
    redk[wave][1][lane] = key.k.lo;
    if (wave == 0) qs[lane] = on ? q : -1;
    __syncthreads();
    if (threadIdx.x < PRE_NCNT * PRE_JOBS) {
        // thread (i, l) sums counter i of job-lane l over the waves: one atomic per workgroup, job and
        // counter, none for a zero
        const int i = threadIdx.x / PRE_JOBS, l = threadIdx.x - i * PRE_JOBS;
        int32_t v = 0;
#pragma unroll
        for (int w = 0; w < PRE_WAVES; ++w) v += red[w][i][l];
        const int jq = qs[l];
        if (jq >= 0 && v != 0) atomicAdd(&out[jq].cnt[i], v);
    } else if (threadIdx.x < (PRE_NCNT + 1) * PRE_JOBS) {
        // thread l of the fifth wave folds job-lane l's key over the waves and stores this slice's
        // partial: every position of the tile inside the chunk, live or not, so none is left unwritten
        const int l = threadIdx.x - PRE_NCNT * PRE_JOBS;
        PreKey k = {PRE_NOKEY, PRE_NOKEY};
#pragma unroll
        for (int w = 0; w < PRE_WAVES; ++w) pre_min(k, true, redk[w][0][l], redk[w][1][l]);
        const int t = tb - t0 + l;
        if (t < nt) part[(size_t)t * gridDim.y + blockIdx.y] = k;
    }
}

// One thread per position of the chunk: the job's slices folded, the row finished.
__global__ __launch_bounds__(256) void k_pre_final(const int32_t* __restrict__ jl, const int32_t* __restrict__ live,
                                                   int32_t nj, int32_t t0, int32_t nt, int32_t ncomp, int slices,
                                                   const int8_t* __restrict__ jcomp, const PreKey* __restrict__ part,
                                                   EvictRow* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int q = query_job(t0 + t, jl, live, nj);
    if (q < 0) return;
    const int comp = jcomp[q];
    if (comp < 0 || comp >= ncomp) return;  // final since k_pre_classify
    PreKey k = {PRE_NOKEY, PRE_NOKEY};
    for (int s = 0; s < slices; ++s) {
        const PreKey p = part[(size_t)t * slices + s];
        pre_min(k, true, p.hi, p.lo);
    }
    EvictRow r = out[q];
    const int members = r.cnt[0], fit = r.cnt[1], able = r.cnt[2];
    const bool pick = members > 0 && (fit > 0 || able > 0);
    r.node = pick ? (int32_t)(uint32_t)k.lo : -1;
    r.victims = pick && fit == 0 ? (int32_t)(uint32_t)k.hi : 0;
    r.top_prio = pick && fit == 0 ? (int32_t)((uint32_t)(k.hi >> 32) ^ 0x80000000u) : 0;
    r.code = members == 0 ? PRE_NO_NODES : (fit > 0 ? PRE_FITS : (able > 0 ? PRE_EVICT : PRE_NONE));
    out[q] = r;
}

// The rows on stream st in two calls, the caller ordering the jobs by component in between: `out` (nj
// rows of 32 B) and *bad (1: a negative demand) are valid when the stream has drained.
hipError_t launch_preempt_classify(hipStream_t st, const int32_t* ptab, int32_t np, int ncomp, const int32_t* jcpu,
                                   const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                   const uint16_t* jpart, int32_t nj, void* out, int8_t* jcomp, int32_t* bad) {
    return launch_per_job(st, nj, k_pre_classify, jcpu, jmem, jgpu, jwall, jpart, nj, ptab, np, (int32_t)ncomp,
                          static_cast<EvictRow*>(out), jcomp, bad);
}

// k_pre_final for a walk of another file (fit_preempt_tl.hip): one chunk's positions [t0, t0 + nt)
hipError_t launch_preempt_final(hipStream_t st, const int32_t* jl, const int32_t* live, int32_t nj, int32_t t0,
                                int32_t nt, int ncomp, int slices, const int8_t* jcomp, const void* part, void* out) {
    if (nt <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pre_final, dim3((nt + 255) / 256), dim3(256), 0, st, jl, live, nj, t0, nt, (int32_t)ncomp,
                       slices, jcomp, static_cast<const PreKey*>(part), static_cast<EvictRow*>(out));
    return hipGetLastError();
}

// Node slices of the walk and the partials it needs (16 bytes each) for a batch of nj jobs: a chunk's
// positions x its slices, at most about 8 workgroups per CU x 64 jobs whatever nj is.
int preempt_slices(int32_t nj, int32_t maxn, int cus) { return explain_slices(std::min(nj, PRE_CHUNK), maxn, cus); }
size_t preempt_partials(int32_t nj, int slices) { return (size_t)std::max(std::min(nj, PRE_CHUNK), 1) * slices; }

// Walk and finalise, a chunk of PRE_CHUNK positions after the other; the stream orders their use of
// the one scratch.  jl / live as launch_explain's; slices: preempt_slices; part: preempt_partials.
hipError_t launch_preempt(hipStream_t st, const NodeRec* rec, const int32_t* voff, const VicEnt* vent,
                          const ExplainComps& C, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                          const int32_t* jwall, const uint16_t* jpart, const int32_t* jprio, int32_t nj,
                          const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, void* part,
                          void* out) {
    if (nj <= 0 || C.ncomp == 0) return hipSuccess;  // no component: every row is final since the classifier
    if (C.ncomp < 0 || C.ncomp > 32 || slices < 1 || slices > 65535) return hipErrorInvalidValue;
    EvictRow* o = static_cast<EvictRow*>(out);
    PreKey* p = static_cast<PreKey*>(part);
    for (int32_t t0 = 0; t0 < nj; t0 += PRE_CHUNK) {
        const int32_t nt = std::min<int32_t>(nj - t0, PRE_CHUNK);
        hipLaunchKernelGGL(k_pre_walk, dim3((nt + PRE_JOBS - 1) / PRE_JOBS, slices), dim3(PRE_WAVES * 64), 0, st, rec,
                           voff, vent, C, jl, live, nj, t0, nt, jcpu, jmem, jgpu, jwall, jpart, jprio, jcomp, o, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_pre_final, dim3((nt + 255) / 256), dim3(256), 0, st, jl, live, nj, t0, nt,
                           (int32_t)C.ncomp, slices, jcomp, p, o);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace fitgpu

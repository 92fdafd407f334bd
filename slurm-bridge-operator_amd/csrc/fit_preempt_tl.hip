// fit_preempt_tl.hip — which running jobs to evict so that a pending job can start NOW on the loaded
// timeline: fit_preempt's question asked of the run lists, reservations included, instead of the
// node rows (include/fitgpu.h fit_preempt_tl).  Read-only.  gfx950.
//
// The victims (fit_load_victims_tl) live in row order, as fit_preempt's: position x owns the entries
// [vspan[x].beg, + vspan[x].len) of `vent`, in eviction order (a (begin, length) pair per position, so
// that fit_evicted_tl shrinks a list in place without moving its neighbours).  An entry is 32 bytes —
// priority, end slot and the three RAW amounts: which entries count depends on the slot, so there is no prefix sum to keep.
// Evicting an entry frees its amounts on the slots [0, end - shift) of its node; `shift` is what
// fit_advance_tl has moved the timeline by since the load, a kernel argument.
//
// A run [a, b) of a node that meets the job's window [0, d) binds at its last slot inside it, because
// what a prefix of victims frees never increases in t: with stop = min(b, d) an entry counts for the
// run iff its end >= stop.  v(n) is the maximum over those runs of the smallest prefix that covers
// the run's shortfall; the score takes a second visit with the final v.
//
// fit_preempt's launches in the query frame (fit_query.h); the classifier and the final kernel ARE
// fit_preempt's (launch_preempt_classify, launch_preempt_final), only the walk is new:
//   k_ptl_walk : every live job × every node position of its component.  Lanes = jobs, positions
//                wave-uniform: the 96-B TlHdr, the runs (header, then the slab four per wait) and the
//                32-B victim entries (four per wait) are scalar loads.  A node takes up to three
//                visits of the runs that meet the wave's windows: (1) open / fits now / the window
//                minima; (2) only when a ballot finds an eligible lane that is short, per run that
//                some lane is short on, the list until every such lane has its prefix or the list
//                ends; (3) only for lanes with a prefix they outrank, the minima with that prefix.
//                Counters and the 128-bit key leave through LDS as k_pre_walk's do: one integer
//                atomicAdd per (workgroup, job, non-zero counter), one 16-byte partial per (job
//                position, node slice).
// Integer sums and a lexicographic minimum do not depend on the order: exact and reproducible.  No
// cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.  Jobs are chunked by
// PRE_CHUNK, as fit_preempt's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "fit_device.h"
#include "fit_pre_row.h"
#include "fit_ptl_node.h"
#include "fit_query.h"

namespace fitgpu {

// the counters of a fit_evict row as the walk adds to them (include/fitgpu.h; EvictRow of fit_preempt.hip)
struct alignas(32) EvictCnt {
    int32_t head[4], cnt[PRE_NCNT];
};
static_assert(sizeof(EvictCnt) == 32 && offsetof(EvictCnt, cnt) == 16, "fit_evict is 32 bytes, its counters at 16");

// ---- fit_load_victims_tl ------------------------------------------------------------------------
// k_vic_check with the end column: one thread per caller's node, its offsets, then — only when they
// lie in order inside [0, nvic] — its entries.  *bad |= 1 on any violation; nothing else is written.
__global__ __launch_bounds__(256) void k_vtl_check(const int32_t* __restrict__ off, int32_t n, int64_t nvic,
                                                   const int32_t* __restrict__ prio, const int32_t* __restrict__ end,
                                                   const int32_t* __restrict__ cpu, const int32_t* __restrict__ mem,
                                                   const int32_t* __restrict__ gpu, int32_t H,
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
            err |= cpu[k] < 0 || mem[k] < 0 || gpu[k] < 0 || end[k] < 0 || end[k] > H;
            err |= k > a && prio[k] < prio[k - 1];
        }
    if (err) atomicOr(bad, 1);
}

// One thread per position: its list copied in order.  off: the caller's CSR (validated), vspan: the
// position-ordered spans (host-built from it).
__global__ __launch_bounds__(256) void k_vtl_build(const int32_t* __restrict__ off, const int32_t* __restrict__ prio,
                                                   const int32_t* __restrict__ end, const int32_t* __restrict__ cpu,
                                                   const int32_t* __restrict__ mem, const int32_t* __restrict__ gpu,
                                                   const int32_t* __restrict__ perm, int32_t nn,
                                                   const VicSpan* __restrict__ vspan, VicTl* __restrict__ vent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn) return;
    const int x = perm[i];
    const int a = off[x], len = off[x + 1] - a, d = vspan[i].beg;
    for (int k = 0; k < len; ++k) {
        VicTl e;
        e.prio = prio[a + k];
        e.end = end[a + k];
        e.cpu = cpu[a + k];
        e.mem = mem[a + k];
        e.gpu = gpu[a + k];
        e.pad[0] = e.pad[1] = e.pad[2] = 0;
        vent[d + k] = e;
    }
}

hipError_t launch_vtl_check(hipStream_t st, const int32_t* off, int32_t n, int64_t nvic, const int32_t* prio,
                            const int32_t* end, const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int32_t H,
                            int32_t* bad) {
    hipLaunchKernelGGL(k_vtl_check, dim3((std::max(n, 1) + 255) / 256), dim3(256), 0, st, off, n, nvic, prio, end, cpu,
                       mem, gpu, H, bad);
    return hipGetLastError();
}

hipError_t launch_vtl_build(hipStream_t st, const int32_t* off, const int32_t* prio, const int32_t* end,
                            const int32_t* cpu, const int32_t* mem, const int32_t* gpu, const int32_t* perm, int32_t nn,
                            const VicSpan* vspan, VicTl* vent) {
    if (nn <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_vtl_build, dim3((nn + 255) / 256), dim3(256), 0, st, off, prio, end, cpu, mem, gpu, perm, nn,
                       vspan, vent);
    return hipGetLastError();
}

// ---- fit_preempt_tl -----------------------------------------------------------------------------
// ptl_runs and ptl_node, the visit of a node's runs and the (job-lane, node position) evaluation, are
// fit_ptl_node.h's: fit_preempt_tl_k's walk shares them.
// The walk's sink of offered keys: one lexicographic minimum per lane
struct PtlMin {
    PreKey k;
    __device__ __forceinline__ void offer(bool has, uint64_t hi, uint64_t lo) { pre_min(k, has, hi, lo); }
};

// grid (job tiles of the chunk, node slices); jl / live: fit_query.h's job list.  The chunk is the
// positions [t0, t0 + nt); part: nt * gridDim.y partials, position-major.  k_pre_walk's frame and fold.
__global__ __launch_bounds__(PRE_WAVES * 64) void k_ptl_walk(
    const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab, const VicSpan* __restrict__ vspan,
    const VicTl* __restrict__ vent, ExplainComps C, int32_t H, int32_t slot_min, int32_t shift,
    const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t nj, int32_t t0, int32_t nt,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int32_t* __restrict__ jprio,
    const int8_t* __restrict__ jcomp, EvictCnt* __restrict__ out, PreKey* __restrict__ part) {
    __shared__ int32_t red[PRE_WAVES][PRE_NCNT][PRE_JOBS];
    __shared__ uint64_t redk[PRE_WAVES][2][PRE_JOBS];
    __shared__ int32_t qs[PRE_JOBS];
    const int nlive = min(query_live(jl, live, nj), t0 + nt);
    const int tb = t0 + (int)blockIdx.x * PRE_JOBS;
    if (tb >= nlive) return;  // block-uniform: the final kernel reads no position at or behind nlive
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
    const int32_t d = tl_dur(j.wall, slot_min);
    const uint32_t pbit = on ? 1u << (jpart[q] & 31) : 0u;
    int32_t n[PRE_NCNT];
#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) n[i] = 0;
    PtlMin key = {{PRE_NOKEY, PRE_NOKEY}};

    QueryWalk w = query_walk(on);
    while (w.rem) {  // wave-uniform: one pass per distinct component
        const QueryRange r = query_next<PRE_WAVES>(w, C, comp, on, wave);
        const uint32_t pb = r.mine ? pbit : 0u;
        for (int x = r.n0; x < r.n1; ++x) ptl_node(hdr[x], x, slab, pb, j, d, H, shift, vspan, vent, n, key);
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

// Walk and finalise, a chunk of PRE_CHUNK positions after the other, as launch_preempt; the rows were
// set up by launch_preempt_classify.  slices: preempt_slices; part: preempt_partials.
hipError_t launch_preempt_tl(hipStream_t st, const TlHdr* hdr, const Seg* slab, const VicSpan* vspan, const VicTl* vent,
                             const ExplainComps& C, int32_t H, int32_t slot_min, int32_t shift, const int32_t* jcpu,
                             const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                             const int32_t* jprio, int32_t nj, const int8_t* jcomp, const int32_t* jl,
                             const int32_t* live, int slices, void* part, void* out) {
    if (nj <= 0 || C.ncomp == 0) return hipSuccess;  // no component: every row is final since the classifier
    if (C.ncomp < 0 || C.ncomp > 32 || slices < 1 || slices > 65535) return hipErrorInvalidValue;
    if (H < 1 || H > TL_MAX_SLOTS || slot_min < 1 || shift < 0) return hipErrorInvalidValue;
    PreKey* p = static_cast<PreKey*>(part);
    for (int32_t t0 = 0; t0 < nj; t0 += PRE_CHUNK) {
        const int32_t nt = std::min<int32_t>(nj - t0, PRE_CHUNK);
        hipLaunchKernelGGL(k_ptl_walk, dim3((nt + PRE_JOBS - 1) / PRE_JOBS, slices), dim3(PRE_WAVES * 64), 0, st, hdr,
                           slab, vspan, vent, C, H, slot_min, shift, jl, live, nj, t0, nt, jcpu, jmem, jgpu, jwall,
                           jpart, jprio, jcomp, static_cast<EvictCnt*>(out), p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_preempt_final(st, jl, live, nj, t0, nt, C.ncomp, slices, jcomp, part, out);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace fitgpu

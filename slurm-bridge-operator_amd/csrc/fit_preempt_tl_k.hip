// fit_preempt_tl_k.hip — which running jobs to evict so that a job of `need` nodes can start NOW on the
// loaded timeline: fit_preempt_tl's question with fit_preempt_k's selection (include/fitgpu.h
// fit_preempt_tl_k).  State, eligibility, v(n), the counters and the key of a
// (job, node) pair are fit_preempt_tl's (fit_ptl_node.h); the picks are the `need` smallest keys
// (fit_pre_top.h).  Read-only.  gfx950.
//
// fit_preempt_k's launches in the query frame (fit_query.h); the classifier and the final kernel ARE
// fit_preempt_k's (launch_preempt_k_classify, launch_preempt_k_final), only the walk is new:
//   k_ptlk_walk<K> : k_ptl_walk's frame — lanes = jobs, node positions wave-uniform, ptl_node's three
//                    visits of the runs that meet the wave's windows — with PreTop<K>, a sorted list
//                    of the K smallest keys per lane in registers, as the sink, K the power of two at
//                    or above kmax.  A node offers at most two keys per lane (it fits, or it can be
//                    freed), each behind PreTop::offer's wave-uniform gate.  Then k_prek_walk's fold
//                    (prek_fold): the counters through LDS, one integer atomicAdd per (workgroup,
//                    job, non-zero counter); the eight waves' lists merged pairwise in three rounds;
//                    one list of kmax 16-byte keys per (job position, node slice), disjoint stores.
// Integer sums and the K smallest of distinct keys do not depend on the order: exact and
// reproducible.  No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.  Jobs are
// chunked by PRE_CHUNK, as fit_preempt_k's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "fit_device.h"
#include "fit_pre_row.h"
#include "fit_pre_top.h"
#include "fit_ptl_node.h"
#include "fit_query.h"

namespace fitgpu {

// grid (job tiles of the chunk, node slices); jl / live: fit_query.h's job list.  The chunk is the
// positions [t0, t0 + nt); part: nt * gridDim.y lists of kmax keys, position-major.  Bounds: positions
// by the component ranges (query_next), runs by min(cnt, TL_MAX_SLOTS) and entries by the list length
// (ptl_node), list stores by t < nt and i < kmax (prek_fold).
template <int K>
__global__ __launch_bounds__(PRE_WAVES * 64) void k_ptlk_walk(
    const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab, const VicSpan* __restrict__ vspan,
    const VicTl* __restrict__ vent, ExplainComps C, int32_t H, int32_t slot_min, int32_t shift,
    const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t nj, int32_t t0, int32_t nt, int32_t kmax,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int32_t* __restrict__ jprio,
    const int8_t* __restrict__ jcomp, EvictKRow* __restrict__ out, PreKey* __restrict__ part) {
    __shared__ uint64_t sm[prek_fold_words<K>()];
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
    const int32_t d = tl_dur(j.wall, slot_min);
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
        for (int x = r.n0; x < r.n1; ++x) ptl_node(hdr[x], x, slab, pb, j, d, H, shift, vspan, vent, n, top);
    }

    // the counters, the waves' lists and this slice's list of kmax keys (fit_pre_top.h)
    prek_fold<K>(sm, qs, wave, lane, on, q, n, top, tb, t0, nt, kmax, out, part);
}

namespace {
template <int K>
hipError_t launch_ptlk(hipStream_t st, const TlHdr* hdr, const Seg* slab, const VicSpan* vspan, const VicTl* vent,
                       const ExplainComps& C, int32_t H, int32_t slot_min, int32_t shift, const int32_t* jcpu,
                       const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                       const int32_t* jprio, int32_t kmax, int32_t nj, const int8_t* jcomp, const int32_t* jl,
                       const int32_t* live, int slices, void* part, void* out, int32_t* out_node, int32_t* out_vic) {
    for (int32_t t0 = 0; t0 < nj; t0 += PRE_CHUNK) {
        const int32_t nt = std::min<int32_t>(nj - t0, PRE_CHUNK);
        hipLaunchKernelGGL(k_ptlk_walk<K>, dim3((nt + PRE_JOBS - 1) / PRE_JOBS, slices), dim3(PRE_WAVES * 64), 0, st,
                           hdr, slab, vspan, vent, C, H, slot_min, shift, jl, live, nj, t0, nt, kmax, jcpu, jmem, jgpu,
                           jwall, jpart, jprio, jcomp, static_cast<EvictKRow*>(out), static_cast<PreKey*>(part));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_preempt_k_final(st, jl, live, nj, t0, nt, C.ncomp, slices, kmax, jcomp, part, out, out_node, out_vic);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

// Walk and finalise, a chunk of PRE_CHUNK positions after the other, as launch_preempt_k; the rows and
// the picks were set up by launch_preempt_k_classify.  slices: preempt_slices; part: preempt_k_partials.
hipError_t launch_preempt_tl_k(hipStream_t st, const TlHdr* hdr, const Seg* slab, const VicSpan* vspan,
                               const VicTl* vent, const ExplainComps& C, int32_t H, int32_t slot_min, int32_t shift,
                               const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                               const uint16_t* jpart, const int32_t* jprio, int32_t kmax, int32_t nj,
                               const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, void* part,
                               void* out, int32_t* out_node, int32_t* out_vic) {
    if (nj <= 0 || C.ncomp == 0) return hipSuccess;  // no component: every row is final since the classifier
    if (C.ncomp < 0 || C.ncomp > 32 || slices < 1 || slices > 65535 || kmax < 1 || kmax > FIT_KMAX)
        return hipErrorInvalidValue;
    if (H < 1 || H > TL_MAX_SLOTS || slot_min < 1 || shift < 0) return hipErrorInvalidValue;
#define PTLK_ARGS                                                                                                  \
    st, hdr, slab, vspan, vent, C, H, slot_min, shift, jcpu, jmem, jgpu, jwall, jpart, jprio, kmax, nj, jcomp, jl, \
        live, slices, part, out, out_node, out_vic
    if (kmax == 1) return launch_ptlk<1>(PTLK_ARGS);
    if (kmax == 2) return launch_ptlk<2>(PTLK_ARGS);
    if (kmax <= 4) return launch_ptlk<4>(PTLK_ARGS);
    return launch_ptlk<8>(PTLK_ARGS);
#undef PTLK_ARGS
}

}  // namespace fitgpu

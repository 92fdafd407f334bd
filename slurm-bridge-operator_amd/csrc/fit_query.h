// fit_query.h — the query frame: what the job-side queries fit_explain, fit_when, fit_room and
// fit_when_k share, fit_place_tl_k's classifier and the timeline writers' `dur` /
// `need` too.  The device pieces are __forceinline__: a kernel built from them compiles to what it
// was when it spelled them out (profiles/query_frame_ab.txt).  The LDS folds differ and stay put.
#pragma once
#include <hip/hip_runtime.h>

#include "fit_device.h"

namespace fitgpu {

constexpr int QUERY_WAVES = 8, QUERY_JOBS = 64;  // a count / walk workgroup: waves (a slice's rows split), jobs (lanes)

// The partition-limit rule (SPEC §2, k_prefilter's order): an unknown partition, then the time, cpus
// and mem ceilings of ptab[4][32] (time, cpus, mem, comp), -1 meaning unlimited.  comp: the
// partition's component, -1 when a limit applies or no node carries the partition's bit.
struct JobLimit { int code, comp; };  // code: LimitCode
__device__ __forceinline__ JobLimit job_limit(int p, int np, const int32_t* __restrict__ ptab, int32_t cpu,
                                              int32_t mem, int32_t wall) {
    if (p >= np) return {LIM_PARTITION, -1};
    const int mt = ptab[p], mc = ptab[32 + p], mm = ptab[64 + p];
    if (mt >= 0 && wall > mt) return {LIM_LIMIT_TIME, -1};
    if (mc >= 0 && cpu > mc) return {LIM_LIMIT_CPUS, -1};
    if (mm >= 0 && mem > mm) return {LIM_LIMIT_MEM, -1};
    return {LIM_NONE, ptab[96 + p]};
}

// d of §2d / §2f - §2j: max(1, ceil(wall / slot_min)), a negative wall counting as 0
__device__ __forceinline__ int32_t tl_dur(int32_t wall, int32_t slot_min) {
    const int64_t dw = ((int64_t)max(wall, 0) + slot_min - 1) / slot_min;
    return (int32_t)max<int64_t>(1, min<int64_t>(dw, 0x7fffffff));
}
// need of a row that its call's check passed (need <= kmax <= FIT_KMAX), clamped all the same
__device__ __forceinline__ int32_t tl_need(const uint16_t* jk, int q, int32_t kmax) {
    return min(max(jk ? (int32_t)jk[q] : 1, 1), min(kmax, FIT_KMAX));
}

// Positions of a batch of nj jobs.  jl != nullptr: the jobs in component order (launch_joblists'
// list, *live of them: those that have a component); jl == nullptr: the caller's order.
__device__ __forceinline__ int query_live(const int32_t* jl, const int32_t* live, int32_t nj) {
    return jl ? min(*live, nj) : nj;
}
// Position t -> job, -1 behind the end.  Lanes = jobs (nlive: query_live's) ...
__device__ __forceinline__ int query_job(int t, int nlive, const int32_t* __restrict__ jl, int32_t nj) {
    int q = -1;
    if (t < nlive) q = jl ? jl[t] : t;
    if (q >= nj) q = -1;
    return q;
}
// ... and one position per wave or workgroup (fit_when_k), a list entry below 0 being -1 as well.
// In fit_when_k's spelling: the one above changes the order of k_whenk_count's 5,775 instructions.
__device__ __forceinline__ int query_job(int t, const int32_t* __restrict__ jl, const int32_t* __restrict__ live,
                                         int32_t nj) {
    if (t >= query_live(jl, live, nj)) return -1;
    const int q = jl ? jl[t] : t;
    return q >= 0 && q < nj ? q : -1;
}

// Lanes = jobs: workgroup blockIdx.x takes positions [blockIdx.x * JOBS, + JOBS), lane l the l-th.
// query_idle (block-uniform): none of them is live.  on: the lane's job has rows to visit.
struct QueryLane { int q, comp; bool on; };
template <int JOBS>
__device__ __forceinline__ bool query_idle(int nlive) { return (int64_t)blockIdx.x * JOBS >= nlive; }
template <int JOBS>
__device__ __forceinline__ QueryLane query_lane(int nlive, const int32_t* __restrict__ jl, int32_t nj,
                                                const int8_t* __restrict__ jcomp, const ExplainComps& C) {
    static_assert(JOBS == 64, "one wave's lanes");
    const int q = query_job(blockIdx.x * JOBS + (threadIdx.x & 63), nlive, jl, nj);
    const int comp = q >= 0 ? (int)jcomp[q] : -1;
    return {q, comp, comp >= 0 && comp < C.ncomp};
}

// Slice s of S of component c's rows: [a, b), `per` rows but for the last ...
__device__ __forceinline__ void query_slice(const ExplainComps& C, int c, int S, int s, int& per, int& a, int& b) {
    const int nb = C.nb[c], ne = C.nb[c + 1];
    per = (ne - nb + S - 1) / S;
    a = min(ne, nb + s * per);
    b = min(ne, a + per);
}
// ... and this workgroup's slice of a job's component as a classifier wrote it: false, nothing to do
__device__ __forceinline__ bool query_slice(const ExplainComps& C, int comp, int& a, int& b) {
    if (comp < 0 || comp >= C.ncomp) return false;
    int per;
    query_slice(C, comp, gridDim.y, blockIdx.y, per, a, b);
    return a < b;
}

// The walk: `for (QueryWalk w = query_walk(on); w.rem;) { r = query_next<WAVES>(w, ...); ... }`, one
// pass per distinct component among a wave's `on` lanes, whatever the order of the jobs.  [n0, n1):
// wave `wave`'s rows of the workgroup's slice of the component; mine: the lanes whose job belongs to
// it.  The loops stay in the kernel: with the row loop handed over as a functor the compiler split
// the accumulator arrays and vectorised across rows.
struct QueryWalk { uint64_t rem; int S, s; };  // `on` lanes still to visit; node slices and this workgroup's
struct QueryRange { int n0, n1; bool mine; };
__device__ __forceinline__ QueryWalk query_walk(bool on) { return {__ballot(on), (int)gridDim.y, (int)blockIdx.y}; }
template <int WAVES>
__device__ __forceinline__ QueryRange query_next(QueryWalk& w, const ExplainComps& C, int comp, bool on, int wave) {
    const int c = __builtin_amdgcn_readlane(comp, __builtin_ctzll(w.rem));
    const bool mine = on && comp == c;
    w.rem &= ~__ballot(mine);
    int per, a, b;
    query_slice(C, c, w.S, w.s, per, a, b);
    const int sub = (per + WAVES - 1) / WAVES;  // rows per wave
    const int n0 = min(b, a + wave * sub), n1 = min(b, n0 + sub);
    return {n0, n1, mine};
}

// Host: one thread per job, 256 per workgroup (classify, finalise) ...
template <class... P, class... A>
hipError_t launch_per_job(hipStream_t st, int32_t nj, void (*k)(P...), A... a) {
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(k, dim3((nj + 255) / 256), dim3(256), 0, st, a...);
    return hipGetLastError();
}
// ... and (tiles of QUERY_JOBS jobs) x (explain_slices() node slices) x QUERY_WAVES waves (count, walk)
template <class... P, class... A>
hipError_t launch_per_tile(hipStream_t st, int32_t nj, int ncomp, int slices, void (*k)(P...), A... a) {
    if (nj <= 0) return hipSuccess;
    if (ncomp < 0 || ncomp > 32 || slices < 1 || slices > 65535) return hipErrorInvalidValue;
    if (ncomp == 0) return hipSuccess;
    hipLaunchKernelGGL(k, dim3((nj + QUERY_JOBS - 1) / QUERY_JOBS, slices), dim3(QUERY_WAVES * 64), 0, st, a...);
    return hipGetLastError();
}

}  // namespace fitgpu

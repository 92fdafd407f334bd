// fit_when.hip — earliest start of each pending job on the timeline: per job, the smallest §2b key
// over the nodes of its partition and how many of them can run it at all / now (include/fitgpu.h
// fit_when).  Read-only: the run lists are only loaded.  gfx950.
//
// Three ordinary bounded launches, whatever J and N are:
//   k_when_classify : per job, the partition-limit code (job_limit), `dur`, the row's
//                     accumulators (key KEY_INF, counters 0) and the job's component
//   k_when_walk     : every live job × every node of its component, in the query frame
//                     (fit_query.h).  Lanes = jobs (demand and the TlWalk state in VGPRs),
//                     node positions wave-uniform: the 96-B TlHdr
//                     comes in with scalar loads and its TL_HEAD runs are stepped; a longer list
//                     continues in the slab, four Seg per wait, until no lane is live.  The walk
//                     is fit_tl_walk.h's with lim = H — no cut: `hosts` needs every node's
//                     answer — and a lane leaves a node at its first completed window.  The 8
//                     waves of a workgroup meet in LDS: per (workgroup, job) one 64-bit atomicMin
//                     of the key and at most three integer atomicAdd, zeros skipped.  Min and
//                     integer sums do not depend on the order: exact and reproducible rows.
//   k_when_final    : the minimum key → start, node (TlHdr::orig), wait_min and the code.
// No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fit_device.h"
#include "fit_query.h"
#include "fit_tl_walk.h"

namespace fitgpu {

constexpr int WH_WAVES = QUERY_WAVES, WH_JOBS = QUERY_JOBS;
constexpr int WH_NCNT = 3;  // members, hosts, now

// fit_eta while the launches run: `key` lies over the row's start / node fields
struct alignas(32) EtaAcc {
    int32_t code, dur;
    unsigned long long key;
    int32_t wait_min, cnt[WH_NCNT];
};
// fit_eta as include/fitgpu.h declares it
struct alignas(32) EtaRow {
    int32_t code, dur, start, node, wait_min, members, hosts, now;
};
static_assert(sizeof(EtaAcc) == 32 && sizeof(EtaRow) == 32 && offsetof(EtaAcc, key) == offsetof(EtaRow, start) &&
                  offsetof(EtaAcc, cnt) == offsetof(EtaRow, members),
              "fit_eta is 32 bytes, the key over start / node");

__global__ __launch_bounds__(256) void k_when_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, int32_t nj,
    const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np, int32_t slot_min,
    EtaAcc* __restrict__ out, int8_t* __restrict__ jcomp, int32_t* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    int comp = lim.comp;
    if (c < 0 || m < 0 || g < 0 || w < 0) {  // the whole call fails (FIT_E_INVAL)
        comp = -1;
        atomicOr(bad, 1);
    }
    EtaAcc r;
    r.code = lim.code;
    r.dur = tl_dur(w, slot_min);
    r.key = KEY_INF;  // start = node = -1
    r.wait_min = -1;
#pragma unroll
    for (int i = 0; i < WH_NCNT; ++i) r.cnt[i] = 0;
    out[q] = r;
    jcomp[q] = (int8_t)comp;
}

// One (job-lane, node) evaluation.  h and x are wave-uniform.  The header's column ceilings and
// d <= H reject a node without a walk: they are upper bounds, valid after reservations too.
__device__ __forceinline__ void when_node(const TlHdr& h, int x, const Seg* __restrict__ slab, uint32_t pbit,
                                          int32_t cpu, int32_t mem, int32_t gpu, int32_t d, int32_t H,
                                          uint64_t& best, int32_t (&n)[WH_NCNT]) {
    const bool mb = (h.mask & pbit) != 0u;
    const bool pre = mb && d <= H && cpu <= h.cpu && mem <= h.mem && gpu <= h.gpu;
    n[0] += mb;
    if (!__ballot(pre)) return;  // wave-uniform
    TlWalk w = tl_walk0(pre);
    const int cn = h.cnt;
    // all TL_HEAD runs unconditionally (`vld` masks those past the list): no branch between the
    // header's scalar loads, so they go out together
#pragma unroll
    for (int i = 0; i < TL_HEAD; ++i)
        tl_step_v(w, i < cn, h.head[i].end, h.head[i].cpu, h.head[i].mem, h.head[i].gpu, cpu, mem, gpu, d, H, H);
    if (cn > TL_HEAD) {
        const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
        for (int b = TL_HEAD; b < cn; b += 4) {
            if (!__ballot(w.live)) break;
            Seg r4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r4[i] = sg[b + i];  // inside the slab row (4 | TL_MAX_SLOTS)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (b + i < cn) tl_step(w, r4[i].end, r4[i].cpu, r4[i].mem, r4[i].gpu, cpu, mem, gpu, d, H, H);
        }
    }
    best = min(best, tl_walk_key(w, cpu, mem, gpu, (uint32_t)x));
    n[1] += w.got;
    n[2] += w.got & (w.kra == 0);
}

// grid (job tiles, node slices); jl / live: fit_query.h's job list.  Each lane judges only its own component.
__global__ __launch_bounds__(WH_WAVES * 64) void k_when_walk(
    const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab, ExplainComps C, int32_t H,
    const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t nj, const int32_t* __restrict__ jcpu,
    const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu, const uint16_t* __restrict__ jpart,
    const int8_t* __restrict__ jcomp, EtaAcc* __restrict__ out) {
    __shared__ uint64_t rkey[WH_WAVES][WH_JOBS];
    __shared__ int32_t red[WH_WAVES][WH_NCNT][WH_JOBS];
    __shared__ int32_t qs[WH_JOBS];
    const int nlive = query_live(jl, live, nj);
    if (query_idle<WH_JOBS>(nlive)) return;  // block-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const QueryLane j = query_lane<WH_JOBS>(nlive, jl, nj, jcomp, C);
    const int q = j.q;
    const bool on = j.on;
    const int32_t cpu = on ? jcpu[q] : 0, mem = on ? jmem[q] : 0, gpu = on ? jgpu[q] : 0;
    const int32_t d = on ? out[q].dur : 1;  // k_when_classify's, before any atomic touches the row
    const uint32_t pbit = on ? 1u << (jpart[q] & 31) : 0u;
    uint64_t best = KEY_INF;
    int32_t n[WH_NCNT];
#pragma unroll
    for (int i = 0; i < WH_NCNT; ++i) n[i] = 0;

    QueryWalk w = query_walk(on);
    while (w.rem) {  // wave-uniform: one pass per distinct component
        const QueryRange r = query_next<WH_WAVES>(w, C, j.comp, on, wave);
        const uint32_t pb = r.mine ? pbit : 0u;
        for (int x = r.n0; x < r.n1; ++x) when_node(hdr[x], x, slab, pb, cpu, mem, gpu, d, H, best, n);
    }

    rkey[wave][lane] = best;
#pragma unroll
    for (int i = 0; i < WH_NCNT; ++i) red[wave][i][lane] = n[i];
    if (wave == 0) qs[lane] = on ? q : -1;
    __syncthreads();
    // wave 0: the key of job-lane l over the waves; waves 1..3: counter (wave - 1).  One atomic per
    // workgroup, job and field, none for KEY_INF or a zero
    if (wave == 0) {
        uint64_t k = KEY_INF;
#pragma unroll
        for (int w = 0; w < WH_WAVES; ++w) k = min(k, rkey[w][lane]);
        const int jq = qs[lane];
        if (jq >= 0 && k != KEY_INF) atomicMin(&out[jq].key, (unsigned long long)k);
    } else if (wave <= WH_NCNT) {
        const int i = wave - 1;
        int32_t v = 0;
#pragma unroll
        for (int w = 0; w < WH_WAVES; ++w) v += red[w][i][lane];
        const int jq = qs[lane];
        if (jq >= 0 && v != 0) atomicAdd(&out[jq].cnt[i], v);
    }
}

__global__ __launch_bounds__(256) void k_when_final(EtaAcc* __restrict__ acc, int32_t nj,
                                                    const TlHdr* __restrict__ hdr, int32_t slot_min) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const EtaAcc a = acc[q];
    if (a.code != ETA_NOW) return;  // partition / limit codes: start = node = wait_min = -1, counters 0
    EtaRow r;
    r.dur = a.dur;
    r.members = a.cnt[0];
    r.hosts = a.cnt[1];
    r.now = a.cnt[2];
    r.start = r.node = r.wait_min = -1;
    if (r.members == 0) {
        r.code = ETA_NO_NODES;
    } else if (r.hosts == 0 || a.key == KEY_INF) {
        r.code = ETA_HORIZON;
    } else {
        r.start = (int32_t)(a.key >> 54);
        r.node = hdr[(uint32_t)a.key & TL_POS_MASK].orig;
        r.wait_min = (int32_t)min<int64_t>((int64_t)r.start * slot_min, 0x7fffffff);
        r.code = r.start > 0 ? ETA_LATER : ETA_NOW;
    }
    *reinterpret_cast<EtaRow*>(acc + q) = r;
}

// The query on stream st in two calls, the caller ordering the jobs by component in between: `out`
// (nj rows of 32 B) and *bad (1: a job has a negative demand) are valid when the stream has drained.
hipError_t launch_when_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                const uint16_t* jpart, int32_t nj, int32_t slot_min, void* out, int8_t* jcomp,
                                int32_t* bad) {
    if (nj > 0 && slot_min < 1) return hipErrorInvalidValue;
    return launch_per_job(st, nj, k_when_classify, jcpu, jmem, jgpu, jwall, jpart, nj, ptab, np, slot_min,
                          static_cast<EtaAcc*>(out), jcomp, bad);
}

// Walk and finalise.  jl / live / slices as launch_explain's.
hipError_t launch_when(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                       int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                       const uint16_t* jpart, int32_t nj, const int8_t* jcomp, const int32_t* jl,
                       const int32_t* live, int slices, void* out) {
    if (nj > 0 && (H < 1 || H > TL_MAX_SLOTS || slot_min < 1)) return hipErrorInvalidValue;
    EtaAcc* o = static_cast<EtaAcc*>(out);
    const hipError_t e = launch_per_tile(st, nj, C.ncomp, slices, k_when_walk, hdr, slab, C, H, jl, live, nj, jcpu,
                                         jmem, jgpu, jpart, jcomp, o);
    return e != hipSuccess ? e : launch_per_job(st, nj, k_when_final, o, nj, hdr, slot_min);
}

}  // namespace fitgpu

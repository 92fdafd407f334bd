// fit_explain.hip — why a job does not fit: per-job member / fit / shortage counts over the node
// rows of its partition (include/fitgpu.h fit_explain).  gfx950.
//
// Three ordinary bounded launches, whatever J and N are:
//   k_explain_classify : per job, the partition-limit code (job_limit), `need`, zeroed counters,
//                        and the job's component (-1: no rows to count)
//   k_explain_count    : every live job × every row of its component, in the query frame
//                        (fit_query.h: lanes = jobs, grid.x tiles the jobs, grid.y slices every
//                        component's rows, 8 waves per slice).  Demand in VGPRs, rows wave-uniform
//                        (scalar loads of a NodeRec's five used dwords), five compares and six adds
//                        per pair; the waves are summed through LDS: one integer atomicAdd per
//                        (workgroup, job, counter), zero sums skipped.  Integer sums do not depend
//                        on the order, so the rows are exact and reproducible.
//   k_explain_final    : members == 0 / fit < need / fit >= need → the code.
// No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_query.h"

namespace fitgpu {

constexpr int EX_WAVES = QUERY_WAVES, EX_JOBS = QUERY_JOBS;
constexpr int EX_NCNT = 6;  // members, fit, short_cpu, short_mem, short_gpu, short_time

// fit_why as the kernels see it (include/fitgpu.h): code, need, then the EX_NCNT counters
struct alignas(32) WhyRow {
    int32_t code, need, cnt[EX_NCNT];
};

__global__ __launch_bounds__(256) void k_explain_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const uint16_t* __restrict__ jk,
    int32_t nj, const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np,
    WhyRow* __restrict__ out, int8_t* __restrict__ jcomp, int32_t* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int kraw = jk ? (int)jk[q] : 1;
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    int comp = lim.comp;
    if (kraw > FIT_KMAX || c < 0 || m < 0 || g < 0 || w < 0) {  // the whole call fails (FIT_E_INVAL)
        comp = -1;
        atomicOr(bad, 1);
    }
    WhyRow r;
    r.code = lim.code;
    r.need = max(kraw, 1);
#pragma unroll
    for (int i = 0; i < EX_NCNT; ++i) r.cnt[i] = 0;
    out[q] = r;
    jcomp[q] = (int8_t)comp;
}

// One (job-lane, node-row) evaluation: the four terms of scan_row (fit_common.h), counted one by
// one.  NodeRec fields are clamped to >= -1 and demands are >= 0, so `free < demand` is what the
// raw columns give.
__device__ __forceinline__ void explain_row(const NodeRec& r, uint32_t pbit, int32_t cpu, int32_t mem, int32_t gpu,
                                            int32_t wall, int32_t (&n)[EX_NCNT]) {
    const int mb = (r.mask & pbit) != 0u;
    const int sc = mb & (r.cpu < cpu), sm = mb & (r.mem < mem), sg = mb & (r.gpu < gpu), st = mb & (r.avail < wall);
    n[0] += mb;
    n[1] += mb & ((sc | sm | sg | st) ^ 1);
    n[2] += sc;
    n[3] += sm;
    n[4] += sg;
    n[5] += st;
}

// grid (job tiles, node slices); jl / live: fit_query.h's job list.  Each lane counts only in its own component.
__global__ __launch_bounds__(EX_WAVES * 64) void k_explain_count(
    const NodeRec* __restrict__ rec, ExplainComps C, const int32_t* __restrict__ jl, const int32_t* __restrict__ live,
    int32_t nj, const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int8_t* __restrict__ jcomp,
    WhyRow* __restrict__ out) {
    __shared__ int32_t red[EX_WAVES][EX_NCNT][EX_JOBS];
    __shared__ int32_t qs[EX_JOBS];
    const int nlive = query_live(jl, live, nj);
    if (query_idle<EX_JOBS>(nlive)) return;  // block-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const QueryLane j = query_lane<EX_JOBS>(nlive, jl, nj, jcomp, C);
    const int q = j.q;
    const bool on = j.on;
    const int32_t cpu = on ? jcpu[q] : 0, mem = on ? jmem[q] : 0, gpu = on ? jgpu[q] : 0, wall = on ? jwall[q] : 0;
    const uint32_t pbit = on ? 1u << (jpart[q] & 31) : 0u;
    int32_t n[EX_NCNT];
#pragma unroll
    for (int i = 0; i < EX_NCNT; ++i) n[i] = 0;

    QueryWalk w = query_walk(on);
    while (w.rem) {  // wave-uniform: one pass per distinct component
        const QueryRange r = query_next<EX_WAVES>(w, C, j.comp, on, wave);
        const uint32_t pb = r.mine ? pbit : 0u;
        int x = r.n0;
        for (; x + 4 <= r.n1; x += 4) {  // four scalar row loads per wait, as k_scan
            NodeRec r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = rec[x + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) explain_row(r[u], pb, cpu, mem, gpu, wall, n);
        }
        for (; x < r.n1; ++x) explain_row(rec[x], pb, cpu, mem, gpu, wall, n);
    }

#pragma unroll
    for (int i = 0; i < EX_NCNT; ++i) red[wave][i][lane] = n[i];
    if (wave == 0) qs[lane] = on ? q : -1;
    __syncthreads();
    // thread (i, l) sums counter i of job-lane l over the waves: one atomic per workgroup, job and
    // counter, none for a zero
    for (int e = threadIdx.x; e < EX_NCNT * EX_JOBS; e += EX_WAVES * 64) {
        const int i = e / EX_JOBS, l = e - i * EX_JOBS;
        int32_t v = 0;
#pragma unroll
        for (int w = 0; w < EX_WAVES; ++w) v += red[w][i][l];
        const int jq = qs[l];
        if (jq >= 0 && v != 0) atomicAdd(&out[jq].cnt[i], v);
    }
}

__global__ __launch_bounds__(256) void k_explain_final(WhyRow* __restrict__ out, int32_t nj) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    if (out[q].code != EX_FITS) return;  // partition / limit codes: counters stay 0
    const int members = out[q].cnt[0], fit = out[q].cnt[1], need = out[q].need;
    out[q].code = members == 0 ? EX_NO_NODES : (fit < need ? EX_RESOURCES : EX_FITS);
}

// The diagnosis on stream st in two calls, the caller ordering the jobs by component in between:
// `out` (nj rows of 32 B) and *bad (1: a negative demand or nodes_k > FIT_KMAX) are valid when the
// stream has drained.
hipError_t launch_explain_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                   const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                   const uint16_t* jpart, const uint16_t* jk, int32_t nj, void* out, int8_t* jcomp,
                                   int32_t* bad) {
    static_assert(sizeof(WhyRow) == 32, "fit_why is 32 bytes");
    return launch_per_job(st, nj, k_explain_classify, jcpu, jmem, jgpu, jwall, jpart, jk, nj, ptab, np,
                          static_cast<WhyRow*>(out), jcomp, bad);
}

// Count and finalise.  jl / live: the component-ordered job list and its length on the device, or
// nullptr for the caller's order.  slices: grid.y of the count (explain_slices).
hipError_t launch_explain(hipStream_t st, const NodeRec* rec, const ExplainComps& C, const int32_t* jcpu,
                          const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                          int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                          void* out) {
    WhyRow* o = static_cast<WhyRow*>(out);
    const hipError_t e = launch_per_tile(st, nj, C.ncomp, slices, k_explain_count, rec, C, jl, live, nj, jcpu, jmem,
                                         jgpu, jwall, jpart, jcomp, o);
    return e != hipSuccess ? e : launch_per_job(st, nj, k_explain_final, o, nj);
}

// Node slices for nj jobs against components of at most maxn rows: enough workgroups to fill the
// chip (8 per CU) while a wave still walks min_rows rows (32 here; fit_when's walk costs far more
// per row and asks for fewer); 1 for a long queue.
int explain_slices(int32_t nj, int32_t maxn, int cus, int min_rows) {
    const int64_t tiles = (nj + EX_JOBS - 1) / EX_JOBS;
    const int64_t want = ((int64_t)cus * 8 + tiles - 1) / std::max<int64_t>(tiles, 1);
    const int64_t most = ((int64_t)maxn + EX_WAVES * min_rows - 1) / (EX_WAVES * min_rows);
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want, most), 4096));
}

}  // namespace fitgpu

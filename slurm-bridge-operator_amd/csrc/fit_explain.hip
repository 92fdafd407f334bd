// fit_explain.hip — why a job does not fit: per-job member / fit / shortage counts over the node
// rows of its partition (include/fitgpu.h fit_explain).  gfx950.
//
// Three ordinary bounded launches, whatever J and N are:
//   k_explain_classify : per job, the partition-limit code (k_prefilter's order), `need`, zeroed
//                        counters, and the job's component (-1: no rows to count)
//   k_explain_count    : every live job × every row of its component.  Lanes = jobs (demand in
//                        VGPRs), rows wave-uniform (scalar loads of a NodeRec's five used dwords),
//                        five compares and six adds per pair.  grid.x tiles the jobs (64 per
//                        workgroup), grid.y splits every component's rows into slices, so one job
//                        against 100k rows still uses the chip; the 8 waves of a workgroup walk
//                        sub-slices and are summed through LDS: one integer atomicAdd per
//                        (workgroup, job, counter), zero sums skipped.  Integer sums do not depend
//                        on the order, so the rows are exact and reproducible.
//   k_explain_final    : members == 0 / fit < need / fit >= need → the code.
// No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"

namespace fitgpu {

constexpr int EX_WAVES = 8;  // waves per count workgroup
constexpr int EX_JOBS = 64;  // jobs per count workgroup (lanes)
constexpr int EX_NCNT = 6;   // members, fit, short_cpu, short_mem, short_gpu, short_time

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
    int code = EX_FITS, comp = -1;
    if (p >= np) {
        code = EX_PARTITION;
    } else {
        const int mt = ptab[p], mc = ptab[32 + p], mm = ptab[64 + p];
        if (mt >= 0 && w > mt) code = EX_LIMIT_TIME;
        else if (mc >= 0 && c > mc) code = EX_LIMIT_CPUS;
        else if (mm >= 0 && m > mm) code = EX_LIMIT_MEM;
        else comp = ptab[96 + p];  // -1: no node carries the partition's bit
    }
    if (kraw > FIT_KMAX || c < 0 || m < 0 || g < 0 || w < 0) {  // the whole call fails (FIT_E_INVAL)
        comp = -1;
        atomicOr(bad, 1);
    }
    WhyRow r;
    r.code = code;
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

// grid (job tiles, node slices).  jl != nullptr: the jobs in component order (launch_joblists'
// list, *live of them), so the lanes of a wave share a node range but at a component boundary;
// jl == nullptr: jobs in the caller's order.  Either way a wave walks the components its lanes
// name one after the other, each lane counting only in its own.
__global__ __launch_bounds__(EX_WAVES * 64) void k_explain_count(
    const NodeRec* __restrict__ rec, ExplainComps C, const int32_t* __restrict__ jl, const int32_t* __restrict__ live,
    int32_t nj, const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int8_t* __restrict__ jcomp,
    WhyRow* __restrict__ out) {
    __shared__ int32_t red[EX_WAVES][EX_NCNT][EX_JOBS];
    __shared__ int32_t qs[EX_JOBS];
    const int nlive = jl ? min(*live, nj) : nj;
    if ((int64_t)blockIdx.x * EX_JOBS >= nlive) return;  // block-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * EX_JOBS + lane;
    int q = -1;
    if (t < nlive) q = jl ? jl[t] : t;
    if (q >= nj) q = -1;
    const int comp = q >= 0 ? (int)jcomp[q] : -1;
    const bool on = comp >= 0 && comp < C.ncomp;
    const int32_t cpu = on ? jcpu[q] : 0, mem = on ? jmem[q] : 0, gpu = on ? jgpu[q] : 0, wall = on ? jwall[q] : 0;
    const uint32_t pbit = on ? 1u << (jpart[q] & 31) : 0u;
    int32_t n[EX_NCNT];
#pragma unroll
    for (int i = 0; i < EX_NCNT; ++i) n[i] = 0;

    const int S = gridDim.y, s = blockIdx.y;
    uint64_t rem = __ballot(on);
    while (rem) {  // wave-uniform: one pass per distinct component among the lanes
        const int first = __builtin_ctzll(rem);
        const int c = __builtin_amdgcn_readlane(comp, first);
        const bool mine = on && comp == c;
        rem &= ~__ballot(mine);
        const int nb = C.nb[c], ne = C.nb[c + 1];
        const int per = (ne - nb + S - 1) / S;          // rows of this component per slice
        const int a = min(ne, nb + s * per), b = min(ne, a + per);
        const int sub = (per + EX_WAVES - 1) / EX_WAVES;  // rows per wave
        const int n0 = min(b, a + wave * sub), n1 = min(b, n0 + sub);
        const uint32_t pb = mine ? pbit : 0u;
        int x = n0;
        for (; x + 4 <= n1; x += 4) {  // four scalar row loads per wait, as k_scan
            NodeRec r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = rec[x + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) explain_row(r[u], pb, cpu, mem, gpu, wall, n);
        }
        for (; x < n1; ++x) explain_row(rec[x], pb, cpu, mem, gpu, wall, n);
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

// The diagnosis on stream st in two calls, so that the caller can order the jobs by component in
// between (launch_joblists over jcomp): `out` (nj rows of 32 B) and *bad (1: a job has a negative
// demand or nodes_k > FIT_KMAX) are valid when the stream has drained.
hipError_t launch_explain_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                   const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                   const uint16_t* jpart, const uint16_t* jk, int32_t nj, void* out, int8_t* jcomp,
                                   int32_t* bad) {
    static_assert(sizeof(WhyRow) == 32, "fit_why is 32 bytes");
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_explain_classify, dim3((nj + 255) / 256), dim3(256), 0, st, jcpu, jmem, jgpu, jwall, jpart,
                       jk, nj, ptab, np, static_cast<WhyRow*>(out), jcomp, bad);
    return hipGetLastError();
}

// Count and finalise.  jl / live: the component-ordered job list and its length on the device, or
// nullptr for the caller's order.  slices: grid.y of the count (explain_slices).
hipError_t launch_explain(hipStream_t st, const NodeRec* rec, const ExplainComps& C, const int32_t* jcpu,
                          const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                          int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                          void* out) {
    if (nj <= 0) return hipSuccess;
    if (C.ncomp < 0 || C.ncomp > 32 || slices < 1 || slices > 65535) return hipErrorInvalidValue;
    WhyRow* o = static_cast<WhyRow*>(out);
    if (C.ncomp > 0) {
        const int tiles = (nj + EX_JOBS - 1) / EX_JOBS;
        hipLaunchKernelGGL(k_explain_count, dim3(tiles, slices), dim3(EX_WAVES * 64), 0, st, rec, C, jl, live, nj,
                           jcpu, jmem, jgpu, jwall, jpart, jcomp, o);
    }
    hipLaunchKernelGGL(k_explain_final, dim3((nj + 255) / 256), dim3(256), 0, st, o, nj);
    return hipGetLastError();
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

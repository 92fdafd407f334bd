// fit_when_k.hip — earliest common start of each multi-node job on the timeline: per job, the
// smallest slot at which `need` distinct member nodes all hold the demand for the job's d slots,
// and the `need` best-fitting of the nodes free there (include/fitgpu.h fit_when_k; DESIGN.md §2f,
// §3.14).  Read-only: the run lists are only loaded.  gfx950.
//
// Ordinary bounded launches, whatever J and N are; the middle four run per chunk of jobs so that
// the scratch stays bounded:
//   k_whenk_classify : per job, the partition-limit code (job_limit), `dur`, `need`, the row's
//                      counters zeroed and the job's component
//   k_whenk_count    : one workgroup per (group of 8 jobs, node slice), threads = nodes.  A thread
//                      visits its node's WHOLE run list once (tl_each_run) and steps the group's
//                      jobs over it: for every maximal feasible stretch [a, b) of at least d slots
//                      of a job, +1 at a and -1 at b - d + 1 of that job's difference array in LDS
//                      (H + 1 words each, 32.8 KB for the group).  The workgroup flushes the
//                      non-zero words to the jobs' arrays in HBM with returnless integer atomics,
//                      lane-contiguous, and adds `members` / `hosts`.  Above 8 jobs on several
//                      components the jobs come in component order (launch_joblists), so that a
//                      group shares its nodes.
//   k_whenk_pick     : one wave per job: tl_first_start over the job's differences.  Stores
//                      start, ready, now.
//   k_whenk_nodes    : one workgroup per (job with a start, node slice), threads = nodes: the one
//                      window [start, start + d) (TL_WINDOW) gives feasibility and the minima,
//                      hence score << TL_POS_BITS | pos.  A thread keeps its 8 smallest keys
//                      (tl_keep); the workgroup extracts its `need` smallest through an LDS
//                      64-bit min per round and stores them per (job, slice).
//   k_whenk_final    : one wave per job: the `need` smallest of the slices' keys -> out_node
//                      (TlHdr::orig, key order), wait_min and the code.
// The run-list pieces named in brackets are fit_tl_walk.h's, shared with fit_place_tl_k.hip.
// count, pick and final are template <bool WIN>: WIN = true is fit_when_k_win,
// the same kernels over each job's allowed starts [from, until - d] only; WIN = false is the code above.
// Cross-workgroup traffic is integer atomicAdd (commutative) or disjoint stores, so rows are exact
// and reproducible.  No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fit_device.h"
#include "fit_query.h"
#include "fit_tl_walk.h"

namespace fitgpu {

constexpr int WK_THREADS = 256;  // threads (= nodes in flight) per count / nodes workgroup
constexpr int WK_GROUP = WHENK_GROUP;  // jobs a count workgroup steps over the runs it loads

// fit_eta_k as include/fitgpu.h declares it
struct EtaKRow {
    int32_t code, dur, need, start, wait_min, members, hosts, now, ready, reserved;
};
static_assert(sizeof(EtaKRow) == 40 && offsetof(EtaKRow, members) == 20, "fit_eta_k is 40 bytes");
static_assert(WHENK_KEYS == FIT_KMAX, "a slice keeps one key per node of the widest job");
static_assert(WHENK_MAX_SLICES * WHENK_KEYS <= 128, "k_whenk_final holds two keys per lane");

__global__ __launch_bounds__(256) void k_whenk_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const uint16_t* __restrict__ jk,
    int32_t kmax, int32_t nj, const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np,
    int32_t slot_min, EtaKRow* __restrict__ out, int8_t* __restrict__ jcomp, int32_t* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const int32_t need = max(jk ? (int32_t)jk[q] : 1, 1);
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    int comp = lim.comp;
    if (c < 0 || m < 0 || g < 0 || w < 0 || need > kmax) {  // the whole call fails (FIT_E_INVAL)
        comp = -1;
        atomicOr(bad, 1);
    }
    EtaKRow r;
    // a job without a component has no member node and is in no job list: its row is final here
    r.code = lim.code == LIM_NONE && comp < 0 ? ETA_NO_NODES : lim.code;
    r.dur = tl_dur(w, slot_min);
    r.need = need;
    r.start = r.wait_min = -1;
    r.members = r.hosts = r.now = r.ready = r.reserved = 0;
    out[q] = r;
    jcomp[q] = (int8_t)comp;
}

// grid (groups of WK_GROUP positions of the chunk [t0, t0 + nj), node slices); diff: the chunk's
// difference arrays, H + 1 words per position, zero before the launch.  A thread loads a node's
// runs once and steps all jobs of the group over them: their demands are block-uniform, the
// stretch state is one register per job.  With the jobs in component order a group is one
// component but for a seam; a group passes once over each distinct component of its jobs, each job
// judging only its own.
// WIN (fit_when_k_win, SPEC §2r / DESIGN.md §3.27): a job counts only its allowed starts
// A = [from, until - d].  A run that ends at or before `from` holds none and is stepped as infeasible,
// so a stretch begins at max(a, from) at the earliest, and a closing stretch [a, b) is cut to
// min(b, until): +1 at max(a, from), -1 at min(b, until) - d + 1, when that range is not empty.  The
// words of a job's array before `from` stay zero.  A job whose A is empty walks nothing.
template <bool WIN>
__global__ __launch_bounds__(WK_THREADS) void k_whenk_count(
    const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab, ExplainComps C, int32_t H, int32_t slot_min,
    int32_t t0, int32_t nj, const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t njobs,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int8_t* __restrict__ jcomp,
    EtaKRow* __restrict__ out, int32_t* __restrict__ diff, WinCols<WIN> win) {
    __shared__ int32_t ld[WK_GROUP][TL_MAX_SLOTS + 1];
    __shared__ int32_t cnt[WK_GROUP][2];  // members, hosts
    const int tb = blockIdx.x * WK_GROUP;  // chunk-local position of the group's first job
    int32_t q[WK_GROUP], comp[WK_GROUP], cpu[WK_GROUP], mem[WK_GROUP], gpu[WK_GROUP], d[WK_GROUP];
    uint32_t pbit[WK_GROUP];
    int32_t fr[WK_GROUP], un[WK_GROUP];  // WIN: the job's window; unused otherwise
    uint32_t valid = 0;
#pragma unroll
    for (int g = 0; g < WK_GROUP; ++g) {
        const int qq = tb + g < nj ? query_job(t0 + tb + g, jl, live, njobs) : -1;
        int c = qq >= 0 ? (int)jcomp[qq] : -1;
        if (c >= C.ncomp) c = -1;
        const bool on = c >= 0;
        q[g] = qq;
        comp[g] = c;
        cpu[g] = on ? jcpu[qq] : 0;
        mem[g] = on ? jmem[qq] : 0;
        gpu[g] = on ? jgpu[qq] : 0;
        d[g] = on ? tl_dur(jwall[qq], slot_min) : 1;  // k_whenk_classify's `dur`
        pbit[g] = on ? 1u << (jpart[qq] & 31) : 0u;
        if constexpr (WIN) {
            fr[g] = on ? tl_win_from(win, qq, H) : 0;
            un[g] = on ? tl_win_until(win, qq, H) : 0;
        }
        valid |= on ? 1u << g : 0u;
    }
    if (!valid) return;  // block-uniform
    for (int i = threadIdx.x; i < WK_GROUP * (TL_MAX_SLOTS + 1); i += WK_THREADS) (&ld[0][0])[i] = 0;
    if (threadIdx.x < WK_GROUP * 2) (&cnt[0][0])[threadIdx.x] = 0;
    __syncthreads();
    int32_t members[WK_GROUP], hosts[WK_GROUP];
#pragma unroll
    for (int g = 0; g < WK_GROUP; ++g) members[g] = hosts[g] = 0;

    uint32_t rem = valid;
    while (rem) {  // block-uniform: one pass per distinct component among the group's jobs
        const int first = __builtin_ctz(rem);
        int c = -1;
#pragma unroll
        for (int g = 0; g < WK_GROUP; ++g) c = g == first ? comp[g] : c;
        uint32_t act = 0;
#pragma unroll
        for (int g = 0; g < WK_GROUP; ++g) act |= ((valid >> g) & 1u) && comp[g] == c ? 1u << g : 0u;
        rem &= ~act;
        int a, b;
        if (!query_slice(C, c, a, b)) continue;
        for (int x = a + threadIdx.x; x < b; x += WK_THREADS) {
            const TlHdr h = hdr[x];
            // members; the header's column ceilings and d <= H reject a node without a walk
            uint32_t lv = 0;
#pragma unroll
            for (int g = 0; g < WK_GROUP; ++g) {
                const bool mb = ((act >> g) & 1u) && (h.mask & pbit[g]);
                members[g] += mb;
                // WIN: some start is allowed at all
                lv |= mb && (WIN ? fr[g] + d[g] <= un[g] : d[g] <= H) && cpu[g] <= h.cpu && mem[g] <= h.mem && gpu[g] <= h.gpu ? 1u << g : 0u;
            }
            if (!lv) continue;
            const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
            const int cn = min(h.cnt, TL_MAX_SLOTS);
            int32_t s0 = 0;         // start of the current run
            int32_t ra[WK_GROUP];   // per job, start of the current feasible stretch (-1: none)
#pragma unroll
            for (int g = 0; g < WK_GROUP; ++g) ra[g] = -1;
            uint32_t any = 0;
            // one run [s0, r.end) with r's columns free, vr false behind the last run: per job, the run
            // holds the demand or the job's stretch ends at s0
            auto step = [&](const Seg& r, bool vr = true) {
#pragma unroll
                for (int g = 0; g < WK_GROUP; ++g) {
                    const bool f = vr & (bool)((lv >> g) & 1u) & (r.cpu >= cpu[g]) & (r.mem >= mem[g]) & (r.gpu >= gpu[g]) &
                                   (WIN ? r.end > fr[g] : true);
                    if (!f && ra[g] >= 0) {
                        const int32_t b = WIN ? min(s0, un[g]) : s0;
                        if (b - ra[g] >= d[g]) {  // starts ra .. b - d: +1 at ra, -1 at b - d + 1 <= H
                            atomicAdd(&ld[g][ra[g]], 1);
                            atomicAdd(&ld[g][b - d[g] + 1], -1);
                            any |= 1u << g;
                        }
                        ra[g] = -1;
                    }
                    // WIN: max(s0, from) < the run's end, which lies behind `from`
                    if (f && ra[g] < 0 && s0 < H) ra[g] = WIN ? max(s0, fr[g]) : s0;
                }
                s0 = min(max(r.end, s0), H);  // canonical lists only grow; held so that 0 <= ra < s0 <= H whatever is read
            };
            tl_each_run(h, sg, cn, step);
            step(Seg{H, 0, 0, 0}, false);
#pragma unroll
            for (int g = 0; g < WK_GROUP; ++g) hosts[g] += (any >> g) & 1u;
        }
    }
#pragma unroll
    for (int g = 0; g < WK_GROUP; ++g) {
        if (members[g]) atomicAdd(&cnt[g][0], members[g]);
        if (hosts[g]) atomicAdd(&cnt[g][1], hosts[g]);
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < WK_GROUP; ++g) {
        if (!((valid >> g) & 1u)) continue;  // block-uniform
        int32_t* df = diff + (int64_t)(tb + g) * (H + 1);
        for (int i = threadIdx.x; i <= H; i += WK_THREADS) {
            const int32_t v = ld[g][i];
            if (v) atomicAdd(&df[i], v);
        }
        if (threadIdx.x == 0 && cnt[g][0]) atomicAdd(&out[q[g]].members, cnt[g][0]);
        if (threadIdx.x == 1 && cnt[g][1]) atomicAdd(&out[q[g]].hosts, cnt[g][1]);
    }
}

// One wave per job, 4 jobs per workgroup: cnt(s) is the prefix sum of the differences.  WIN: over
// the allowed starts only (tl_first_start_in), `now` being cnt(from); an empty A leaves the row as
// d > H does.
template <bool WIN>
__global__ __launch_bounds__(256) void k_whenk_pick(const int32_t* __restrict__ diff, int32_t H, int32_t t0,
                                                    int32_t nj, const int32_t* __restrict__ jl,
                                                    const int32_t* __restrict__ live, int32_t njobs,
                                                    const int8_t* __restrict__ jcomp, EtaKRow* __restrict__ out,
                                                    WinCols<WIN> win) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    if (t >= nj) return;  // wave-uniform
    const int q = query_job(t0 + t, jl, live, njobs);
    if (q < 0 || jcomp[q] < 0) return;  // rejected, or no member at all: start stays -1
    const int32_t need = out[q].need, d = out[q].dur;
    TlStart f;
    if constexpr (WIN) {
        const int32_t from = tl_win_from(win, q, H), last = tl_win_until(win, q, H) - d;
        if (from > last) return;
        f = tl_first_start_in(diff + (int64_t)t * (H + 1), from, last, need, lane);
    } else {
        if (d > H) return;
        f = tl_first_start(diff + (int64_t)t * (H + 1), H, need, lane);
    }
    if (lane == 0) {
        out[q].now = f.now;
        out[q].start = f.start;
        out[q].ready = f.ready;
    }
}

// grid (positions of the chunk, node slices); top: WHENK_KEYS keys per (position, slice), KEY_INF
// before the launch.
__global__ __launch_bounds__(WK_THREADS) void k_whenk_nodes(
    const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab, ExplainComps C, int32_t H, int32_t t0,
    const int32_t* __restrict__ jl, const int32_t* __restrict__ live, int32_t njobs,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const uint16_t* __restrict__ jpart, const int8_t* __restrict__ jcomp, const EtaKRow* __restrict__ out,
    unsigned long long* __restrict__ top) {
    __shared__ unsigned long long best;
    const int q = query_job(t0 + blockIdx.x, jl, live, njobs);
    if (q < 0) return;  // block-uniform
    const int32_t start = out[q].start;
    int a, b;
    if (start < 0 || !query_slice(C, jcomp[q], a, b)) return;  // block-uniform
    const int32_t cpu = jcpu[q], mem = jmem[q], gpu = jgpu[q];
    const int32_t d = out[q].dur, need = min(out[q].need, WHENK_KEYS);
    const int32_t stop = start + d;  // <= H: k_whenk_pick found the start among s + d <= H
    const uint32_t pbit = 1u << (jpart[q] & 31);
    uint64_t key[WHENK_KEYS];
#pragma unroll
    for (int i = 0; i < WHENK_KEYS; ++i) key[i] = KEY_INF;
    for (int x = a + threadIdx.x; x < b; x += WK_THREADS) {
        const TlHdr h = hdr[x];
        if (!(h.mask & pbit) || cpu > h.cpu || mem > h.mem || gpu > h.gpu) continue;
        const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
        const int cn = min(h.cnt, TL_MAX_SLOTS);
        TL_WINDOW(h, sg, cn, start, stop, cpu, mem, gpu, mc, mm, mg, fits)
        if (!fits) continue;
        tl_keep(key, tl_key(0, mc, mm, mg, cpu, mem, gpu, (uint32_t)x));
    }
    // the workgroup's `need` smallest: per round the minimum of the threads' heads; keys are
    // distinct (the position), so exactly one thread owns it and moves its list up
    unsigned long long* o = top + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * WHENK_KEYS;
    for (int r = 0; r < need; ++r) {
        if (threadIdx.x == 0) best = KEY_INF;
        __syncthreads();
        if (key[0] != KEY_INF) atomicMin(&best, (unsigned long long)key[0]);
        __syncthreads();
        const uint64_t w = best;
        __syncthreads();  // every thread has read `best` before the next round resets it
        if (w == KEY_INF) break;  // block-uniform
        if (key[0] == w) {
#pragma unroll
            for (int i = 0; i + 1 < WHENK_KEYS; ++i) key[i] = key[i + 1];
            key[WHENK_KEYS - 1] = KEY_INF;
            o[r] = w;
        }
    }
}

// One wave per position, 4 per workgroup: the wave holds the slices' keys, two per lane, and takes
// the `need` smallest in `need` rounds of a wave minimum; lane 0 writes the row.  WIN: a job without
// a start whose window is not the whole range ends as ETA_WINDOW.
template <bool WIN>
__global__ __launch_bounds__(256) void k_whenk_final(EtaKRow* __restrict__ out, int32_t t0, int32_t nj,
                                                     const int32_t* __restrict__ jl,
                                                     const int32_t* __restrict__ live, int32_t njobs,
                                                     const unsigned long long* __restrict__ top, int slices,
                                                     const TlHdr* __restrict__ hdr, int32_t slot_min, int32_t kmax,
                                                     int32_t* __restrict__ out_node, int32_t H, WinCols<WIN> win) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    if (t >= nj) return;  // wave-uniform, as every return below
    const int q = query_job(t0 + t, jl, live, njobs);
    if (q < 0) return;
    EtaKRow r = out[q];
    if (r.code != ETA_NOW) return;  // limit codes and jobs without a component: final since k_whenk_classify
    if (r.members == 0) {
        r.code = ETA_NO_NODES;
    } else if (r.start < 0) {
        r.code = ETA_HORIZON;
        if constexpr (WIN)
            if (tl_win_from(win, q, H) != 0 || tl_win_until(win, q, H) != H) r.code = ETA_WINDOW;
        r.ready = 0;
    } else {
        r.wait_min = (int32_t)min<int64_t>((int64_t)r.start * slot_min, 0x7fffffff);
        r.code = r.start > 0 ? ETA_LATER : ETA_NOW;
        const unsigned long long* k = top + (int64_t)t * slices * WHENK_KEYS;
        const int n = slices * WHENK_KEYS;  // <= 128 = two per lane
        uint64_t k0 = lane < n ? k[lane] : KEY_INF, k1 = 64 + lane < n ? k[64 + lane] : KEY_INF;
        for (int i = 0; i < r.need && i < kmax; ++i) {
            uint64_t m = min(k0, k1);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)m, off), hi = __shfl_xor((uint32_t)(m >> 32), off);
                m = min(m, ((uint64_t)hi << 32) | lo);
            }
            if (m == KEY_INF) break;  // cannot happen: ready >= need nodes passed k_whenk_nodes
            if (lane == 0) out_node[(int64_t)q * kmax + i] = hdr[(uint32_t)m & TL_POS_MASK].orig;
            k0 = k0 == m ? KEY_INF : k0;  // keys are distinct: one lane gives it up
            k1 = k1 == m ? KEY_INF : k1;
        }
    }
    if (lane == 0) out[q] = r;
}

// The query on stream st.  Classify the whole batch first (`out`: nj rows of 40 B; out_node:
// nj * kmax words, all -1 afterwards; *bad: 1 for a negative demand or nodes_k > kmax) ...
hipError_t launch_whenk_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                 const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                 const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t nj,
                                 int32_t slot_min, void* out, int32_t* out_node, int8_t* jcomp, int32_t* bad) {
    if (nj <= 0) return hipSuccess;
    if (slot_min < 1 || kmax < 1 || kmax > FIT_KMAX) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(out_node, 0xff, sizeof(int32_t) * (size_t)nj * kmax, st);
    if (e != hipSuccess) return e;
    return launch_per_job(st, nj, k_whenk_classify, jcpu, jmem, jgpu, jwall, jpart, jk, kmax, nj, ptab, np, slot_min,
                          static_cast<EtaKRow*>(out), jcomp, bad);
}

// ... then, per chunk of at most WHENK_CHUNK positions [t0, t0 + nj) of the batch: count, pick, nodes,
// finalise.  jl / live: the component-ordered job list and its length on the device (njobs jobs in
// all), or nullptr for the caller's order.  diff: nj * (H + 1) words and top: nj * slices *
// WHENK_KEYS keys of scratch, reused by the next chunk on the same stream.
template <bool WIN>
static hipError_t whenk_chunk(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                              int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                              const int32_t* jwall, const uint16_t* jpart, int32_t t0, int32_t nj, int32_t njobs,
                              int32_t kmax, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                              int32_t* diff, unsigned long long* top, void* out, int32_t* out_node,
                              WinCols<WIN> win) {
    if (nj <= 0) return hipSuccess;
    if (C.ncomp < 1 || C.ncomp > 32 || slices < 1 || slices > WHENK_MAX_SLICES || nj > WHENK_CHUNK || H < 1 ||
        H > TL_MAX_SLOTS || slot_min < 1 || kmax < 1 || kmax > FIT_KMAX || t0 < 0 || t0 + nj > njobs)
        return hipErrorInvalidValue;
    EtaKRow* o = static_cast<EtaKRow*>(out);
    hipError_t e = hipMemsetAsync(diff, 0, sizeof(int32_t) * (size_t)nj * (H + 1), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(top, 0xff, sizeof(unsigned long long) * (size_t)nj * slices * WHENK_KEYS, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_whenk_count<WIN>), dim3((nj + WK_GROUP - 1) / WK_GROUP, slices), dim3(WK_THREADS), 0, st, hdr, slab,
                       C, H, slot_min, t0, nj, jl, live, njobs, jcpu, jmem, jgpu, jwall, jpart, jcomp, o, diff, win);
    hipLaunchKernelGGL((k_whenk_pick<WIN>), dim3((nj + 3) / 4), dim3(256), 0, st, diff, H, t0, nj, jl, live, njobs, jcomp,
                       o, win);
    hipLaunchKernelGGL(k_whenk_nodes, dim3(nj, slices), dim3(WK_THREADS), 0, st, hdr, slab, C, H, t0, jl, live, njobs,
                       jcpu, jmem, jgpu, jpart, jcomp, o, top);
    hipLaunchKernelGGL((k_whenk_final<WIN>), dim3((nj + 3) / 4), dim3(256), 0, st, o, t0, nj, jl, live, njobs, top,
                       slices, hdr, slot_min, kmax, out_node, H, win);
    return hipGetLastError();
}

hipError_t launch_whenk_chunk(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                              int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                              const int32_t* jwall, const uint16_t* jpart, int32_t t0, int32_t nj, int32_t njobs,
                              int32_t kmax, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                              int32_t* diff, unsigned long long* top, void* out, int32_t* out_node) {
    return whenk_chunk<false>(st, hdr, slab, C, H, slot_min, jcpu, jmem, jgpu, jwall, jpart, t0, nj, njobs, kmax, jcomp,
                              jl, live, slices, diff, top, out, out_node, WinCols<false>{});
}

// fit_when_k_win: the same sequence with the windowed count, pick and final; nb / dl: the job columns
// not_before and deadline on the device, either nullptr (all 0 / none).
hipError_t launch_whenk_chunk_win(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                                  int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                                  const int32_t* jwall, const uint16_t* jpart, int32_t t0, int32_t nj, int32_t njobs,
                                  int32_t kmax, const int8_t* jcomp, const int32_t* jl, const int32_t* live,
                                  int slices, int32_t* diff, unsigned long long* top, void* out, int32_t* out_node,
                                  const int32_t* nb, const int32_t* dl) {
    return whenk_chunk<true>(st, hdr, slab, C, H, slot_min, jcpu, jmem, jgpu, jwall, jpart, t0, nj, njobs, kmax, jcomp,
                             jl, live, slices, diff, top, out, out_node, WinCols<true>{nb, dl});
}

}  // namespace fitgpu

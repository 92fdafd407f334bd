// fit_place_tl_k.hip — priority-order backfill of multi-node jobs on the timeline: per job, in
// index order, fit_when_k's common start and node list against the run lists as the jobs before it
// left them, then the reservation on every one of its nodes (include/fitgpu.h fit_place_tl_k;
// DESIGN.md §2g, §3.15).  gfx950.
//
// Ordinary bounded launches on the context's stream:
//   k_ptlk_classify : per job, the partition-limit rule (fit_query.h job_limit), the reject result in
//                     out_node / out_start, and the job's component in launch_joblists' coding
//                     (-2 rejected, -3 bad input, -1 no member node)
//   launch_joblists : the jobs of each component, in index order inside a component
//   k_ptlk_commit   : ONE workgroup per partition component, looping over its component's jobs of
//                     the chunk in order.  Per job: (count) threads stride over the component's
//                     nodes, visit each whole run list (tl_each_run) and add +1 / -1 at the ends
//                     of every stretch of feasible starts to a difference array in LDS; (pick) one
//                     wave finds the first s with cnt >= need (tl_first_start); (nodes) the count
//                     walk also scores each node's FIRST window, and a thread keeps its 8 smallest
//                     keys (tl_keep): when no node is free before the start these are the answer;
//                     otherwise threads evaluate the one window [start, start + d) on their nodes
//                     again (tl_window).  `need` rounds of an LDS 64-bit minimum take the
//                     workgroup's smallest; (reserve) one wave per pick reserves with tl_reserve_any and refreshes the
//                     node's header (tl_refresh_head).
// The run-list pieces named in brackets are fit_tl_walk.h's, shared with fit_when_k.hip.
// k_ptlk_commit is template <bool WIN>: WIN = true is fit_place_tl_k_win, the
// same kernel over each job's allowed starts [from, until - d] only; WIN = false is the code above.
// A component's rows are read and written by its workgroup alone, so nothing here waits for another
// workgroup: no persistent grid, no launch lock, no watchdog.  Between jobs the waves of the
// workgroup hand the run lists on through __syncthreads(), i.e. a workgroup-scope release before and
// acquire after the barrier: all waves share the CU's vector L1, which the CU's own stores keep
// current.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_dense.h"
#include "fit_tl_walk.h"

namespace fitgpu {

constexpr int PTLK_RWAVES = FIT_KMAX;  // waves that reserve side by side, one pick each
static_assert(PTLK_THREADS % 64 == 0 && PTLK_THREADS <= 1024, "whole waves, one workgroup");

__global__ __launch_bounds__(256) void k_ptlk_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const uint16_t* __restrict__ jk,
    int32_t kmax, int32_t nj, const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np,
    int32_t* __restrict__ out_node, int32_t* __restrict__ out_start, int8_t* __restrict__ jcomp) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const int32_t need = max(jk ? (int32_t)jk[q] : 1, 1);
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    const bool rej = lim.code != LIM_NONE;
    int comp = rej ? -2 : lim.comp;  // -1: no node carries the partition's bit (unplaced)
    if (c < 0 || m < 0 || g < 0 || w < 0 || need > kmax) comp = -3;  // the whole call fails (FIT_E_INVAL)
    for (int i = 0; i < kmax; ++i) out_node[(int64_t)q * kmax + i] = rej && i == 0 ? -2 : -1;
    out_start[q] = -1;
    jcomp[q] = (int8_t)comp;
}

// LDS of k_ptlk_commit, all in the dynamic region and every part a multiple of 16 bytes: the
// reservation scratch of H + 2 Seg per reserving wave, the picks, the start and the difference array.
__host__ __device__ inline int ptlk_rwaves(int threads) {
    return threads / 64 < PTLK_RWAVES ? threads / 64 : PTLK_RWAVES;
}
__host__ __device__ inline size_t ptlk_scr_bytes(int threads, int32_t H) {
    return sizeof(Seg) * (size_t)ptlk_rwaves(threads) * (H + 2);
}

// grid = components; jl: the component-ordered job list, jb[c] .. jb[c + 1] component c's range of
// it; this launch takes positions [t0, t0 + chunk) of every component's range.
// WIN (fit_place_tl_k_win, SPEC §2r / DESIGN.md §3.27): a job's starts are A = [from, until - d].
// The count clips every stretch as k_whenk_count<true> does; a run that ends at or before `from` is
// stepped as infeasible, so the stretch minima begin at the first run that meets max(a, from) and
// the "first window" a thread scores is the node's first ALLOWED window [ra, ra + d), ra + d <=
// until.  The array holds allowed starts only, hence tl_first_start_in's `early` is "some node has
// an allowed start in [from, start)", which is what the shortcut needs.
template <bool WIN>
__global__ __launch_bounds__(PTLK_THREADS) void k_ptlk_commit(
    TlHdr* hdr, Seg* slab, ExplainComps C, int32_t H, int32_t slot_min, const int32_t* __restrict__ jl,
    const int32_t* __restrict__ jb, int32_t t0, int32_t chunk, const int32_t* __restrict__ jcpu,
    const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu, const int32_t* __restrict__ jwall,
    const uint16_t* __restrict__ jpart, const uint16_t* __restrict__ jk, int32_t kmax, int32_t* out_node,
    int32_t* out_start, int32_t* __restrict__ placed_total, WinCols<WIN> win) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int c = blockIdx.x;
    if (c >= C.ncomp) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int rw = ptlk_rwaves(nt);
    Seg* scr = reinterpret_cast<Seg*>(smem);
    unsigned long long* pick = reinterpret_cast<unsigned long long*>(smem + ptlk_scr_bytes(nt, H));
    int32_t* sh = reinterpret_cast<int32_t*>(pick + FIT_KMAX);  // sh[0]: the job's start
    int32_t* diff = sh + 4;                                     // H + 1 words
    const int nb = C.nb[c], ne = C.nb[c + 1];
    const int lo = min(jb[c + 1], jb[c] + t0), hi = min(jb[c + 1], lo + chunk);
    int32_t placed = 0;
    for (int i = tid; i <= H; i += nt) diff[i] = 0;
    __syncthreads();
    for (int t = lo; t < hi; ++t) {  // every branch on a job's values below is workgroup-uniform
        const int q = jl[t];
        const int32_t cpu = jcpu[q], mem = jmem[q], gpu = jgpu[q];
        const int32_t need = tl_need(jk, q, kmax);
        const int32_t d = tl_dur(jwall[q], slot_min);  // fit_when_k's `dur`
        const uint32_t pbit = 1u << (jpart[q] & 31);
        int32_t from = 0, until = H;
        if constexpr (WIN) {
            from = tl_win_from(win, q, H);
            until = tl_win_until(win, q, H);
            if (from + d > until) continue;  // no allowed start: unplaced, nothing touched
        } else {
            if (d > H) continue;  // no window inside the horizon: unplaced, nothing touched
        }
        // the last job's readers of pick[] are behind its closing barrier; two barriers lie between
        // this reset and the first minimum
        if (tid < FIT_KMAX) pick[tid] = KEY_INF;

        // ---- count: +1 at a, -1 at b - d + 1 for every feasible stretch [a, b) of at least d slots.
        // On the way a thread keeps, sorted, the 8 smallest §2b keys of its nodes: the node's earliest
        // start e_n, then the score of the window [e_n, e_n + d), then the position (tl_step's rule)
        uint64_t key[FIT_KMAX];
#pragma unroll
        for (int i = 0; i < FIT_KMAX; ++i) key[i] = KEY_INF;
        for (int x = nb + tid; x < ne; x += nt) {
            const TlHdr h = hdr[x];
            // the header's column ceilings reject a node without a walk
            if (!(h.mask & pbit) || cpu > h.cpu || mem > h.mem || gpu > h.gpu) continue;
            const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
            const int cn = min(h.cnt, TL_MAX_SLOTS);
            int32_t s0 = 0, ra = -1;  // start of the current run, of the current feasible stretch (-1: none)
            int32_t mc = 0, mm = 0, mg = 0;         // minima of the current stretch's runs so far
            int32_t ks = -1, kc = 0, km = 0, kg = 0;  // the first window: its start and minima, frozen
            auto step = [&](const Seg& r, bool vr = true) {  // vr false: behind the last run
                bool f = vr & (r.cpu >= cpu) & (r.mem >= mem) & (r.gpu >= gpu);
                if constexpr (WIN) f &= r.end > from;
                if (!f && ra >= 0) {
                    int32_t b = s0;
                    if constexpr (WIN) b = min(s0, until);
                    if (b - ra >= d) {  // starts ra .. b - d: +1 at ra, -1 at b - d + 1 <= H
                        atomicAdd(&diff[ra], 1);
                        atomicAdd(&diff[b - d + 1], -1);
                    }
                    ra = -1;
                }
                const int32_t e1 = min(max(r.end, s0), H);  // canonical lists only grow; held so that 0 <= ra < s0 <= H whatever is read
                if (f && s0 < H) {
                    const bool nw = ra < 0;
                    if constexpr (WIN) ra = nw ? max(s0, from) : ra;  // < e1: the run ends behind `from`
                    else ra = nw ? s0 : ra;
                    mc = nw ? r.cpu : min(mc, r.cpu);
                    mm = nw ? r.mem : min(mm, r.mem);
                    mg = nw ? r.gpu : min(mg, r.gpu);
                    bool first = ks < 0 && e1 - ra >= d;  // the run that holds slot ra + d - 1 closes the first window
                    if constexpr (WIN) first = first && ra + d <= until;
                    if (first) {
                        ks = ra;
                        kc = mc;
                        km = mm;
                        kg = mg;
                    }
                }
                s0 = e1;
            };
            tl_each_run(h, sg, cn, step);
            step(Seg{H, 0, 0, 0}, false);
            if (ks < 0) continue;
            tl_keep(key, tl_key(ks, kc, km, kg, cpu, mem, gpu, (uint32_t)x));
        }
        __syncthreads();

        // ---- pick: the first start with `need` nodes free together
        if (wave == 0) {
            TlStart f;
            if constexpr (WIN) f = tl_first_start_in(diff, from, until - d, need, lane);
            else f = tl_first_start(diff, H, need, lane);
            if (lane == 0) {
                sh[0] = f.start;
                sh[1] = f.early;  // some node is free before the start: its first window is not the job's
            }
        }
        __syncthreads();
        const int32_t start = sh[0];
        // the array is read; the next count adds to it behind at least one more barrier
        for (int i = tid; i <= H; i += nt) diff[i] = 0;
        if (start < 0) {  // fewer than `need` nodes free together anywhere: unplaced
            __syncthreads();
            continue;
        }

        // ---- nodes: when no node is free before the start, the members free from it are exactly those
        // whose earliest start it is, and their windows are the ones the count walk scored: the keys are
        // there, in (score, position) order behind the common start.  Otherwise the one window
        // [start, start + d) gives feasibility and the minima.
        const int32_t stop = start + d;  // <= H: the differences only mark starts s with s + d <= H
        if (sh[1]) {
#pragma unroll
            for (int i = 0; i < FIT_KMAX; ++i) key[i] = KEY_INF;
            for (int x = nb + tid; x < ne; x += nt) {
                const TlHdr h = hdr[x];
                if (!(h.mask & pbit) || cpu > h.cpu || mem > h.mem || gpu > h.gpu) continue;
                const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
                const int cn = min(h.cnt, TL_MAX_SLOTS);
                int32_t mc, mm, mg;
                if (!tl_window(h, sg, cn, start, stop, cpu, mem, gpu, mc, mm, mg)) continue;
                tl_keep(key, tl_key(start, mc, mm, mg, cpu, mem, gpu, (uint32_t)x));
            }
        }
        // either way a key that counts carries `start` in its top bits; a later first window does not
        // (KEY_INF is no node's key: check_timeline_args keeps the positions one short of the field)
        auto counts = [&](uint64_t k) { return k != KEY_INF && (int32_t)(k >> 54) == start; };
        // the workgroup's `need` smallest, one slot of pick[] per round: keys are distinct (the
        // position), so exactly one thread owns a round's minimum and moves its list up
        int got = 0;
        for (int r = 0; r < need; ++r) {
            if (counts(key[0])) atomicMin(&pick[r], (unsigned long long)key[0]);
            __syncthreads();
            const uint64_t w = pick[r];
            if (w == KEY_INF) break;
            if (key[0] == w) {
#pragma unroll
                for (int i = 0; i + 1 < FIT_KMAX; ++i) key[i] = key[i + 1];
                key[FIT_KMAX - 1] = KEY_INF;
            }
            ++got;
        }
        if (got < need) {  // cannot happen: cnt(start) >= need nodes passed the same test.  All or nothing.
            __syncthreads();
            continue;
        }

        // ---- reserve: one wave per pick, each with its own scratch; the node's header follows its list
        if (wave < rw)
            for (int r = wave; r < need; r += rw) {
                const uint32_t pos = (uint32_t)pick[r] & TL_POS_MASK;  // in [nb, ne): a position this workgroup read
                TlHdr* hp = hdr + pos;
                Seg* sg = slab + (int64_t)pos * TL_MAX_SLOTS;
                const int n = min(hp->cnt, TL_MAX_SLOTS);
                const int nn = tl_reserve_any(sg, n, start, stop, cpu, mem, gpu, scr + (size_t)wave * (H + 2));
                tl_refresh_head(hp, sg, nn, H, lane);
                if (lane == 0) out_node[(int64_t)q * kmax + r] = hp->orig;
            }
        if (tid == 0) {
            out_start[q] = start;
            ++placed;
        }
        __syncthreads();  // the next job reads what these waves stored
    }
    if (tid == 0 && placed) atomicAdd(placed_total, placed);
}

// Classify the whole batch: out_node (nj * kmax words) and out_start (nj) hold the reject results
// and -1 elsewhere afterwards, jcomp the components for launch_joblists.
hipError_t launch_ptlk_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t nj,
                                int32_t* out_node, int32_t* out_start, int8_t* jcomp) {
    if (nj <= 0) return hipSuccess;
    if (kmax < 1 || kmax > FIT_KMAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ptlk_classify, dim3((nj + 255) / 256), dim3(256), 0, st, jcpu, jmem, jgpu, jwall, jpart, jk,
                       kmax, nj, ptab, np, out_node, out_start, jcomp);
    return hipGetLastError();
}

// threads of a commit workgroup: a thread per node of the largest component, whole waves, at most
// PTLK_THREADS
int ptlk_threads(int32_t max_component_nodes) {
    return std::max(64, std::min(PTLK_THREADS, (max_component_nodes + 63) / 64 * 64));
}

size_t ptlk_lds_bytes(int threads, int32_t H) {
    return ptlk_scr_bytes(threads, H) + sizeof(unsigned long long) * FIT_KMAX + sizeof(int32_t) * 4 +
           sizeof(int32_t) * (((size_t)H + 1 + 3) & ~(size_t)3);
}

// Positions [t0, t0 + chunk) of every component's job list, in order, on stream st.
template <bool WIN>
static hipError_t ptlk_commit(hipStream_t st, int threads, TlHdr* hdr, Seg* slab, const ExplainComps& C, int32_t H,
                              int32_t slot_min, const int32_t* jl, const int32_t* jb, int32_t t0, int32_t chunk,
                              const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                              const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t* out_node,
                              int32_t* out_start, int32_t* placed, WinCols<WIN> win) {
    if (C.ncomp < 1 || C.ncomp > 32 || threads < 64 || threads > PTLK_THREADS || threads % 64 || H < 1 ||
        H > TL_MAX_SLOTS || slot_min < 1 || kmax < 1 || kmax > FIT_KMAX || t0 < 0 || chunk < 1 || chunk > PTLK_CHUNK)
        return hipErrorInvalidValue;
    const size_t lds = ptlk_lds_bytes(threads, H);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_ptlk_commit<WIN>), dim3(C.ncomp), dim3(threads), lds, st, hdr, slab, C, H, slot_min, jl, jb,
                       t0, chunk, jcpu, jmem, jgpu, jwall, jpart, jk, kmax, out_node, out_start, placed, win);
    return hipGetLastError();
}

hipError_t launch_ptlk_commit(hipStream_t st, int threads, TlHdr* hdr, Seg* slab, const ExplainComps& C, int32_t H,
                              int32_t slot_min, const int32_t* jl, const int32_t* jb, int32_t t0, int32_t chunk,
                              const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                              const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t* out_node,
                              int32_t* out_start, int32_t* placed) {
    return ptlk_commit<false>(st, threads, hdr, slab, C, H, slot_min, jl, jb, t0, chunk, jcpu, jmem, jgpu, jwall, jpart,
                              jk, kmax, out_node, out_start, placed, WinCols<false>{});
}

// fit_place_tl_k_win: the windowed commit; nb / dl: the job columns not_before and deadline on the
// device, either nullptr (all 0 / none).
hipError_t launch_ptlk_commit_win(hipStream_t st, int threads, TlHdr* hdr, Seg* slab, const ExplainComps& C, int32_t H,
                                  int32_t slot_min, const int32_t* jl, const int32_t* jb, int32_t t0, int32_t chunk,
                                  const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                  const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t* out_node,
                                  int32_t* out_start, int32_t* placed, const int32_t* nb, const int32_t* dl) {
    return ptlk_commit<true>(st, threads, hdr, slab, C, H, slot_min, jl, jb, t0, chunk, jcpu, jmem, jgpu, jwall, jpart,
                             jk, kmax, out_node, out_start, placed, WinCols<true>{nb, dl});
}

}  // namespace fitgpu

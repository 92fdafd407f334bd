// fit_unplace_tl.hip — hand reservations back to the loaded timeline: per row, its demand added to
// the slots [start, start + d) of every one of its nodes (include/fitgpu.h fit_unplace_tl;
// DESIGN.md §2h, §3.16).  gfx950.
//
// Ordinary bounded launches on the context's stream:
//   k_utl_inverse : caller's node id -> node position (TlHdr::orig read the other way; -1: the node
//                   is in no partition and has no run list)
//   k_utl_check   : one thread per row of the WHOLE batch: the §2h tests of a live row (demands,
//                   need, start, its <= 8 node ids for range and duplicates), the bad-input flag and
//                   the window count of the row's chunk.  Nothing is written to the timeline before
//                   the host has seen the flag.
//   per chunk of at most UTL_CHUNK rows:
//   k_utl_count   : one thread per row: an integer atomic per touched node counts its windows; the
//                   thread that takes a node's count from 0 appends the node to the touched list
//   k_utl_offsets : one thread per touched node: its range of the window array (an atomic add of its
//                   count: the order of the ranges is free)
//   k_utl_scatter : one thread per row: its windows into their nodes' ranges (order inside a node is
//                   free: the §2h arithmetic commutes and associates)
//   k_utl_apply   : ONE wave (a 64-thread workgroup) per touched node, so no two waves ever edit one
//                   list.  The wave expands the node's run list to its dense H slots x 3 columns in
//                   LDS, adds every window of the node to it, 64 slots per step, and writes the
//                   canonical run list back: a slot ends a run when the next slot differs (ballot +
//                   lanes-below prefix, tl_reserve_any's merge step).  The same pass takes the wave
//                   maximum of every column for the header's ceilings.  The wave then waits for its
//                   own list stores and refreshes cnt, head[] and the ceilings, as k_ptlk_commit's
//                   reserving waves do.
// The dense form costs H / 64 steps to expand and to write back whatever the node's windows are, and
// a window costs d / 64 steps: there is no slow case for many windows on one node, and the list that
// comes out is canonical by construction (at most H runs: the slab row cannot overflow).
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; integer
// atomics and disjoint stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_reserve.h"

namespace fitgpu {

static_assert(sizeof(UtlWin) == 32, "one window is two 16-byte loads");

// d of §2h: max(1, ceil(wall / slot_min)), a negative wall counting as 0 (k_ptlk_commit's `d`)
__device__ __forceinline__ int32_t utl_dur(int32_t wall, int32_t slot_min) {
    const int64_t dw = ((int64_t)max(wall, 0) + slot_min - 1) / slot_min;
    return (int32_t)max<int64_t>(1, min<int64_t>(dw, 0x7fffffff));
}

__global__ __launch_bounds__(256) void k_utl_inverse(const TlHdr* __restrict__ hdr, int32_t nn, int32_t n,
                                                     int32_t* __restrict__ inv) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nn) return;
    const int32_t o = hdr[x].orig;
    if (o >= 0 && o < n) inv[o] = x;
}

// g[2]: the bad-input flag; g[4 + q / chunk]: windows of that chunk's live rows, one atomic per wave
// and chunk (the address is not uniform, so the compiler does not fold a wave's adds itself: every
// live row adding on its own made this the longest kernel of the call, 135 us at 16,384 rows)
__global__ __launch_bounds__(256) void k_utl_check(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const uint16_t* __restrict__ jk, int32_t kmax, const int32_t* __restrict__ node,
    const int32_t* __restrict__ start, int32_t nj, int32_t n, int32_t H, int32_t chunk, int32_t* __restrict__ g) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t s = q < nj ? start[q] : -1;  // a row with start < 0 is skipped whatever else it holds
    int32_t need = 0;                          // windows this row adds: 0 for a skipped or a bad row
    if (s >= 0) {
        need = max(jk ? (int32_t)jk[q] : 1, 1);
        bool bad = jcpu[q] < 0 || jmem[q] < 0 || jgpu[q] < 0 || need > kmax || s >= H;
        if (!bad) {
            int32_t id[FIT_KMAX];
#pragma unroll
            for (int i = 0; i < FIT_KMAX; ++i) id[i] = i < need ? node[(int64_t)q * kmax + i] : -1 - i;
#pragma unroll
            for (int i = 0; i < FIT_KMAX; ++i) {
                if (i < need && (id[i] < 0 || id[i] >= n)) bad = true;
#pragma unroll
                for (int k = i + 1; k < FIT_KMAX; ++k)
                    if (k < need && id[i] == id[k]) bad = true;
            }
        }
        if (bad) {
            atomicOr(&g[2], 1);
            need = 0;
        }
    }
    // every lane of the wave is here: per chunk index among its live rows, one sum and one add
    const int32_t ci = q < nj ? q / chunk : -1;
    uint64_t todo = __ballot(need > 0);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int32_t lci = __shfl(ci, lead);
        const bool mine = need > 0 && ci == lci;
        int32_t sum = mine ? need : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == lead) atomicAdd(&g[4 + lci], sum);
        todo &= ~__ballot(mine);
    }
}

// Rows [t0, t0 + nj) of a batch that k_utl_check passed.  g[0]: touched nodes so far.
__global__ __launch_bounds__(256) void k_utl_count(const uint16_t* __restrict__ jk, int32_t kmax,
                                                   const int32_t* __restrict__ node,
                                                   const int32_t* __restrict__ start, int32_t t0, int32_t nj,
                                                   int32_t n, const int32_t* __restrict__ inv,
                                                   int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ touched, int32_t cap,
                                                   int32_t* __restrict__ g) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    const int q = t0 + t;
    if (start[q] < 0) return;
    const int32_t need = min(max(jk ? (int32_t)jk[q] : 1, 1), min(kmax, FIT_KMAX));
    for (int i = 0; i < need; ++i) {
        const int32_t id = node[(int64_t)q * kmax + i];
        const int32_t pos = id >= 0 && id < n ? inv[id] : -1;  // in range: k_utl_check passed the batch
        if (pos < 0) continue;  // a node in no partition: every slot is -1 and stays so
        if (atomicAdd(&cnt[pos], 1) == 0) {
            const int32_t k = atomicAdd(&g[0], 1);
            if (k < cap) touched[k] = pos;  // cap >= the distinct nodes a chunk can name: always true
        }
    }
}

// g[1]: windows handed out so far.  first[pos]: the node's range start; fill[pos]: its scatter cursor.
__global__ __launch_bounds__(256) void k_utl_offsets(const int32_t* __restrict__ touched, int32_t cap,
                                                     const int32_t* __restrict__ cnt, int32_t* __restrict__ first,
                                                     int32_t* __restrict__ fill, int32_t* __restrict__ g) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= min(g[0], cap)) return;
    const int32_t pos = touched[t];
    const int32_t o = atomicAdd(&g[1], cnt[pos]);
    first[pos] = o;
    fill[pos] = o;
}

__global__ __launch_bounds__(256) void k_utl_scatter(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jk, int32_t kmax,
    const int32_t* __restrict__ node, const int32_t* __restrict__ start, int32_t t0, int32_t nj, int32_t H,
    int32_t slot_min, int32_t n, const int32_t* __restrict__ inv, int32_t* __restrict__ fill,
    UtlWin* __restrict__ win, int32_t wcap) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    const int q = t0 + t;
    const int32_t s = start[q];
    if (s < 0) return;
    const int32_t need = min(max(jk ? (int32_t)jk[q] : 1, 1), min(kmax, FIT_KMAX));
    const int32_t d = utl_dur(jwall[q], slot_min);
    const int32_t e = (int32_t)min<int64_t>((int64_t)s + d, H);  // clipped at the horizon
    const UtlWin w{s, e, jcpu[q], jmem[q], jgpu[q], {0, 0, 0}};
    for (int i = 0; i < need; ++i) {
        const int32_t id = node[(int64_t)q * kmax + i];
        const int32_t pos = id >= 0 && id < n ? inv[id] : -1;
        if (pos < 0) continue;
        const int32_t k = atomicAdd(&fill[pos], 1);
        if (k >= 0 && k < wcap) win[k] = w;  // k < the chunk's window total <= wcap
    }
}

// §2h, one column of one slot: -1 stays -1, any other value rises and saturates
__device__ __forceinline__ int32_t utl_add(int32_t v, int32_t dem) {
    return v == -1 ? -1 : (int32_t)min<int64_t>((int64_t)v + dem, 0x7fffffff);
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_utl_apply(TlHdr* hdr, Seg* slab, int32_t H, const int32_t* __restrict__ touched,
                                                  int32_t cap, int32_t* cnt, const int32_t* __restrict__ first,
                                                  const UtlWin* __restrict__ win, int32_t wcap,
                                                  const int32_t* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) int32_t utl_dense[];
    const int b = blockIdx.x;
    if (b >= min(g[0], cap)) return;
    const int lane = threadIdx.x;
    const int32_t pos = touched[b];
    int32_t* dc = utl_dense;
    int32_t* dm = dc + H;
    int32_t* dg = dm + H;
    TlHdr* hp = hdr + pos;
    Seg* sg = slab + (int64_t)pos * TL_MAX_SLOTS;
    const int n = min(hp->cnt, TL_MAX_SLOTS);

    // ---- expand: 64 runs per load, then run by run the wave fills the run's slots
    int32_t a = 0;  // end of the runs expanded so far
    for (int r0 = 0; r0 < n; r0 += 64) {
        const Seg mine = r0 + lane < n ? sg[r0 + lane] : Seg{H, -1, -1, -1};
        const int m = min(64, n - r0);
        for (int k = 0; k < m; ++k) {
            const int32_t e = min(max(__shfl(mine.end, k), a), H);  // canonical lists only grow
            const int32_t vc = __shfl(mine.cpu, k), vm = __shfl(mine.mem, k), vg = __shfl(mine.gpu, k);
            for (int s = a + lane; s < e; s += 64) {
                dc[s] = vc;
                dm[s] = vm;
                dg[s] = vg;
            }
            a = e;
        }
    }
    for (int s = a + lane; s < H; s += 64) dc[s] = dm[s] = dg[s] = -1;  // a list that stops short: unusable
    __syncthreads();

    // ---- add: 64 windows per load, a window's slots 64 per step
    const int32_t w0 = first[pos], nw = cnt[pos];
    for (int i0 = 0; i0 < nw; i0 += 64) {
        const int32_t wi = w0 + i0 + lane;
        const UtlWin mine = (i0 + lane < nw && wi >= 0 && wi < wcap) ? win[wi] : UtlWin{0, 0, 0, 0, 0, {0, 0, 0}};
        const int m = min(64, nw - i0);
        for (int k = 0; k < m; ++k) {
            const int32_t ws = max(__shfl(mine.s, k), 0), we = min(__shfl(mine.e, k), H);
            const int32_t jc = __shfl(mine.cpu, k), jm = __shfl(mine.mem, k), jg = __shfl(mine.gpu, k);
            for (int s = ws + lane; s < we; s += 64) {
                dc[s] = utl_add(dc[s], jc);
                dm[s] = utl_add(dm[s], jm);
                dg[s] = utl_add(dg[s], jg);
            }
            __syncthreads();  // one wave: the next window's lanes read what these lanes stored
        }
    }
    __syncthreads();

    // ---- write back: slot s ends a run when it is the last or its successor differs
    int no = 0;
    int32_t xc = -1, xm = -1, xg = -1;
    for (int base = 0; base < H; base += 64) {
        const int s = base + lane;
        const bool v = s < H;
        const int32_t pc = v ? dc[s] : 0, pm = v ? dm[s] : 0, pg = v ? dg[s] : 0;
        const bool more = s + 1 < H;
        const int32_t qc = more ? dc[s + 1] : 0, qm = more ? dm[s + 1] : 0, qg = more ? dg[s + 1] : 0;
        const bool keep = v && (!more || pc != qc || pm != qm || pg != qg);
        const uint64_t mk = __ballot(keep);
        if (keep) sg[no + lanes_below(mk)] = Seg{s + 1, pc, pm, pg};  // no + ... < H <= TL_MAX_SLOTS
        no += __popcll(mk);
        if (v) {
            xc = max(xc, pc);
            xm = max(xm, pm);
            xg = max(xg, pg);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        xc = max(xc, __shfl_xor(xc, off));
        xm = max(xm, __shfl_xor(xm, off));
        xg = max(xg, __shfl_xor(xg, off));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the list's writes before its re-read
    if (lane < TL_HEAD) hp->head[lane] = lane < no ? sg[lane] : Seg{H, -1, -1, -1};
    if (lane == 0) {
        hp->cnt = no;
        hp->cpu = max(hp->cpu, xc);  // values rose: the ceilings rise with them
        hp->mem = max(hp->mem, xm);
        hp->gpu = max(hp->gpu, xg);
        cnt[pos] = 0;  // the next chunk counts from zero
    }
}

hipError_t launch_utl_inverse(hipStream_t st, const TlHdr* hdr, int32_t nn, int32_t n, int32_t* inv) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(inv, 0xff, sizeof(int32_t) * (size_t)n, st);
    if (e != hipSuccess || nn <= 0) return e;
    hipLaunchKernelGGL(k_utl_inverse, dim3((nn + 255) / 256), dim3(256), 0, st, hdr, nn, n, inv);
    return hipGetLastError();
}

hipError_t launch_utl_check(hipStream_t st, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                            const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t nj,
                            int32_t n, int32_t H, int32_t chunk, int32_t* g) {
    if (nj <= 0) return hipSuccess;
    if (kmax < 1 || kmax > FIT_KMAX || chunk < 1 || chunk > UTL_CHUNK || H < 1 || H > TL_MAX_SLOTS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_utl_check, dim3((nj + 255) / 256), dim3(256), 0, st, jcpu, jmem, jgpu, jk, kmax, node, start,
                       nj, n, H, chunk, g);
    return hipGetLastError();
}

// Rows [t0, t0 + nj) with `windows` windows between them (k_utl_check's count of the chunk), on
// stream st.  cnt[nn] is zero before and after; g[0] and g[1] are reset here.
hipError_t launch_utl_chunk(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, int32_t slot_min,
                            const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                            const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t t0,
                            int32_t nj, int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                            int32_t* fill, int32_t* touched, UtlWin* win, int32_t* g) {
    if (nj <= 0 || windows <= 0 || nn <= 0) return hipSuccess;
    if (nj > UTL_CHUNK || kmax < 1 || kmax > FIT_KMAX || windows > nj * kmax || H < 1 || H > TL_MAX_SLOTS ||
        slot_min < 1 || t0 < 0)
        return hipErrorInvalidValue;
    const int32_t cap = std::min(windows, nn);  // distinct nodes the chunk can touch
    hipError_t e = hipMemsetAsync(g, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const dim3 rows((nj + 255) / 256), nodes((cap + 255) / 256), th(256);
    hipLaunchKernelGGL(k_utl_count, rows, th, 0, st, jk, kmax, node, start, t0, nj, n, inv, cnt, touched, cap, g);
    hipLaunchKernelGGL(k_utl_offsets, nodes, th, 0, st, touched, cap, cnt, first, fill, g);
    hipLaunchKernelGGL(k_utl_scatter, rows, th, 0, st, jcpu, jmem, jgpu, jwall, jk, kmax, node, start, t0, nj, H,
                       slot_min, n, inv, fill, win, windows);
    hipLaunchKernelGGL(k_utl_apply, dim3(cap), dim3(64), sizeof(int32_t) * 3 * (size_t)H, st, hdr, slab, H, touched,
                       cap, cnt, first, win, windows, g);
    return hipGetLastError();
}

}  // namespace fitgpu

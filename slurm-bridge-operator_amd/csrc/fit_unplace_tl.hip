// fit_unplace_tl.hip — hand reservations back to the loaded timeline: per row, its demand added to
// the slots [start, start + d) of every one of its nodes (include/fitgpu.h fit_unplace_tl;
// DESIGN.md §2h, §3.16).  gfx950.
//
// Ordinary bounded launches on the context's stream.  The first five kernels serve fit_unplace_tl
// AND fit_hold_tl (fit_hold_tl.hip): the two calls take the same rows, field for field.
//   k_utl_inverse : caller's node id -> node position (TlHdr::orig read the other way; -1: the node
//                   is in no partition and has no run list)
//   k_utl_check   : one thread per row of the WHOLE batch: the §2h tests of a live row (demands,
//                   need, start, its <= 8 node ids for range and duplicates), the bad-input flag and
//                   the window count of the row's chunk.  Nothing is written to the timeline before
//                   the host has seen the flag.
//   rows [t0, t0 + nj) — a chunk of at most UTL_CHUNK rows here, the whole call for fit_hold_tl:
//   k_utl_count   : one thread per row: an integer atomic per touched node counts its windows; the
//                   thread that takes a node's count from 0 appends the node to the touched list.
//                   A row on a node in no partition raises its flag where the caller gives flags
//                   (fit_hold_tl: every slot of such a node reads -1, which no demand fits).
//   k_utl_offsets : one thread per touched node: its range of the window array (an atomic add of its
//                   count: the order of the ranges is free)
//   k_utl_scatter : one thread per row: its windows, each with its row index, into their nodes'
//                   ranges (order inside a node is free: the §2h arithmetic commutes and associates)
//   k_utl_apply   : ONE wave (a 64-thread workgroup) per touched node, so no two waves ever edit one
//                   list: the dense edit of fit_tl_dense.h with §2h's saturating add, the ceilings
//                   raised along with the values.
// The layout of the counter words g is fit_device.h's.
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; integer
// atomics and disjoint stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_dense.h"

namespace fitgpu {

__global__ __launch_bounds__(256) void k_utl_inverse(const TlHdr* __restrict__ hdr, int32_t nn, int32_t n,
                                                     int32_t* __restrict__ inv) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nn) return;
    const int32_t o = hdr[x].orig;
    if (o >= 0 && o < n) inv[o] = x;
}

// g[2] and g[4 + q / chunk]: one atomic per wave and chunk (the address is not uniform, so the
// compiler does not fold a wave's adds itself: every live row adding on its own made this the
// longest kernel of the call, 135 us at 16,384 rows)
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

// Rows [t0, t0 + nj) of a batch that k_utl_check passed.  flag: null, or a word per row of the batch.
__global__ __launch_bounds__(256) void k_utl_count(const uint16_t* __restrict__ jk, int32_t kmax,
                                                   const int32_t* __restrict__ node,
                                                   const int32_t* __restrict__ start, int32_t t0, int32_t nj,
                                                   int32_t n, const int32_t* __restrict__ inv,
                                                   int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ touched, int32_t cap,
                                                   int32_t* __restrict__ flag, int32_t* __restrict__ g) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    const int q = t0 + t;
    if (start[q] < 0) return;
    const int32_t need = tl_need(jk, q, kmax);
    for (int i = 0; i < need; ++i) {
        const int32_t id = node[(int64_t)q * kmax + i];
        const int32_t pos = id >= 0 && id < n ? inv[id] : -1;  // in range: k_utl_check passed the batch
        if (pos < 0) {  // a node in no partition: every slot is -1 and stays so
            if (flag) flag[q] = 1;
            continue;
        }
        if (atomicAdd(&cnt[pos], 1) == 0) {
            const int32_t k = atomicAdd(&g[0], 1);
            if (k < cap) touched[k] = pos;  // cap >= the distinct nodes the rows can name: always true
        }
    }
}

// first[pos]: the node's range start; fill[pos]: its scatter cursor.
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
    TlWin* __restrict__ win, int32_t wcap) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    const int q = t0 + t;
    const int32_t s = start[q];
    if (s < 0) return;
    const int32_t need = tl_need(jk, q, kmax);
    const int32_t d = tl_dur(jwall[q], slot_min);
    const int32_t e = (int32_t)min<int64_t>((int64_t)s + d, H);  // clipped at the horizon
    const TlWin w{s, e, jcpu[q], jmem[q], jgpu[q], q, {0, 0}};
    for (int i = 0; i < need; ++i) {
        const int32_t id = node[(int64_t)q * kmax + i];
        const int32_t pos = id >= 0 && id < n ? inv[id] : -1;
        if (pos < 0) continue;
        const int32_t k = atomicAdd(&fill[pos], 1);
        if (k >= 0 && k < wcap) win[k] = w;  // k < the rows' window total <= wcap
    }
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_utl_apply(TlHdr* hdr, Seg* slab, int32_t H, const int32_t* __restrict__ touched,
                                                  int32_t cap, int32_t* cnt, const int32_t* __restrict__ first,
                                                  const TlWin* __restrict__ win, int32_t wcap,
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
    tl_dense_expand<false>(sg, min(hp->cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    __syncthreads();
    tl_dense_windows(win, first[pos], cnt[pos], wcap, H, lane, dc, dm, dg, utl_add);
    __syncthreads();
    const TlDenseOut o = tl_dense_write(sg, H, lane, dc, dm, dg);
    tl_refresh_head(hp, sg, o.no, H, lane);
    if (lane == 0) {
        hp->cpu = max(hp->cpu, o.xc);  // values rose: the ceilings rise with them
        hp->mem = max(hp->mem, o.xm);
        hp->gpu = max(hp->gpu, o.xg);
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

// The `windows` windows (k_utl_check's count) of rows [t0, t0 + nj), nj > 0, grouped by node on
// stream st: afterwards touched[0 .. g[0]) are the nodes, win[first[pos] .. + cnt[pos]) a node's
// windows.  cnt[nn] and g[0..1] are zero on entry; win holds `windows` entries, touched
// min(windows, nn).  With no node position at all only the count runs (it raises the flags).
hipError_t launch_utl_group(hipStream_t st, int32_t nn, int32_t H, int32_t slot_min, const int32_t* jcpu,
                            const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jk,
                            int32_t kmax, const int32_t* node, const int32_t* start, int32_t t0, int32_t nj,
                            int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                            int32_t* fill, int32_t* touched, TlWin* win, int32_t* flag, int32_t* g) {
    if (H < 1 || H > TL_MAX_SLOTS || slot_min < 1) return hipErrorInvalidValue;
    const hipError_t e = launch_utl_ranges(st, nn, jk, kmax, node, start, t0, nj, windows, n, inv, cnt, first, fill,
                                           touched, flag, g);
    if (e != hipSuccess || std::min(windows, nn) <= 0) return e;
    hipLaunchKernelGGL(k_utl_scatter, dim3((nj + 255) / 256), dim3(256), 0, st, jcpu, jmem, jgpu, jwall, jk, kmax, node,
                       start, t0, nj, H, slot_min, n, inv, fill, win, windows);
    return hipGetLastError();
}

// The first two steps of launch_utl_group, which need only a row's node list and start: the count
// per node with the touched list, then every touched node's range of the window array.  fit_set_tl's
// rows (one node each, `from` for start) take them as they are and scatter their own window format.
hipError_t launch_utl_ranges(hipStream_t st, int32_t nn, const uint16_t* jk, int32_t kmax, const int32_t* node,
                             const int32_t* start, int32_t t0, int32_t nj, int32_t windows, int32_t n,
                             const int32_t* inv, int32_t* cnt, int32_t* first, int32_t* fill, int32_t* touched,
                             int32_t* flag, int32_t* g) {
    if (kmax < 1 || kmax > FIT_KMAX || windows < 1 || (int64_t)windows > (int64_t)nj * kmax || t0 < 0 || nn < 0)
        return hipErrorInvalidValue;
    const int32_t cap = std::min(windows, nn);  // distinct nodes the rows can touch
    const dim3 rows((nj + 255) / 256), th(256);
    hipLaunchKernelGGL(k_utl_count, rows, th, 0, st, jk, kmax, node, start, t0, nj, n, inv, cnt, touched, cap, flag, g);
    if (cap > 0)
        hipLaunchKernelGGL(k_utl_offsets, dim3((cap + 255) / 256), th, 0, st, touched, cap, cnt, first, fill, g);
    return hipGetLastError();
}

// Rows [t0, t0 + nj) with `windows` windows between them (k_utl_check's count of the chunk), on
// stream st.  cnt[nn] is zero before and after; g[0] and g[1] are reset here.
hipError_t launch_utl_chunk(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, int32_t slot_min,
                            const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                            const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t t0,
                            int32_t nj, int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                            int32_t* fill, int32_t* touched, TlWin* win, int32_t* g) {
    if (nj <= 0 || windows <= 0 || nn <= 0) return hipSuccess;
    if (nj > UTL_CHUNK) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(g, 0, 2 * sizeof(int32_t), st);
    if (e == hipSuccess)
        e = launch_utl_group(st, nn, H, slot_min, jcpu, jmem, jgpu, jwall, jk, kmax, node, start, t0, nj, windows, n,
                             inv, cnt, first, fill, touched, win, nullptr, g);
    if (e != hipSuccess) return e;
    const int32_t cap = std::min(windows, nn);
    hipLaunchKernelGGL(k_utl_apply, dim3(cap), dim3(64), sizeof(int32_t) * 3 * (size_t)H, st, hdr, slab, H, touched,
                       cap, cnt, first, win, windows, g);
    return hipGetLastError();
}

}  // namespace fitgpu

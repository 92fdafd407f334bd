// fit_hold_tl.hip — re-apply recorded reservations to the loaded timeline: per row, its demand
// subtracted from the slots [start, start + d) of every one of its recorded nodes, unless a slot of
// one of its windows cannot carry the sum of ALL the call's windows on it (include/fitgpu.h
// fit_hold_tl).  gfx950.
//
// Ordinary bounded launches on the context's stream.  The node id -> position table, the check of
// the whole batch and the grouping of the windows by node are fit_unplace_tl.hip's (launch_utl_inverse,
// launch_utl_check, launch_utl_group: the rows are its rows, field for field; a row on a node in no
// partition is refused by the grouping's count).  After the host has seen the bad-input flag and the
// window count, on the windows of the WHOLE call:
//   k_htl_judge   : ONE wave (a 64-thread workgroup) per touched node.  The wave expands the node's
//                   run list to its dense H slots x 3 columns in LDS as the ROOM of each slot, takes
//                   every window of the node off it with arithmetic that saturates below instead of
//                   wrapping, and so knows the over slots: the ones whose room went below zero in any
//                   column (a -1 slot starts below zero).  An inclusive count of the over slots then
//                   answers each window in two LDS reads, 64 windows per step; a window that covers
//                   an over slot ORs its row's refused flag (an integer atomic).  The timeline is not
//                   written.
//   k_htl_apply   : after the judge pass on the stream, one wave per touched node again: expand,
//                   subtract the windows of the rows whose flag is clear, write the canonical run
//                   list back with cnt, head[] and the exact ceilings.
//   k_htl_final   : one thread per row: out_state, and per wave one 64-bit atomic for each count
// Expansion, window loop, write-back and header refresh are fit_tl_dense.h's.
// The grouping covers the whole call, not a chunk of it: the judging of §2j is per call.
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; integer
// atomics and disjoint stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_dense.h"

namespace fitgpu {

// room left after one more demand (>= 0); it stops at TL_OVER instead of wrapping, and a room below
// zero never comes back: three demands of INT32_MAX leave an INT32_MAX slot below zero
__device__ __forceinline__ int32_t htl_take(int32_t room, int32_t dem) {
    return (int32_t)max<int64_t>((int64_t)room - dem, TL_OVER);
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_htl_judge(const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab,
                                                  int32_t H, const int32_t* __restrict__ touched, int32_t cap,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ first,
                                                  const TlWin* __restrict__ win, int32_t wcap, int32_t nj,
                                                  int32_t* __restrict__ flag, const int32_t* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) int32_t htl_dense[];
    const int b = blockIdx.x;
    if (b >= min(g[0], cap)) return;
    const int lane = threadIdx.x;
    const int32_t pos = touched[b];
    int32_t* dc = htl_dense;
    int32_t* dm = dc + H;
    int32_t* dg = dm + H;
    tl_dense_expand<true>(slab + (int64_t)pos * TL_MAX_SLOTS, min(hdr[pos].cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    __syncthreads();
    const int32_t w0 = first[pos], nw = cnt[pos];
    tl_dense_windows(win, w0, nw, wcap, H, lane, dc, dm, dg, htl_take);  // every live window counts
    __syncthreads();

    // ---- the over slots, counted inclusively into the cpu column: dc[s] = over slots in [0, s]
    int32_t run = 0;
    for (int base = 0; base < H; base += 64) {
        const int s = base + lane;
        const bool over = s < H && (dc[s] < 0 || dm[s] < 0 || dg[s] < 0);
        const uint64_t mk = __ballot(over);
        if (s < H) dc[s] = run + lanes_below(mk) + (over ? 1 : 0);
        run += __popcll(mk);
    }
    __syncthreads();
    if (run == 0) return;  // the common case: nothing on this node is refused

    // ---- a window that covers an over slot refuses its row
    for (int i0 = 0; i0 < nw; i0 += 64) {
        const int32_t wi = w0 + i0 + lane;
        if (i0 + lane >= nw || wi < 0 || wi >= wcap) continue;
        const TlWin w = win[wi];
        const int32_t ws = max(w.s, 0), we = min(w.e, H);
        if (we <= ws || w.row < 0 || w.row >= nj) continue;
        if (dc[we - 1] - (ws > 0 ? dc[ws - 1] : 0) > 0) atomicOr(&flag[w.row], 1);
    }
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_htl_apply(TlHdr* hdr, Seg* slab, int32_t H,
                                                  const int32_t* __restrict__ touched, int32_t cap,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ first,
                                                  const TlWin* __restrict__ win, int32_t wcap, int32_t nj,
                                                  const int32_t* __restrict__ flag, const int32_t* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) int32_t htl_dense[];
    const int b = blockIdx.x;
    if (b >= min(g[0], cap)) return;
    const int lane = threadIdx.x;
    const int32_t pos = touched[b];
    int32_t* dc = htl_dense;
    int32_t* dm = dc + H;
    int32_t* dg = dm + H;
    TlHdr* hp = hdr + pos;
    Seg* sg = slab + (int64_t)pos * TL_MAX_SLOTS;
    tl_dense_expand<false>(sg, min(hp->cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    __syncthreads();

    // ---- subtract the held windows: the judge pass found sum <= value on each of their slots, so
    // nothing clamps, nothing goes below 0 and no -1 slot is covered
    const bool held_here = tl_dense_windows(
        win, first[pos], cnt[pos], wcap, H, lane, dc, dm, dg, [](int32_t v, int32_t dem) { return v - dem; },
        [&](const TlWin& w, bool have) -> int { return have && w.row >= 0 && w.row < nj && flag[w.row] == 0; });
    if (!held_here) return;  // every window of the node is refused: its list stays as it is
    __syncthreads();
    const TlDenseOut o = tl_dense_write(sg, H, lane, dc, dm, dg);
    tl_refresh_head(hp, sg, o.no, H, lane);
    if (lane == 0) {
        hp->cpu = o.xc;  // the wave maximum is at hand: the ceilings are exact again, as after a load
        hp->mem = o.xm;
        hp->gpu = o.xg;
    }
}

// tot[0]: nodes of the held rows (*applied); tot[1]: refused rows
__global__ __launch_bounds__(256) void k_htl_final(const uint16_t* __restrict__ jk, int32_t kmax,
                                                   const int32_t* __restrict__ start, int32_t nj,
                                                   const int32_t* __restrict__ flag, int32_t* __restrict__ out_state,
                                                   unsigned long long* __restrict__ tot) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t add = 0, ref = 0;
    if (q < nj) {
        int32_t st = -1;  // FIT_HOLD_SKIPPED
        if (start[q] >= 0) {
            ref = flag[q] != 0;
            st = ref ? 0 : 1;  // FIT_HOLD_REFUSED : FIT_HOLD_HELD
            add = ref ? 0 : tl_need(jk, q, kmax);
        }
        out_state[q] = st;
    }
    // every lane of the wave is here
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        add += __shfl_xor(add, off);
        ref += __shfl_xor(ref, off);
    }
    if (lane == 0) {
        if (add) atomicAdd(&tot[0], (unsigned long long)add);
        if (ref) atomicAdd(&tot[1], (unsigned long long)ref);
    }
}

// The whole call's `windows` windows (launch_utl_check's count, summed) grouped by node, judged and
// applied on stream st.  cnt[nn], flag[nj] and g[0..1] are zero on entry; win holds `windows` entries,
// touched min(windows, nn).  Nothing is written to the timeline before k_htl_apply.
hipError_t launch_htl_hold(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, int32_t slot_min,
                           const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                           const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t nj,
                           int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                           int32_t* fill, int32_t* touched, TlWin* win, int32_t* flag, int32_t* g) {
    if (nj <= 0 || windows <= 0) return hipSuccess;
    hipError_t e = launch_utl_group(st, nn, H, slot_min, jcpu, jmem, jgpu, jwall, jk, kmax, node, start, 0, nj, windows,
                                    n, inv, cnt, first, fill, touched, win, flag, g);
    const int32_t cap = std::min(windows, nn);  // distinct nodes the call can touch
    if (e != hipSuccess || cap <= 0) return e;
    const size_t lds = sizeof(int32_t) * 3 * (size_t)H;
    hipLaunchKernelGGL(k_htl_judge, dim3(cap), dim3(64), lds, st, hdr, slab, H, touched, cap, cnt, first, win, windows,
                       nj, flag, g);
    hipLaunchKernelGGL(k_htl_apply, dim3(cap), dim3(64), lds, st, hdr, slab, H, touched, cap, cnt, first, win, windows,
                       nj, flag, g);
    return hipGetLastError();
}

// out_state of every row and the two counts; tot[0..1] are zero on entry
hipError_t launch_htl_final(hipStream_t st, const uint16_t* jk, int32_t kmax, const int32_t* start, int32_t nj,
                            const int32_t* flag, int32_t* out_state, unsigned long long* tot) {
    if (nj <= 0) return hipSuccess;
    if (kmax < 1 || kmax > FIT_KMAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_htl_final, dim3((nj + 255) / 256), dim3(256), 0, st, jk, kmax, start, nj, flag, out_state,
                       tot);
    return hipGetLastError();
}

}  // namespace fitgpu

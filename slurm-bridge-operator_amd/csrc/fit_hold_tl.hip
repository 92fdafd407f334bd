// fit_hold_tl.hip — re-apply recorded reservations to the loaded timeline: per row, its demand
// subtracted from the slots [start, start + d) of every one of its recorded nodes, unless a slot of
// one of its windows cannot carry the sum of ALL the call's windows on it (include/fitgpu.h
// fit_hold_tl).  gfx950.
//
// Ordinary bounded launches on the context's stream.  The node id -> position table and the check of
// the whole batch are fit_unplace_tl's (launch_utl_inverse, launch_utl_check: the rows are its rows,
// field for field); after the host has seen the bad-input flag and the window count:
//   k_htl_count   : one thread per row of the WHOLE call: an integer atomic per touched node counts
//                   its windows; the thread that takes a node's count from 0 appends the node to the
//                   touched list.  A node in no partition has no run list: every slot of it reads -1,
//                   so the row is refused here.
//   k_htl_offsets : one thread per touched node: its range of the window array
//   k_htl_scatter : one thread per row: its windows, each with its row index, into their nodes' ranges
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
//                   list back (k_utl_apply's write-back) with cnt, head[] and the exact ceilings.
//   k_htl_final   : one thread per row: out_state, and per wave one 64-bit atomic for each count
// The grouping covers the whole call, not a chunk of it: the judging of §2j is per call.
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; integer
// atomics and disjoint stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_reserve.h"

namespace fitgpu {

static_assert(sizeof(HtlWin) == 32, "one window is two 16-byte loads");

constexpr int32_t HTL_OVER = INT32_MIN;  // the room of a slot that cannot be used at all

// d of §2j: max(1, ceil(wall / slot_min)), a negative wall counting as 0 (k_utl_scatter's `d`)
__device__ __forceinline__ int32_t htl_dur(int32_t wall, int32_t slot_min) {
    const int64_t dw = ((int64_t)max(wall, 0) + slot_min - 1) / slot_min;
    return (int32_t)max<int64_t>(1, min<int64_t>(dw, 0x7fffffff));
}

// need of a row that k_utl_check passed (need <= kmax <= FIT_KMAX), clamped all the same
__device__ __forceinline__ int32_t htl_need(const uint16_t* jk, int q, int32_t kmax) {
    return min(max(jk ? (int32_t)jk[q] : 1, 1), min(kmax, FIT_KMAX));
}

// g[0]: touched nodes so far
__global__ __launch_bounds__(256) void k_htl_count(const uint16_t* __restrict__ jk, int32_t kmax,
                                                   const int32_t* __restrict__ node,
                                                   const int32_t* __restrict__ start, int32_t nj, int32_t n,
                                                   const int32_t* __restrict__ inv, int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ touched, int32_t cap,
                                                   int32_t* __restrict__ flag, int32_t* __restrict__ g) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    if (start[q] < 0) return;
    const int32_t need = htl_need(jk, q, kmax);
    for (int i = 0; i < need; ++i) {
        const int32_t id = node[(int64_t)q * kmax + i];
        const int32_t pos = id >= 0 && id < n ? inv[id] : -1;  // in range: k_utl_check passed the batch
        if (pos < 0) {  // a node in no partition: every slot reads -1, which no demand fits
            flag[q] = 1;
            continue;
        }
        if (atomicAdd(&cnt[pos], 1) == 0) {
            const int32_t k = atomicAdd(&g[0], 1);
            if (k < cap) touched[k] = pos;  // cap >= the distinct nodes the call can name: always true
        }
    }
}

// g[1]: windows handed out so far.  first[pos]: the node's range start; fill[pos]: its scatter cursor.
__global__ __launch_bounds__(256) void k_htl_offsets(const int32_t* __restrict__ touched, int32_t cap,
                                                     const int32_t* __restrict__ cnt, int32_t* __restrict__ first,
                                                     int32_t* __restrict__ fill, int32_t* __restrict__ g) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= min(g[0], cap)) return;
    const int32_t pos = touched[t];
    const int32_t o = atomicAdd(&g[1], cnt[pos]);
    first[pos] = o;
    fill[pos] = o;
}

__global__ __launch_bounds__(256) void k_htl_scatter(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jk, int32_t kmax,
    const int32_t* __restrict__ node, const int32_t* __restrict__ start, int32_t nj, int32_t H, int32_t slot_min,
    int32_t n, const int32_t* __restrict__ inv, int32_t* __restrict__ fill, HtlWin* __restrict__ win,
    int32_t wcap) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int32_t s = start[q];
    if (s < 0) return;
    const int32_t need = htl_need(jk, q, kmax);
    const int32_t d = htl_dur(jwall[q], slot_min);
    const int32_t e = (int32_t)min<int64_t>((int64_t)s + d, H);  // clipped at the horizon
    const HtlWin w{s, e, jcpu[q], jmem[q], jgpu[q], q, {0, 0}};
    for (int i = 0; i < need; ++i) {
        const int32_t id = node[(int64_t)q * kmax + i];
        const int32_t pos = id >= 0 && id < n ? inv[id] : -1;
        if (pos < 0) continue;
        const int32_t k = atomicAdd(&fill[pos], 1);
        if (k >= 0 && k < wcap) win[k] = w;  // k < the call's window total <= wcap
    }
}

// The node's run list, dense in LDS, by the whole wave: 64 runs per load, then run by run the wave
// fills the run's slots (k_utl_apply's expansion).  ROOM: a value below 0 becomes HTL_OVER.
template <bool ROOM>
__device__ __forceinline__ void htl_expand(const Seg* sg, int n, int32_t H, int lane, int32_t* dc, int32_t* dm,
                                           int32_t* dg) {
    int32_t a = 0;  // end of the runs expanded so far
    for (int r0 = 0; r0 < n; r0 += 64) {
        const Seg mine = r0 + lane < n ? sg[r0 + lane] : Seg{H, -1, -1, -1};
        const int m = min(64, n - r0);
        for (int k = 0; k < m; ++k) {
            const int32_t e = min(max(__shfl(mine.end, k), a), H);  // canonical lists only grow
            int32_t vc = __shfl(mine.cpu, k), vm = __shfl(mine.mem, k), vg = __shfl(mine.gpu, k);
            if (ROOM) {
                vc = vc < 0 ? HTL_OVER : vc;
                vm = vm < 0 ? HTL_OVER : vm;
                vg = vg < 0 ? HTL_OVER : vg;
            }
            for (int s = a + lane; s < e; s += 64) {
                dc[s] = vc;
                dm[s] = vm;
                dg[s] = vg;
            }
            a = e;
        }
    }
    for (int s = a + lane; s < H; s += 64) dc[s] = dm[s] = dg[s] = ROOM ? HTL_OVER : -1;  // a list that stops short
}

// room left after one more demand (>= 0); it stops at HTL_OVER instead of wrapping, and a room below
// zero never comes back: three demands of INT32_MAX leave an INT32_MAX slot below zero
__device__ __forceinline__ int32_t htl_take(int32_t room, int32_t dem) {
    return (int32_t)max<int64_t>((int64_t)room - dem, HTL_OVER);
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_htl_judge(const TlHdr* __restrict__ hdr, const Seg* __restrict__ slab,
                                                  int32_t H, const int32_t* __restrict__ touched, int32_t cap,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ first,
                                                  const HtlWin* __restrict__ win, int32_t wcap, int32_t nj,
                                                  int32_t* __restrict__ flag, const int32_t* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) int32_t htl_dense[];
    const int b = blockIdx.x;
    if (b >= min(g[0], cap)) return;
    const int lane = threadIdx.x;
    const int32_t pos = touched[b];
    int32_t* dc = htl_dense;
    int32_t* dm = dc + H;
    int32_t* dg = dm + H;
    htl_expand<true>(slab + (int64_t)pos * TL_MAX_SLOTS, min(hdr[pos].cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    __syncthreads();

    // ---- take: 64 windows per load, a window's slots 64 per step; every live window counts
    const int32_t w0 = first[pos], nw = cnt[pos];
    for (int i0 = 0; i0 < nw; i0 += 64) {
        const int32_t wi = w0 + i0 + lane;
        const HtlWin mine = (i0 + lane < nw && wi >= 0 && wi < wcap) ? win[wi] : HtlWin{0, 0, 0, 0, 0, 0, {0, 0}};
        const int m = min(64, nw - i0);
        for (int k = 0; k < m; ++k) {
            const int32_t ws = max(__shfl(mine.s, k), 0), we = min(__shfl(mine.e, k), H);
            const int32_t jc = __shfl(mine.cpu, k), jm = __shfl(mine.mem, k), jg = __shfl(mine.gpu, k);
            for (int s = ws + lane; s < we; s += 64) {
                dc[s] = htl_take(dc[s], jc);
                dm[s] = htl_take(dm[s], jm);
                dg[s] = htl_take(dg[s], jg);
            }
            __syncthreads();  // one wave: the next window's lanes read what these lanes stored
        }
    }
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
        const HtlWin w = win[wi];
        const int32_t ws = max(w.s, 0), we = min(w.e, H);
        if (we <= ws || w.row < 0 || w.row >= nj) continue;
        if (dc[we - 1] - (ws > 0 ? dc[ws - 1] : 0) > 0) atomicOr(&flag[w.row], 1);
    }
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_htl_apply(TlHdr* hdr, Seg* slab, int32_t H,
                                                  const int32_t* __restrict__ touched, int32_t cap,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ first,
                                                  const HtlWin* __restrict__ win, int32_t wcap, int32_t nj,
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
    htl_expand<false>(sg, min(hp->cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    __syncthreads();

    // ---- subtract the held windows: the judge pass found sum <= value on each of their slots, so
    // nothing clamps, nothing goes below 0 and no -1 slot is covered
    const int32_t w0 = first[pos], nw = cnt[pos];
    int held_here = 0;
    for (int i0 = 0; i0 < nw; i0 += 64) {
        const int32_t wi = w0 + i0 + lane;
        const bool have = i0 + lane < nw && wi >= 0 && wi < wcap;
        const HtlWin mine = have ? win[wi] : HtlWin{0, 0, 0, 0, 0, 0, {0, 0}};
        const int held = have && mine.row >= 0 && mine.row < nj && flag[mine.row] == 0;
        const int m = min(64, nw - i0);
        for (int k = 0; k < m; ++k) {
            if (!__shfl(held, k)) continue;  // wave-uniform
            held_here = 1;
            const int32_t ws = max(__shfl(mine.s, k), 0), we = min(__shfl(mine.e, k), H);
            const int32_t jc = __shfl(mine.cpu, k), jm = __shfl(mine.mem, k), jg = __shfl(mine.gpu, k);
            for (int s = ws + lane; s < we; s += 64) {
                dc[s] -= jc;
                dm[s] -= jm;
                dg[s] -= jg;
            }
            __syncthreads();  // one wave: the next window's lanes read what these lanes stored
        }
    }
    if (!held_here) return;  // every window of the node is refused: its list stays as it is
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
        hp->cpu = xc;  // the wave maximum is at hand: the ceilings are exact again, as after a load
        hp->mem = xm;
        hp->gpu = xg;
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
            add = ref ? 0 : htl_need(jk, q, kmax);
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
                           int32_t* fill, int32_t* touched, HtlWin* win, int32_t* flag, int32_t* g) {
    if (nj <= 0 || windows <= 0) return hipSuccess;
    if (kmax < 1 || kmax > FIT_KMAX || (int64_t)windows > (int64_t)nj * kmax || H < 1 || H > TL_MAX_SLOTS ||
        slot_min < 1 || nn < 0)
        return hipErrorInvalidValue;
    const int32_t cap = std::min(windows, nn);  // distinct nodes the call can touch
    const dim3 rows((nj + 255) / 256), th(256);
    hipLaunchKernelGGL(k_htl_count, rows, th, 0, st, jk, kmax, node, start, nj, n, inv, cnt, touched, cap, flag, g);
    if (cap > 0) {
        const dim3 nodes((cap + 255) / 256);
        const size_t lds = sizeof(int32_t) * 3 * (size_t)H;
        hipLaunchKernelGGL(k_htl_offsets, nodes, th, 0, st, touched, cap, cnt, first, fill, g);
        hipLaunchKernelGGL(k_htl_scatter, rows, th, 0, st, jcpu, jmem, jgpu, jwall, jk, kmax, node, start, nj, H,
                           slot_min, n, inv, fill, win, windows);
        hipLaunchKernelGGL(k_htl_judge, dim3(cap), dim3(64), lds, st, hdr, slab, H, touched, cap, cnt, first, win,
                           windows, nj, flag, g);
        hipLaunchKernelGGL(k_htl_apply, dim3(cap), dim3(64), lds, st, hdr, slab, H, touched, cap, cnt, first, win,
                           windows, nj, flag, g);
    }
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

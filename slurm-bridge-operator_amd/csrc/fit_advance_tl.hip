// fit_advance_tl.hip — move the loaded timeline forward with the clock: every node's run list
// shifted left by a slots, 1 <= a <= H, and a tail run for the a new slots at the far end
// (include/fitgpu.h fit_advance_tl).  gfx950.
//
// Ordinary bounded launches on the context's stream:
//   k_atl_check : one thread per caller's node id: a tail entry below -1 raises the bad-input flag.
//                 Nothing is written to the timeline before the host has seen the flag.
//   k_atl_move  : ONE wave (a 64-thread workgroup) per node position, whatever the list's length.
//                 64 runs per step into registers: drop the runs that end at or before a, store the
//                 survivors at `index - dropped` with `end - a`, merge or append the tail run
//                 {H, tail}, take the exact column maxima on the way; the wave then waits for its
//                 own list stores and re-reads the first TL_HEAD runs for the header
//                 (tl_refresh_head).  A sub-wave group of 8 lanes per short list, with one wave per longer list
//                 in a second launch, was built and measured: it did not win.
// The move is in place.  That is safe because (1) a lane's store needs its own load's data, and a
// wave's load instruction has returned for all 64 lanes before the store instruction that uses it
// issues: one step's loads all precede its stores; (2) dropped >= 0, so the stores of the step that
// loaded runs [r0, r0 + 64) land at indices < r0 + 64, below everything a later step loads, and the
// last run — whose values decide between merge and append — is loaded before the first store; (3) a
// position belongs to exactly one wave: no other wave touches its list or its header.  A canonical
// list has at most H - a survivors (their new ends are distinct in [1, H - a]), so with the tail
// run at most H <= TL_MAX_SLOTS: the slab row cannot overflow.
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; disjoint
// stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_dense.h"

namespace fitgpu {

__global__ __launch_bounds__(256) void k_atl_check(const int32_t* __restrict__ tc, const int32_t* __restrict__ tm,
                                                   const int32_t* __restrict__ tg, int32_t n,
                                                   int32_t* __restrict__ g) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    if (tc[x] < -1 || tm[x] < -1 || tg[x] < -1) atomicOr(g, 1);
}

// §2i, one column of the tail run: a column that is -1 at slot H - 1 stays -1; otherwise the
// caller's level (>= -1: k_atl_check passed it), or with no tails the slot H - 1 value itself
__device__ __forceinline__ int32_t atl_tail(int32_t last, const int32_t* __restrict__ t, int32_t orig, int32_t n) {
    if (last == -1 || !t || orig < 0 || orig >= n) return last;
    return max(t[orig], -1);
}

// grid = node positions; workgroup = one wave.  The strided loop makes one pass (grid = nn); it is
// kept because the same body without it measured 53-54 us against 41 us.
__global__ __launch_bounds__(64) void k_atl_move(TlHdr* hdr, Seg* slab, int32_t nn, int32_t n, int32_t H, int32_t a,
                                                 const int32_t* __restrict__ tc, const int32_t* __restrict__ tm,
                                                 const int32_t* __restrict__ tg) {
    const int lane = threadIdx.x;
    for (int32_t pos = blockIdx.x; pos < nn; pos += gridDim.x) {
        TlHdr* hp = hdr + pos;
        Seg* sg = slab + (int64_t)pos * TL_MAX_SLOTS;
        const int cnt = min(max(hp->cnt, 0), TL_MAX_SLOTS);
        const int32_t orig = hp->orig;
        const Seg last = cnt > 0 ? sg[cnt - 1] : Seg{H, -1, -1, -1};  // before the first store
        const int32_t vc = atl_tail(last.cpu, tc, orig, n), vm = atl_tail(last.mem, tm, orig, n),
                      vg = atl_tail(last.gpu, tg, orig, n);
        const bool merge = cnt > 0 && last.end > a && last.cpu == vc && last.mem == vm && last.gpu == vg;
        int no = 0;
        int32_t xc = vc, xm = vm, xg = vg;
        for (int r0 = 0; r0 < cnt; r0 += 64) {
            const int i = r0 + lane;
            const Seg r = i < cnt ? sg[i] : Seg{H, -1, -1, -1};
            const bool keep = i < cnt && r.end > a;
            const uint64_t mk = __ballot(keep);
            if (keep) {
                sg[no + lanes_below(mk)] = Seg{i == cnt - 1 && merge ? H : r.end - a, r.cpu, r.mem, r.gpu};  // <= i
                xc = max(xc, r.cpu);
                xm = max(xm, r.mem);
                xg = max(xg, r.gpu);
            }
            no += __popcll(mk);
        }
        if (!merge) {
            if (lane == 0 && no < TL_MAX_SLOTS) sg[no] = Seg{H, vc, vm, vg};  // no <= H - a: always true
            no = min(no + 1, TL_MAX_SLOTS);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            xc = max(xc, __shfl_xor(xc, off));
            xm = max(xm, __shfl_xor(xm, off));
            xg = max(xg, __shfl_xor(xg, off));
        }
        tl_refresh_head(hp, sg, no, H, lane);
        if (lane == 0) {
            hp->cpu = xc;  // exact: the only place a ceiling ever falls
            hp->mem = xm;
            hp->gpu = xg;
        }
    }
}

hipError_t launch_atl_check(hipStream_t st, const int32_t* tc, const int32_t* tm, const int32_t* tg, int32_t n,
                            int32_t* g) {
    if (n <= 0) return hipSuccess;
    if (!tc || !tm || !tg) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_atl_check, dim3((n + 255) / 256), dim3(256), 0, st, tc, tm, tg, n, g);
    return hipGetLastError();
}

hipError_t launch_atl_advance(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t n, int32_t H, int32_t a,
                              const int32_t* tc, const int32_t* tm, const int32_t* tg) {
    if (nn <= 0) return hipSuccess;
    if (H < 1 || H > TL_MAX_SLOTS || a < 1 || a > H || (!tc != !tm) || (!tc != !tg)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_atl_move, dim3(nn), dim3(64), 0, st, hdr, slab, nn, n, H, a, tc, tm, tg);
    return hipGetLastError();
}

}  // namespace fitgpu

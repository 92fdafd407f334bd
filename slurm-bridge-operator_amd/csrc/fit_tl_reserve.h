// fit_tl_reserve.h — the wave-cooperative general reservation on one node's run list (DESIGN.md
// §3.8), shared by the backfill engines (fit_timeline.hip) and the multi-node backfill
// (fit_place_tl_k.hip).  Moved here verbatim from fit_timeline.hip: both functions are
// __forceinline__, so the engines' generated code is what it was.
#pragma once
#include <hip/hip_runtime.h>

#include "fit_device.h"

namespace fitgpu {

__device__ __forceinline__ int lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// Reserve (jc, jm, jg) on slots [s, e) of a run list, general form (any length, any address
// space), by the whole wave: the runs from the one before the window to the end are split at s
// and e into LDS scratch (prefix sums over piece counts), equal neighbours merge, and the result
// is written back.  Returns the new run count.
__device__ __forceinline__ int tl_reserve_any(Seg* sg, int n, int32_t s, int32_t e, int32_t jc,
                                              int32_t jm, int32_t jg, Seg* scr) {
    const int lane = threadIdx.x & 63;
    int i0 = n;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        const uint64_t m = __ballot(i < n && sg[i].end > s);
        if (m) {
            i0 = b + __builtin_ctzll(m);
            break;
        }
    }
    const int r0 = max(i0 - 1, 0);
    int np = 0;
    for (int b = r0; b < n; b += 64) {
        const int i = b + lane;
        const bool v = i < n;
        const Seg g = v ? sg[i] : Seg{0, 0, 0, 0};
        const int32_t a = (v && i > 0) ? sg[i - 1].end : 0;
        const bool ov = v && a < e && g.end > s;
        const bool hd = ov && a < s;
        const bool tl = ov && g.end > e;
        const int pc = v ? (ov ? 1 + (int)hd + (int)tl : 1) : 0;
        const uint64_t m0 = __ballot(pc & 1), m1 = __ballot(pc >> 1);
        int o = np + lanes_below(m0) + 2 * lanes_below(m1);
        if (v) {
            if (!ov) {
                scr[o] = g;
            } else {
                if (hd) scr[o++] = Seg{s, g.cpu, g.mem, g.gpu};
                scr[o++] = Seg{min(g.end, e), g.cpu - jc, g.mem - jm, g.gpu - jg};
                if (tl) scr[o] = g;
            }
        }
        np += __popcll(m0) + 2 * __popcll(m1);
    }
    int no = 0;
    for (int b = 0; b < np; b += 64) {
        const int k = b + lane;
        const Seg p = k < np ? scr[k] : Seg{0, 0, 0, 0};
        const Seg q = k + 1 < np ? scr[k + 1] : Seg{0, -2, -2, -2};
        const bool keep = k < np && (k + 1 >= np || p.cpu != q.cpu || p.mem != q.mem || p.gpu != q.gpu);
        const uint64_t mk = __ballot(keep);
        if (keep) sg[r0 + no + lanes_below(mk)] = p;
        no += __popcll(mk);
    }
    return r0 + no;
}

}  // namespace fitgpu

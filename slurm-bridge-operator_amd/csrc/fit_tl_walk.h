// fit_tl_walk.h — the exact earliest-start walk over one node's run list (SPEC §2b; DESIGN.md
// §3.8) and its key, shared by the backfill engines (fit_timeline.hip), the multi-node backfill
// (fit_place_tl_k.hip) and the read-only queries (fit_when.hip, fit_when_k.hip).  Every function is
// __forceinline__.
#pragma once
#include <hip/hip_runtime.h>

#include "fit_device.h"
#include "fit_key.h"  // fit_score: the score field of tl_key

namespace fitgpu {

__device__ __forceinline__ uint64_t tl_key(int32_t s, int32_t mc, int32_t mm, int32_t mg,
                                           int32_t jc, int32_t jm, int32_t jg, uint32_t pos) {
    const int32_t dg = mg - jg, dc = mc - jc, dm = mm - jm;  // (g, c, m: the order tl_key always had)
    const uint32_t sc = fit_score(dc, dm, dg);
    return ((uint64_t)(uint32_t)s << 54) | ((uint64_t)sc << TL_POS_BITS) | pos;
}

// Per-lane state of the earliest-start walk over one node's runs.
struct TlWalk {
    int32_t ra, mc, mm, mg, a;  // start of the current feasible stretch (-1: none), its minima, run start
    bool live;
    // the first d-slot stretch's start and minima, frozen when it completes; the key is packed
    // once after the walk (tl_walk_key) instead of at every run (C5 129.4 -> 128.1 ms, round 3)
    int32_t kra, kmc, kmm, kmg;
    bool got;
};
__device__ __forceinline__ TlWalk tl_walk0(bool live) {
    return TlWalk{-1, 0, 0, 0, 0, live, 0, 0, 0, 0, false};
}

// One run: extend / break the feasible stretch; a stretch of d slots gives the key.  A lane
// stops once every start it could still find is later than `lim` (the start of its cut key).
// Straight-line: every lane computes the step, only a live lane's key / liveness change (a
// finished lane's stretch fields are never read again), so lanes that diverge on "fits" cost no
// exec-mask branches.  `vld` false: a lane's runs past its list's end (it stays false for the
// rest of the walk, so only the key and liveness need the gate).
__device__ __forceinline__ void tl_step_v(TlWalk& w, bool vld, int32_t end, int32_t c, int32_t m,
                                          int32_t g, int32_t jc, int32_t jm, int32_t jg, int32_t d,
                                          int32_t H, int32_t lim, uint32_t pos) {
    const bool f = (c >= jc) & (m >= jm) & (g >= jg);
    const bool nw = w.ra < 0;
    const int32_t ra = f ? (nw ? w.a : w.ra) : -1;
    const int32_t mc = nw ? c : min(w.mc, c), mm = nw ? m : min(w.mm, m), mg = nw ? g : min(w.mg, g);
    const bool done = f & (end - ra >= d);
    const bool kill = f ? (ra > lim) : ((end + d > H) | (end > lim));
    const bool fin = w.live & vld & done;
    w.kra = fin ? ra : w.kra;
    w.kmc = fin ? mc : w.kmc;
    w.kmm = fin ? mm : w.kmm;
    w.kmg = fin ? mg : w.kmg;
    w.got = w.got | fin;
    w.live = vld ? (w.live & !done & !kill) : w.live;
    w.ra = ra;
    w.mc = mc;
    w.mm = mm;
    w.mg = mg;
    w.a = end;
}

__device__ __forceinline__ void tl_step(TlWalk& w, int32_t end, int32_t c, int32_t m, int32_t g,
                                        int32_t jc, int32_t jm, int32_t jg, int32_t d, int32_t H,
                                        int32_t lim, uint32_t pos) {
    tl_step_v(w, true, end, c, m, g, jc, jm, jg, d, H, lim, pos);
}

// the walk's key (KEY_INF: no window found)
__device__ __forceinline__ uint64_t tl_walk_key(const TlWalk& w, int32_t jc, int32_t jm,
                                                int32_t jg, uint32_t pos) {
    return w.got ? tl_key(w.kra, w.kmc, w.kmm, w.kmg, jc, jm, jg, pos) : KEY_INF;
}

}  // namespace fitgpu

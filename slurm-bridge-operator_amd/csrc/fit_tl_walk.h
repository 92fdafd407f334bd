// fit_tl_walk.h — reading one node's run list (SPEC §2b).  Every function is
// __forceinline__.
//   tl_key, TlWalk, tl_step(_v), tl_walk_key : the exact earliest-start walk and its key, for the
//       backfill engines (fit_timeline.hip) and fit_when.hip; the key also for the two below
//   tl_each_run, TL_WINDOW / tl_window, tl_keep, tl_first_start : what the multi-node kernels
//       (fit_when_k.hip, fit_place_tl_k.hip) share: the visit of every run, header then slab; the
//       one window [start, stop); a lane's sorted key list; the first common start from a
//       difference array
//   WinCols, tl_win_from / tl_win_until, tl_first_start_in : the per-job window of allowed starts of
//       the windowed instantiations (fit_when_k_win, fit_place_tl_k_win; SPEC §2r)
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
                                          int32_t H, int32_t lim) {
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
                                        int32_t lim) {
    tl_step_v(w, true, end, c, m, g, jc, jm, jg, d, H, lim);
}

// the walk's key (KEY_INF: no window found)
__device__ __forceinline__ uint64_t tl_walk_key(const TlWalk& w, int32_t jc, int32_t jm,
                                                int32_t jg, uint32_t pos) {
    return w.got ? tl_key(w.kra, w.kmc, w.kmm, w.kmg, jc, jm, jg, pos) : KEY_INF;
}

// ---- the multi-node kernels' pieces (fit_when_k.hip, fit_place_tl_k.hip) ----------------------

// Every run of one node, in order: the TL_HEAD runs of the header copy h, then the slab row sg four
// Seg per wait; cn = min(h.cnt, TL_MAX_SLOTS).  f(const Seg&) is called per run.  A batch is loaded
// whole, runs behind the list's end included (f never sees them): it stays inside the slab row
// because 4 divides TL_HEAD and TL_MAX_SLOTS, whatever cn is.  TL_WINDOW's loops rest on the same.
static_assert(TL_HEAD % 4 == 0 && TL_MAX_SLOTS % 4 == 0, "the visits load four Seg at a time inside a slab row");
template <class F>
__device__ __forceinline__ void tl_each_run(const TlHdr& h, const Seg* sg, int cn, F f) {
#pragma unroll
    for (int i = 0; i < TL_HEAD; ++i)
        if (i < cn) f(h.head[i]);
    for (int i = TL_HEAD; i < cn; i += 4) {
        Seg r4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r4[k] = sg[i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < cn) f(r4[k]);
    }
}

// The one window [start, stop) of a node: declares mc, mm, mg, the minima of the runs that meet the
// window, and fits: every one of them holds (cpu, mem, gpu) and the list reaches `stop`.  The visit
// is tl_each_run's, left at the first run that fails or closes the window.  A macro because
// k_whenk_nodes is 8 % slower through the function below and 24 % slower with the visit as a gated
// tl_each_run, the same loops scheduled differently (profiles/tl_runs_ab.txt); k_ptlk_commit, which
// is bound by its SGPRs, is the faster one through the function.
#define TL_WINDOW(h, sg, cn, start, stop, cpu, mem, gpu, mc, mm, mg, fits)                               \
    int32_t mc = 0x7fffffff, mm = 0x7fffffff, mg = 0x7fffffff;                                           \
    bool fits;                                                                                           \
    {                                                                                                    \
        bool ok = true, closed = false; /* closed: the runs seen cover the window */                     \
        /* runs end in increasing order and the walk stops at the first that reaches `stop`, so a run */ \
        /* meets the window exactly when it ends behind `start` */                                       \
        auto run = [&](const Seg& r) {                                                                   \
            if (r.end <= start) return;                                                                  \
            ok = (r.cpu >= cpu) & (r.mem >= mem) & (r.gpu >= gpu);                                       \
            mc = min(mc, r.cpu);                                                                         \
            mm = min(mm, r.mem);                                                                         \
            mg = min(mg, r.gpu);                                                                         \
            closed = r.end >= stop;                                                                      \
        };                                                                                               \
        _Pragma("unroll") for (int i = 0; i < TL_HEAD; ++i)                                              \
            if (i < cn && ok && !closed) run(h.head[i]);                                                 \
        for (int i = TL_HEAD; i < cn && ok && !closed; i += 4) {                                         \
            Seg r4[4];                                                                                   \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) r4[k] = sg[i + k];                             \
            _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                \
                if (i + k < cn && ok && !closed) run(r4[k]);                                             \
        }                                                                                                \
        fits = ok && closed;                                                                             \
    }
__device__ __forceinline__ bool tl_window(const TlHdr& h, const Seg* sg, int cn, int32_t start, int32_t stop,
                                          int32_t cpu, int32_t mem, int32_t gpu, int32_t& mc, int32_t& mm,
                                          int32_t& mg) {
    TL_WINDOW(h, sg, cn, start, stop, cpu, mem, gpu, c, m, g, fits)
    mc = c;
    mm = m;
    mg = g;
    return fits;
}

// Keep k if it is among the K smallest keys seen: key[] is a lane's sorted register list, k carries
// the larger one on.  Beside topk_insert (fit_common.h: compares first, then a clamp per entry, tuned
// for the scan) and PreTop (fit_preempt_k.hip: 128-bit keys), which stay as they are.
template <int K>
__device__ __forceinline__ void tl_keep(uint64_t (&key)[K], uint64_t k) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const uint64_t lo = min(k, key[i]);
        k = max(k, key[i]);
        key[i] = lo;
    }
}

// One wave over a difference array of H + 1 words (HBM or LDS): cnt(s), the number of nodes free for
// a start at s, is the prefix sum, taken 64 slots per step.  Starts lie in [0, H - d]; word H only
// takes -1s.  start: the first s with cnt(s) >= need (-1: none), ready: cnt(start), now: cnt(0),
// early: some s < start has cnt(s) > 0.  A caller pays for the results it reads only.
struct TlStart {
    int32_t start, ready, now;
    bool early;
};
__device__ __forceinline__ TlStart tl_first_start(const int32_t* diff, int32_t H, int32_t need, int lane) {
    TlStart r{-1, 0, diff[0], false};  // cnt(0) is the first word itself (H >= 1)
    int32_t carry = 0;
    for (int base = 0; base < H; base += 64) {
        const int s = base + lane;
        int32_t v = s < H ? diff[s] : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t u = __shfl_up(v, off);
            if (lane >= off) v += u;
        }
        v += carry;  // cnt(s)
        const uint64_t hit = __ballot(s < H && v >= need);
        const uint64_t some = __ballot(s < H && v > 0);
        if (hit) {
            const int first = __builtin_ctzll(hit);
            r.start = base + first;
            r.ready = __shfl(v, first);
            r.early |= (some & ((1ull << first) - 1ull)) != 0;
            break;
        }
        r.early |= some != 0;
        carry = __shfl(v, 63);
    }
    return r;
}

// ---- the window of allowed starts (SPEC §2r) ---------------------------------------------------

// The two optional job columns of the windowed entry points, as a kernel's last argument.  The
// unwindowed instantiation carries the empty struct and reads nothing of it.
template <bool WIN>
struct WinCols {};
template <>
struct WinCols<true> {
    const int32_t* nb;  // not_before per job; nullptr: all 0
    const int32_t* dl;  // deadline per job; nullptr: none
};
__device__ __forceinline__ int32_t tl_win_from(const WinCols<false>&, int, int32_t) { return 0; }
__device__ __forceinline__ int32_t tl_win_until(const WinCols<false>&, int, int32_t H) { return H; }
// from = clamp(not_before, 0, H), until = clamp(deadline, 0, H): no value is an error
__device__ __forceinline__ int32_t tl_win_from(const WinCols<true>& w, int q, int32_t H) {
    return w.nb ? min(max(w.nb[q], 0), H) : 0;
}
__device__ __forceinline__ int32_t tl_win_until(const WinCols<true>& w, int q, int32_t H) {
    return w.dl ? min(max(w.dl[q], 0), H) : H;
}

// tl_first_start over the allowed starts [from, last] only (last = until - d; the caller has
// from <= last < H).  The count walks clip every stretch to the window, so the words before `from`
// are zero and the words behind `last` take only -1s: the prefix sum may begin, with no carry, at
// the 64-slot block that holds `from`, and cnt(from) is the word at `from` itself.  now: cnt(from);
// early: some s in [from, start) has cnt(s) > 0.
__device__ __forceinline__ TlStart tl_first_start_in(const int32_t* diff, int32_t from, int32_t last, int32_t need,
                                                     int lane) {
    TlStart r{-1, 0, diff[from], false};
    int32_t carry = 0;
    for (int base = from & ~63; base <= last; base += 64) {
        const int s = base + lane;
        int32_t v = s <= last ? diff[s] : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t u = __shfl_up(v, off);
            if (lane >= off) v += u;
        }
        v += carry;  // cnt(s)
        const uint64_t hit = __ballot(s <= last && v >= need);
        const uint64_t some = __ballot(s <= last && v > 0);
        if (hit) {
            const int first = __builtin_ctzll(hit);
            r.start = base + first;
            r.ready = __shfl(v, first);
            r.early |= (some & ((1ull << first) - 1ull)) != 0;
            break;
        }
        r.early |= some != 0;
        carry = __shfl(v, 63);
    }
    return r;
}

}  // namespace fitgpu

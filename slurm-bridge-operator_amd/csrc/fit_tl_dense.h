// fit_tl_dense.h — the dense per-node edit of a run list, shared by the calls that write windows to
// the loaded timeline: fit_unplace_tl (k_utl_apply) and fit_hold_tl (k_htl_judge, k_htl_apply); the
// header refresh at its end is also fit_advance_tl's (k_atl_move) and fit_place_tl_k's
// (k_ptlk_commit); fit_evicted_tl (k_etl_apply) and fit_set_tl (k_stl_apply, with
// tl_dense_windows_slots for tl_dense_windows) run the same edit with their own window step.
// DESIGN.md §3.16.  Every piece is __forceinline__ and is called by one whole wave (a 64-thread
// workgroup, or one wave of a larger one for tl_refresh_head), so the kernels built from them compile
// to what they were when each spelled the pieces out.
//
// The edit: ONE wave per node expands the node's run list to H slots x 3 columns in LDS
// (tl_dense_expand), runs every window of the node over the columns, 64 slots per step
// (tl_dense_windows), writes the canonical run list back (tl_dense_write) and refreshes the node's
// header (tl_refresh_head).  The dense form costs H / 64 steps to expand and to write back whatever
// the node's windows are, and a window costs d / 64 steps: there is no slow case for many windows on
// one node, and the list that comes out is canonical by construction (at most H runs: the slab row
// cannot overflow).
#pragma once
#include <hip/hip_runtime.h>

#include "fit_device.h"
#include "fit_query.h"  // tl_dur, tl_need: a row's slots and node count
#include "fit_tl_reserve.h"

namespace fitgpu {

constexpr int32_t TL_OVER = INT32_MIN;  // ROOM columns: the room of a slot that cannot be used at all

// §2h, one column of one slot: -1 stays -1, any other value rises and saturates (fit_unplace_tl's
// and fit_evicted_tl's op)
__device__ __forceinline__ int32_t utl_add(int32_t v, int32_t dem) {
    return v == -1 ? -1 : (int32_t)min<int64_t>((int64_t)v + dem, 0x7fffffff);
}

// Expand: 64 runs per load, then run by run the wave fills the run's slots.  ROOM: the columns hold
// the room of each slot, a value below 0 becoming TL_OVER.  The caller's __syncthreads() follows.
template <bool ROOM>
__device__ __forceinline__ void tl_dense_expand(const Seg* sg, int n, int32_t H, int lane, int32_t* dc, int32_t* dm,
                                                int32_t* dg) {
    int32_t a = 0;  // end of the runs expanded so far
    for (int r0 = 0; r0 < n; r0 += 64) {
        const Seg mine = r0 + lane < n ? sg[r0 + lane] : Seg{H, -1, -1, -1};
        const int m = min(64, n - r0);
        for (int k = 0; k < m; ++k) {
            const int32_t e = min(max(__shfl(mine.end, k), a), H);  // canonical lists only grow
            int32_t vc = __shfl(mine.cpu, k), vm = __shfl(mine.mem, k), vg = __shfl(mine.gpu, k);
            if (ROOM) {
                vc = vc < 0 ? TL_OVER : vc;
                vm = vm < 0 ? TL_OVER : vm;
                vg = vg < 0 ? TL_OVER : vg;
            }
            for (int s = a + lane; s < e; s += 64) {
                dc[s] = vc;
                dm[s] = vm;
                dg[s] = vg;
            }
            a = e;
        }
    }
    for (int s = a + lane; s < H; s += 64) dc[s] = dm[s] = dg[s] = ROOM ? TL_OVER : -1;  // a list that stops short
}

// For each window of win[w0, w0 + nw): 64 windows per load, each broadcast in turn, its slots 64 per
// step through op(value, demand) on every column.  pick(window, loaded) is evaluated by the lane that
// loaded the window; a window whose pick is false is passed over (wave-uniform).  Returns whether
// any window was run.
struct TlEveryWindow {};
template <class Op, class Pick = TlEveryWindow>
__device__ __forceinline__ bool tl_dense_windows(const TlWin* __restrict__ win, int32_t w0, int32_t nw, int32_t wcap,
                                                 int32_t H, int lane, int32_t* dc, int32_t* dm, int32_t* dg, Op op,
                                                 Pick pick = {}) {
    constexpr bool ALL = __is_same(Pick, TlEveryWindow);
    int any = 0;
    for (int i0 = 0; i0 < nw; i0 += 64) {
        const int32_t wi = w0 + i0 + lane;
        const bool have = i0 + lane < nw && wi >= 0 && wi < wcap;
        const TlWin mine = have ? win[wi] : TlWin{0, 0, 0, 0, 0, 0, {0, 0}};
        [[maybe_unused]] int on = 1;
        if constexpr (!ALL) on = pick(mine, have);
        const int m = min(64, nw - i0);
        for (int k = 0; k < m; ++k) {
            if constexpr (!ALL)
                if (!__shfl(on, k)) continue;  // wave-uniform
            any = 1;
            const int32_t ws = max(__shfl(mine.s, k), 0), we = min(__shfl(mine.e, k), H);
            const int32_t jc = __shfl(mine.cpu, k), jm = __shfl(mine.mem, k), jg = __shfl(mine.gpu, k);
            for (int s = ws + lane; s < we; s += 64) {
                dc[s] = op(dc[s], jc);
                dm[s] = op(dm[s], jm);
                dg[s] = op(dg[s], jg);
            }
            __syncthreads();  // one wave: the next window's lanes read what these lanes stored
        }
    }
    return any;
}

// tl_dense_windows' sibling for an operation that is not a function of (value, demand) per column
// (fit_set_tl: the largest row index stands, kept in a fourth column): for each window of
// win[w0, w0 + nw), 64 per load and each broadcast in turn, op(slot, cpu, mem, gpu, row) for every
// slot of the window; the columns are op's own.  Slot s is lane s % 64's in EVERY window (a window
// starts its walk at the 64-slot boundary at or below its first slot), so whatever op keeps per slot
// is read and written by one lane in program order: the windows need no barrier between them.  The
// caller's barriers stand between this and the passes that walk the slots otherwise.
template <class SlotOp>
__device__ __forceinline__ void tl_dense_windows_slots(const TlWin* __restrict__ win, int32_t w0, int32_t nw,
                                                       int32_t wcap, int32_t H, int lane, SlotOp op) {
    for (int i0 = 0; i0 < nw; i0 += 64) {
        const int32_t wi = w0 + i0 + lane;
        const bool have = i0 + lane < nw && wi >= 0 && wi < wcap;
        const TlWin mine = have ? win[wi] : TlWin{0, 0, 0, 0, 0, 0, {0, 0}};
        const int m = min(64, nw - i0);
        for (int k = 0; k < m; ++k) {
            // k is wave-uniform: scalar reads of lane k's registers, no LDS round trip per window
            const int32_t ws = max(__builtin_amdgcn_readlane(mine.s, k), 0);
            const int32_t we = min(__builtin_amdgcn_readlane(mine.e, k), H);
            const int32_t jc = __builtin_amdgcn_readlane(mine.cpu, k), jm = __builtin_amdgcn_readlane(mine.mem, k);
            const int32_t jg = __builtin_amdgcn_readlane(mine.gpu, k), row = __builtin_amdgcn_readlane(mine.row, k);
            for (int s = (ws & ~63) + lane; s < we; s += 64)
                if (s >= ws) op(s, jc, jm, jg, row);
        }
    }
}

// Write back: slot s ends a run when it is the last or its successor differs (ballot + lanes-below
// prefix, tl_reserve_any's merge step).  The same pass takes the wave maximum of every column.
struct TlDenseOut {
    int no;              // runs written
    int32_t xc, xm, xg;  // the column maxima, in every lane
};
__device__ __forceinline__ TlDenseOut tl_dense_write(Seg* sg, int32_t H, int lane, const int32_t* dc,
                                                     const int32_t* dm, const int32_t* dg) {
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
    return {no, xc, xm, xg};
}

// Header refresh after a wave rewrote its node's list to `no` runs: the wave waits for its own list
// stores, re-reads the first TL_HEAD runs into head[] and sets cnt.  The ceilings are the caller's:
// fit_unplace_tl raises them (max(old, new)), fit_hold_tl and fit_advance_tl set the exact maxima,
// fit_place_tl_k leaves them (reservations only lower values: they stay upper bounds).
__device__ __forceinline__ void tl_refresh_head(TlHdr* hp, const Seg* sg, int no, int32_t H, int lane) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the list's writes before its re-read
    if (lane < TL_HEAD) hp->head[lane] = lane < no ? sg[lane] : Seg{H, -1, -1, -1};
    if (lane == 0) hp->cnt = no;
}

}  // namespace fitgpu

// fit_engine_frame.h — the round protocol of a committer block and the task loop of a scan worker
// of the persistent engines, parametrised by values and by the scan functor.
// k_engine (fit_persistent.hip) is built on it and keeps what is its own: the plan's k0 choice, the
// commit call, the next-window policy and the scan of one task.  k_engine_tl (fit_timeline.hip)
// runs the same protocol from its own text: on the frame it measured 0.2-0.6 % slower at C5
// (profiles/engine_frame_ab.txt).  Hand-offs follow the recipe at the top of fit_persistent.hip.
//
// Target accounting.  When a round calls wait_tiles, the target of its parity equals the number of
// tasks ever published for that parity: round_open adds what the committer publishes when that is
// the whole window (and a paired first tile's extra half-slice tasks always), round_close adds the
// tiles of a window published just in time, the helpers' included, once their count is final.
#pragma once
#include "fit_commit_mw.h"
#include "fit_engine_ctl.h"

namespace fitgpu {

// One count per buffer set, selected rather than indexed: an indexed array would keep the whole
// of RoundAcct in scratch.
struct ByParity {
    unsigned v0 = 0u, v1 = 0u;
    __device__ __forceinline__ unsigned get(int par) const { return par ? v1 : v0; }
    __device__ __forceinline__ void set(int par, unsigned x) {
        v0 = par ? v0 : x;
        v1 = par ? x : v1;
    }
};

// What a committer carries from round to round (wave 0's copy is the one used).
struct RoundAcct {
    ByParity target;  // tasks published by the rounds of each parity
    // job tiles published by the last round of each parity: only their bounds can differ from
    // KEY_INF (the host sets them all before the launch), so only those are reset
    ByParity used;
    int64_t evals = 0, placed = 0, rounds = 0, sr = 0, sd = 0, tc = 0, tw = 0;
    int64_t t0 = 0, t1 = 0;  // realtime at the round's start / when its tiles were published
};

// The launch constants of a committer block (uniform).
struct Committer {
    EngineCtl* ctl;
    unsigned long long* ring;  // the component's task ring (comp_ring)
    CompPlan* plans;
    uint64_t* bnd;
    int c;        // component
    unsigned wd;  // watchdog ticks
};

// The plan of the round at `cursor` with window w in buffer set par; the caller sets k0.
__device__ __forceinline__ void round_plan(CompPlan& P, const CompState& S, int32_t cursor, int w, int par) {
    P.nb = S.nb;
    P.ne = S.ne;
    P.sb = S.sb;
    P.se = S.se;
    P.nslice = S.nslice;
    P.sub = S.sub;
    P.ks = S.ks;
    P.jbase = cursor;
    P.w = w;
    P.blk0 = 0;
    P.cand_off = par ? S.cand_alt : S.cand_off;
    P.slot0 = par ? S.slot_alt : S.slot0;
    P.pair_off = S.pair_off + (par ? PAIR_AREA : 0);
}

// Open round `rnd` (every wave of the block; wave 0 works): wait for the buffer set, write the plan
// and the resets through, publish the first job tiles, acquire.  true: the wait failed (the launch
// drains; block-uniform).
//   ahead  > 0: the committer publishes that many job tiles, the commit's helpers the rest just in
//          time (commit_publish); 0: the whole window now
//   whole  the commit needs the whole window scanned first (the single-wave commit)
//   plain  the previous round left plain stores that the scans read: release them
//   tfeas  the tiles' feasibility masks to clear, or nullptr
//   pubt   the LDS word counting the window's published job tiles
__device__ __forceinline__ bool round_open(const Committer& K, const CompState& S, const CompPlan& P,
                                           unsigned rnd, RoundAcct& A, unsigned ahead, bool whole,
                                           bool plain, unsigned long long* tfeas, uint32_t* pubt,
                                           int* s_fail) {
    const int lane = threadIdx.x & 63;
    const int par = (int)(rnd & 1u), c = K.c;
    MW_CLK(rs0);
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) {
        A.t0 = (int64_t)__builtin_amdgcn_s_memrealtime();
        // the tiles of the round before last (this round's buffer set; also those past its stop)
        // must all be complete before their buffers and counters are reused; the previous
        // round's may still be in flight, in the other set
        unsigned target = A.target.get(par);
        bool fail = !wait_tiles(K.ctl, c, par, target, K.wd, rnd);
        const unsigned ntj = (unsigned)((P.w + SCAN_JOBS - 1) / SCAN_JOBS);
        // written through (sc1), like the tile counters: the helpers that publish tiles just in
        // time need no release of their own (R1: stored, drained, then the block barrier, then
        // their task stores)
        store_through(&K.plans[2 * c + par], P);
        const int nres = min((int)A.used.get(par) * SCAN_JOBS, S.wmax);  // within the slot region
        for (int i = lane; i < nres; i += 64) store_through64(&K.bnd[P.slot0 + i], KEY_INF);
        for (unsigned i = lane; i < ntj; i += 64) {
            __hip_atomic_store(&K.ctl->tdone[par][c][i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tfeas) __hip_atomic_store(&tfeas[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // only when the first tile is paired: no other tile reads the pair counters
        const bool pair = (P.k0 & 2) != 0;
        if (pair && lane < 32)
            __hip_atomic_store(&K.ctl->tpair[par][c][lane], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // what a commit writes for the next scan it stores through, as the plan and the resets
        // above (drained here, before the publish); plain stores are released instead
        // (≈1.7-6.5 us on the round-start path)
        if (plain) release_agent();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // just in time, the ring never holds a whole window of tiles that a new round's first
        // tile would queue behind — and the tiles past a stop are never scanned
        const unsigned npub = ahead > 0u ? min(ntj, ahead) : ntj;
#ifdef FIT_STAMPS
        // before the tasks turn visible: a worker may pick tile 0 at once
        if (lane == 0) {
            __hip_atomic_store(&K.ctl->pub[c], __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
#endif
        if (pair) {  // tile 0 as 2 x nslice half-slices, then the rest
            engine_publish(K.ctl, K.ring, 0u, 1u, 2u * (unsigned)S.nslice, rnd, (unsigned)c);
            if (npub > 1u) engine_publish(K.ctl, K.ring, 1u, npub, (unsigned)S.nslice, rnd, (unsigned)c);
            target += (unsigned)S.nslice;  // tile 0's extra tasks
        } else {
            engine_publish(K.ctl, K.ring, 0u, npub, (unsigned)S.nslice, rnd, (unsigned)c);
        }
        if (lane == 0) *pubt = npub;
        if (npub == ntj) target += npub * (unsigned)S.nslice;  // else: round_close
        A.target.set(par, target);
        if (whole && !fail) fail = !wait_tiles(K.ctl, c, par, target, K.wd, rnd);
        acquire_agent();  // what this block's last commit wrote back: CU-wide view for all waves
        if (lane == 0) *s_fail = fail;
        {
            MW_CLK(rs1);
            MW_ADD(16, rs1 - rs0);
        }
    }
    __syncthreads();
    A.t1 = (int64_t)__builtin_amdgcn_s_memrealtime();
    return *s_fail != 0;
}

// Close the round after its commit returned R in every wave (M: the commit's shared block, stable
// after the commit's closing barrier).  jit: the window was published just in time.  site0: the
// trip site of a commit that gave up without naming one.  false: the launch drains.
template <class Sh>
__device__ __forceinline__ bool round_close(const Committer& K, const CompState& S, const CompPlan& P,
                                            unsigned rnd, RoundAcct& A, const CommitResult& R, bool jit,
                                            const Sh* M, unsigned site0) {
    const int par = (int)(rnd & 1u), c = K.c;
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) {
        // every tile published this round (the committer's and the helpers') must be complete
        // before a later round reuses its buffer set: count them
        if (jit) A.target.set(par, A.target.get(par) + M->pubt * (unsigned)S.nslice);
        A.used.set(par, M->pubt);
    }
    if (threadIdx.x == 0) engine_round_finished(K.ctl, c, rnd);
    if (R.stop == 3) {  // a commit wait gave up: M->fail names it (TRIP_PEER: drained)
        if (threadIdx.x == 0) {
            const unsigned site = M->fail ? M->fail : site0;
            const unsigned tl = site == TRIP_HELPER_TILE ? M->trip_arg : 0u;
            trip_record(K.ctl, site == TRIP_PEER ? 0u : 2u, site, (unsigned)c, rnd, M->trip_arg, M->pubt,
                        ld_agent(&K.ctl->tdone[par][c][tl & (ENGINE_TILES - 1)]), (unsigned)S.nslice,
                        (unsigned long long)A.t1);
        }
        return false;
    }
    if (R.done == 0) {  // the next round would rescan the same state: never progresses
        if (threadIdx.x == 0)
            trip_record(K.ctl, 4u, TRIP_NO_PROGRESS, (unsigned)c, rnd, (unsigned)P.jbase, M->pubt, 0u, 0u,
                        (unsigned long long)A.t1);
        return false;
    }
    const int64_t t2 = (int64_t)__builtin_amdgcn_s_memrealtime();
    A.tw += A.t1 - A.t0;
    A.tc += t2 - A.t1;
    A.evals += (int64_t)P.w * (S.se - S.sb);
    A.placed += R.placed;
    ++A.rounds;
    A.sr += R.stop == 1;
    A.sd += R.stop == 2;
    return true;
}

// After the last round (wave 0): the component's totals, then it counts as finished.
__device__ __forceinline__ void rounds_end(const Committer& K, CompOut* co, const RoundAcct& A,
                                           int32_t jobs_done) {
    release_agent();  // last round's write-backs / placements (kernel end also flushes)
    if ((threadIdx.x & 63) == 0) {
        co[K.c] = CompOut{A.evals, A.placed, jobs_done, A.rounds, A.sr, A.sd, A.tc, A.tw};
        __hip_atomic_fetch_add(&K.ctl->finished, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The task loop of a scan worker block, until the launch is over.  wi: the worker's index in
// wbusy; task_slot: 8 B of LDS behind the scan's merge buffer.
//   scan(P, tile, s, c, par, rnd) -> counts  scans block-slice s of job tile `tile` of component c
//       with the round's plan (half-size block-slices already set for a paired first tile);
//       false: the task does not complete its tile's block-slice (the first half of a pair)
//   stamp(c, t0, now)  FIT_STAMPS builds, thread 0, after a round's first tile
template <class Scan, class Stamp>
__device__ __forceinline__ void scan_worker(EngineCtl* ctl, unsigned long long* ring, const CompPlan* plans,
                                            int ncomp, unsigned wd, int64_t* wbusy, int wi,
                                            unsigned long long* task_slot, Scan scan, Stamp stamp) {
    const unsigned wgrp = worker_group(ncomp);  // this XCD's ring group (fit_engine_ctl.h)
    TaskClaim claim;
    int64_t busy = 0;     // realtime ticks (100 MHz) spent scanning
    int64_t scanned = 0;  // (job, node) evaluations of the tiles scanned (dropped ones excluded)
    for (;;) {
        if (threadIdx.x == 0) {
            unsigned long long task = next_task(ctl, ring, ncomp, wgrp, claim, wd);
            if (task != TASK_EXIT && task_dropped(ctl, task)) task |= TASK_SKIP;
            *task_slot = task;
        }
        __syncthreads();
        const unsigned long long task = *task_slot;
        if (task == TASK_EXIT) {  // block-uniform
            if (threadIdx.x == 0) {
                wbusy[2 * wi] = busy;
                wbusy[2 * wi + 1] = scanned;
            }
            return;
        }
        const int64_t t0 = (int64_t)__builtin_amdgcn_s_memrealtime();
        const bool skip = (task & TASK_SKIP) != 0ull;  // block-uniform
        const int c = (int)(task & 63u);
        const int s = (int)task_slice(task);
        const int tile = (int)task_tile(task);
        const int par = (int)(task_round(task) & 1u);  // the round's buffer set
        bool counts = true;  // (thread 0) the task completes its tile's block-slice
        if (!skip) {
            if (threadIdx.x == 0) acquire_agent();
            else __builtin_amdgcn_s_dcache_inv();
            __syncthreads();
            CompPlan P = plans[2 * c + par];
            if (tile == 0 && (P.k0 & 2)) {  // the paired first tile: half-size block-slices
                P.sub = (P.sub + 1) / 2;
                P.nslice *= 2;
            }
            counts = scan(P, tile, s, c, par, task_round(task));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
#ifdef FIT_STAMPS
            if (threadIdx.x == 0 && tile == 0)  // the round's first tile: pickup delay, scan time
                stamp(c, (unsigned long long)t0, (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
            const int a = P.sb + s * SCAN_WAVES * P.sub, b = min(P.se, a + SCAN_WAVES * P.sub);
            scanned += (int64_t)max(min(SCAN_JOBS, P.w - tile * SCAN_JOBS), 0) * max(b - a, 0);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // the tile's outputs were written through (sc1 stores, agent atomics) and every storing
            // wave waited for them (vmcnt(0) above, then the barrier): the counts need no release
            // fence (cdna_hip_programming.md §6 Guideline 16 R1)
            if (counts)
                __hip_atomic_fetch_add(&ctl->tdone[par][c][tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // the tile count must land before the done count: once a committer sees `done` reach
            // its target it resets the tile counters for the next round, and a late increment
            // would then mark a tile of that round complete before it was scanned
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(&ctl->done[c][2 + par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            busy += (int64_t)__builtin_amdgcn_s_memrealtime() - t0;
        }
        __syncthreads();  // task_slot is rewritten by thread 0 next iteration
    }
}

}  // namespace fitgpu

// fit_commit_mw.h — the commit of one component's window by a whole 8-wave workgroup
// (DESIGN.md §3.7): one DECIDER wave walks the jobs in priority order; seven HELPER waves
// pre-resolve the jobs ahead of it against a slightly stale snapshot of the dirty state.
//
// Why it is exact.  Let the decider have resolved jobs [0, v) when a helper snapshots the
// state for job t (v >= t - (MW_M - 1), enforced by the helper).  The helper records the MW_M
// smallest keys <= B among (clean candidates of t) ∪ (dirty rows), each item tagged clean (with
// its node row) or dirty (its slot).  When the decider reaches t, only the nodes written by jobs
// [v, t) — at most MW_M - 1 of them, the decider's own last decisions, kept in its "written
// ring" — can differ from the snapshot.  It drops every item whose node is in the live part of
// the ring and evaluates the live ring rows at their current state.  If the list held MW_M items,
// at least one survives and every unlisted node has a key above it; if it held fewer, it held
// every candidate <= B.  Either way
//     best = min(surviving items, live ring rows)
// is the sequential answer restricted to keys <= B, and the SPEC stop rule reduces to
// "best > B with B finite" (a clean candidate is always <= B).  The argument needs nothing of a
// row or bitmap word the helper read after the snapshot: any node changed after v is in the live
// ring, so a torn or newer read of it only produces an item the decider drops.
//
// How an item is found stale.  "Its node is in the live ring" is "its node was written by a job in
// [v, t)", and the shared state already says so in one LDS word per item, which the helper names
// in the item (MwItem::chk_*): a clean item passed the helper's bitmap test, so its node's bit is
// set now exactly when a job in [v, t) dirtied it; a dirty item's row carries `ver`, the last job
// that created or changed it, and the item is stale exactly when ver >= v.  Both words are written
// by the decider alone (its bookkeeping, in issue order before its next read), so the probe
// crosses no wave.
//
// "Jobs" above are the window's LIVE jobs (round 3): a job that no node fits at the round's start
// is unplaced whatever the decisions before it, so the helpers skip it (per-tile feasibility
// masks from the scan, mw_skip_live) and record i, ring lane i & 7 and the snapshot counts all
// index the i-th live job; the record header carries its window index, and a record whose index
// is the window size ends the window.
//
// Cost model (measured on gfx950, tools/ubench: one wave alone) — what shapes the code below:
// a dependent VALU op ≈ 4.7 cycles, any scalar branch ≈ 25-30, a VALU → SGPR → SALU hand-off
// ≈ 20-36, v_readlane → v_writelane ≈ 8.6, one LDS round trip ≈ 50-64.  So the decider's job
// step is straight-line VALU with ONE exception branch per job (record not ready, B exceeded,
// dirty set full, end of window), the written ring lives in lanes 0..7 (slot = job & 7, a
// compile-time lane in the 8-way unrolled loop), item staleness is one ds_read_b32 per lane at an
// address the helper precomputed, issued at the top of the step and consumed after the ring
// rows' keys (its round trip is covered; the DPP compare against the rotated ring it replaced
// was 21 more instructions per job), the minimum over ring rows and items is three 64-bit DPP
// steps over 8 lanes, and the next job's record is read while this one is decided.  The
// decision's bookkeeping (dirty row, bitmap bit, placement) is issued by the decider itself as
// fire-and-forget LDS writes.
//
// LDS protocol (one workgroup), C++ memory model at workgroup scope on LDS ("local"):
//   decider → helpers: dirty rows, bitmap, then {decided, nu} by a release store;
//   helpers: relaxed poll of {decided, nu}, then an acquire fence, then rows / bitmap.
//   helper → decider: record items and header, then the record's ready word by a release store;
//   decider: relaxed load of the ready word, an acquire fence, then the record's data.
// On gfx950 (no threadgroup split) a workgroup-scope release / acquire on LDS is an
// `s_waitcnt lgkmcnt(0)` before the store / after the load (checked in the ISA); both sit where
// the counter is already drained, so the protocol costs no cycles on the decider's chain.
// (Primitives: fit_wave.h — lds_*, global views, write-through loads, DPP minima; key: fit_key.h.)
#pragma once
#include "fit_common.h"
#include "fit_engine_ctl.h"
#include "fit_wave.h"  // LDS hand-offs and addresses, global views, fused DPP minima, writelane

namespace fitgpu {

#ifndef MW_ITEMS
#define MW_ITEMS 8
#endif
constexpr int MW_M = MW_ITEMS;          // items per pre-resolved record (> snapshot lag)
constexpr int MW_R = 8;                 // record ring; slot t & 7 frees once job t-8 is decided
#ifndef MW_SNAP
#define MW_SNAP MW_ITEMS  // a helper snapshots job t's state once the decider has resolved t - (MW_SNAP - 1)
#endif
static_assert(MW_SNAP >= 1 && MW_SNAP <= MW_ITEMS, "a later snapshot only shortens the ring span");
constexpr int MW_WAVES = SCAN_WAVES;    // 1 decider + MW_H helpers
constexpr int MW_H = MW_WAVES - 1;  // helpers: waves 1..7
static_assert(MW_M == 8, "the decider holds one item per lane of its 8-lane ring group");
static_assert(MW_R >= MW_M, "record slot reuse relies on the lag bound");

#ifndef MW_HSLEEP
#define MW_HSLEEP 1  // helper back-off per missing decided job, in units of 64 cycles (12 before the
                      // 4-entry helpers: C3 k_engine 32.2 -> 31.2 ms at 0-2)
#endif
constexpr int MW_EPL = (MAX_SLICES * KS + 63) / 64;  // candidate entries per helper lane
static_assert(MW_EPL <= 2, "at most two candidate entries per lane");

// The dirty set of this commit (DESIGN.md §3.7 "recycling"), chosen per component at launch
// (MwShared::ucap):
//   MW_UCAP = 64 rows, one per helper lane (3 entries per lane with the candidates), with
//     recycling: when the set is full the decider RETIRES a row that fits no job of the component
//     any more (below the component's minimum demand in one resource; resources only shrink) — its
//     values wait in retired[] for the round's write-back and the fresh node takes its slot — up
//     to MW_RCAP rows a round;
//   UCAP = 128 rows, two per helper lane, a full set stops the round: components whose round
//     start is dear (k_engine: those scanned with fewer keys per slice), where rounds count more
//     than the helpers' entries (C3o).
// UCAP is also the capacity of the single-wave commit and the host-driven rounds (fit_common.h).
constexpr int MW_UCAP = 64;
#ifndef MW_RETIRE
#define MW_RETIRE 128  // 0: a full set always stops the round (no recycling)
#endif
constexpr int MW_RCAP = MW_RETIRE;
static_assert(UCAP == 2 * MW_UCAP, "retired[] lies over the rows a 64-row set leaves unused");
static_assert(MW_RCAP * 16 <= (UCAP - MW_UCAP) * 32, "retired[] fits there");
static_assert(MW_UCAP + MW_RCAP < 256, "a 256-job window of fresh nodes still fills the set");

struct alignas(16) MwRow {  // dirty row, current state
    int32_t cpu, mem, gpu, avail;
    uint32_t mask, pos;
    int32_t orig, ver;  // ver: last job (record index) that created or changed it; read back by
                        // the decider's staleness probe of a dirty item
};

struct alignas(16) MwRet {  // a retired row: what the round's write-back stores
    uint32_t pos;
    int32_t cpu, mem, gpu;
};

struct alignas(16) MwItem {  // 48 B, read whole by the decider (three 16-B reads)
    uint32_t pos, score;  // key = score << 32 | pos
    int32_t tag, orig;    // tag: dirty slot (>= 0) or -1 (a clean candidate; row below)
    int32_t cpu, mem, gpu, avail;
    uint32_t mask;
    // the staleness probe: the item is stale iff (LDS word at chk_addr & chk_mask) >= chk_thr.
    //   clean item: its node's bitmap word, mask = thr = the node's bit (set by a fresh placement)
    //   dirty item: &rows[tag].ver, mask = ~0, thr = the record's snapshot v (ver >= 0 always)
    // chk_addr always lies inside MwShared: commit_window_mw points every item at MwShared::pad
    // before the window starts, and only helpers write items after that.
    uint32_t chk_addr, chk_mask, chk_thr;
};

struct alignas(16) MwHdr {
    uint32_t ready;  // i + 1 once record i is complete (release store, last)
    int32_t v, n, q;
    int32_t cpu, mem, gpu, wall;
    uint32_t pbit;
    int32_t tj;      // the record's job (window index); P.w: the window has no live job left
    uint64_t B;
};

struct alignas(16) MwRec {
    MwHdr h;
    MwItem it[MW_M];
};

struct alignas(16) MwShared {
    uint64_t dn;       // {decided (low 32), nu (high 32)}: the helpers' snapshot, release-stored
    uint32_t halt;     // decider stopped
    uint32_t fail;     // helper / decider watchdog: the TripSite of the first wait that gave up
    int32_t res[4];    // CommitResult of the window
    uint32_t pubt;     // job tiles of the window published to the task ring (MwTiles::ring)
    uint32_t wd;       // watchdog: realtime ticks a wait may last (set by the committer; the
                       // commit's own waits use spin bounds, see MW_SPIN_LIMIT)
    uint32_t trip_arg; // the failed wait's tile / record
    uint32_t pad[1];   // the sink of an unwritten item's staleness probe (mw_reset_items)
    uint32_t nret;     // rows in retired[] this round (set by the decider at its end)
    int32_t mind[3];   // the component's minimum cpu / mem / gpu demand over its non-rejected jobs
                       // (set by the committer at launch): a row below one of them is dead
    uint32_t ucap;     // dirty capacity of this component's commits: MW_UCAP (recycling) or UCAP
    uint32_t slim;     // 1: the component is one partition (CompState::onepart, set by the committer
                       // at launch): the decider runs the slim ring (mw_decide SP)
    MwRec rec[MW_R];
    MwRow rows[UCAP];  // ucap == MW_UCAP: rows[MW_UCAP ..) hold retired[] (mw_retired)
    uint32_t bitmap[1];  // (ne - nb + 31) / 32 words, dirty membership by position
};

__device__ __forceinline__ MwRet* mw_retired(MwShared* S) {
    return reinterpret_cast<MwRet*>(&S->rows[MW_UCAP]);
}

__host__ __device__ constexpr size_t mw_lds_bytes(int32_t max_component_nodes) {
    return sizeof(MwShared) + (size_t)((max_component_nodes + 31) / 32) * 4;
}

#ifdef FIT_STAMPS
// [comp][0] decider cycles, [1] decider waiting for records (slow path), [2] decided jobs,
// [3] helper cycles (sum), [4] helper wait-for-snapshot, [5] helper jobs, [6] items written,
// [7] (unused), [8] (unused), [9] decider waits in each round's first 8 jobs,
// [10..12] first-tile scan (workers), [13] helper tile waits, [14] helper snapshot → record,
// [15] helper snapshot → extraction start, [16] committer: round end → tiles published (wait for
// the round before last, resets, release, publish), [17] decider: start → record 0 ready,
// [18] rounds
constexpr int MW_NSTAMP = 24;
__device__ unsigned long long g_mw[64][MW_NSTAMP];
#define MW_CLK(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define MW_DECL(v) unsigned long long v = 0
#define MW_ACC(v, x) v += (x)
#define MW_ADD(I_, V_) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_mw[blockIdx.x & 63][I_], (unsigned long long)(V_)); } while (0)
#else
#define MW_CLK(v)
#define MW_DECL(v)
#define MW_ACC(v, x)
#define MW_ADD(I_, V_)
#endif

// The commit's waits — the helpers' waits for scan tiles, and the decider <-> helper waits inside
// the block — keep round 4's spin bound (MW_SPIN_LIMIT polls, ≈ 4-8 s).  Every other wait of the
// engine has a time deadline (fit_engine_ctl.h WaitClock), and those bound what the commit waits
// for: its tiles come from scan workers whose own waits trip on time and drain the launch.  A time
// check in the helper's tile-wait loop — any extra branch there, in fact — changes the code LLVM
// generates for the whole (VGPR-limited) helper (different unrolling and branch layout) and cost
// C3 +0.55 ms / C2 +0.3 ms in paired A/Bs (profiles/r05_watchdog_ab.txt); so the loop keeps its
// round-4 shape and only the failing branch records its site.
constexpr unsigned MW_SPIN_LIMIT = 1u << 24;

// A commit wait gave up (uniform call; helper or decider): the block's first failure names its
// TripSite and argument in `fail` / `trip_arg`; `fail` stops every wave of the block and the
// committer turns it into the launch's trip record (fit_engine_ctl.h trip_record).
// Every lane stores the same values (no lane test: a lane id kept live for it cost the decider a
// VGPR across its whole loop); two waves failing at once may leave the later one's site.
__device__ __forceinline__ void commit_fail(uint32_t* fail, uint32_t* trip_arg, uint32_t site,
                                            uint32_t arg) {
    if (lds_ld(fail) == 0u) {
        lds_st(trip_arg, arg);
        lds_st(fail, site);
    }
}

// Tile readiness: the window's scan tiles complete while the window is being
// committed; a helper waits for the (job tile)'s per-tile counter to reach nslice before reading
// that tile's candidates, bound and job row; an agent-scope acquire when a tile turns ready drops
// the CU's L1 (it may hold stale lines of these reused buffers), so the reads stay plain loads.
// tdone == nullptr: the whole window was acquired before the commit (no waits).
struct MwTiles {
    const unsigned* tdone;  // per-tile completed slice counts of this component's window
    unsigned need;          // nslice
    // just-in-time publishing (k_engine, ENGINE_AHEAD > 0): the committer publishes the window's
    // first ENGINE_AHEAD job tiles; a helper that moves on to tile k publishes the tiles up to
    // k + ENGINE_AHEAD - 1 first.  ring == nullptr: every tile was published up front.
    unsigned long long* ring;
    EngineCtl* ctl;
    unsigned round;  // task round tag
    unsigned comp;
    unsigned ntj;    // job tiles of the window
    // per job tile: jobs with a node that fits them at the round's start (k_engine's scan ORs
    // them in before it counts the tile done); nullptr: every job of the window is live
    const unsigned long long* feas;
};
#ifndef ENGINE_AHEAD
#define ENGINE_AHEAD 4  // 0: every tile of the window published up front
#endif

// The plan copied into SGPRs: an out-of-line function receives it through a generic pointer, and
// fields loaded that way sit in VGPRs, so the compiler cannot prove the job loop uniform (it
// would run it under exec masks with its counter in a VGPR).
__device__ __forceinline__ CompPlan plan_sgpr(const CompPlan& q) {
    CompPlan p;
    p.nb = rfl(q.nb);
    p.ne = rfl(q.ne);
    p.sb = rfl(q.sb);
    p.se = rfl(q.se);
    p.nslice = rfl(q.nslice);
    p.sub = rfl(q.sub);
    p.jbase = rfl(q.jbase);
    p.w = rfl(q.w);
    p.blk0 = rfl(q.blk0);
    p.ks = rfl(q.ks);
    p.cand_off = (int64_t)(((uint64_t)(uint32_t)rfl((int32_t)(q.cand_off >> 32)) << 32) |
                           (uint32_t)rfl((int32_t)q.cand_off));
    p.slot0 = rfl(q.slot0);
    return p;
}

// One CommitResult through the shared block's res[4]: one lane puts it, every wave gets it after
// the next barrier.
__device__ __forceinline__ void put_result(int32_t* res, const CommitResult& r) {
    res[0] = r.done;
    res[1] = r.stop;
    res[2] = r.dirty;
    res[3] = r.placed;
}
__device__ __forceinline__ CommitResult get_result(const int32_t* res) {
    return CommitResult{res[0], res[1], res[2], res[3]};
}

// Publish the window's job tiles [pubt, upto) (uniform; lane 0 claims the range by an LDS CAS).
// Sh: the commit's shared block (MwShared, TmShared).
template <class Sh>
__device__ __noinline__ void commit_publish(const MwTiles& T, Sh* S, unsigned upto) {
    const int lane = threadIdx.x & 63;
    unsigned from = upto;  // nothing claimed
    if (lane == 0) {
        unsigned cur = lds_ld(&S->pubt);
        while (cur < upto) {  // a failed exchange reloads cur
            if (__hip_atomic_compare_exchange_strong(&S->pubt, &cur, upto, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                from = cur;
                break;
            }
        }
    }
    from = (unsigned)__builtin_amdgcn_readlane((int)from, 0);
    if (from >= upto) return;
    // claimed [from, upto): what the tasks' scans read — the round's plan, bounds, tile counters
    // (written through) and the last commit's write-backs (written through, or released) — was
    // stored and drained by the committer wave before the block barrier this wave has passed: no
    // fence here (R1)
    engine_publish(T.ctl, T.ring, from, upto, T.need, T.round, T.comp);
}

// Wait until job tt's scan tile is complete (uniform; `ready` = tiles known complete, they finish
// roughly in order).  false: the decider halted / a watchdog tripped.
__device__ __forceinline__ bool mw_tile_ready(const MwTiles& T, int tt, int& ready, MwShared* S) {
    if (!T.tdone) return true;
    const int tile = __builtin_amdgcn_readfirstlane(tt) / SCAN_JOBS;
    if (tile < ready) return true;
    if (T.ring && (unsigned)tile + ENGINE_AHEAD > lds_ld(&S->pubt))
        commit_publish(T, S, min((unsigned)tile + ENGINE_AHEAD, T.ntj));
    for (unsigned sp = 0;; ++sp) {
        if (__hip_atomic_load(gview(T.tdone) + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >=
            T.need)
            break;
        if (lds_ld(&S->halt) | lds_ld(&S->fail)) return false;
        if (sp > MW_SPIN_LIMIT) {
            lds_st(&S->trip_arg, (uint32_t)tile);
            lds_st(&S->fail, TRIP_HELPER_TILE);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    // the tile's outputs are read with sc1 loads (ld_through): no acquire fence; this only keeps
    // the compiler from moving them above the poll
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    ready = tile + 1;
    return true;
}

// ---------------------------------------------------------------------------- live jobs
// A job with no node that fits it at the round's start state is unplaced whatever the jobs
// before it take (node state only shrinks within a placement) and changes nothing: the commit
// skips it (its output is already FIT_UNPLACED from k_prefilter).  The decider then walks the
// LIVE jobs only: record i (ring lane i & 7, snapshot counts, ready word) belongs to the i-th
// live job of the window, whose window index the record's header carries; a record whose job
// index is the window size ends the window.  C3: ~14 % of a component's jobs (the ones nothing
// fits once the cluster has filled) no longer cost a decider step.
struct MwCursor {
    int ct;       // job tile of the cursor
    uint64_t cm;  // live jobs of tile ct not yet taken
};
// move the cursor to the next job tile (uniform): its live-job mask once the tile is complete;
// false: halted / watchdog.  Past the window's last tile the mask stays empty.
__device__ __forceinline__ bool mw_cursor_tile(const MwTiles& T, const CompPlan& P, MwCursor& C,
                                               int& ready, MwShared* S) {
    if ((C.ct + 1) * SCAN_JOBS >= P.w) {
        C.cm = 0ull;
        return true;
    }
    ++C.ct;
    const int n = min(SCAN_JOBS, P.w - C.ct * SCAN_JOBS);
    const uint64_t valid = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    if (T.feas) {
        if (!mw_tile_ready(T, C.ct * SCAN_JOBS, ready, S)) return false;
        const uint64_t f = __hip_atomic_load(gview(T.feas) + C.ct, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)f);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(f >> 32));
        C.cm = (((uint64_t)hi << 32) | lo) & valid;
    } else {
        C.cm = valid;
    }
    return true;
}
// the k-th next live job (1 <= k <= 64, window index; P.w once the window has none left)
__device__ __forceinline__ bool mw_skip_live(const MwTiles& T, const CompPlan& P, MwCursor& C,
                                             int& ready, MwShared* S, int k, int& tj) {
    for (;;) {  // uniform; a tile holds ~7 records of each helper, so this rarely loops
        const int pc = __builtin_popcountll(C.cm);
        if (pc >= k) break;
        if ((C.ct + 1) * SCAN_JOBS >= P.w) {
            C.cm = 0ull;
            tj = P.w;
            return true;
        }
        k -= pc;
        if (!mw_cursor_tile(T, P, C, ready, S)) return false;
    }
    for (int j = 1; j < k; ++j) C.cm &= C.cm - 1ull;
    tj = C.ct * SCAN_JOBS + (int)__builtin_ctzll(C.cm);
    C.cm &= C.cm - 1ull;
    return true;
}

// The tile hand-off copied into SGPRs: mw_helper receives it in private memory (a by-value
// aggregate of an out-of-line callee), and every field read from there is a scratch load whose
// vmcnt wait would drain the helper's prefetched job stream.
__device__ __forceinline__ MwTiles tiles_sgpr(const MwTiles& T) {
    return MwTiles{rfl_ptr(T.tdone), (unsigned)rfl((int32_t)T.need), rfl_ptr(T.ring),
                   rfl_ptr(T.ctl), (unsigned)rfl((int32_t)T.round), (unsigned)rfl((int32_t)T.comp),
                   (unsigned)rfl((int32_t)T.ntj), rfl_ptr(T.feas)};
}

// ------------------------------------------------------------------------------- helper
// Helper entry lists: MW_EPL clean candidates + UPL dirty rows per lane, each key tagged with
// its entry index in the low bits (positions < 2^29, FIT_MAX_NODES), INF stays INF.
// (UPL_MW = dirty rows per lane, 1 or 2, and MW_NE = MW_EPL + UPL_MW are mw_helper's template
// constants; the macros below use them by name)
static_assert(MW_EPL + UCAP / 64 <= 8, "entry index takes 3 bits (and 4 bits of item index each in 32)");
static_assert(MW_M <= 15, "item index + 1 fits 4 bits");
__device__ __forceinline__ uint64_t mw_tag(uint64_t k, int e) {
    return k == KEY_INF ? KEY_INF
                        : (k & 0xffffffff00000000ull) | (uint32_t)(((uint32_t)k << 3) | (uint32_t)e);
}
__device__ __forceinline__ void mw_cas(uint64_t& a, uint64_t& b) {
    const uint64_t lo = umin64(a, b), hi = umax64(a, b);
    a = lo;
    b = hi;
}
// ascending sort of a lane's entries (static indices only): the optimal networks for 4 (5
// comparators) and 6 (12), odd-even transposition otherwise
template <int N>
__device__ __forceinline__ void mw_sort(uint64_t (&q)[N]) {
    if constexpr (N == 4) {
        mw_cas(q[0], q[1]); mw_cas(q[2], q[3]);
        mw_cas(q[0], q[2]); mw_cas(q[1], q[3]);
        mw_cas(q[1], q[2]);
    } else if constexpr (N == 6) {
        mw_cas(q[0], q[5]); mw_cas(q[1], q[3]); mw_cas(q[2], q[4]);
        mw_cas(q[1], q[2]); mw_cas(q[3], q[4]);
        mw_cas(q[0], q[3]); mw_cas(q[2], q[5]);
        mw_cas(q[0], q[1]); mw_cas(q[2], q[3]); mw_cas(q[4], q[5]);
        mw_cas(q[1], q[2]); mw_cas(q[3], q[4]);
    } else {
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int i = r & 1; i + 1 < N; i += 2) mw_cas(q[i], q[i + 1]);
    }
}

// Extraction of the record's items: the nmax_ smallest tagged entries, one wave minimum each.
// straight-line: each minimum lands in every lane (DPP row minima, then the permlane16 / 32
// swaps of gfx950), so no VALU -> SGPR -> SALU hand-off sits on the helper's chain; the rounds
// stop at nmax_ (a uniform branch: round 4, C3 26.39 -> 26.02 ms, C2 14.95 -> 14.75 ms — a shorter
// helper record leaves the decider's SIMD and the LDS to the decider sooner); rounds past the last
// entry take nothing (stopping there too was slower)
#define MW_EXTRACT                                                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < MW_M; ++i_) {                                  \
            if (i_ >= nmax_) break; /* uniform: a record needs nmax_ items at most */          \
            const uint32_t hh_ = (uint32_t)(q_[0] >> 32), ll_ = (uint32_t)q_[0];              \
            const uint32_t mh_ = wave_min32_all(hh_);                                          \
            const uint32_t ml_ = wave_min32_all(hh_ == mh_ ? ll_ : 0xffffffffu);               \
            const bool take_ = i_ < nmax_ && (mh_ & ml_) != 0xffffffffu;                       \
            const bool me_ = take_ && hh_ == mh_ && ll_ == ml_; /* tagged keys are unique */   \
            n_ += take_ ? 1 : 0;                                                               \
            sel_ = me_ ? sel_ | ((uint32_t)(i_ + 1) << (4u * (ml_ & 7u))) : sel_;              \
            _Pragma("unroll") for (int e = 0; e + 1 < MW_NE; ++e)                              \
                q_[e] = me_ ? q_[e + 1] : q_[e];                                               \
            q_[MW_NE - 1] = me_ ? KEY_INF : q_[MW_NE - 1];                                     \
        }                                                                                      \
        n_ = rfl(n_);

// Helper h (1..MW_H) pre-resolves records i = h-1, h-1+H, ... (record i: the i-th live job of the
// window, tj[] its window index).  Loads run two records ahead (keys, job row, bound) and one
// record ahead (the node rows of the candidates); the three register sets are indexed by literal
// constants only (3-way unrolled loop).
#define MW_HSTEP(A, B_, C)                                                                     \
    {                                                                                          \
        _Pragma("unroll") for (int e = 0; e < MW_EPL; ++e) { /* record i+H's candidates' rows */\
            const uint64_t k_ = kk[B_][e];                                                     \
            const uint32_t p_ = k_ != KEY_INF ? (uint32_t)k_ : (uint32_t)P.nb;                 \
            const NodeRec r_ = ld_node(rec + p_);                                              \
            rc[B_][e] = r_.cpu;                                                                \
            rm[B_][e] = r_.mem;                                                                \
            rg[B_][e] = r_.gpu;                                                                \
            ra[B_][e] = r_.avail;                                                              \
            rk[B_][e] = r_.mask;                                                               \
            ro[B_][e] = r_.orig;                                                               \
        }                                                                                      \
        {                                                                                      \
            MW_CLK(tw0_);                                                                      \
            int tn_;                                                                           \
            if (!mw_skip_live(T, P, cur, ready, S, MW_H, tn_)) goto hdone;                     \
            tj[C] = tn_;                                                                       \
            const int tt_ = min(tn_, wlast) + z;                                               \
            if (!mw_tile_ready(T, tt_, ready, S)) goto hdone;                                  \
            {                                                                                  \
                MW_CLK(tw1_);                                                                  \
                MW_ACC(a_ht, tw1_ - tw0_);                                                     \
            }                                                                                  \
            _Pragma("unroll") for (int e = 0; e < MW_EPL; ++e)                                  \
                kk[C][e] = has[e] ? ld_through(cand + eoff[e] + (int64_t)tt_ * E) : KEY_INF;   \
            jr[C] = ld_job_through(wjob + P.slot0 + tt_);                                      \
            jbd[C] = ld_through(bnd + P.slot0 + tt_);                                          \
        }                                                                                      \
        /* snapshot: the decider has resolved at least i - (MW_M - 1) records (and so has read  \
           record slot i & 7's previous one) */                                                \
        uint64_t dn_;                                                                          \
        MW_CLK(hw0_);                                                                          \
        for (unsigned sp_ = 0;; ++sp_) {                                                       \
            dn_ = __hip_atomic_load(&S->dn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   \
            const int lag_ = i - (MW_SNAP - 1) - rfl((int32_t)(uint32_t)dn_);                  \
            if (lag_ <= 0) break;                                                              \
            if ((sp_ & 7u) == 7u && (lds_ld(&S->halt) | lds_ld(&S->fail))) goto hdone;         \
            if (sp_ > MW_SPIN_LIMIT) {                                                         \
                lds_st(&S->fail, TRIP_HELPER_SNAP);                                            \
                goto hdone;                                                                    \
            }                                                                                  \
            /* the decider needs ~1k cycles a job: sleep about that long per missing job      \
               instead of polling (every poll is an LDS access the decider queues behind) */   \
            for (int s_ = min(lag_, 8); s_ > 0; --s_) __builtin_amdgcn_s_sleep(MW_HSLEEP);     \
        }                                                                                      \
        lds_acquire(); /* the rows / bitmap the decider released with dn_ */                   \
        const uint32_t v_ = (uint32_t)rfl((int32_t)(uint32_t)dn_);                             \
        const int nu_ = rfl((int32_t)(uint32_t)(dn_ >> 32));                                   \
        MwRec* R_ = &S->rec[i & (MW_R - 1)];                                                   \
        if (tj[A] >= P.w) { /* no live job left: the end record (B = 0, nothing fits) */       \
            if (lane == 0) {                                                                   \
                *reinterpret_cast<v4i32*>(&R_->h.cpu) = v4i32{0, 0, 0, 0};                     \
                *reinterpret_cast<uint4*>(&R_->h.pbit) = make_uint4(0u, (uint32_t)P.w, 0u, 0u);\
                R_->h.v = (int32_t)v_;                                                         \
                R_->h.n = 0;                                                                   \
                R_->h.q = -1;                                                                  \
                lds_release();                                                                 \
                lds_st(&R_->h.ready, (uint32_t)i + 1u);                                        \
            }                                                                                  \
            goto hdone;                                                                        \
        }                                                                                      \
        {                                                                                      \
            MW_CLK(hw1_);                                                                      \
            MW_ACC(a_hw, hw1_ - hw0_);                                                         \
            MW_ACC(a_hp, -(long long)hw1_);                                                    \
            MW_ACC(a_hx, -(long long)hw1_);                                                    \
        }                                                                                      \
        const JobRec& J_ = jr[A];                                                              \
        const uint64_t Bd_ = jbd[A];                                                           \
        uint64_t x0[MW_EPL];                                                                   \
        _Pragma("unroll") for (int e = 0; e < MW_EPL; ++e) {                                   \
            const uint64_t k_ = kk[A][e];                                                      \
            const bool ok_ = k_ <= Bd_ && k_ != KEY_INF;                                       \
            const uint32_t rel_ = ok_ ? (uint32_t)k_ - (uint32_t)P.nb : 0u;                    \
            const bool dirty_ = (S->bitmap[rel_ >> 5] >> (rel_ & 31)) & 1u;                    \
            x0[e] = ok_ && !dirty_ ? k_ : KEY_INF;                                             \
        }                                                                                      \
        uint64_t xd[UPL_MW];                                                                   \
        MwRow wr_[UPL_MW];                                                                     \
        _Pragma("unroll") for (int u = 0; u < UPL_MW; ++u) {                                   \
            xd[u] = KEY_INF;                                                                   \
            wr_[u] = MwRow{0, 0, 0, 0, 0u, 0u, 0, 0};                                          \
            const int u_ = u * 64 + lane;                                                      \
            if (u * 64 < nu_) { /* uniform: rows [0, nu) exist */                              \
                wr_[u] = S->rows[u_ < nu_ ? u_ : 0];                                           \
                const uint64_t y_ = fit_key(wr_[u].cpu, wr_[u].mem, wr_[u].gpu, wr_[u].avail,  \
                                            wr_[u].mask, wr_[u].pos, J_.cpu, J_.mem, J_.gpu,   \
                                            J_.wall, J_.pbit);                                 \
                xd[u] = u_ < nu_ && y_ <= Bd_ ? y_ : KEY_INF;                                  \
            }                                                                                  \
        }                                                                                      \
        int n_ = 0;                                                                            \
        {                                                                                      \
            MW_CLK(hx_);                                                                       \
            MW_ACC(a_hx, hx_);                                                                 \
        }                                                                                      \
        /* every entry tagged with its index (pos << 3 | e keeps the order of distinct nodes) and\
           sorted per lane once; each extraction is then one wave minimum over the lane heads  \
           plus a predicated shift in the winning lane */                                      \
        uint64_t q_[MW_NE];                                                                    \
        _Pragma("unroll") for (int e = 0; e < MW_EPL; ++e) q_[e] = mw_tag(x0[e], e);           \
        _Pragma("unroll") for (int u = 0; u < UPL_MW; ++u) q_[MW_EPL + u] = mw_tag(xd[u], MW_EPL + u);\
        mw_sort(q_);                                                                           \
        /* item index + 1 of each entry, 4 bits per entry (0: not taken) */                     \
        uint32_t sel_ = 0u;                                                                    \
        /* at most i - v nodes can change before record i is decided: i - v + 1 items suffice */\
        const int nmax_ = min(MW_M, i - (int)v_ + 1);                                          \
        MW_EXTRACT                                                                             \
        /* items: the lanes that gave an entry store it (exec-masked: only those lanes use   \
           the LDS, which the decider shares) */                                               \
        _Pragma("unroll") for (int e = 0; e < MW_EPL; ++e) {                                   \
            const uint32_t ix_ = (sel_ >> (4 * e)) & 15u;                                      \
            if (ix_) { /* probe: the node's bitmap bit */                                      \
                const uint32_t rel_ = (uint32_t)x0[e] - (uint32_t)P.nb;                        \
                const uint32_t bit_ = 1u << (rel_ & 31u);                                      \
                R_->it[ix_ - 1u] = MwItem{(uint32_t)x0[e], (uint32_t)(x0[e] >> 32), -1,        \
                                          ro[A][e], rc[A][e], rm[A][e], rg[A][e], ra[A][e],    \
                                          rk[A][e], mw_lds_addr(&S->bitmap[rel_ >> 5]), bit_,  \
                                          bit_};                                               \
            }                                                                                  \
        }                                                                                      \
        _Pragma("unroll") for (int u = 0; u < UPL_MW; ++u) {                                   \
            const uint32_t ix_ = (sel_ >> (4 * (MW_EPL + u))) & 15u;                           \
            if (ix_) /* probe: the row's version against the snapshot */                       \
                R_->it[ix_ - 1u] = MwItem{(uint32_t)xd[u], (uint32_t)(xd[u] >> 32),            \
                                          u * 64 + lane, wr_[u].orig, wr_[u].cpu, wr_[u].mem,  \
                                          wr_[u].gpu, wr_[u].avail, wr_[u].mask,               \
                                          mw_lds_addr(&S->rows[u * 64 + lane].ver),            \
                                          0xffffffffu, v_};                                    \
        }                                                                                      \
        if (lane == 0) {                                                                       \
            *reinterpret_cast<v4i32*>(&R_->h.cpu) = v4i32{J_.cpu, J_.mem, J_.gpu, J_.wall};    \
            *reinterpret_cast<uint4*>(&R_->h.pbit) =                                           \
                make_uint4(J_.pbit, (uint32_t)tj[A], (uint32_t)Bd_, (uint32_t)(Bd_ >> 32));    \
            R_->h.v = (int32_t)v_;                                                             \
            R_->h.n = n_;                                                                      \
            R_->h.q = J_.q;                                                                    \
            lds_release(); /* items and header before the ready word */                        \
            lds_st(&R_->h.ready, (uint32_t)i + 1u);                                            \
        }                                                                                      \
        {                                                                                      \
            MW_CLK(hp1_);                                                                      \
            MW_ACC(a_hp, hp1_);                                                                \
        }                                                                                      \
        MW_ACC(a_hn, 1);                                                                       \
        MW_ACC(a_hi, n_);                                                                      \
        i += MW_H;                                                                             \
    }

template <int UPL_MW>
__device__ __noinline__ void mw_helper(const CompPlan& Pref, MwShared* Sin,
                                       const NodeRec* __restrict__ rec_,
                                       const uint64_t* __restrict__ cand_,
                                       const uint64_t* __restrict__ bnd_,
                                       const JobRec* __restrict__ wjob_, int h, MwTiles Tin) {
    constexpr int MW_NE = MW_EPL + UPL_MW;
    const MwTiles T = tiles_sgpr(Tin);
    const GAS NodeRec* const rec = gview(rec_);
    const GAS uint64_t* const cand = gview(cand_);
    const GAS uint64_t* const bnd = gview(bnd_);
    const GAS JobRec* const wjob = gview(wjob_);
    // by value: a reference into the caller's stack is re-read (flat load + full vmcnt wait) after
    // every LDS store, which would drain the job-stream prefetch each step
    const CompPlan P = plan_sgpr(Pref);
    MwShared* const S = lds_opaque(Sin);
    const int lane = threadIdx.x & 63;
    const int E = P.nslice * P.ks;
    bool has[MW_EPL];       // candidate entry lane + 64 e of the job's E entries
    int64_t eoff[MW_EPL];
#pragma unroll
    for (int e = 0; e < MW_EPL; ++e) {
        has[e] = lane + 64 * e < E;
        eoff[e] = P.cand_off + (has[e] ? lane + 64 * e : 0);
    }
    const int wlast = P.w - 1;
    const int z = opaque_zero();
    const int hh = rfl(h);  // uniform (h arrives in a VGPR: the callee is out of line)
    int i = hh - 1;         // record index

    uint64_t kk[3][MW_EPL], jbd[3];
    JobRec jr[3];
    int32_t rc[3][MW_EPL], rm[3][MW_EPL], rg[3][MW_EPL], ra[3][MW_EPL], ro[3][MW_EPL];
    uint32_t rk[3][MW_EPL];
    int tj[3];      // window index of the job of each register set (P.w: past the last live job)
    int ready = 0;  // scan tiles known complete
    MwCursor cur{-1, 0ull};
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // records i and i + H
        if (!mw_skip_live(T, P, cur, ready, S, s == 0 ? hh : MW_H, tj[s])) return;
        const int tt = min(tj[s], wlast) + z;
        if (!mw_tile_ready(T, tt, ready, S)) return;  // halted / watchdog
#pragma unroll
        for (int e = 0; e < MW_EPL; ++e)
            kk[s][e] = has[e] ? ld_through(cand + eoff[e] + (int64_t)tt * E) : KEY_INF;
        jr[s] = ld_job_through(wjob + P.slot0 + tt);
        jbd[s] = ld_through(bnd + P.slot0 + tt);
    }
#pragma unroll
    for (int e = 0; e < MW_EPL; ++e) {
        const uint32_t p = kk[0][e] != KEY_INF ? (uint32_t)kk[0][e] : (uint32_t)P.nb;
        const NodeRec r = ld_node(rec + p);
        rc[0][e] = r.cpu;
        rm[0][e] = r.mem;
        rg[0][e] = r.gpu;
        ra[0][e] = r.avail;
        rk[0][e] = r.mask;
        ro[0][e] = r.orig;
    }
    MW_DECL(a_hw);
    MW_DECL(a_hn);
    MW_DECL(a_hi);
    MW_DECL(a_ht);  // waiting for scan tiles (prefetch of record i + 2H)
    MW_DECL(a_hp);  // snapshot → record published
    MW_DECL(a_hx);  // snapshot → extraction start (dirty rows read, candidates filtered)
    MW_CLK(h0);
    for (;;) {
        MW_HSTEP(0, 1, 2)
        MW_HSTEP(1, 2, 0)
        MW_HSTEP(2, 0, 1)
    }
hdone:;
    MW_CLK(h1);
    MW_ADD(3, h1 - h0);
    MW_ADD(4, a_hw);
    MW_ADD(5, a_hn);
    MW_ADD(6, a_hi);
    MW_ADD(13, a_ht);
    MW_ADD(14, a_hp);
    MW_ADD(15, a_hx);
}
#undef MW_HSTEP

// ------------------------------------------------------------------------------ decider
// One wave; lanes 0..7 carry the "written ring" (the decisions of the last 8 jobs: job t's entry
// in lane t & 7 — its node's position and row as that job left it, its dirty slot, the job) and
// record t's items (lane i: item i).  A ring entry is live for job t iff its job >= the record's
// snapshot v; when a node is written again its older entry dies, so a live entry always holds
// the node's current row.
struct MwRing {
    v4i32 a;       // cpu, mem, gpu, avail   (= MwRow's first 16 B)
    v4i32 b;       // mask, pos, orig, job   (= MwRow's last 16 B; job -1: dead)
    int32_t slot;  // dirty slot
};

struct MwRecRegs {  // one record as this lane sees it: header (every lane) and item lane & 7
    v4u32 h0, h1, h2;  // {ready, v, n, q}, {cpu, mem, gpu, wall}, {pbit, -, B lo, B hi}
    v4u32 i0, i1, i2;  // {pos, score, tag, orig}, {cpu, mem, gpu, avail}, {mask, chk_addr, chk_mask, chk_thr}
};

struct MwDec {
    int t, nu, placed, stop;  // t: records decided (live jobs)
    int done;                 // window jobs resolved when the walk ended (its stop / end record)
    bool exit;  // the window is finished (end, stop or watchdog): later steps change nothing
    int nret;       // rows appended to retired[] this round
    uint64_t dead;  // slots found dead (and listed in retired[]) whose slot is not reused yet
#ifdef MW_SEGSTAMP
    unsigned long long seg[8], prev;
#endif
};
// diagnostic (never shipped): cycles per segment of a decider step, s_memtime at each point.  The
// decider bench keeps its one launch's sums; in the engine (a -DMW_SEGSTAMP variant build) every
// decider adds its sums and, in g_seg[8], its live jobs (fit_debug_mw_seg, tools/mw_seg.py).
#ifdef MW_SEGSTAMP
__device__ unsigned long long g_seg[9];
#define MW_SEG(D_, i)                                                                           \
    do {                                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        unsigned long long now_;                                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");            \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        if (i > 0) D_.seg[i] += now_ - D_.prev;                                                 \
        D_.prev = now_;                                                                         \
    } while (0)
#else
#define MW_SEG(D_, i)
#endif

__device__ __forceinline__ void mw_read_rec(const MwRec* R, int i8, MwRecRegs& x) {
    const __attribute__((address_space(3))) v4u32* hp = lds4(&R->h);
    const __attribute__((address_space(3))) v4u32* ip = lds4(&R->it[i8]);
    x.h0 = hp[0];
    x.h1 = hp[1];
    x.h2 = hp[2];
    x.i0 = ip[0];
    x.i1 = ip[1];
    x.i2 = ip[2];
}

// Before a window starts (all threads of the block, ahead of its first barrier): the staleness
// probe of every item of every record is pointed at MwShared::pad (one 16-B store per item: its
// last 16 B, {mask, chk_addr, chk_mask, chk_thr}).  The decider issues an item's probe before it
// knows that the record is complete or that the lane holds one of its n items; such an item is
// this one or a helper's earlier one, so the read never leaves MwShared.  chk_addr is one aligned
// 32-bit word, so a read that races a helper's store sees the old address or the new one, never
// a mix; the mask and threshold read beside it may belong to the other item, but a record read
// before its ready word is read again, and that first decision is dropped.  The rest of such an
// item is never used (lane >= n, or the re-read), so it is left as it is.
__device__ __forceinline__ void mw_reset_items(MwShared* S, unsigned tid) {
    static_assert(sizeof(MwItem) == 48 && offsetof(MwItem, mask) == 32, "the probe is the last 16 B");
    static_assert((MW_M & (MW_M - 1)) == 0, "item index by shift and mask");
    const uint32_t sink = mw_lds_addr(&S->pad[0]);
    for (unsigned i = tid; i < MW_R * MW_M; i += blockDim.x)
        *reinterpret_cast<v4u32*>(&S->rec[i / MW_M].it[i % MW_M].mask) = v4u32{0u, sink, 0u, 0u};
}

// The decider's dirty set is full and job t's winner is a fresh node at position `pos` (uniform;
// the step's exception path only).  Returns the slot of a dead row — one with less than the
// component's minimum demand in one resource — after setting the fresh node's bitmap bit; the
// step's apply path then rewrites the slot with ver = t.  -1: no row is dead, or the round's
// retired list is full.
// The dead slots come from one pass over the rows (one per lane, one ballot), kept in D.dead (an
// SGPR pair) and used bit by bit; the pass runs again only when they are used up.  The pass also
// appends every dead row it keeps to retired[] (a masked store per lane, nothing to wait for), so
// taking a slot later reads nothing: a dead row never changes again, and one that is still in
// rows[] at the round's end is written back from both places with the same values.
// Why it is exact: the retired node keeps its bitmap bit, so no clean list offers
// it, and it fits no job of the component, so leaving the set changes no decision (its ring entry
// evaluates to KEY_INF); an item of a record in flight that names the slot is dropped by its probe
// (ver = t >= its snapshot), and the fresh node is in the live ring of every such record.
__device__ __forceinline__ int mw_recycle(MwShared* S, const CompPlan& P, MwDec& D, uint32_t pos) {
    if (D.dead == 0ull) {  // uniform
        const int room = MW_RCAP - D.nret;
        if (room <= 0) return -1;
        const int lane = threadIdx.x & 63;
        const MwRow r = S->rows[lane];  // all MW_UCAP = 64 rows exist: the set is full
        const int32_t mc = S->mind[0], mm = S->mind[1], mg = S->mind[2];
        const uint64_t all = __ballot(r.cpu < mc || r.mem < mm || r.gpu < mg);
        // the first `room` of them
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(all >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)all, 0u));
        const bool mine = ((all >> lane) & 1ull) && rank < room;
        const uint64_t dm = __ballot(mine);
        if (dm == 0ull) return -1;
        if (mine) mw_retired(S)[D.nret + rank] = MwRet{r.pos, r.cpu, r.mem, r.gpu};
        D.nret += (int)__builtin_popcountll(dm);
        D.dead = dm;
        // drained here, once per pass: left pending, the stores make the compiler wait before the
        // next record's reads on the step's straight line
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    }
    const int s = (int)__builtin_ctzll(D.dead);
    D.dead &= D.dead - 1ull;
    {  // the fresh node's bitmap bit, by one lane (as the apply path's bookkeeping does)
        const uint32_t rel = pos - (uint32_t)P.nb;
        const uint32_t ba = mw_lds_addr(&S->bitmap[rel >> 5]);
        const uint32_t bv = 1u << (rel & 31);
        uint64_t sv;
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_mov_b64 exec, 1\n\t"
            "ds_or_b32 %[ba], %[bv]\n\t"
            "s_mov_b64 exec, %[sv]"
            : [sv] "=&s"(sv)
            : [ba] "v"(ba), [bv] "v"(bv)
            : "memory");
    }
    return s;
}

// The slim ring's placement store (mw_decide SP): a group of up to 64 parked placements {job oq,
// winner's position ov (-1: unplaced)} is translated to node ids by one load per lane, issued when
// the group is complete and consumed when the NEXT group is complete (or at the decider's end), so
// the decider's chain never waits for it.  pos lies in the component's [nb, ne): it comes from a
// key of one of its nodes.
#ifndef MW_POSOUT
#define MW_POSOUT 1  // 0: the slim ring keeps the node id (the A/B arm of the position store)
#endif
struct MwPend {
    int32_t q, id;  // per lane: job of the pending group (-1: none), its node id (loaded)
};
__device__ __forceinline__ void mw_store_pending(MwPend& pend, int32_t* out, int kmax) {
    if (pend.q >= 0) ((GAS int32_t*)out)[(int64_t)pend.q * kmax] = pend.id;
    pend.q = -1;
}
__device__ __forceinline__ void mw_store_group(MwPend& pend, int32_t oq, int32_t ov, int32_t* out,
                                               int kmax, const GAS NodeRec* rec) {
    // the group before: its ids were loaded 64 jobs ago.  Waited for here, on every path and
    // before the store: left to the compiler, the wait lands behind the (exec-masked) store, where
    // it waits for that store as well before pend.id may be rewritten.
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
    mw_store_pending(pend, out, kmax);
    pend.q = oq;
    pend.id = -1;
    if (oq >= 0 && ov >= 0) pend.id = rec[ov].orig;
}

// One job of the decider: job D.t with record `cur` (its data read after an acquire of the ready
// word `flag`; refreshed in place on the slow path), `nxt` receives record t+1.  E = t & 7 is a
// compile-time constant.  Straight-line: the decision is computed unconditionally and selected (no
// exec-masked region), its bookkeeping is masked with `go` instead of branched around, and the
// only branch is the rare exception (record not ready, B exceeded, dirty set full).  Once D.exit
// is set the step has no effect: the caller tests it once per 8 jobs.
// RC: the 64-row set with recycling (MwShared::ucap == MW_UCAP); else UCAP rows and the
// parent's code, instruction for instruction.
// SP: the slim ring of a component that is exactly one partition (MwShared::slim).  Every node's
// mask and every job's pbit is then that partition's bit, so the ring rows' partition test is
// always true: the ring's mask lane is set to all ones once and never selected, read or written
// again (rows[].mask holds all ones, which the helpers' unchanged tests pass).  The node id leaves
// the ring as well: the winner's POSITION is parked as the placement and translated to its id
// (rec[pos].orig, static: write-backs touch cpu, mem and gpu only) where 64 placements are stored
// (mw_store_group).  rows[].orig and the items' orig / mask are then unused.  !SP: the code of
// components of several partitions, unchanged.
template <int E, bool RC, bool SP>
__device__ __forceinline__ void mw_decide(MwShared* S, const CompPlan& P, MwDec& D, MwRing& R,
                                          MwRecRegs& cur, MwRecRegs& nxt, uint32_t& flag,
                                          int32_t& oq, int32_t& ov, int32_t* out, int kmax,
                                          uint64_t& waitcyc, MwPend& pend,
                                          const GAS NodeRec* rec) {
    const int lane = threadIdx.x & 63;
    const int t = D.t;
    constexpr bool PO = SP && MW_POSOUT;  // the node id off the ring
#ifdef MW_DECIDER_BENCH
    if (t >= P.w) D.exit = true;  // pre-filled records: no end record
#endif
    MW_SEG(D, 0);
    // publish the decisions so far (the previous job's row / bitmap writes were issued before
    // record t's reads, all of which are complete here): release store of {decided, nu}
    lds_release();
    __hip_atomic_store(&S->dn, ((uint64_t)(uint32_t)D.nu << 32) | (uint32_t)t, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
    // ready word of record t+1 (relaxed; acquired below, before its data is read)
    // t == E (mod 8) while the window runs (each window starts at t = 0 and every step before an
    // exit advances t by one; after an exit the record read below is never used)
    const MwRec* Rn = &S->rec[(E + 1) & (MW_R - 1)];
    const uint32_t flag_n = lds_ld(&Rn->h.ready);
    MW_SEG(D, 1);

    // the decision of job t against record `x`
    struct Dec {
        uint64_t bs;  // best key (uniform)
        int32_t sc, sm, sg, sa, sk, so, ss;  // per lane: its candidate's row, demand subtracted
        int w, wslot;
        bool placed, fresh, stopB, full;
    };
    auto decide = [&](const MwRecRegs& x) {
        Dec d;
        const int32_t v = (int32_t)x.h0.y, n = (int32_t)x.h0.z;
        const int32_t jc = (int32_t)x.h1.x, jm = (int32_t)x.h1.y, jg = (int32_t)x.h1.z,
                      jw = (int32_t)x.h1.w;
        const uint32_t jp = x.h2.x;
        const uint64_t B = ((uint64_t)x.h2.w << 32) | x.h2.z;
        // item staleness: was its node written by a job in [v, t)?  The helper left the LDS word
        // that answers it (MwItem::chk_*): a clean item's bitmap word — its bit is set by the
        // fresh placement that dirtied the node after the snapshot — or a dirty item's row
        // version.  Both are written by this wave only (the bookkeeping of the jobs before t, in
        // issue order before this read).  Issued here, consumed after the ring rows' keys.
        // In bounds even when record t is not complete yet: chk_addr is a single aligned word,
        // the window's initial one or a helper's, never torn (mw_reset_items).
        const uint32_t pv = *(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)x.i2.y;
        // live ring rows at their current state
        const bool live = R.b.w >= v;
        const uint64_t rk0 = SP ? fit_key(R.a.x, R.a.y, R.a.z, R.a.w, ~0u, (uint32_t)R.b.y, jc, jm,
                                          jg, jw, ~0u)  // one partition: no test
                                : fit_key(R.a.x, R.a.y, R.a.z, R.a.w, (uint32_t)R.b.x, (uint32_t)R.b.y,
                                          jc, jm, jg, jw, jp);
        const uint64_t rkey = live ? rk0 : KEY_INF;
        const uint32_t ip = x.i0.x;
        const bool stale = (pv & x.i2.z) >= x.i2.w;
        const uint64_t ik0 = ((uint64_t)x.i0.y << 32) | ip;
        const uint64_t ikey = (lane < n && !stale) ? ik0 : KEY_INF;
        const bool tr = rkey < ikey;  // this lane's ring row beats its item
        const uint64_t cand = tr ? rkey : ikey;
        // the winner's fields, demand already subtracted (selected per lane, read from one)
        d.sc = (tr ? R.a.x : (int32_t)x.i1.x) - jc;
        d.sm = (tr ? R.a.y : (int32_t)x.i1.y) - jm;
        d.sg = (tr ? R.a.z : (int32_t)x.i1.z) - jg;
        d.sa = tr ? R.a.w : (int32_t)x.i1.w;
        d.sk = SP ? 0 : tr ? R.b.x : (int32_t)x.i2.x;
        d.so = PO ? 0 : tr ? R.b.z : (int32_t)x.i0.w;
        d.ss = tr ? R.slot : (int32_t)x.i0.z;
        const uint64_t best = min8_2pass(cand);
        // lanes 0..7 all hold `best`; the winner is the lane whose candidate equals it
        const uint64_t mine = __ballot(cand == best) & 0xffull;
        d.w = __builtin_ctzll(mine | 0x100ull) & 7;
        const uint32_t bhi = (uint32_t)readlane((int32_t)(best >> 32), 0);
        const uint32_t blo = (uint32_t)readlane((int32_t)(uint32_t)best, 0);
        d.bs = ((uint64_t)bhi << 32) | blo;
        d.placed = d.bs != KEY_INF;
        d.wslot = readlane(d.ss, d.w);
        d.fresh = d.placed && d.wslot < 0;
        d.full = d.fresh && D.nu >= (RC ? MW_UCAP : UCAP);
        d.stopB = B != KEY_INF && d.bs > B;
        return d;
    };
    Dec d = decide(cur);
    MW_SEG(D, 2);
#ifdef MW_DECIDER_BENCH
    const bool rec_missing = false;  // diagnostic: records pre-filled, never "not ready"
#else
    const bool rec_missing = flag != (uint32_t)t + 1u;
#endif
    if (__builtin_expect(!D.exit && (rec_missing || d.stopB || d.full), 0)) {  // the one branch
        if (rec_missing) {  // record t not complete when read: wait for it, read it again
            MW_CLK(c0);
            for (unsigned sp = 0;; ++sp) {
                flag = lds_ld(&S->rec[t & (MW_R - 1)].h.ready);
                if (flag == (uint32_t)t + 1u) break;
                if (sp > MW_SPIN_LIMIT || lds_ld(&S->fail)) {
                    lds_st(&S->fail, TRIP_DECIDER_REC);
                    D.stop = 3;
                    D.exit = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(0);
            }
            lds_acquire();
            mw_read_rec(&S->rec[t & (MW_R - 1)], lane & 7, cur);
            {
                MW_CLK(c1);
                MW_ACC(waitcyc, c1 - c0);
            }
            d = decide(cur);
        }
        // the dirty set is full: a dead row's slot takes the fresh node (mw_recycle), and the step
        // goes on as if the node had been dirty in that slot
        if constexpr (RC && MW_RCAP > 0) {
            if (!D.exit && d.full && !d.stopB) {
                const int s = mw_recycle(S, P, D, (uint32_t)d.bs);
                if (s >= 0) {
                    d.wslot = s;
                    d.fresh = false;
                    d.full = false;
                }
            }
        }
        if (!D.exit && (d.stopB || d.full)) {
            // the end record (no live job left: B = 0, nothing fits) or a stop at the record's
            // job: candidate list exhausted (rescan) / dirty set full
            D.done = (int32_t)cur.h2.y;
            if (D.done < P.w) D.stop = d.stopB ? 1 : 2;
            D.exit = true;
        }
    }
    // ---- apply job t (masked by `go`; the ring is not read again once D.exit is set) ----------
    MW_SEG(D, 3);
    const bool go = !D.exit;
    const bool placed = d.placed && go, fresh = d.fresh && go;
    const int w = d.w;
    const int32_t pos = (int32_t)(uint32_t)d.bs;
    const int32_t nc = readlane(d.sc, w), nm = readlane(d.sm, w), ng = readlane(d.sg, w);
    const int32_t na = readlane(d.sa, w);
    const int32_t nk = SP ? 0 : readlane(d.sk, w), no = PO ? pos : readlane(d.so, w);
    const int32_t slot = fresh ? D.nu : d.wslot;
    // an older ring entry of the same node dies (lane E is rewritten below)
    R.b.w = (placed && R.b.y == pos) ? -1 : R.b.w;
    R.a.x = writelane_c<E>(nc, R.a.x);
    R.a.y = writelane_c<E>(nm, R.a.y);
    R.a.z = writelane_c<E>(ng, R.a.z);
    R.a.w = writelane_c<E>(na, R.a.w);
    if constexpr (!SP) R.b.x = writelane_c<E>(nk, R.b.x);
    R.b.y = writelane_c<E>(pos, R.b.y);
    if constexpr (!PO) R.b.z = writelane_c<E>(no, R.b.z);
    R.b.w = writelane_c<E>(placed ? t : -1, R.b.w);
    R.slot = writelane_c<E>(slot, R.slot);
    MW_SEG(D, 4);
    // read record t+1's data after acquiring its ready word (the load above is long done)
    flag = flag_n;
    lds_acquire();
    mw_read_rec(Rn, lane & 7, nxt);
    MW_SEG(D, 5);
    // bookkeeping: dirty row, bitmap bit — fire-and-forget LDS writes, no branch: lane E alone
    // (exec = its bit, or none when the job is not placed) stores the new row and ORs the bitmap
    // bit (0 when the node was already dirty): 3 LDS ops of one lane instead of 64 lanes' worth of
    // traffic in the LDS pipe the helpers share
    {
        typedef __attribute__((address_space(3))) MwRow* LRow;
        const uint32_t ra = (uint32_t)(uintptr_t)(LRow)&S->rows[slot];
        const uint32_t rel = (uint32_t)pos - (uint32_t)P.nb;
        const uint32_t ba = mw_lds_addr(&S->bitmap[rel >> 5]);
        const uint32_t bv = fresh ? 1u << (rel & 31) : 0u;
        const uint32_t pl = (uint32_t)rfl(placed ? 1 : 0);
        const uint64_t m = ((uint64_t)(uint32_t)rfl((int32_t)(pl << E)) |
                            ((uint64_t)(uint32_t)rfl(0) << 32));  // exec mask: SGPR pair
        uint64_t sv;
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_mov_b64 exec, %[m]\n\t"
            "ds_write_b128 %[ra], %[a]\n\t"
            "ds_write_b128 %[ra], %[b] offset:16\n\t"
            "ds_or_b32 %[ba], %[bv]\n\t"
            "s_mov_b64 exec, %[sv]"
            : [sv] "=&s"(sv)
            : [m] "s"(m), [ra] "v"(ra), [a] "v"(R.a), [b] "v"(R.b), [ba] "v"(ba), [bv] "v"(bv)
            : "memory");
    }
    D.nu += fresh;
    D.placed += placed;
    MW_SEG(D, 6);
    // placement of job t parked in lane t & 63 (after an exit that lane is past the last store)
    oq = writelane(rfl((int32_t)cur.h0.w), t & 63, oq);
    ov = writelane(placed ? no : -1, t & 63, ov);
    if (E == 7 && go && (t & 63) == 63) {  // uniform, once per 64 jobs: store 64 placements
        if constexpr (PO) {
            mw_store_group(pend, oq, ov, out, kmax, rec);
        } else {
            if (oq >= 0) ((GAS int32_t*)out)[(int64_t)oq * kmax] = ov;
        }
        oq = -1;
    }
    D.t = t + (go ? 1 : 0);
    MW_SEG(D, 7);
}

// Out of line (as is mw_helper): called once per round, each gets its own register allocation
// instead of sharing the persistent kernel's (which otherwise spills SGPRs in this loop).
template <bool RC, bool SP = false>
__device__ __noinline__ CommitResult mw_decider(const CompPlan& Pref, MwShared* Sin,
                                                int32_t* __restrict__ out, int kmax,
                                                const NodeRec* __restrict__ rec_ = nullptr) {
    const GAS NodeRec* const rec = gview(rec_);  // SP: the placement store's id lookup
    MwPend pend{-1, -1};
    const CompPlan P = plan_sgpr(Pref);  // by value (see mw_helper)
    MwShared* const S = lds_opaque(Sin);
    const int lane = threadIdx.x & 63;
    __builtin_amdgcn_s_setprio(3);  // shares its SIMD with a helper wave
    MwDec D{0, 0, 0, 0, 0, false, 0, 0ull};
#ifdef MW_SEGSTAMP
    for (int i = 0; i < 8; ++i) D.seg[i] = 0;
    D.prev = 0;
#endif
    MwRing R;
    R.a = v4i32{0, 0, 0, 0};
    R.b = v4i32{SP ? -1 : 0, -1, -1, -1};  // dead, position matching no item (SP: mask all ones)
    R.slot = -1;
    int32_t oq = -1, ov = -1;  // placement of job t parked in lane t & 63, stored 64 at a time
    uint64_t waitcyc = 0;
    MW_CLK(d0);
    // record 0: wait for its ready word, acquire, read
    MwRecRegs ra, rb;
    uint32_t flag = 0;
    if (P.w > 0) {
        for (unsigned sp = 0;; ++sp) {
            flag = lds_ld(&S->rec[0].h.ready);
#ifdef MW_DECIDER_BENCH
            break;
#endif
            if (flag == 1u) break;
            if (sp > MW_SPIN_LIMIT || lds_ld(&S->fail)) {
                lds_st(&S->fail, TRIP_DECIDER_REC);
                D.stop = 3;
                D.exit = true;
                break;
            }
            __builtin_amdgcn_s_sleep(0);
        }
        lds_acquire();
        mw_read_rec(&S->rec[0], lane & 7, ra);
    } else {
        D.exit = true;
    }
    {
        MW_CLK(r0c);
        MW_ADD(17, r0c - d0);
        MW_ADD(18, 1);
    }
    // 8-way unrolled: the ring lane (t & 7) is a constant in every step; the two record register
    // sets alternate with the step's parity; the exit is tested once per 8 steps
    while (!D.exit) {
        mw_decide<0, RC, SP>(S, P, D, R, ra, rb, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<1, RC, SP>(S, P, D, R, rb, ra, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<2, RC, SP>(S, P, D, R, ra, rb, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<3, RC, SP>(S, P, D, R, rb, ra, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<4, RC, SP>(S, P, D, R, ra, rb, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<5, RC, SP>(S, P, D, R, rb, ra, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<6, RC, SP>(S, P, D, R, ra, rb, flag, oq, ov, out, kmax, waitcyc, pend, rec);
        mw_decide<7, RC, SP>(S, P, D, R, rb, ra, flag, oq, ov, out, kmax, waitcyc, pend, rec);
    }
    const int t = D.t;
    if constexpr (SP && MW_POSOUT) {  // the pending group, then the last, partial one
        mw_store_group(pend, lane < (t & 63) ? oq : -1, ov, out, kmax, rec);
        mw_store_pending(pend, out, kmax);
    } else {
        if (oq >= 0 && lane < (t & 63)) ((GAS int32_t*)out)[(int64_t)oq * kmax] = ov;  // last group
    }
    // final {decided, nu}, then halt (the helpers' exit)
    lds_release();
    __hip_atomic_store(&S->dn, ((uint64_t)(uint32_t)D.nu << 32) | (uint32_t)t, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
    lds_st(&S->nret, (uint32_t)D.nret);
    lds_st(&S->halt, 1u);
    MW_CLK(d1);
    MW_ADD(0, d1 - d0);
#ifdef MW_SEGSTAMP
    if (lane == 0) {
#ifdef MW_DECIDER_BENCH
        for (int i = 0; i < 8; ++i) g_seg[i] = D.seg[i];
#else
        for (int i = 0; i < 8; ++i) atomicAdd(&g_seg[i], D.seg[i]);
        atomicAdd(&g_seg[8], (unsigned long long)t);
#endif
    }
#endif
    MW_ADD(1, waitcyc);
    MW_ADD(2, t);
#ifdef MW_DECIDER_BENCH
    D.done = t;
#endif
    return CommitResult{D.done, D.stop, D.nu, D.placed};
}

// All MW_WAVES waves of the block call this; returns the same result in every wave.
__device__ __forceinline__ CommitResult commit_window_mw(const CompPlan& P, MwShared* S,
                                                         NodeRec* __restrict__ rec,
                                                         const uint64_t* __restrict__ cand,
                                                         const uint64_t* __restrict__ bnd,
                                                         const JobRec* __restrict__ wjob,
                                                         int32_t* __restrict__ out, int kmax,
                                                         MwTiles T = MwTiles{nullptr, 0u, nullptr, nullptr, 0u, 0u, 0u, nullptr}) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwords = (P.ne - P.nb + 31) >> 5;
    for (int i = threadIdx.x; i < nwords; i += MW_WAVES * 64) S->bitmap[i] = 0u;
    if (threadIdx.x < MW_R) S->rec[threadIdx.x].h.ready = 0u;
    mw_reset_items(S, threadIdx.x);
    if (threadIdx.x == 0) {
        S->dn = 0ull;
        S->halt = 0u;
        S->fail = 0u;
        S->nret = 0u;
    }
    __syncthreads();
    if (wave == 0) {
        // block-uniform: the 64-row set with recycling, or UCAP rows
        // ... and the slim ring where the component is one partition
        const bool rc = S->ucap == (uint32_t)MW_UCAP;
        const CommitResult r = S->slim ? (rc ? mw_decider<true, true>(P, S, out, kmax, rec)
                                             : mw_decider<false, true>(P, S, out, kmax, rec))
                                       : (rc ? mw_decider<true>(P, S, out, kmax)
                                             : mw_decider<false>(P, S, out, kmax));
        if (threadIdx.x == 0) put_result(S->res, r);
    } else {
        // waves 1.. : helpers 1..MW_H, with one or two dirty rows per lane (block-uniform)
        if (S->ucap == (uint32_t)MW_UCAP) mw_helper<1>(P, S, rec, cand, bnd, wjob, wave, T);
        else mw_helper<2>(P, S, rec, cand, bnd, wjob, wave, T);
    }
    __syncthreads();
    const CommitResult r = get_result(S->res);
    // write the dirty rows back for the next round's scan, through (sc1: the next round's
    // publish needs no release fence for them; {cpu, mem} as one 8-B word, then gpu)
    for (int u = threadIdx.x; u < r.dirty; u += MW_WAVES * 64) {
        const MwRow w = S->rows[u];
        NodeRec* d = rec + w.pos;
        __hip_atomic_store(reinterpret_cast<uint64_t*>(&d->cpu),
                           (uint64_t)(uint32_t)w.cpu | ((uint64_t)(uint32_t)w.mem << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&d->gpu, w.gpu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the rows retired this round: no other row of the round names their nodes
    for (int u = threadIdx.x; u < (int)S->nret; u += MW_WAVES * 64) {
        const MwRet w = mw_retired(S)[u];
        NodeRec* d = rec + w.pos;
        __hip_atomic_store(reinterpret_cast<uint64_t*>(&d->cpu),
                           (uint64_t)(uint32_t)w.cpu | ((uint64_t)(uint32_t)w.mem << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&d->gpu, w.gpu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave, before the barrier
    __syncthreads();
    return r;
}

}  // namespace fitgpu

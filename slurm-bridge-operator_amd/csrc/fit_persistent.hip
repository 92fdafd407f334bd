// fit_persistent.hip — the whole placement in ONE launch.
//
// Blocks [0, C) are committers: wave 0 of block c owns partition component c; it publishes each
// round's scan tiles into a device task ring, waits for its per-component done counter, then
// runs commit_window (fit_common.h) on the results.  Blocks [C, C+W) are scan workers: they
// claim tiles from the ring in order and run scan_tile.  Components therefore advance at their
// own pace — no host round trip and no global round barrier — while the scan work of all of
// them shares the whole chip.
//
// Cross-workgroup hand-offs follow cdna_hip_programming.md §6 Guideline 16 (placement-
// independent, agent scope):
//   producer: plain stores → every storing wave `s_waitcnt vmcnt(0)` → barrier → one lane
//             release fence → `s_waitcnt vmcnt(0)` → relaxed agent atomic (counter / granule)
//   consumer: relaxed agent poll → ONE acquire fence → `s_waitcnt vmcnt(0)` (→ barrier) → plain
//             loads; plus `s_dcache_inv` because node rows, plans and job rows are read through
//             the scalar cache, which an acquire fence does not invalidate.
// Every spin is bounded; a watchdog trip sets ctl->error and drains every block.
#include <algorithm>

#include "fit_engine_frame.h"

namespace fitgpu {

// Windows holding a multi-node job: the single-wave commit (fit_common.h), kept out of line so
// its registers are allocated apart from the decider / helper / worker loops.
__device__ __noinline__ CommitResult engine_commit_single(int c, const CompPlan P, NodeRec* rec,
                                                          const uint64_t* cand,
                                                          const uint64_t* bnd, const JobRec* wjob,
                                                          int32_t* out, int kmax,
                                                          uint32_t* bitmap, uint32_t* scratch) {
    // the bitmap's LDS address as an opaque SGPR value: seen through, the compiler re-derives it
    // from the dynamic-LDS offset table at every access (a scalar load + lgkmcnt(0) wait each);
    // the arrays as global pointers (commit_window: no flat accesses)
    typedef __attribute__((address_space(3))) uint32_t* LdsWords;
    uint32_t a = (uint32_t)(uintptr_t)(LdsWords)bitmap;
    asm volatile("" : "+s"(a));
    uint32_t sa = (uint32_t)(uintptr_t)(LdsWords)scratch;  // 256 B of LDS the helpers do not use here
    asm volatile("" : "+s"(sa));
    return commit_window<MW_EPL, true>(c, P, (GAS NodeRec*)rec, gview(cand), 0, 1, gview(bnd), gview(wjob),
                                       (GAS int32_t*)out, kmax, (LdsWords)(uintptr_t)a, sa);
}

#ifndef MW_SLIM
#define MW_SLIM 1  // 0: every component runs the full ring (the A/B arm of the slim ring)
#endif
#ifndef FIT_K0
#define FIT_K0 4  // > 0: a round's first job tile keeps FIT_K0 keys per block-slice (scan_tile KW)
#endif
#ifndef FIT_K0W
#define FIT_K0W 8  // > 0: the first job tile after a rescan inside the previous round's first tile keeps
                   // FIT_K0W keys per block-slice, unpaired, for K0W_ROUNDS rounds ("wide"): runs of
                   // identical jobs (array tasks) drain the FIT_K0 lists' bound within a few jobs
#endif
#ifndef K0W_ROUNDS
#define K0W_ROUNDS 8
#endif
#ifndef K_T0PAIR4
#define K_T0PAIR4 1  // ... also a 4-key component's (C3o: one 100k-node component, 32 slices x 4 keys)
#endif
#ifndef K_T0PAIR
#define K_T0PAIR 1  // k_engine: a k = 1 window's first job tile as 2 x nslice half-size block-slices, paired
#endif
// A round's first job tile stages its block-slice's node rows in LDS behind the merge buffer and
// the task slot (scan_tile STAGE) when they fit: SCAN_WAVES * P.sub <= STAGE_ROWS (C3: 8 x 98).
constexpr size_t STAGE_OFF = (sizeof(uint64_t) * (SCAN_WAVES / 2) * KS * 64 + 16 + 63) & ~(size_t)63;
constexpr int STAGE_ROWS = 1024;

__global__ __launch_bounds__(SCAN_WAVES * 64) void k_engine(
    EngineCtl* __restrict__ ctl, unsigned long long* __restrict__ ring,
    const CompState* __restrict__ cs, CompOut* __restrict__ co, CompPlan* __restrict__ plans,
    int ncomp, NodeRec* __restrict__ rec, const int32_t* __restrict__ jl,
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem,
    const int32_t* __restrict__ jgpu, const int32_t* __restrict__ jwall,
    const uint16_t* __restrict__ jpart, const uint16_t* __restrict__ jk,
    uint64_t* __restrict__ cand, uint64_t* __restrict__ bnd, JobRec* __restrict__ wjob,
    int32_t* __restrict__ out, int kmax, int64_t* __restrict__ wbusy,
    const int32_t* __restrict__ jpk, unsigned wd, const int32_t* __restrict__ jmin,
    const EngineCompIds ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) stamp_start(ctl);

    if ((int)blockIdx.x < ncomp) {
        // ================================================================== committer
        // Wave 0 runs the round protocol (publish tiles, wait, acquire); then all 8 waves commit
        // the window together: wave 0 decides, waves 1..7 pre-resolve (fit_commit_mw.h).
        __shared__ int s_fail;
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const int c = blockIdx.x;
        const CompState S = cs[c];
        MwShared* M = reinterpret_cast<MwShared*>(smem);
        if (threadIdx.x == 0) {
            M->wd = wd;  // the commit waits' deadline (fit_commit_mw.h)
            // the component's minimum demands (k_prefilter), read once: a dirty row below one of
            // them fits none of its jobs and may be retired (fit_commit_mw.h mw_recycle)
            const int32_t* mn = jmin + 3 * ids.id[c];
            M->mind[0] = mn[0];
            M->mind[1] = mn[1];
            M->mind[2] = mn[2];
            // 64 dirty rows with recycling where a round start is cheap; a component scanned with
            // fewer keys per slice (its sub-slices would exceed the target: > 16k nodes) pays its
            // round starts dearly and keeps 128 rows (C3o: 837 rounds against 1,100)
            M->ucap = S.ks == KS ? (uint32_t)MW_UCAP : (uint32_t)UCAP;
            // one partition: no partition test on the decider's ring, positions parked as
            // placements (fit_commit_mw.h mw_decide SP)
            M->slim = MW_SLIM && S.onepart != 0 ? 1u : 0u;
        }
        const Committer K{ctl, comp_ring(ring, c, ncomp), plans, bnd, c, wd};
        RoundAcct A;
        int32_t cursor = S.jstart, win = S.wmin;
        bool prev_multi = false;  // the previous round ran the single-wave commit (plain row stores)
        int wide_left = 0;        // rounds left whose first tile is wide (FIT_K0W)
        while (cursor < S.jend) {
            const int w = min(win, S.jend - cursor);
            const unsigned rnd = (unsigned)A.rounds + 1u;  // task round tag
            const int par = (int)(rnd & 1u);                // buffer set of this round
            CompPlan P;
            round_plan(P, S, cursor, w, par);
            // a window holding a multi-node job is committed by wave 0 alone (commit_window
            // handles k > 1) after its whole scan; the decider/helper pipeline covers k = 1
            // windows and starts at once: helpers wait per job tile (MwTiles)
            const bool multi = jpk[cursor + w] != jpk[cursor];
            // a multi-node job needs k <= KS keys in its first tile; a k = 1 window's first tile
            // keeps FIT_K0 keys per block-slice and is scanned as paired half-slices (K_T0PAIR)
            // (the pair scratch holds 4 keys: the FIT_K0 list, or a 4-key component's own, C3o)
            // — unless a recent round stopped for a rescan inside its first tile: then FIT_K0W keys
            // per block-slice, unpaired (bit 2; components with ks <= FIT_K0W keep their first tile)
            const bool wide = !multi && FIT_K0W > 0 && FIT_K0W < S.ks && wide_left > 0;
            const bool pair = !multi && !wide && K_T0PAIR && 2 * S.nslice <= 64 &&
                              ((FIT_K0 > 0 && FIT_K0 <= 4 && FIT_K0 < S.ks) || (K_T0PAIR4 && S.ks <= 4));
            P.k0 = multi ? 0 : wide ? 4 : (1 | (pair ? 2 : 0));
            // (a k = 1 window: ENGINE_AHEAD job tiles now; after a single-wave commit: a release)
            if (round_open(K, S, P, rnd, A, multi ? 0u : (unsigned)ENGINE_AHEAD, multi, prev_multi,
                           &ctl->tfeas[par][c][0], &M->pubt, &s_fail))
                break;  // block-uniform
            const unsigned ntj = (unsigned)((w + SCAN_JOBS - 1) / SCAN_JOBS);
            const bool jit = ENGINE_AHEAD > 0 && M->pubt < ntj;  // block-uniform (before the commit)
            CommitResult R;
            if (!multi) {
                R = commit_window_mw(P, M, rec, cand, bnd, wjob, out, kmax,
                                     MwTiles{&ctl->tdone[par][c][0], (unsigned)S.nslice, jit ? K.ring : nullptr,
                                             ctl, rnd, (unsigned)c, ntj, &ctl->tfeas[par][c][0]});
            } else {
                if (wave == 0) {
                    const CommitResult r0 =
                        engine_commit_single(c, P, rec, cand, bnd, wjob, out, kmax, M->bitmap,
                                             reinterpret_cast<uint32_t*>(&M->rows[0]));
                    if (lane == 0) put_result(M->res, r0);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // row write-back stores
                }
                __syncthreads();
                R = get_result(M->res);
                __syncthreads();
            }
            if (!round_close(K, S, P, rnd, A, R, jit, M, (unsigned)TRIP_SINGLE_TILE)) break;
            prev_multi = multi;
            if (R.stop == 1 && R.done < SCAN_JOBS) wide_left = K0W_ROUNDS;
            else if (wide_left > 0) --wide_left;
            cursor += R.done;
#ifndef ENGINE_WGROW
#define ENGINE_WGROW 10  // next window after a stop, in eighths of the jobs the round resolved
#endif
            win = max(S.wmin, min(S.wmax, R.stop ? (ENGINE_WGROW * R.done) / 8 : 2 * w));
        }
        if (wave == 0) rounds_end(K, co, A, cursor - S.jstart);
        return;
    }

    // ====================================================================== scan worker
    unsigned long long* task_slot =
        reinterpret_cast<unsigned long long*>(smem + sizeof(uint64_t) * (SCAN_WAVES / 2) * KS * 64);
    scan_worker(
        ctl, ring, plans, ncomp, wd, wbusy, (int)blockIdx.x - ncomp, task_slot,
        [&](CompPlan& P, int tile, int s, int c, int par, unsigned rnd) {
            const bool pair = tile == 0 && (P.k0 & 2);  // half-size block-slices, paired (K_T0PAIR)
            bool counts = true;
            switch (P.ks) {  // block-uniform; the host picks one of these (engine.cpp)
#define SCAN_K(K_)                                                                               \
    case K_:                                                                                      \
        if (FIT_K0W > 0 && FIT_K0W < K_ && tile == 0 && (P.k0 & 4)) { /* wide, unpaired */          \
            constexpr int KW_ = (FIT_K0W > 0 && FIT_K0W < K_ ? FIT_K0W : K_);                        \
            uint64_t(*xkw)[KW_][64] = reinterpret_cast<uint64_t(*)[KW_][64]>(smem);                 \
            if (SCAN_WAVES * P.sub <= STAGE_ROWS) /* block-uniform */                               \
                scan_tile<true, KW_, K_, true>(P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart,   \
                                               jk, cand, bnd, wjob, xkw, &ctl->tfeas[par][c][tile],    \
                                               reinterpret_cast<NodeRec*>(smem + STAGE_OFF));     \
            else                                                                                  \
                scan_tile<true, KW_, K_>(P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, \
                                         cand, bnd, wjob, xkw, &ctl->tfeas[par][c][tile]);             \
        } else if (FIT_K0 > 0 && FIT_K0 < K_ && tile == 0 && (P.k0 & 1)) {                        \
            constexpr int K0_ = (FIT_K0 > 0 && FIT_K0 < K_ ? FIT_K0 : K_);                        \
            uint64_t(*xk0)[K0_][64] = reinterpret_cast<uint64_t(*)[K0_][64]>(smem);               \
            bool done_ = false;                                                                   \
            if constexpr (K0_ <= 4) { /* the pair scratch holds 4 keys */                          \
                done_ = pair;                                                                     \
                if (pair && SCAN_WAVES * P.sub <= STAGE_ROWS) /* block-uniform */                  \
                    counts = scan_tile<true, K0_, K_, true, true>(                                \
                        P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, cand, bnd, wjob, xk0, \
                        &ctl->tfeas[par][c][tile], reinterpret_cast<NodeRec*>(smem + STAGE_OFF),     \
                        &ctl->tpair[par][c][0]);                                                  \
                else if (pair)                                                                    \
                    counts = scan_tile<true, K0_, K_, false, true>(                               \
                        P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, cand, bnd, wjob, xk0, \
                        &ctl->tfeas[par][c][tile], nullptr, &ctl->tpair[par][c][0]);              \
            }                                                                                     \
            if (done_) {                                                                          \
            } else if (SCAN_WAVES * P.sub <= STAGE_ROWS) /* block-uniform */                       \
                scan_tile<true, K0_, K_, true>(P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, \
                                               jk, cand, bnd, wjob, xk0, &ctl->tfeas[par][c][tile],    \
                                               reinterpret_cast<NodeRec*>(smem + STAGE_OFF));     \
            else                                                                                  \
                scan_tile<true, K0_, K_>(P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, \
                                         cand, bnd, wjob, xk0, &ctl->tfeas[par][c][tile]);             \
        } else if (K_ <= 4 && pair) { /* a 4-key component's first tile, paired */               \
            if constexpr (K_ <= 4) {                                                              \
                uint64_t(*xk4)[K_][64] = reinterpret_cast<uint64_t(*)[K_][64]>(smem);             \
                if (SCAN_WAVES * P.sub <= STAGE_ROWS) /* block-uniform */                         \
                    counts = scan_tile<true, K_, K_, true, true>(                                 \
                        P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, cand, bnd, wjob, xk4, \
                        &ctl->tfeas[par][c][tile], reinterpret_cast<NodeRec*>(smem + STAGE_OFF),     \
                        &ctl->tpair[par][c][0]);                                                  \
                else                                                                              \
                    counts = scan_tile<true, K_, K_, false, true>(                                \
                        P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, cand, bnd, wjob, xk4, \
                        &ctl->tfeas[par][c][tile], nullptr, &ctl->tpair[par][c][0]);              \
            }                                                                                     \
        } else {                                                                                  \
            scan_tile<true, K_>(P, tile, s, rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, cand,    \
                                bnd, wjob, reinterpret_cast<uint64_t(*)[K_][64]>(smem),           \
                                &ctl->tfeas[par][c][tile]);                                            \
        }                                                                                         \
        break;
                SCAN_K(16)
                SCAN_K(8)
                SCAN_K(4)
                SCAN_K(2)
#undef SCAN_K
                default:  // no scan kernel for this key count: trip the watchdog, never guess
                    if (threadIdx.x == 0)
                        trip_record(ctl, 8u, TRIP_NO_KERNEL, (unsigned)c, rnd, (unsigned)P.ks, 0u, 0u, 0u,
                                    realtime());
                    break;
            }
            return counts;
        },
        [&](int c, unsigned long long t0, unsigned long long now) {  // pickup delay, scan time
#ifdef FIT_STAMPS
            atomicAdd(&g_mw[c][10], t0 - ctl->pub[c]);
            atomicAdd(&g_mw[c][11], 1ull);
            atomicAdd(&g_mw[c][12], now - t0);
#endif
        });
}

size_t engine_lds_bytes(int32_t max_component_nodes) {
    const size_t scan = STAGE_OFF + sizeof(NodeRec) * STAGE_ROWS;
    return std::max(scan, mw_lds_bytes(max_component_nodes));
}

size_t engine_ctl_bytes() { return sizeof(EngineCtl); }
size_t engine_ctl_error_offset() { return offsetof(EngineCtl, error); }
size_t engine_ctl_trip_offset() { return offsetof(EngineCtl, trip); }
size_t engine_ring_bytes() { return sizeof(unsigned long long) * QRING * QGROUPS; }
size_t engine_ring_tasks() { return QCAP; }  // task slots per ring
int engine_ring_groups() { return (int)QGROUPS; }  // rings (components c % groups share one)

int engine_blocks_per_cu(size_t lds) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_engine, SCAN_WAVES * 64, lds) !=
        hipSuccess)
        return 0;
    return n;
}

hipError_t launch_engine(int blocks, size_t lds, hipStream_t st, void* ctl, void* ring,
                         const void* cs, void* co, CompPlan* plans, int ncomp, NodeRec* rec,
                         const int32_t* jl, const int32_t* jcpu, const int32_t* jmem,
                         const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                         const uint16_t* jk, uint64_t* cand, uint64_t* bnd, JobRec* wjob,
                         int32_t* out, int kmax, int64_t* wbusy, const int32_t* jpk, unsigned wd,
                         const int32_t* jmin, const EngineCompIds& ids) {
    hipLaunchKernelGGL(k_engine, dim3(blocks), dim3(SCAN_WAVES * 64), lds, st,
                       static_cast<EngineCtl*>(ctl), static_cast<unsigned long long*>(ring),
                       static_cast<const CompState*>(cs), static_cast<CompOut*>(co), plans, ncomp,
                       rec, jl, jcpu, jmem, jgpu, jwall, jpart, jk, cand, bnd, wjob, out, kmax,
                       wbusy, jpk, wd, jmin, ids);
    return hipGetLastError();
}

}  // namespace fitgpu

#ifdef FIT_TILE0_STAMPS
extern "C" int fit_debug_tile0(unsigned long long* out /* 8 */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fitgpu::g_tile0), sizeof(fitgpu::g_tile0)) == hipSuccess ? 0 : -2;
}
#endif
#ifdef MW_SEGSTAMP
// the decider's per-segment cycle sums over the launches so far and, in [8], its live jobs
extern "C" int fit_debug_mw_seg(unsigned long long* out /* 9 */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fitgpu::g_seg), sizeof(fitgpu::g_seg)) == hipSuccess ? 0 : -2;
}
#endif
#ifdef FIT_STAMPS
// the single-wave commit's segment stamps of this TU (multi-node windows; fit_common.h STAMP)
extern "C" int fit_debug_commit_stamps_pe(unsigned long long* out /* 64 x 8 */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fitgpu::g_stamps), sizeof(fitgpu::g_stamps)) ==
                   hipSuccess ? 0 : -2;
}
extern "C" int fit_debug_mw_stamps(unsigned long long* out /* 64 x 16 */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fitgpu::g_mw), sizeof(fitgpu::g_mw)) == hipSuccess
               ? 0 : -2;
}
#endif

// fit_wave.h — the lane-, wave- and LDS-level building blocks of the device code: workgroup-scope
// LDS hand-offs, LDS addresses and pointer laundering, global address-space views and loads, lane
// reads and writes, wave reductions and scans (DPP).  What belongs to one commit or engine stays in
// its own header; the agent-scope hand-offs are fit_engine_ctl.h's, which states their recipe.
#pragma once
#include <hip/hip_runtime.h>
#include "fit_device.h"

namespace fitgpu {

// ---- LDS hand-off primitives (workgroup scope, LDS only) ------------------------------------
__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); }
__device__ __forceinline__ void lds_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); }

// ---- global address-space views and loads ----------------------------------------------------
// global address-space views of the helper's buffers: a plain (generic) pointer in a non-inlined
// function compiles to flat loads, which also count in lgkmcnt — every LDS wait would then drain
// the prefetched job stream
#ifdef __HIP_DEVICE_COMPILE__
#define GAS __attribute__((address_space(1)))
#else  // (the host pass only parses device code)
#define GAS
#endif
template <class T>
__device__ __forceinline__ const GAS T* gview(const T* p) {
    return (const GAS T*)p;
}

typedef int32_t v4i32 __attribute__((ext_vector_type(4)));
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ NodeRec ld_node(const GAS NodeRec* p) {
    const GAS v4i32* q = (const GAS v4i32*)p;
    const v4i32 a = q[0], b = q[1];
    NodeRec r;
    r.cpu = a.x;
    r.mem = a.y;
    r.gpu = a.z;
    r.avail = a.w;
    r.mask = (uint32_t)b.x;
    r.orig = b.y;
    r.pad0 = b.z;
    r.pad1 = b.w;
    return r;
}
__device__ __forceinline__ JobRec ld_job(const GAS JobRec* p) {
    const GAS v4i32* q = (const GAS v4i32*)p;
    const v4i32 a = q[0], b = q[1];
    JobRec r;
    r.q = a.x;
    r.cpu = a.y;
    r.mem = a.z;
    r.gpu = a.w;
    r.wall = b.x;
    r.pbit = (uint32_t)b.y;
    r.k = b.z;
    r.pad = b.w;
    return r;
}

// Write-through reads of a scan tile's outputs (candidates, bound, job row), which the scan workers
// store through (sc1) and count with an agent-scope add: a helper that has seen the tile's count
// reach its target in a relaxed agent poll reads them with sc1 loads, which bypass this CU's L1,
// instead of an acquire fence (≈1.7 us, once per tile per helper, and on every round's start:
// cdna_hip_programming.md §6 Guideline 16; MI355X_MICROARCH.md hand-off table, row 1 — one block
// per CU, 8-B sc1 stores and loads, the polling wave loads after its poll matched).
__device__ __forceinline__ uint64_t ld_through(const GAS uint64_t* p) {
    return __hip_atomic_load(const_cast<GAS uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ JobRec ld_job_through(const GAS JobRec* p) {
    const GAS uint64_t* q = (const GAS uint64_t*)p;
    const uint64_t w0 = ld_through(q), w1 = ld_through(q + 1), w2 = ld_through(q + 2), w3 = ld_through(q + 3);
    JobRec r;
    r.q = (int32_t)(uint32_t)w0;
    r.cpu = (int32_t)(uint32_t)(w0 >> 32);
    r.mem = (int32_t)(uint32_t)w1;
    r.gpu = (int32_t)(uint32_t)(w1 >> 32);
    r.wall = (int32_t)(uint32_t)w2;
    r.pbit = (uint32_t)(w2 >> 32);
    r.k = (int32_t)(uint32_t)w3;
    r.pad = (int32_t)(uint32_t)(w3 >> 32);
    return r;
}

// a VGPR zero the compiler cannot see through: keeps uniform loads of data written by other
// workgroups in this launch on the vector path (vmcnt, in order) instead of the scalar cache
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

// A dynamic-LDS pointer the compiler cannot re-derive: in an out-of-line function the constant
// shared base is otherwise rematerialised from the dynlds offset table (an s_load + lgkmcnt(0)
// wait) on every loop iteration; laundered through an SGPR it is computed once.  The round trip
// through address space 3 keeps every access a ds_* instruction.
template <class T>
__device__ __forceinline__ T* lds_opaque(T* p) {
    uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) T*)p;
    asm volatile("" : "+s"(a));
    return (T*)(__attribute__((address_space(3))) T*)(uintptr_t)a;
}

// ---- LDS addresses (what a ds_* instruction takes) -------------------------------------------
// The 32-bit LDS address of an object in shared memory, two ways that compile differently
// (profiles/engine_frame_ab.txt): mw_lds_addr, an address-space cast, for new code; lds_addr, the
// generic pointer's low word, for the timeline commit (the cast gives tm_decider another allocation).
template <class T>
__device__ __forceinline__ uint32_t mw_lds_addr(T* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) T*)p;
}
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)p; }

// lds_opaque for an LDS address that depends on runtime values: made uniform first, so that it
// can live in an SGPR
template <class T>
__device__ __forceinline__ T* tm_lds(T* p) {
    typedef __attribute__((address_space(3))) T* Lds;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)mw_lds_addr(p));  // uniform
    return lds_opaque((T*)(Lds)(uintptr_t)a);
}

typedef __attribute__((address_space(3))) v4i32 lds_v4i32;
__device__ __forceinline__ void lds_st4(uint32_t a, v4i32 v) { *(lds_v4i32*)(uintptr_t)a = v; }
__device__ __forceinline__ int32_t lds_ld1(uint32_t a) {
    return *(const __attribute__((address_space(3))) int32_t*)(uintptr_t)a;
}
__device__ __forceinline__ const __attribute__((address_space(3))) v4u32* lds4(const void* p) {
    return (const __attribute__((address_space(3))) v4u32*)(uintptr_t)p;
}

// ---- lanes -------------------------------------------------------------------------------------
// a value / pointer made uniform (SGPRs): see plan_sgpr and tiles_sgpr (fit_commit_mw.h) for why
__device__ __forceinline__ int32_t rfl(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }
template <class Q>
__device__ __forceinline__ Q* rfl_ptr(Q* p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    return (Q*)(uintptr_t)(((uint64_t)(uint32_t)rfl((int32_t)(v >> 32)) << 32) |
                           (uint32_t)rfl((int32_t)(uint32_t)v));
}

// v_writelane_b32: lane `l` of `old` := SGPR `x` (no clang builtin on this toolchain)
__device__ __forceinline__ int32_t writelane(int32_t x, int l, int32_t old) {
    int32_t r;
    // the lane select goes through M0 (one SGPR operand per VALU instruction on gfx9)
    asm("v_writelane_b32 %0, %1, m0" : "=v"(r) : "s"(__builtin_amdgcn_readfirstlane(x)), "{m0}"(l), "0"(old));
    return r;
}
template <int L>
__device__ __forceinline__ int32_t writelane_c(int32_t x, int32_t old) {  // compile-time lane
    int32_t r;
    asm("v_writelane_b32 %0, %1, %2" : "=v"(r) : "s"(__builtin_amdgcn_readfirstlane(x)), "i"(L), "0"(old));
    return r;
}
__device__ __forceinline__ int32_t readlane(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t rdlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// the previous lane's value (lane 0: `first`) / the next lane's (lane 63: `last`): DPP wave shifts
__device__ __forceinline__ int32_t wave_shr1(int32_t v, int32_t first) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int32_t wave_shl1(int32_t v, int32_t last) {
    return __builtin_amdgcn_update_dpp(last, v, 0x130, 0xf, 0xf, false);
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a < b ? b : a; }

// ---- wave-wide reductions, builtin form (DPP; call with a full EXEC mask) ----------------------
// dpp_min and the fused dpp_min32 below do the same step with different code: the builtin is a DPP
// move plus the ALU op, scheduled freely; the fused form is one instruction in an asm volatile.  Use
// the fused one in new code; the host-driven rounds and the single-wave commit are tuned on this one.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp_min(uint32_t v) {
    return min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffff, (int)v, CTRL, ROWMASK,
                                                        0xf, false));
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = dpp_min<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
    v = dpp_min<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
    v = dpp_min<0x124, 0xf>(v);  // row_ror:4
    v = dpp_min<0x128, 0xf>(v);  // row_ror:8
    v = dpp_min<0x142, 0xa>(v);  // row_bcast:15
    v = dpp_min<0x143, 0xc>(v);  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// min over the wave of a packed (score << 32 | position) key: 32-bit min of the scores, then of
// the positions among the lanes holding that score (usually one lane: a readlane).
__device__ __forceinline__ uint64_t wave_min_key(uint64_t v) {
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t mh = wave_min_u32(hi);
    const uint64_t eq = __ballot(hi == mh);
    uint32_t ml;
    if (__popcll(eq) == 1)
        ml = (uint32_t)__builtin_amdgcn_readlane((int)lo, __builtin_ctzll(eq));
    else
        ml = wave_min_u32(hi == mh ? lo : 0xffffffffu);
    return ((uint64_t)mh << 32) | ml;
}

// wave_min_key plus the lane holding the minimum (the lowest such lane)
__device__ __forceinline__ uint64_t wave_min_key_lane(uint64_t v, int& lane) {
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t mh = wave_min_u32(hi);
    const uint64_t eq = __ballot(hi == mh);
    uint32_t ml;
    if (__popcll(eq) == 1) {
        lane = __builtin_ctzll(eq);
        ml = (uint32_t)__builtin_amdgcn_readlane((int)lo, lane);
    } else {
        ml = wave_min_u32(hi == mh ? lo : 0xffffffffu);
        lane = __builtin_ctzll(__ballot(hi == mh && lo == ml));
    }
    return ((uint64_t)mh << 32) | ml;
}

// ---- DPP building blocks ---------------------------------------------------------------------
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    if constexpr (ROWMASK == 0xf)  // every lane has a source: a plain DPP move
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
    else  // lanes of rows outside the mask keep their value
        return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWMASK, 0xf, false);
}
// one 64-bit min step against the DPP-permuted value (2 moves, a 64-bit compare, 2 selects)
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ uint64_t dpp_min64(uint64_t v) {
    const uint32_t lo = dpp32<CTRL, ROWMASK>((uint32_t)v), hi = dpp32<CTRL, ROWMASK>((uint32_t)(v >> 32));
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    return o < v ? o : v;
}
// minimum over each group of 8 lanes, in all 8 of them: quad swaps, then the half-row mirror
__device__ __forceinline__ uint64_t min8_64(uint64_t v) {
    v = dpp_min64<0xb1>(v);   // quad_perm [1,0,3,2]
    v = dpp_min64<0x4e>(v);   // quad_perm [2,3,0,1]
    return dpp_min64<0x141>(v);  // row_half_mirror
}
// Fused DPP ALU ops in inline asm (hipcc emits a DPP move plus the ALU op for the builtins).
// Each string opens with the two wait states a DPP read of a VGPR written by the previous VALU
// instruction needs (cdna_hip_programming.md: DPP hazard; `s_nop 1`).
#define MW_DPP_MIN(v, CTL) asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 " CTL : "+v"(v))
__device__ __forceinline__ uint32_t dppmin_qp1032(uint32_t v) { MW_DPP_MIN(v, "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"); return v; }
__device__ __forceinline__ uint32_t dppmin_qp2301(uint32_t v) { MW_DPP_MIN(v, "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"); return v; }
__device__ __forceinline__ uint32_t dppmin_hmirror(uint32_t v) { MW_DPP_MIN(v, "row_half_mirror row_mask:0xf bank_mask:0xf"); return v; }
__device__ __forceinline__ uint32_t dppmin_mirror(uint32_t v) { MW_DPP_MIN(v, "row_mirror row_mask:0xf bank_mask:0xf"); return v; }
__device__ __forceinline__ uint32_t dppmin_bcast15(uint32_t v) { MW_DPP_MIN(v, "row_bcast:15 row_mask:0xa bank_mask:0xf"); return v; }
__device__ __forceinline__ uint32_t dppmin_bcast31(uint32_t v) { MW_DPP_MIN(v, "row_bcast:31 row_mask:0xc bank_mask:0xf"); return v; }
#undef MW_DPP_MIN
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ uint32_t dpp_min32(uint32_t v) {
    if constexpr (CTRL == 0xb1) return dppmin_qp1032(v);
    else if constexpr (CTRL == 0x4e) return dppmin_qp2301(v);
    else if constexpr (CTRL == 0x141) return dppmin_hmirror(v);
    else if constexpr (CTRL == 0x140) return dppmin_mirror(v);
    else if constexpr (CTRL == 0x142) return dppmin_bcast15(v);
    else return dppmin_bcast31(v);
}
// d = src ^ (x rotated by K within its row of 16 lanes); NOP: src of the DPP just written
template <int K, bool NOP>
__device__ __forceinline__ uint32_t dpp_ror_xor(uint32_t x, uint32_t y) {
    uint32_t d;
    if constexpr (NOP)
        asm volatile("s_nop 1\n\tv_xor_b32_dpp %0, %1, %2 row_ror:%3 row_mask:0xf bank_mask:0xf"
                     : "=v"(d) : "v"(x), "v"(y), "i"(K));
    else
        asm volatile("v_xor_b32_dpp %0, %1, %2 row_ror:%3 row_mask:0xf bank_mask:0xf"
                     : "=v"(d) : "v"(x), "v"(y), "i"(K));
    return d;
}
// 64-bit minimum over each group of 8 lanes, in all 8: the 32-bit minimum of the high words,
// then of the low words among the lanes holding it (fused DPP mins, no 64-bit compares)
__device__ __forceinline__ uint64_t min8_2pass(uint64_t v) {
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    uint32_t mh = dpp_min32<0xb1>(hi);
    mh = dpp_min32<0x4e>(mh);
    mh = dpp_min32<0x141>(mh);
    uint32_t ml = hi == mh ? lo : 0xffffffffu;
    ml = dpp_min32<0xb1>(ml);
    ml = dpp_min32<0x4e>(ml);
    ml = dpp_min32<0x141>(ml);
    return ((uint64_t)mh << 32) | ml;
}
// 32-bit minimum over the wave, valid in lane 63
__device__ __forceinline__ uint32_t wave_min32_l63(uint32_t v) {
    v = dpp_min32<0xb1>(v);
    v = dpp_min32<0x4e>(v);
    v = dpp_min32<0x141>(v);
    v = dpp_min32<0x140>(v);
    v = dpp_min32<0x142, 0xa>(v);
    return dpp_min32<0x143, 0xc>(v);
}
// minimum over the wave, valid in lane 63
__device__ __forceinline__ uint64_t wave_min64_l63(uint64_t v) {
    v = dpp_min64<0xb1>(v);
    v = dpp_min64<0x4e>(v);
    v = dpp_min64<0x141>(v);       // row_half_mirror: 8-lane groups
    v = dpp_min64<0x140>(v);       // row_mirror: whole rows of 16
    v = dpp_min64<0x142, 0xa>(v);  // row_bcast:15 → rows 1 and 3
    return dpp_min64<0x143, 0xc>(v);  // row_bcast:31 → rows 2 and 3
}
// 32-bit minimum over the wave, in every lane: four fused DPP minima, then the permlane16 / 32
// swaps of gfx950 — no readlane, no branch, so no VALU -> SGPR -> SALU hand-off on the caller's chain
__device__ __forceinline__ uint32_t wave_min32_all(uint32_t v) {
    v = dpp_min32<0xb1>(v);
    v = dpp_min32<0x4e>(v);
    v = dpp_min32<0x141>(v);
    v = dpp_min32<0x140>(v);  // every lane: its row's minimum
    {
        const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        v = min((uint32_t)p[0], (uint32_t)p[1]);
    }
    const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return min((uint32_t)p[0], (uint32_t)p[1]);
}

// Three independent inclusive min-scans (a run list's cpu / mem / gpu columns), interleaved so
// that each fused v_min_i32_dpp reads a VGPR written two instructions earlier (the DPP hazard's
// two wait states, cdna_hip_programming.md) — 18 VALU and one s_nop.  A lane whose DPP source does
// not exist (row_shr at a row's start) or whose row the row_mask leaves out keeps its value
// (bound_ctrl not set), i.e. min(v, TL_BIG) = v.
__device__ __forceinline__ void wave_scan_min3(int32_t& a, int32_t& b, int32_t& c) {
#define TL_L3(CTL) "v_min_i32_dpp %0, %0, %0 " CTL "\n\tv_min_i32_dpp %1, %1, %1 " CTL \
                   "\n\tv_min_i32_dpp %2, %2, %2 " CTL "\n\t"
    asm volatile("s_nop 1\n\t"
                 TL_L3("row_shr:1 row_mask:0xf bank_mask:0xf")
                 TL_L3("row_shr:2 row_mask:0xf bank_mask:0xf")
                 TL_L3("row_shr:4 row_mask:0xf bank_mask:0xf")
                 TL_L3("row_shr:8 row_mask:0xf bank_mask:0xf")
                 TL_L3("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 TL_L3("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 : "+v"(a), "+v"(b), "+v"(c));
#undef TL_L3
}

}  // namespace fitgpu

// fit_pre_top.h — what fit_preempt_k's and fit_preempt_tl_k's kernels share (DESIGN.md §2m / §2o,
// §3.21 / §3.23): the row as the kernels see it, the order of two keys, the sorted list of the K
// smallest keys a lane has been offered, and the fold that ends a `_k` walk — the counters through
// LDS, the eight waves' lists merged pairwise, one list of kmax keys per (job position, node slice).
// __forceinline__: a kernel built from these compiles to what it was when it spelled them out.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fit_device.h"
#include "fit_pre_row.h"

namespace fitgpu {

// fit_evict_k as the kernels see it (include/fitgpu.h)
struct alignas(8) EvictKRow {
    int32_t code, need, evict_nodes, victims, top_prio, cnt[PRE_NCNT], reserved;
};
static_assert(sizeof(EvictKRow) == 40 && offsetof(EvictKRow, cnt) == 20, "fit_evict_k is 40 bytes, its counters at 20");

__device__ __forceinline__ bool prek_less(uint64_t ahi, uint64_t alo, uint64_t bhi, uint64_t blo) {
    return ahi < bhi || (ahi == bhi && alo < blo);
}
// a <= b afterwards
__device__ __forceinline__ void prek_cx(PreKey& a, PreKey& b) {
    const bool sw = prek_less(b.hi, b.lo, a.hi, a.lo);
    const PreKey lo = {sw ? b.hi : a.hi, sw ? b.lo : a.lo}, hi = {sw ? a.hi : b.hi, sw ? a.lo : b.lo};
    a = lo;
    b = hi;
}

// The K smallest keys a lane has been offered, ascending; PRE_NOKEY fills the rest.  Every index is
// a constant after unrolling: the list lives in registers.
template <int K>
struct PreTop {
    static_assert(K == 1 || K == 2 || K == 4 || K == 8, "a power of two up to FIT_KMAX");
    PreKey k[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < K; ++i) k[i] = {PRE_NOKEY, PRE_NOKEY};
    }
    // pre_row's sink.  Wave-uniform gate: the chain runs only when some lane's key enters its list.
    __device__ __forceinline__ void offer(bool has, uint64_t hi, uint64_t lo) {
        const bool in = has && prek_less(hi, lo, k[K - 1].hi, k[K - 1].lo);
        if (__ballot(in) == 0ull) return;
        PreKey x = {in ? hi : PRE_NOKEY, in ? lo : PRE_NOKEY};
#pragma unroll
        for (int i = 0; i < K; ++i) prek_cx(k[i], x);  // x carries the larger one down; the last falls out
    }
    // The K smallest of this list and the sorted list b: min(k[i], b[K - 1 - i]) holds them as a
    // bitonic sequence, log2(K) half-cleaner stages sort it.
    __device__ __forceinline__ void merge(const PreKey (&b)[K]) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const bool lt = prek_less(b[K - 1 - i].hi, b[K - 1 - i].lo, k[i].hi, k[i].lo);
            k[i].hi = lt ? b[K - 1 - i].hi : k[i].hi;
            k[i].lo = lt ? b[K - 1 - i].lo : k[i].lo;
        }
#pragma unroll
        for (int d = K / 2; d >= 1; d /= 2)
#pragma unroll
            for (int i = 0; i < K; ++i)
                if ((i & d) == 0) prek_cx(k[i], k[i + d]);
    }
};

// The fold's LDS buffer in 8-byte words: four waves' lists, [wave][key][hi, lo][lane]; before that the
// eight waves' counters
template <int K>
constexpr int prek_fold_words() {
    constexpr int KEY_WORDS = (PRE_WAVES / 2) * K * 2 * PRE_JOBS;
    constexpr int CNT_WORDS = PRE_WAVES * PRE_NCNT * PRE_JOBS / 2;
    return KEY_WORDS > CNT_WORDS ? KEY_WORDS : CNT_WORDS;
}

// The end of a `_k` walk, called by the whole workgroup of PRE_WAVES waves: lane `lane` of wave `wave`
// holds job q's counters n and list top over the wave's share of the nodes (on: q is a job of a
// component).  sm: prek_fold_words<K>() words of LDS, qs: PRE_JOBS.  The tile starts at position tb
// of the chunk [t0, t0 + nt); part: nt * gridDim.y lists of kmax keys, position-major.  It is
// k_prek_walk's fold word for word; that kernel keeps its own text, because calling this function
// instead changed its listing.
template <int K>
__device__ __forceinline__ void prek_fold(uint64_t* sm, int32_t* qs, int wave, int lane, bool on, int q,
                                          const int32_t (&n)[PRE_NCNT], PreTop<K>& top, int tb, int32_t t0,
                                          int32_t nt, int32_t kmax, EvictKRow* out,
                                          PreKey* part) {
    // the counters: thread (i, l) sums counter i of job-lane l over the waves, one atomic per
    // workgroup, job and counter, none for a zero
    int32_t* red = reinterpret_cast<int32_t*>(sm);  // [wave][counter][lane]
#pragma unroll
    for (int i = 0; i < PRE_NCNT; ++i) red[(wave * PRE_NCNT + i) * PRE_JOBS + lane] = n[i];
    if (wave == 0) qs[lane] = on ? q : -1;
    __syncthreads();
    if (threadIdx.x < PRE_NCNT * PRE_JOBS) {
        const int i = threadIdx.x / PRE_JOBS, l = threadIdx.x - i * PRE_JOBS;
        int32_t v = 0;
#pragma unroll
        for (int w = 0; w < PRE_WAVES; ++w) v += red[(w * PRE_NCNT + i) * PRE_JOBS + l];
        const int jq = qs[l];
        if (jq >= 0 && v != 0) atomicAdd(&out[jq].cnt[i], v);
    }
    // the lists: waves [h, 2h) hand theirs to waves [0, h), h = 4, 2, 1
#pragma unroll
    for (int h = PRE_WAVES / 2; h >= 1; h /= 2) {
        __syncthreads();  // the buffer's readers of the round before (the counters' the first time) are done
        if (wave >= h && wave < 2 * h) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                sm[(((wave - h) * K + i) * 2 + 0) * PRE_JOBS + lane] = top.k[i].hi;
                sm[(((wave - h) * K + i) * 2 + 1) * PRE_JOBS + lane] = top.k[i].lo;
            }
        }
        __syncthreads();
        if (wave < h) {
            PreKey b[K];
#pragma unroll
            for (int i = 0; i < K; ++i)
                b[i] = {sm[((wave * K + i) * 2 + 0) * PRE_JOBS + lane], sm[((wave * K + i) * 2 + 1) * PRE_JOBS + lane]};
            top.merge(b);
        }
    }
    // this slice's list: every position of the tile inside the chunk, live or not, so none is left
    // unwritten
    const int t = tb - t0 + lane;
    if (wave == 0 && t < nt) {
        PreKey* dst = part + ((size_t)t * gridDim.y + blockIdx.y) * kmax;
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (i < kmax) dst[i] = top.k[i];
    }
}

}  // namespace fitgpu

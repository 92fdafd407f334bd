// fit_evicted_tl.hip — the caller reports which entries of which nodes' victim lists it has evicted:
// each entry's amounts go back to the slots [0, e') of its node, e' = max(end - shift, 0), and the
// entry leaves its list (include/fitgpu.h fit_evicted_tl).  gfx950.
//
// Ordinary bounded launches on the context's stream, inside the timeline writers' check / verdict /
// write frame (engine.cpp tl_write_impl).  Node id -> position is fit_unplace_tl's k_utl_inverse.
//   k_etl_check : one thread per row of a chunk: the node id, the position against the CURRENT length
//                 of that node's list (a node in no partition has no list: length 0), then an atomic
//                 exchange on the entry's mark word (VicTl::pad[0]): an entry already marked is a
//                 duplicate.  A good row counts for its node; the thread that takes a node's count
//                 from 0 appends the node to the touched list, as k_utl_count does.  Every chunk's
//                 check runs before the host reads the flag, so the marks of the WHOLE call are set
//                 before any list is compacted: every position refers to the lists as they were.
//   k_etl_clear : the failure path: one thread per row takes the mark of every row that could have
//                 set one back to 0.  Marks are scratch: they are 0 outside a call.
//   k_etl_apply : ONE wave (a 64-thread workgroup) per touched node, so no two waves ever edit one run
//                 list or one victim list: the dense edit of fit_tl_dense.h.  The list goes by 64
//                 entries per step: a marked entry's window [0, e') runs over the three columns with
//                 §2h's saturating add, the unmarked entries are compacted in place (ballot +
//                 lanes-below prefix).  A store goes to an index at or below the block just loaded and
//                 one wave does both, in program order: safe step by step.  Then the canonical run
//                 list, the header, the raised ceilings and the list's new length.
// Every window starts at slot 0, so slot s is always lane s % 64's: the windows need no barrier
// between them.  One launch sequence is bounded whatever m is: the checks are chunked by UTL_CHUNK
// rows, and the apply's work per wave is its node's list and H slots, not the rows.
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; integer
// atomics and disjoint stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_dense.h"

namespace fitgpu {

static_assert(sizeof(VicTl) == 32 && sizeof(VicSpan) == 8, "an entry is two 16-byte loads, a span one 8-byte load");

// The entry row q names, or nullptr: node id in [0, n), a position, 0 <= pos < the list's length.
__device__ __forceinline__ VicTl* etl_entry(const int32_t* __restrict__ node, const int32_t* __restrict__ pos, int q,
                                            int32_t n, const int32_t* __restrict__ inv,
                                            const VicSpan* __restrict__ vspan, VicTl* vent, int32_t* x) {
    const int32_t id = node[q], p = pos[q];
    *x = id >= 0 && id < n ? inv[id] : -1;
    if (*x < 0) return nullptr;  // outside the table, or in no partition: no list
    const VicSpan sp = vspan[*x];
    return p >= 0 && p < sp.len ? vent + sp.beg + p : nullptr;
}

// Rows [t0, t0 + nj).  g[0]: touched nodes so far, g[2]: the bad-input flag (fit_device.h's words).
__global__ __launch_bounds__(256) void k_etl_check(const int32_t* __restrict__ node, const int32_t* __restrict__ pos,
                                                   int32_t t0, int32_t nj, int32_t n,
                                                   const int32_t* __restrict__ inv,
                                                   const VicSpan* __restrict__ vspan, VicTl* vent,
                                                   int32_t* __restrict__ cnt, int32_t* __restrict__ touched,
                                                   int32_t cap, int32_t* __restrict__ g) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    int32_t x;
    VicTl* e = etl_entry(node, pos, t0 + t, n, inv, vspan, vent, &x);
    if (!e || atomicExch(&e->pad[0], 1) != 0) {  // out of range, or the same (node, pos) pair twice
        atomicOr(&g[2], 1);
        return;
    }
    if (atomicAdd(&cnt[x], 1) == 0) {
        const int32_t k = atomicAdd(&g[0], 1);
        if (k < cap) touched[k] = x;  // cap >= the distinct nodes the rows can name: always true
    }
}

__global__ __launch_bounds__(256) void k_etl_clear(const int32_t* __restrict__ node, const int32_t* __restrict__ pos,
                                                   int32_t nj, int32_t n, const int32_t* __restrict__ inv,
                                                   const VicSpan* __restrict__ vspan, VicTl* vent) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    int32_t x;
    VicTl* e = etl_entry(node, pos, t, n, inv, vspan, vent, &x);
    if (e) e->pad[0] = 0;  // rows of one pair store the same 0
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 3 columns of H words.
__global__ __launch_bounds__(64) void k_etl_apply(TlHdr* hdr, Seg* slab, int32_t H, int32_t shift,
                                                  const int32_t* __restrict__ touched, int32_t cap, VicSpan* vspan,
                                                  VicTl* vent, const int32_t* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) int32_t etl_dense[];
    const int b = blockIdx.x;
    if (b >= min(g[0], cap)) return;
    const int lane = threadIdx.x;
    const int32_t pos = touched[b];
    int32_t* dc = etl_dense;
    int32_t* dm = dc + H;
    int32_t* dg = dm + H;
    TlHdr* hp = hdr + pos;
    Seg* sg = slab + (int64_t)pos * TL_MAX_SLOTS;
    tl_dense_expand<false>(sg, min(hp->cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    __syncthreads();
    const VicSpan sp = vspan[pos];
    VicTl* ve = vent + sp.beg;
    int keep_n = 0;  // entries kept so far: the compacted list's length
    for (int i0 = 0; i0 < sp.len; i0 += 64) {
        const bool have = i0 + lane < sp.len;
        const VicTl mine = have ? ve[i0 + lane] : VicTl{0, 0, 0, 0, 0, {0, 0, 0}};
        const bool gone = have && mine.pad[0] != 0;
        const int32_t ee = min(max(mine.end - shift, 0), H);  // e', inside the horizon
        uint64_t todo = __ballot(gone && ee > 0);             // an entry with e' = 0 adds nothing
        while (todo) {                                        // wave-uniform
            const int k = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int32_t we = __shfl(ee, k);
            const int32_t jc = __shfl(mine.cpu, k), jm = __shfl(mine.mem, k), jg = __shfl(mine.gpu, k);
            for (int s = lane; s < we; s += 64) {  // slot s is this lane's in every window: no barrier
                dc[s] = utl_add(dc[s], jc);
                dm[s] = utl_add(dm[s], jm);
                dg[s] = utl_add(dg[s], jg);
            }
        }
        const bool keep = have && !gone;
        const uint64_t mk = __ballot(keep);
        if (keep) ve[keep_n + lanes_below(mk)] = mine;  // keep_n + ... <= i0 + lane; its mark is 0
        keep_n += __popcll(mk);
    }
    __syncthreads();
    const TlDenseOut o = tl_dense_write(sg, H, lane, dc, dm, dg);
    tl_refresh_head(hp, sg, o.no, H, lane);
    if (lane == 0) {
        hp->cpu = max(hp->cpu, o.xc);  // values rose: the ceilings rise with them
        hp->mem = max(hp->mem, o.xm);
        hp->gpu = max(hp->gpu, o.xg);
        vspan[pos].len = keep_n;
    }
}

hipError_t launch_etl_check(hipStream_t st, const int32_t* node, const int32_t* pos, int32_t t0, int32_t nj, int32_t n,
                            const int32_t* inv, const VicSpan* vspan, VicTl* vent, int32_t* cnt, int32_t* touched,
                            int32_t cap, int32_t* g) {
    if (nj <= 0) return hipSuccess;
    if (nj > UTL_CHUNK || t0 < 0 || cap < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_etl_check, dim3((nj + 255) / 256), dim3(256), 0, st, node, pos, t0, nj, n, inv, vspan, vent,
                       cnt, touched, cap, g);
    return hipGetLastError();
}

hipError_t launch_etl_clear(hipStream_t st, const int32_t* node, const int32_t* pos, int32_t nj, int32_t n,
                            const int32_t* inv, const VicSpan* vspan, VicTl* vent) {
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_etl_clear, dim3((nj + 255) / 256), dim3(256), 0, st, node, pos, nj, n, inv, vspan, vent);
    return hipGetLastError();
}

hipError_t launch_etl_apply(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t H, int32_t shift, const int32_t* touched,
                            int32_t cap, VicSpan* vspan, VicTl* vent, const int32_t* g) {
    if (cap <= 0) return hipSuccess;
    if (H < 1 || H > TL_MAX_SLOTS || shift < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_etl_apply, dim3(cap), dim3(64), sizeof(int32_t) * 3 * (size_t)H, st, hdr, slab, H, shift,
                       touched, cap, vspan, vent, g);
    return hipGetLastError();
}

}  // namespace fitgpu

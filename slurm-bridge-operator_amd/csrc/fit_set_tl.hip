// fit_set_tl.hip — overwrite windows of the loaded timeline with a level per column: row q sets the
// slots [from, min(to, H)) of its node to (cpu, mem, gpu), -1 closing a column; where rows overlap,
// the row with the largest index stands (include/fitgpu.h fit_set_tl).  gfx950.
//
// Ordinary bounded launches on the context's stream, inside the timeline writers' check / verdict /
// write frame (engine.cpp tl_write_impl).  Node id -> position is fit_unplace_tl's k_utl_inverse, the
// count of a chunk's windows per node and their ranges its k_utl_count and k_utl_offsets
// (launch_utl_ranges: a row is a one-node row whose start is `from`); the counter words g are
// fit_device.h's, g[3] taken for the ignored rows.
//   k_stl_check   : one thread per row of the WHOLE batch: the §2q tests of a live row, the bad-input
//                   flag, the rows of the row's chunk whose node has a run list (its windows) and the
//                   live rows whose node has none (ignored), each summed per wave before its atomic.
//                   Nothing is written to the timeline before the host has seen the flag.
//   rows [t0, t0 + nj) — a chunk of at most UTL_CHUNK rows:
//   k_stl_scatter : one thread per row: its window with its row index into its node's range (order
//                   inside a node is free: k_stl_apply orders by row index)
//   k_stl_apply   : ONE wave (a 64-thread workgroup) per touched node, so no two waves ever edit one
//                   list: the dense edit of fit_tl_dense.h over FOUR columns, the fourth holding the
//                   index of the row that last wrote each slot (-1 at the start of the launch).  A
//                   window writes a slot only when its row is larger than the stored one, so the
//                   result is that of the rows in index order whatever order the scatter left.  Chunks
//                   run in stream order and a later chunk holds larger indices only: it always wins.
//                   Then the canonical run list, the header and the EXACT ceilings (values fall as
//                   well as rise).
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog; integer
// atomics and disjoint stores only.  The kernel end orders one launch against the next.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_device.h"
#include "fit_tl_dense.h"

namespace fitgpu {

// g[2], g[3] and g[4 + q / chunk]: one atomic per wave and word, as k_utl_check does (DESIGN.md §3.16
// records what one atomic per row cost).  inv: k_utl_inverse's table, complete before this launch.
__global__ __launch_bounds__(256) void k_stl_check(const int32_t* __restrict__ node, const int32_t* __restrict__ from,
                                                   const int32_t* __restrict__ to, const int32_t* __restrict__ cpu,
                                                   const int32_t* __restrict__ mem, const int32_t* __restrict__ gpu,
                                                   int32_t m, int32_t n, int32_t H, int32_t chunk,
                                                   const int32_t* __restrict__ inv, int32_t* __restrict__ g) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t f = q < m ? from[q] : -1;  // a row with from < 0 is skipped whatever else it holds
    int32_t need = 0, ign = 0, bad = 0;      // a window of the row's chunk / a live row without a list
    if (f >= 0) {
        const int32_t id = node[q];
        bad = id < 0 || id >= n || f >= H || to[q] <= f || cpu[q] < -1 || mem[q] < -1 || gpu[q] < -1;
        if (!bad) {
            need = inv[id] >= 0;
            ign = !need;
        }
    }
    // every lane of the wave is here
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&g[2], 1);
    const int32_t igs = __popcll(__ballot(ign));
    if (igs && lane == 0) atomicAdd(&g[3], igs);
    const int32_t ci = q < m ? q / chunk : -1;
    uint64_t todo = __ballot(need > 0);
    while (todo) {  // per chunk index among the wave's windows, one sum and one add
        const int lead = __builtin_ctzll(todo);
        const int32_t lci = __shfl(ci, lead);
        const uint64_t mine = __ballot(need > 0 && ci == lci);
        if (lane == lead) atomicAdd(&g[4 + lci], (int32_t)__popcll(mine));
        todo &= ~mine;
    }
}

// Rows [t0, t0 + nj) of a batch that k_stl_check passed; fill[pos]: the node's scatter cursor.
__global__ __launch_bounds__(256) void k_stl_scatter(const int32_t* __restrict__ node, const int32_t* __restrict__ from,
                                                     const int32_t* __restrict__ to, const int32_t* __restrict__ cpu,
                                                     const int32_t* __restrict__ mem, const int32_t* __restrict__ gpu,
                                                     int32_t t0, int32_t nj, int32_t H, int32_t n,
                                                     const int32_t* __restrict__ inv, int32_t* __restrict__ fill,
                                                     TlWin* __restrict__ win, int32_t wcap) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nj) return;
    const int q = t0 + t;
    const int32_t s = from[q];
    if (s < 0) return;
    const int32_t id = node[q];
    const int32_t pos = id >= 0 && id < n ? inv[id] : -1;  // in range: k_stl_check passed the batch
    if (pos < 0) return;                                   // a node in no partition: ignored
    const int32_t k = atomicAdd(&fill[pos], 1);
    if (k >= 0 && k < wcap) win[k] = TlWin{s, min(to[q], H), cpu[q], mem[q], gpu[q], q, {0, 0}};
}

// grid = an upper bound of the touched nodes; workgroup = one wave.  LDS: 4 columns of H words.
__global__ __launch_bounds__(64) void k_stl_apply(TlHdr* hdr, Seg* slab, int32_t H, const int32_t* __restrict__ touched,
                                                  int32_t cap, int32_t* cnt, const int32_t* __restrict__ first,
                                                  const TlWin* __restrict__ win, int32_t wcap,
                                                  const int32_t* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) int32_t stl_dense[];
    const int b = blockIdx.x;
    if (b >= min(g[0], cap)) return;
    const int lane = threadIdx.x;
    const int32_t pos = touched[b];
    int32_t* dc = stl_dense;
    int32_t* dm = dc + H;
    int32_t* dg = dm + H;
    int32_t* dr = dg + H;  // the row that last wrote the slot
    TlHdr* hp = hdr + pos;
    Seg* sg = slab + (int64_t)pos * TL_MAX_SLOTS;
    tl_dense_expand<false>(sg, min(hp->cnt, TL_MAX_SLOTS), H, lane, dc, dm, dg);
    for (int s = lane; s < H; s += 64) dr[s] = -1;
    __syncthreads();
    tl_dense_windows_slots(win, first[pos], cnt[pos], wcap, H, lane,
                           [&](int s, int32_t jc, int32_t jm, int32_t jg, int32_t row) {
                               if (row > dr[s]) {  // the largest index stands
                                   dc[s] = jc;
                                   dm[s] = jm;
                                   dg[s] = jg;
                                   dr[s] = row;
                               }
                           });
    __syncthreads();
    const TlDenseOut o = tl_dense_write(sg, H, lane, dc, dm, dg);
    tl_refresh_head(hp, sg, o.no, H, lane);
    if (lane == 0) {
        hp->cpu = o.xc;  // values fall as well as rise: the ceilings are the exact maxima, as after a load
        hp->mem = o.xm;
        hp->gpu = o.xg;
        cnt[pos] = 0;  // the next chunk counts from zero
    }
}

hipError_t launch_stl_check(hipStream_t st, const int32_t* node, const int32_t* from, const int32_t* to,
                            const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int32_t m, int32_t n, int32_t H,
                            int32_t chunk, const int32_t* inv, int32_t* g) {
    if (m <= 0) return hipSuccess;
    if (chunk < 1 || chunk > UTL_CHUNK || H < 1 || H > TL_MAX_SLOTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stl_check, dim3((m + 255) / 256), dim3(256), 0, st, node, from, to, cpu, mem, gpu, m, n, H,
                       chunk, inv, g);
    return hipGetLastError();
}

// Rows [t0, t0 + nj) with `windows` windows between them (k_stl_check's count of the chunk), on
// stream st.  cnt[nn] is zero before and after; g[0] and g[1] are reset here.
hipError_t launch_stl_chunk(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, const int32_t* node,
                            const int32_t* from, const int32_t* to, const int32_t* cpu, const int32_t* mem,
                            const int32_t* gpu, int32_t t0, int32_t nj, int32_t windows, int32_t n, const int32_t* inv,
                            int32_t* cnt, int32_t* first, int32_t* fill, int32_t* touched, TlWin* win, int32_t* g) {
    if (nj <= 0 || windows <= 0 || nn <= 0) return hipSuccess;
    if (nj > UTL_CHUNK || windows > nj || H < 1 || H > TL_MAX_SLOTS) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(g, 0, 2 * sizeof(int32_t), st);
    if (e == hipSuccess)
        e = launch_utl_ranges(st, nn, nullptr, 1, node, from, t0, nj, windows, n, inv, cnt, first, fill, touched,
                              nullptr, g);
    if (e != hipSuccess) return e;
    const int32_t cap = std::min(windows, nn);  // distinct nodes the rows can touch
    hipLaunchKernelGGL(k_stl_scatter, dim3((nj + 255) / 256), dim3(256), 0, st, node, from, to, cpu, mem, gpu, t0, nj,
                       H, n, inv, fill, win, windows);
    hipLaunchKernelGGL(k_stl_apply, dim3(cap), dim3(64), sizeof(int32_t) * 4 * (size_t)H, st, hdr, slab, H, touched,
                       cap, cnt, first, win, windows, g);
    return hipGetLastError();
}

}  // namespace fitgpu

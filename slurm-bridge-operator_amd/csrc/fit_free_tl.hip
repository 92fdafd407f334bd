// fit_free_tl.hip — per-partition free capacity at every timeline slot: for each partition p and
// slot t, over the member nodes that are open at t, the exact sums of the three columns, the node
// count and the column maxima (include/fitgpu.h fit_free_tl).  Read-only: the
// run lists and their headers are only loaded.  gfx950.
//
// Three ordinary bounded launches on the context's stream:
//   k_free_init : the accumulator planes, one thread per (partition, slot): sums and count 0, maxima -1.
//   k_free_walk : grid (chunk of node positions, partition), 256 threads.  A workgroup leaves at once
//                 when no header of its chunk has bit p (positions are grouped by component, so on
//                 disjoint partitions the work is about one pass over the lists).  Thread `tid` owns
//                 the slots tid + 256 i and keeps their seven accumulators in registers over the
//                 whole chunk.  The node loop is wave-uniform: the 96-B TlHdr comes in with scalar
//                 loads, and a list of at most TL_HEAD runs is walked from the header alone — a closed
//                 run costs one scalar test, so a node that is closed everywhere costs its header.
//                 A longer list is not walked run by run (1,024 runs x 4 slots per thread): every
//                 thread finds the run of each of its slots by binary search in the slab row, at
//                 most 10 loads per slot whatever the list's length.
//                 The partials meet in the planes through integer atomics, zeros skipped.  The planes
//                 are one array per field, [partition][slot], so the 64 lanes of a wave add to 64
//                 consecutive words.  Integer add and max do not depend on the order: exact and
//                 reproducible rows.
//   k_free_pack : the planes into the caller's 40-byte rows, one thread per row.
// Nothing waits for another workgroup: no persistent grid, no launch lock, no watchdog.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "fit_device.h"

namespace fitgpu {

constexpr int FREE_THREADS = 256;
constexpr int FREE_MAXS = TL_MAX_SLOTS / FREE_THREADS;  // slots a thread owns, at most
static_assert(FREE_MAXS * FREE_THREADS == TL_MAX_SLOTS, "a thread owns whole strides of the horizon");

// fit_free as include/fitgpu.h declares it
struct alignas(8) FreeRow {
    int64_t cpu, mem, gpu;
    int32_t nodes, max_cpu, max_mem, max_gpu;
};
static_assert(sizeof(FreeRow) == FREE_ROW_BYTES && offsetof(FreeRow, nodes) == 24, "fit_free is 40 bytes");

// The accumulators of one owned slot
struct FreeAcc {
    int64_t c, m, g;
    int32_t n, xc, xm, xg;
};

// One open cell (node, slot) with values c, m, g >= 0, if `in`
__device__ __forceinline__ void free_cell(FreeAcc& A, bool in, int32_t c, int32_t m, int32_t g) {
    A.c += in ? c : 0;
    A.m += in ? m : 0;
    A.g += in ? g : 0;
    A.n += in;
    A.xc = max(A.xc, in ? c : -1);
    A.xm = max(A.xm, in ? m : -1);
    A.xg = max(A.xg, in ? g : -1);
}

// One run [a, r.end) of a header, wave-uniform: a closed run (a negative column) is skipped whole
template <int NS>
__device__ __forceinline__ void free_run(FreeAcc (&A)[NS], int tid, int32_t a, const Seg& r) {
    if ((r.cpu | r.mem | r.gpu) < 0) return;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int t = tid + FREE_THREADS * i;
        free_cell(A[i], t >= a && t < r.end, r.cpu, r.mem, r.gpu);
    }
}

__global__ __launch_bounds__(256) void k_free_init(unsigned long long* __restrict__ sum, int32_t* __restrict__ cnt,
                                                   int32_t rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
#pragma unroll
    for (int f = 0; f < 3; ++f) sum[(int64_t)f * rows + i] = 0ull;
    cnt[i] = 0;
#pragma unroll
    for (int f = 1; f < 4; ++f) cnt[(int64_t)f * rows + i] = -1;
}

// grid (chunks, parts).  sum: 3 planes of parts * H 64-bit words (cpu, mem, gpu); cnt: 4 planes of
// parts * H words (nodes, max_cpu, max_mem, max_gpu).  NS = ceil(H / 256).
template <int NS>
__global__ __launch_bounds__(FREE_THREADS) void k_free_walk(const TlHdr* __restrict__ hdr,
                                                            const Seg* __restrict__ slab, int32_t nn, int32_t chunk,
                                                            int32_t H, unsigned long long* __restrict__ sum,
                                                            int32_t* __restrict__ cnt) {
    const int tid = threadIdx.x;
    const int p = blockIdx.y;
    const uint32_t pbit = 1u << p;
    const int32_t n0 = blockIdx.x * chunk, n1 = min(n0 + chunk, nn);
    int any = 0;
    for (int x = n0 + tid; x < n1; x += FREE_THREADS) any |= (hdr[x].mask & pbit) != 0u;
    if (!__syncthreads_or(any)) return;  // block-uniform

    FreeAcc A[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) A[i] = FreeAcc{0, 0, 0, 0, -1, -1, -1};

    for (int x = n0; x < n1; ++x) {  // wave-uniform: scalar header loads
        const TlHdr& h = hdr[x];
        if (!(h.mask & pbit)) continue;
        const int cn = min(max(h.cnt, 0), TL_MAX_SLOTS);
        if (cn <= TL_HEAD) {
            int32_t a = 0;
#pragma unroll
            for (int i = 0; i < TL_HEAD; ++i)
                if (i < cn) {
                    free_run<NS>(A, tid, a, h.head[i]);
                    a = h.head[i].end;
                }
        } else {
            const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int t = tid + FREE_THREADS * i;
                int lo = 0, hi = cn - 1;  // first run with end > t; both stay inside [0, cn)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sg[mid].end > t) hi = mid;
                    else lo = mid + 1;
                }
                const Seg r = sg[lo];
                free_cell(A[i], t < H && t < r.end && (r.cpu | r.mem | r.gpu) >= 0, r.cpu, r.mem, r.gpu);
            }
        }
    }

    const int64_t rows = (int64_t)gridDim.y * H;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int t = tid + FREE_THREADS * i;
        if (t >= H || A[i].n == 0) continue;
        const int64_t o = (int64_t)p * H + t;
        if (A[i].c) atomicAdd(sum + o, (unsigned long long)A[i].c);
        if (A[i].m) atomicAdd(sum + rows + o, (unsigned long long)A[i].m);
        if (A[i].g) atomicAdd(sum + 2 * rows + o, (unsigned long long)A[i].g);
        atomicAdd(cnt + o, A[i].n);
        atomicMax(cnt + rows + o, A[i].xc);
        atomicMax(cnt + 2 * rows + o, A[i].xm);
        atomicMax(cnt + 3 * rows + o, A[i].xg);
    }
}

__global__ __launch_bounds__(256) void k_free_pack(const unsigned long long* __restrict__ sum,
                                                   const int32_t* __restrict__ cnt, int32_t rows,
                                                   FreeRow* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    FreeRow r;
    r.cpu = (int64_t)sum[i];
    r.mem = (int64_t)sum[(int64_t)rows + i];
    r.gpu = (int64_t)sum[2 * (int64_t)rows + i];
    r.nodes = cnt[i];
    r.max_cpu = cnt[(int64_t)rows + i];
    r.max_mem = cnt[2 * (int64_t)rows + i];
    r.max_gpu = cnt[3 * (int64_t)rows + i];
    out[i] = r;
}

// The profile on stream st.  scratch: FREE_ROW_BYTES * parts * H bytes, 8-byte aligned; out: parts * H
// rows, 8-byte aligned.  Every row is written, whatever nn is.
hipError_t launch_free_tl(hipStream_t st, const TlHdr* hdr, const Seg* slab, int32_t nn, int32_t H, int32_t parts,
                          int32_t chunk, void* scratch, void* out) {
    if (H < 1 || H > TL_MAX_SLOTS || parts < 1 || parts > 32 || chunk < 1 || !scratch || !out)
        return hipErrorInvalidValue;
    const int32_t rows = parts * H;
    unsigned long long* sum = static_cast<unsigned long long*>(scratch);
    int32_t* cnt = reinterpret_cast<int32_t*>(sum + 3 * (size_t)rows);
    const dim3 per_row((rows + 255) / 256);
    hipLaunchKernelGGL(k_free_init, per_row, dim3(256), 0, st, sum, cnt, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nn > 0) {
        const dim3 grid((nn + chunk - 1) / chunk, parts), block(FREE_THREADS);
        switch ((H + FREE_THREADS - 1) / FREE_THREADS) {
            case 1: hipLaunchKernelGGL(k_free_walk<1>, grid, block, 0, st, hdr, slab, nn, chunk, H, sum, cnt); break;
            case 2: hipLaunchKernelGGL(k_free_walk<2>, grid, block, 0, st, hdr, slab, nn, chunk, H, sum, cnt); break;
            case 3: hipLaunchKernelGGL(k_free_walk<3>, grid, block, 0, st, hdr, slab, nn, chunk, H, sum, cnt); break;
            default: hipLaunchKernelGGL(k_free_walk<4>, grid, block, 0, st, hdr, slab, nn, chunk, H, sum, cnt); break;
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_free_pack, per_row, dim3(256), 0, st, sum, cnt, rows, static_cast<FreeRow*>(out));
    return hipGetLastError();
}

}  // namespace fitgpu

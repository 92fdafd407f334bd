// fit_room.hip — how many more copies of a job fit now: per job, the feasible member nodes, the
// copies each takes (the smallest floor(free / demand) over the demanded resources), their 64-bit
// sum, the roomiest node and the resource that binds on each (include/fitgpu.h fit_room; DESIGN.md
// §2e, §3.13).  gfx950.
//
// fit_explain's three bounded launches, in the query frame (fit_query.h):
//   k_room_classify : per job, the partition-limit code, zeroed counters, the job's component
//   k_room_count    : every live job × every row of its component.  Lanes = jobs, rows wave-uniform
//                     (scalar loads of a NodeRec, four per wait), grid.y = explain_slices(), the 8
//                     waves of a workgroup summed through LDS, one atomic per (workgroup, job,
//                     non-zero quantity): five 32-bit adds, one 64-bit add (copies) and one 64-bit
//                     max (per << 32 | ~node id: the largest per, the lowest node id on a tie).
//                     Integer sums and a max do not depend on the order: exact and reproducible.
//   k_room_final    : decodes the max word in place and sets NO_NODES / NONE / SOME.
// No cross-workgroup wait of any kind: no watchdog, no persistent-launch lock.
//
// The quotients.  A lane's divisors are loop-invariant, so each is turned into a 32-bit reciprocal
// M = min(floor(2^32 / d), 2^32 - 1) once, before the row loop; per row q = mulhi(n, M), then
// q += (n - q * d >= d).  With r = 2^32 mod d < d, n * M / 2^32 = n / d - n * r / (d * 2^32), and
// n < 2^31 makes the last term < 1/2: mulhi never exceeds floor(n / d) and is at most one short of
// it, so one fix-up is exact for 0 <= n < 2^31, 1 <= d < 2^31 (d = 1: M is the clamped 2^32 - 1).
// The plain `n / d` form was measured against it and dropped.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fit_device.h"
#include "fit_query.h"

namespace fitgpu {

constexpr int RM_WAVES = QUERY_WAVES, RM_JOBS = QUERY_JOBS;
constexpr int RM_N32 = 5;  // members, nodes, by_gpu, by_cpu, by_mem
constexpr int32_t RM_UNBOUNDED = 0x7fffffff;

// fit_room as the kernels see it (include/fitgpu.h).  Between k_room_count and k_room_final `best`
// holds the by_gpu count and the 8 bytes at best_node the max word; k_room_final moves both.
struct alignas(8) RoomRow {
    int32_t code, members, nodes, best;
    int64_t copies;
    int32_t best_node, by_gpu, by_cpu, by_mem;
};
static_assert(sizeof(RoomRow) == 40 && offsetof(RoomRow, copies) == 16 && offsetof(RoomRow, best_node) == 24,
              "fit_room is 40 bytes, its 64-bit words at 16 and 24");

__global__ __launch_bounds__(256) void k_room_classify(
    const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, int32_t nj,
    const int32_t* __restrict__ ptab /* [4][32]: time, cpus, mem, comp */, int32_t np, RoomRow* __restrict__ out,
    int8_t* __restrict__ jcomp, int32_t* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    const int p = jpart[q];
    const int32_t c = jcpu[q], m = jmem[q], g = jgpu[q], w = jwall[q];
    const JobLimit lim = job_limit(p, np, ptab, c, m, w);
    int comp = lim.comp;
    if (c < 0 || m < 0 || g < 0 || w < 0) {  // the whole call fails (FIT_E_INVAL)
        comp = -1;
        atomicOr(bad, 1);
    }
    RoomRow r;
    r.code = lim.code;
    r.members = r.nodes = r.best = 0;
    r.copies = 0;
    // a limit code's row is final here; the others count into zeros (the max word's low half too)
    r.best_node = lim.code != LIM_NONE ? -1 : 0;
    r.by_gpu = r.by_cpu = r.by_mem = 0;
    out[q] = r;
    jcomp[q] = (int8_t)comp;
}

// A lane's demand for one resource: the divisor, its reciprocal, and whether it divides at all.
struct RoomDiv {
    uint32_t d, M;
    bool has;
};
__device__ __forceinline__ RoomDiv room_div(int32_t demand) {
    RoomDiv v;
    v.d = (uint32_t)demand;
    v.has = demand > 0;
    // floor(2^32 / d) in 32 bits: floor((X + 1) / d) = X / d + (X % d == d - 1) for X = 2^32 - 1;
    // d = 1 clamps to X
    const uint32_t X = 0xffffffffu, dd = demand > 1 ? v.d : 1u, q = X / dd;
    v.M = demand > 1 ? q + (X - q * dd == dd - 1u) : (v.has ? X : 0u);
    return v;
}
// floor(n / d) for a feasible node's n >= d >= 1; INT32_MAX for d = 0.  On a node that is not
// feasible n may be NodeRec's clamped -1: the value is then not used (room_row selects 0).
__device__ __forceinline__ int32_t room_quot(int32_t free, const RoomDiv& v) {
    const uint32_t n = (uint32_t)free;
    uint32_t q = __umulhi(n, v.M);
    q += (n - q * v.d >= v.d);
    return v.has ? (int32_t)q : RM_UNBOUNDED;
}

struct RoomAcc {
    int32_t n[RM_N32];
    int64_t copies;
    uint64_t key;  // per << 32 | ~node id of the roomiest node so far, 0: none
};

// One (job-lane, node-row) evaluation.  Feasibility is explain_row's four terms; NodeRec fields are
// clamped to >= -1 and demands are >= 0, so `free < demand` is what the raw columns give, and a
// feasible node has free >= demand >= 0 in every column: only such a node's quotients are used.
__device__ __forceinline__ void room_row(const NodeRec& r, uint32_t pbit, const RoomDiv& dc, const RoomDiv& dm,
                                         const RoomDiv& dg, int32_t wall, RoomAcc& a) {
    const int mb = (r.mask & pbit) != 0u;
    const int ok = mb & (r.cpu >= (int32_t)dc.d) & (r.mem >= (int32_t)dm.d) & (r.gpu >= (int32_t)dg.d) &
                   (r.avail >= wall);
    const int32_t qg = room_quot(r.gpu, dg), qc = room_quot(r.cpu, dc),
                  qm = room_quot(r.mem, dm);
    const int32_t per = ok ? min(qg, min(qc, qm)) : 0;
    // the binding resource: the first of gpu, cpu, mem that is demanded and attains the minimum
    const int bg = ok & dg.has & (qg == per);
    const int bc = ok & (bg ^ 1) & dc.has & (qc == per);
    const int bm = ok & ((bg | bc) ^ 1) & dm.has;
    a.n[0] += mb;
    a.n[1] += ok;
    a.n[2] += bg;
    a.n[3] += bc;
    a.n[4] += bm;
    a.copies += per;
    const uint64_t key = per > 0 ? ((uint64_t)(uint32_t)per << 32) | (uint32_t)~r.orig : 0ull;
    a.key = key > a.key ? key : a.key;
}

// grid (job tiles, node slices); jl / live: fit_query.h's job list.
__global__ __launch_bounds__(RM_WAVES * 64) void k_room_count(
    const NodeRec* __restrict__ rec, ExplainComps C, const int32_t* __restrict__ jl, const int32_t* __restrict__ live,
    int32_t nj, const int32_t* __restrict__ jcpu, const int32_t* __restrict__ jmem, const int32_t* __restrict__ jgpu,
    const int32_t* __restrict__ jwall, const uint16_t* __restrict__ jpart, const int8_t* __restrict__ jcomp,
    RoomRow* __restrict__ out) {
    __shared__ int32_t red[RM_WAVES][RM_N32][RM_JOBS];
    __shared__ uint64_t red64[RM_WAVES][2][RM_JOBS];  // copies, max word
    __shared__ int32_t qs[RM_JOBS];
    const int nlive = query_live(jl, live, nj);
    if (query_idle<RM_JOBS>(nlive)) return;  // block-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const QueryLane j = query_lane<RM_JOBS>(nlive, jl, nj, jcomp, C);
    const int q = j.q;
    const bool on = j.on;
    const RoomDiv dc = room_div(on ? jcpu[q] : 0), dm = room_div(on ? jmem[q] : 0), dg = room_div(on ? jgpu[q] : 0);
    const int32_t wall = on ? jwall[q] : 0;
    const uint32_t pbit = on ? 1u << (jpart[q] & 31) : 0u;
    RoomAcc acc;
#pragma unroll
    for (int i = 0; i < RM_N32; ++i) acc.n[i] = 0;
    acc.copies = 0;
    acc.key = 0;

    QueryWalk w = query_walk(on);
    while (w.rem) {  // wave-uniform: one pass per distinct component
        const QueryRange r = query_next<RM_WAVES>(w, C, j.comp, on, wave);
        const uint32_t pb = r.mine ? pbit : 0u;
        int x = r.n0;
        for (; x + 4 <= r.n1; x += 4) {  // four scalar row loads per wait, as k_scan
            NodeRec r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = rec[x + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) room_row(r[u], pb, dc, dm, dg, wall, acc);
        }
        for (; x < r.n1; ++x) room_row(rec[x], pb, dc, dm, dg, wall, acc);
    }

#pragma unroll
    for (int i = 0; i < RM_N32; ++i) red[wave][i][lane] = acc.n[i];
    red64[wave][0][lane] = (uint64_t)acc.copies;
    red64[wave][1][lane] = acc.key;
    if (wave == 0) qs[lane] = on ? q : -1;
    __syncthreads();
    // thread (i, l) folds quantity i of job-lane l over the waves: one atomic per workgroup, job and
    // quantity, none for a zero.  The by_gpu count goes to `best`, the max word to the 8 bytes at
    // best_node, until k_room_final.
    for (int e = threadIdx.x; e < (RM_N32 + 2) * RM_JOBS; e += RM_WAVES * 64) {
        const int i = e / RM_JOBS, l = e - i * RM_JOBS;
        const int jq = qs[l];
        if (jq < 0) continue;
        RoomRow* o = out + jq;
        if (i < RM_N32) {
            int32_t v = 0;
#pragma unroll
            for (int w = 0; w < RM_WAVES; ++w) v += red[w][i][l];
            int32_t* dst = i == 0 ? &o->members : i == 1 ? &o->nodes : i == 2 ? &o->best : i == 3 ? &o->by_cpu : &o->by_mem;
            if (v != 0) atomicAdd(dst, v);
        } else if (i == RM_N32) {
            uint64_t v = 0;
#pragma unroll
            for (int w = 0; w < RM_WAVES; ++w) v += red64[w][0][l];
            if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&o->copies), (unsigned long long)v);
        } else {
            uint64_t v = 0;
#pragma unroll
            for (int w = 0; w < RM_WAVES; ++w) v = red64[w][1][l] > v ? red64[w][1][l] : v;
            if (v != 0) atomicMax(reinterpret_cast<unsigned long long*>(&o->best_node), (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(256) void k_room_final(RoomRow* __restrict__ out, int32_t nj) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nj) return;
    RoomRow r = out[q];
    if (r.code != ROOM_SOME) return;  // partition / limit codes: final since k_room_classify
    // little-endian: the max word's low half (~node id) lies at best_node, its high half (per) at
    // by_gpu; the by_gpu count waits in best
    const int32_t per = r.by_gpu, inv = r.best_node;
    r.by_gpu = r.best;
    r.best = per;
    r.best_node = per > 0 ? ~inv : -1;
    r.code = r.members == 0 ? ROOM_NO_NODES : (r.copies == 0 ? ROOM_NONE : ROOM_SOME);
    out[q] = r;
}

// The rows on stream st in two calls, the caller ordering the jobs by component in between: `out` (nj
// rows of 40 B, 8-byte aligned) and *bad (1: a negative demand) are valid when the stream has drained.
hipError_t launch_room_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                                int32_t nj, void* out, int8_t* jcomp, int32_t* bad) {
    return launch_per_job(st, nj, k_room_classify, jcpu, jmem, jgpu, jwall, jpart, nj, ptab, np,
                          static_cast<RoomRow*>(out), jcomp, bad);
}

// Count and finalise.  jl / live / slices as launch_explain's.
hipError_t launch_room(hipStream_t st, const NodeRec* rec, const ExplainComps& C, const int32_t* jcpu,
                       const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                       int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, void* out) {
    RoomRow* o = static_cast<RoomRow*>(out);
    const hipError_t e = launch_per_tile(st, nj, C.ncomp, slices, k_room_count, rec, C, jl, live, nj, jcpu, jmem, jgpu,
                                         jwall, jpart, jcomp, o);
    return e != hipSuccess ? e : launch_per_job(st, nj, k_room_final, o, nj);
}

}  // namespace fitgpu

// fit_pre_row.h — what fit_preempt's and fit_preempt_k's walks share: the
// 128-bit key of a (job, node) pair and the evaluation of one (job-lane, node-row) pair against the
// row's victims.  What becomes of an offered key is the kernel's: `Sink` keeps one minimum
// (fit_preempt.hip) or the k smallest (fit_preempt_k.hip).  __forceinline__: a kernel built from
// these compiles to what it was when it spelled them out.
#pragma once
#include <hip/hip_runtime.h>

#include "fit_device.h"
#include "fit_key.h"
#include "fit_query.h"

namespace fitgpu {

constexpr int PRE_WAVES = QUERY_WAVES, PRE_JOBS = QUERY_JOBS;
constexpr int PRE_NCNT = 4;  // members, fit, able, outranked
constexpr uint32_t PRE_SAT = 0x7fffffffu;
static_assert(PRE_CHUNK % PRE_JOBS == 0, "a chunk is whole job tiles");

// The key of a (job, node) pair as two words, smaller is better; PRE_NOKEY: no node.
//   hi = (top ^ 2^31) << 32 | v     top's order as an unsigned; a node that fits now: 0
//   lo = score << 32 | node id
struct PreKey {
    uint64_t hi, lo;
};
static_assert(sizeof(PreKey) == 16, "one partial is 16 bytes");
constexpr uint64_t PRE_NOKEY = ~0ull;
__device__ __forceinline__ void pre_min(PreKey& k, bool has, uint64_t hi, uint64_t lo) {
    const bool lt = has && (hi < k.hi || (hi == k.hi && lo < k.lo));
    k.hi = lt ? hi : k.hi;
    k.lo = lt ? lo : k.lo;
}

// A lane's job
struct PreJob {
    int32_t cpu, mem, gpu, wall, prio;
};

// One (job-lane, node-row) evaluation; x: the row's position, wave-uniform.  Eligible: a member with
// avail >= wall and no column clamped to -1.  NodeRec fields are clamped to >= -1 and demands are
// >= 0, so "fits now" is explain_row's four terms.  key.offer(has, hi, lo): the lanes with `has` have
// the key (hi, lo) on this row; called by the whole wave.
template <class Sink>
__device__ __forceinline__ void pre_row(const NodeRec& r, int x, uint32_t pbit, const PreJob& j,
                                        const int32_t* __restrict__ voff, const VicEnt* __restrict__ vent,
                                        int32_t (&n)[PRE_NCNT], Sink& key) {
    const bool mb = (r.mask & pbit) != 0u;
    const bool elig = mb && r.avail >= j.wall && (r.cpu | r.mem | r.gpu) >= 0;
    const bool fits = elig && r.cpu >= j.cpu && r.mem >= j.mem && r.gpu >= j.gpu;
    n[0] += mb;
    n[1] += fits;
    const uint64_t lo0 = ((uint64_t)fit_score(r.cpu - j.cpu, r.mem - j.mem, r.gpu - j.gpu) << 32) | (uint32_t)r.orig;
    key.offer(fits, 0ull, lo0);
    const bool shrt = elig && !fits;
    if (__ballot(shrt) == 0ull) return;  // wave-uniform: no lane needs this row's victims
    const int a = voff[x], b = voff[x + 1];
    if (b <= a) return;
    // free >= 0 on an eligible row, the sums and the demands are < 2^31: unsigned 32-bit sums are exact
    const uint32_t fc = (uint32_t)r.cpu, fm = (uint32_t)r.mem, fg = (uint32_t)r.gpu;
    const uint32_t dc = (uint32_t)j.cpu, dm = (uint32_t)j.mem, dg = (uint32_t)j.gpu;
    // the sums do not decrease along the list: if the whole list does not free enough, no prefix does
    const VicEnt all = vent[b - 1];
    bool look = shrt && fc + (uint32_t)all.cpu >= dc && fm + (uint32_t)all.mem >= dm && fg + (uint32_t)all.gpu >= dg;
    // A looking lane ends at the last entry at the latest (there it is outranked or fits), so the
    // clamped reads past the end, which repeat the last entry, find no lane looking.
    for (int i = a; i < b && __ballot(look) != 0ull; i += 4) {
        VicEnt e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = vent[min(i + u, b - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool held = look && e[u].prio >= j.prio;  // the first entry the job does not outrank
            const uint32_t hc = fc + (uint32_t)e[u].cpu, hm = fm + (uint32_t)e[u].mem, hg = fg + (uint32_t)e[u].gpu;
            const bool ok = look && !held && hc >= dc && hm >= dm && hg >= dg;
            n[2] += ok;
            n[3] += held;
            const uint32_t v = (uint32_t)(min(i + u, b - 1) - a + 1);
            const uint32_t sc = fit_score((int32_t)(min(hc, PRE_SAT) - dc), (int32_t)(min(hm, PRE_SAT) - dm),
                                          (int32_t)(min(hg, PRE_SAT) - dg));
            const uint64_t hi = ((uint64_t)((uint32_t)e[u].prio ^ 0x80000000u) << 32) | v;
            key.offer(ok, hi, ((uint64_t)sc << 32) | (uint32_t)r.orig);
            look = look && !held && !ok;
        }
    }
}

}  // namespace fitgpu

// fit_ptl_node.h — what fit_preempt_tl's and fit_preempt_tl_k's walks share: the
// visit of a node's runs that meet a wave's windows and the evaluation of one (job-lane, node
// position) pair against the position's victims with ends.  What becomes of an offered key is the
// kernel's: `Sink` keeps one minimum (fit_preempt_tl.hip) or the k smallest (fit_preempt_tl_k.hip).
// __forceinline__: a kernel built from these compiles to what it was when it spelled them out.
#pragma once
#include <hip/hip_runtime.h>

#include "fit_device.h"
#include "fit_pre_row.h"
#include "fit_query.h"

namespace fitgpu {

static_assert(sizeof(VicTl) == 32, "one victim is one 32-byte scalar load");

// The runs of one node that meet the window of a lane of `act`, in order: f(a, run) for the run
// [a, run.end), called by the whole wave.  Header runs, then the slab row four Seg per wait (inside
// the row: 4 | TL_HEAD, 4 | TL_MAX_SLOTS; fit_tl_walk.h); left at the first run that starts behind
// every such lane's window.
template <class F>
__device__ __forceinline__ void ptl_runs(const TlHdr& h, const Seg* sg, int cn, bool act, int32_t d, F f) {
    int32_t a = 0;
#pragma unroll
    for (int i = 0; i < TL_HEAD; ++i)
        if (i < cn && __ballot(act && a < d) != 0ull) {
            f(a, h.head[i]);
            a = h.head[i].end;
        }
    for (int i = TL_HEAD; i < cn && __ballot(act && a < d) != 0ull; i += 4) {
        Seg r4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r4[k] = sg[i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < cn && __ballot(act && a < d) != 0ull) {
                f(a, r4[k]);
                a = r4[k].end;
            }
    }
}

// One (job-lane, node position) evaluation; h and x are wave-uniform.  Eligible: a member with
// d <= H whose window holds no closed slot.  The header's column ceilings are not consulted: victims
// raise values above them.  key.offer as pre_row's.
template <class Sink>
__device__ __forceinline__ void ptl_node(const TlHdr& h, int x, const Seg* __restrict__ slab, uint32_t pbit,
                                         const PreJob& j, int32_t d, int32_t H, int32_t shift,
                                         const VicSpan* __restrict__ vspan, const VicTl* __restrict__ vent,
                                         int32_t (&n)[PRE_NCNT], Sink& key) {
    const bool mb = (h.mask & pbit) != 0u;
    n[0] += mb;
    // the list's span ahead of every branch: its one 8-byte scalar load goes out with the header's
    const VicSpan sp = vspan[x];
    const int va = sp.beg, len = sp.len;
    const int cn = min(h.cnt, TL_MAX_SLOTS);
    const bool act = mb && d <= H && cn > 0;
    if (__ballot(act) == 0ull) return;  // wave-uniform
    const Seg* sg = slab + (int64_t)x * TL_MAX_SLOTS;
    // free >= 0 on an open slot, the saturated sums and the demands are < 2^31: unsigned 32-bit sums are exact
    const uint32_t dc = (uint32_t)j.cpu, dm = (uint32_t)j.mem, dg = (uint32_t)j.gpu;

    // (1) the window as it stands
    bool closed = false, all = true;
    int32_t mc = 0x7fffffff, mm = 0x7fffffff, mg = 0x7fffffff;
    ptl_runs(h, sg, cn, act, d, [&](int32_t a, const Seg& r) {
        const bool in = act && a < d;
        closed |= in && (r.cpu | r.mem | r.gpu) < 0;
        all &= !in || (r.cpu >= j.cpu && r.mem >= j.mem && r.gpu >= j.gpu);
        mc = in ? min(mc, r.cpu) : mc;
        mm = in ? min(mm, r.mem) : mm;
        mg = in ? min(mg, r.gpu) : mg;
    });
    const bool elig = act && !closed;
    const bool fits = elig && all;
    n[1] += fits;
    key.offer(fits, 0ull, ((uint64_t)fit_score(mc - j.cpu, mm - j.mem, mg - j.gpu) << 32) | (uint32_t)h.orig);
    const bool shrt = elig && !fits;
    if (__ballot(shrt) == 0ull) return;  // wave-uniform: no lane needs this node's victims
    if (len <= 0) return;
    const VicTl* ve = vent + va;

    // (2) per run a lane is short on, its smallest covering prefix; v = the largest of them, top = the
    // priority of entry v - 1.  dead: a run that no prefix covers.
    bool dead = false;
    int32_t v = 0, top = 0;
    ptl_runs(h, sg, cn, shrt, d, [&](int32_t a, const Seg& r) {
        const bool sh = shrt && a < d && !(r.cpu >= j.cpu && r.mem >= j.mem && r.gpu >= j.gpu);
        if (__ballot(sh) == 0ull) return;
        const int32_t stop = min(r.end, d);
        const uint32_t fc = (uint32_t)r.cpu, fm = (uint32_t)r.mem, fg = (uint32_t)r.gpu;
        uint32_t sc = 0, sm = 0, sg3 = 0;
        bool look = sh;
        int32_t vr = 0, pr = 0;
        for (int i = 0; i < len && __ballot(look) != 0ull; i += 4) {
            VicTl e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = ve[min(i + u, len - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // a clamped read past the end repeats the last entry: it counts for nothing
                const bool cnt = i + u < len && max(e[u].end - shift, 0) >= stop;
                sc = cnt ? min(sc + (uint32_t)e[u].cpu, PRE_SAT) : sc;
                sm = cnt ? min(sm + (uint32_t)e[u].mem, PRE_SAT) : sm;
                sg3 = cnt ? min(sg3 + (uint32_t)e[u].gpu, PRE_SAT) : sg3;
                const bool ok = look && cnt && fc + sc >= dc && fm + sm >= dm && fg + sg3 >= dg;
                vr = ok ? i + u + 1 : vr;
                pr = ok ? e[u].prio : pr;
                look = look && !ok;
            }
        }
        dead |= look;
        const bool up = sh && vr > v;
        top = up ? pr : top;
        v = up ? vr : v;
    });
    // priorities do not decrease along the list: v <= L exactly when the job outranks entry v - 1
    const bool able = shrt && !dead && top < j.prio;
    n[2] += able;
    n[3] += shrt && !dead && top >= j.prio;
    if (__ballot(able) == 0ull) return;

    // (3) the window minima with the first v entries gone
    uint32_t ec = PRE_SAT, em = PRE_SAT, eg = PRE_SAT;
    ptl_runs(h, sg, cn, able, d, [&](int32_t a, const Seg& r) {
        const bool in = able && a < d;
        const int32_t stop = min(r.end, d);
        uint32_t sc = 0, sm = 0, sg3 = 0;
        for (int i = 0; i < len && __ballot(in && i < v) != 0ull; i += 4) {
            VicTl e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = ve[min(i + u, len - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool cnt = i + u < v && max(e[u].end - shift, 0) >= stop;  // v <= len
                sc = cnt ? min(sc + (uint32_t)e[u].cpu, PRE_SAT) : sc;
                sm = cnt ? min(sm + (uint32_t)e[u].mem, PRE_SAT) : sm;
                sg3 = cnt ? min(sg3 + (uint32_t)e[u].gpu, PRE_SAT) : sg3;
            }
        }
        ec = in ? min(ec, min((uint32_t)r.cpu + sc, PRE_SAT)) : ec;
        em = in ? min(em, min((uint32_t)r.mem + sm, PRE_SAT)) : em;
        eg = in ? min(eg, min((uint32_t)r.gpu + sg3, PRE_SAT)) : eg;
    });
    const uint32_t s = fit_score((int32_t)(ec - dc), (int32_t)(em - dm), (int32_t)(eg - dg));
    const uint64_t hi = ((uint64_t)((uint32_t)top ^ 0x80000000u) << 32) | (uint32_t)v;
    key.offer(able, hi, ((uint64_t)s << 32) | (uint32_t)h.orig);
}

}  // namespace fitgpu

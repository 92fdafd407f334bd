// fit_key.h — SPEC §2's score and key: the device code's single definition of the ordering every
// engine reproduces.  The oracle (oracle/fitref.c) states it independently.
#pragma once
#include <hip/hip_runtime.h>
#include "fit_device.h"

namespace fitgpu {

// score = min(dg, 255) << 24 | min(dc, 4095) << 12 | min(dm >> 10, 4095), lower is better: the
// gpus, cpus and memory (in steps of 1024) a node would keep free after the job, each capped.
constexpr uint32_t SCORE_GPU_CAP = 255u, SCORE_CPU_CAP = 4095u, SCORE_MEM_CAP = 4095u;
constexpr int SCORE_GPU_SHIFT = 24, SCORE_CPU_SHIFT = 12, SCORE_MEM_STEP = 10;

// dc, dm, dg: free minus demand; a negative one is capped, and the caller's feasibility test drops it
__device__ __forceinline__ uint32_t fit_score(int32_t dc, int32_t dm, int32_t dg) {
    return (min((uint32_t)dg, SCORE_GPU_CAP) << SCORE_GPU_SHIFT) |
           (min((uint32_t)dc, SCORE_CPU_CAP) << SCORE_CPU_SHIFT) |
           min((uint32_t)dm >> SCORE_MEM_STEP, SCORE_MEM_CAP);
}

// SPEC §2 key of a node row at position pos for a job (KEY_INF: no fit); two argument styles, one body
__device__ __forceinline__ uint64_t fit_key(int32_t cf, int32_t mf, int32_t gf, int32_t av,
                                            uint32_t mask, uint32_t pos, int32_t jc, int32_t jm,
                                            int32_t jg, int32_t jw, uint32_t jp) {
    const int32_t dc = cf - jc, dm = mf - jm, dg = gf - jg, da = av - jw;
    const bool ok = (dc | dm | dg | da) >= 0 && (mask & jp);
    const uint32_t sc = fit_score(dc, dm, dg);  // before the select, as it was written: the listings
    return ok ? (((uint64_t)sc << 32) | pos) : KEY_INF;  // of mw_decider / mw_helper depend on it
}
__device__ __forceinline__ uint64_t fit_key(int32_t cf, int32_t mf, int32_t gf, int32_t av,
                                            uint32_t mask, uint32_t pos, const JobRec& J) {
    return fit_key(cf, mf, gf, av, mask, pos, J.cpu, J.mem, J.gpu, J.wall, J.pbit);
}

}  // namespace fitgpu

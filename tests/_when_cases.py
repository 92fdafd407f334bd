"""The checker of fit_when, shared by tests/test_when_gpu.py and the lifecycle tests
(not a test module).  ref_when restates §2d in numpy over the dense [n, H, 3] timeline that
Engine.read_timeline returns; it shares nothing with the run-length walk of the kernels."""
import numpy as np

from fitgpu import (ETA_DTYPE, FIT_ETA_HORIZON, FIT_ETA_LATER, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM,
                    FIT_ETA_LIMIT_TIME, FIT_ETA_NO_NODES, FIT_ETA_NOW, FIT_ETA_PARTITION, synth)

INF = synth.INT32_MAX


def ref_when(tl, mask, parts, jobs, slot_min):
    """DESIGN.md §2d over the dense timeline tl[n, H, 3] (-1 = holds nothing): every job alone.
    Per job and member node: ok[t] = all(col[t] >= demand); the earliest s whose window of d slots
    is all ok; the key (s, score from the window minima minus the demand, node id)."""
    n, H, _ = tl.shape
    P, J = parts.p, jobs.j
    out = np.zeros(J, ETA_DTYPE)
    out["start"] = out["node"] = out["wait_min"] = -1
    tl64 = tl.astype(np.int64)
    ids = np.arange(n)
    for q in range(J):
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        wall, p = int(jobs.wall[q]), int(jobs.part[q])
        d = max(1, -(-wall // slot_min))
        out["dur"][q] = d
        if p >= P:
            out["code"][q] = FIT_ETA_PARTITION
            continue
        if parts.max_time_min[p] >= 0 and wall > parts.max_time_min[p]:
            out["code"][q] = FIT_ETA_LIMIT_TIME
            continue
        if parts.max_cpus_per_node[p] >= 0 and dem[0] > parts.max_cpus_per_node[p]:
            out["code"][q] = FIT_ETA_LIMIT_CPUS
            continue
        if parts.max_mem_per_node[p] >= 0 and dem[1] > parts.max_mem_per_node[p]:
            out["code"][q] = FIT_ETA_LIMIT_MEM
            continue
        mem = ids[((mask.astype(np.int64) >> p) & 1) != 0]
        out["members"][q] = len(mem)
        if len(mem) == 0:
            out["code"][q] = FIT_ETA_NO_NODES
            continue
        if d > H:
            out["code"][q] = FIT_ETA_HORIZON
            continue
        sub = tl64[mem]                                      # [m, H, 3]
        ok = (sub >= dem[None, None, :]).all(axis=2)         # [m, H]
        t = np.arange(H)
        last_bad = np.maximum.accumulate(np.where(ok, -1, t[None, :]), axis=1)
        win = (t[None, :] - last_bad) >= d                   # a window of d ok slots ends at t
        has = win.any(axis=1)
        s = win.argmax(axis=1) - d + 1                       # earliest start (valid where has)
        out["hosts"][q] = has.sum()
        out["now"][q] = (has & (s == 0)).sum()
        if not has.any():
            out["code"][q] = FIT_ETA_HORIZON
            continue
        hm, hs = mem[has], s[has]
        idx = hs[:, None] + np.arange(d)[None, :]            # [h, d] slots of each node's window
        wmin = np.take_along_axis(sub[has], idx[:, :, None], axis=1).min(axis=1) - dem[None, :]  # [h, 3]
        score = (np.minimum(wmin[:, 2], 255) << 24) | (np.minimum(wmin[:, 0], 4095) << 12) | \
            np.minimum(wmin[:, 1] >> 10, 4095)
        best = np.lexsort((hm, score, hs))[0]                # the smallest (start, score, node id)
        out["start"][q], out["node"][q] = hs[best], hm[best]
        out["wait_min"][q] = min(int(hs[best]) * slot_min, INF)
        out["code"][q] = FIT_ETA_LATER if hs[best] > 0 else FIT_ETA_NOW
    return out

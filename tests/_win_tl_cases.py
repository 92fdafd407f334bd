"""Cases and the checker of fit_when_k_win / fit_place_tl_k_win, shared by
tests/test_win_tl.py and tests/test_win_tl_gpu.py (not a test module).  ref_when_k_win restates §2r
in numpy over the dense [n, H, 3] timeline: feasibility of every start slot first, then the slice
to the job's allowed starts A.  It shares nothing with the run-length walk of the kernels, and it
does not call _when_k_cases.ref_when_k: the tests compare the two."""
import functools

import numpy as np

import _place_tl_k_cases as pk
import _when_k_cases as wk
from fitgpu import (ETA_K_DTYPE, FIT_ETA_HORIZON, FIT_ETA_LATER, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM,
                    FIT_ETA_LIMIT_TIME, FIT_ETA_NO_NODES, FIT_ETA_NOW, FIT_ETA_PARTITION, FIT_ETA_WINDOW,
                    FIT_REJECTED, synth)

INF = synth.INT32_MAX
NONE = INF  # a deadline that is none


def window(H, not_before, deadline):
    """(from, until) of one job: both clamped to [0, H]."""
    return min(max(int(not_before), 0), H), min(max(int(deadline), 0), H)


def columns(j, not_before, deadline):
    nb = np.zeros(j, np.int32) if not_before is None else np.asarray(not_before, np.int32)
    dl = np.full(j, NONE, np.int32) if deadline is None else np.asarray(deadline, np.int32)
    return nb, dl


def ref_when_k_win(tl, mask, parts, jobs, slot_min, kmax, not_before=None, deadline=None):
    """§2r, every job alone: feas[m, s] = member m holds the demand on every slot of [s, s + d), for
    every s with s + d <= H; the allowed starts are the columns from .. until - d of it."""
    n, H, _ = tl.shape
    J = jobs.j
    nb, dl = columns(J, not_before, deadline)
    rows = np.zeros(J, ETA_K_DTYPE)
    rows["start"] = rows["wait_min"] = -1
    nodes = np.full((J, kmax), -1, np.int32)
    tl64 = tl.astype(np.int64)
    for q in range(J):
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        wall, p = int(jobs.wall[q]), int(jobs.part[q])
        need = max(int(jobs.nodes_k[q]), 1)
        d = max(1, (wall + slot_min - 1) // slot_min)
        rows["dur"][q], rows["need"][q] = d, need
        if p >= parts.p:
            rows["code"][q] = FIT_ETA_PARTITION
        elif parts.max_time_min[p] >= 0 and wall > parts.max_time_min[p]:
            rows["code"][q] = FIT_ETA_LIMIT_TIME
        elif parts.max_cpus_per_node[p] >= 0 and dem[0] > parts.max_cpus_per_node[p]:
            rows["code"][q] = FIT_ETA_LIMIT_CPUS
        elif parts.max_mem_per_node[p] >= 0 and dem[1] > parts.max_mem_per_node[p]:
            rows["code"][q] = FIT_ETA_LIMIT_MEM
        if rows["code"][q]:
            continue
        mem = np.flatnonzero((mask.astype(np.int64) >> p) & 1)
        rows["members"][q] = len(mem)
        if len(mem) == 0:
            rows["code"][q] = FIT_ETA_NO_NODES
            continue
        frm, until = window(H, nb[q], dl[q])
        rows["code"][q] = FIT_ETA_HORIZON if (frm == 0 and until == H) else FIT_ETA_WINDOW
        if frm + d > until:
            continue                                          # A is empty
        ok = (tl64[mem] >= dem[None, None, :]).all(axis=2)    # [m, H]
        bad = np.concatenate([np.zeros((len(mem), 1), np.int64), np.cumsum(~ok, axis=1)], axis=1)
        feas = (bad[:, d:] - bad[:, :H - d + 1]) == 0         # [m, H - d + 1]: no bad slot in [s, s + d)
        allowed = feas[:, frm:until - d + 1]                  # column i is start frm + i
        cnt = allowed.sum(axis=0)
        rows["hosts"][q] = allowed.any(axis=1).sum()
        rows["now"][q] = cnt[0]
        hit = np.flatnonzero(cnt >= need)
        if hit.size == 0:
            continue
        s = frm + int(hit[0])
        rows["start"][q], rows["ready"][q] = s, cnt[hit[0]]
        rows["wait_min"][q] = min(s * slot_min, INF)
        rows["code"][q] = FIT_ETA_LATER if s > 0 else FIT_ETA_NOW
        free = mem[feas[:, s]]
        left = tl64[free, s:s + d].min(axis=1) - dem[None, :]  # minima over [s, s + d) only
        score = (np.minimum(left[:, 2], 255) << 24) | (np.minimum(left[:, 0], 4095) << 12) | \
            np.minimum(left[:, 1] >> 10, 4095)
        nodes[q, :need] = free[np.lexsort((free, score))[:need]]
    return rows, nodes


def ref_place_tl_k_win(tl, mask, parts, jobs, slot_min, kmax, not_before=None, deadline=None):
    """§2r's committing half: (out[J, kmax], start[J], final dense timeline).  tl is not changed."""
    tl = np.array(tl, np.int32, copy=True)
    J = jobs.j
    nb, dl = columns(J, not_before, deadline)
    out = np.full((J, kmax), -1, np.int32)
    start = np.full(J, -1, np.int32)
    for q in range(J):
        one = wk.one_job(jobs, q)
        rows, nodes = ref_when_k_win(tl, mask, parts, one, slot_min, kmax, nb[q:q + 1], dl[q:q + 1])
        code = int(rows["code"][0])
        if code in pk.REJECT_CODES:
            out[q, 0] = FIT_REJECTED
        elif code in (FIT_ETA_NOW, FIT_ETA_LATER):
            need, s, d = int(rows["need"][0]), int(rows["start"][0]), int(rows["dur"][0])
            out[q, :need] = nodes[0, :need]
            start[q] = s
            tl[nodes[0, :need], s:s + d] -= np.array([one.cpu[0], one.mem[0], one.gpu[0]], np.int32)[None, None, :]
    return out, start, tl


def stats_of(out, start):
    placed = int((start >= 0).sum())
    rejected = int((out[:, 0] == FIT_REJECTED).sum())
    return dict(jobs=len(start), placed=placed, unplaced=len(start) - placed - rejected, rejected=rejected, engine=4)


def durs(jobs, slot_min):
    return np.maximum(1, (jobs.wall.astype(np.int64) + slot_min - 1) // slot_min).astype(np.int32)


# ---- the hand table ------------------------------------------------------------------------------
# wk.hand_case()'s cluster: H = 8, L = 5.  cpus per slot at load:
#   n0: 4 4 4 - - - - -   n1: 0 0 0 4 4 4 4 4   n2: 1 1 1 1 1 8 8 8   n3: 4 everywhere, partition 1
# (cpu, mem, gpu, wall, part, k), not_before, deadline
_A = (2, 1024, 0, 10)
HAND = [
    (_A + (0, 1), 0, NONE),
    (_A + (0, 1), 2, NONE),
    (_A + (0, 1), 2, 4),
    (_A + (0, 1), 1, 3),
    (_A + (0, 2), 6, NONE),
    (_A + (0, 2), 7, NONE),    # A is empty
    (_A + (0, 2), 0, 6),
    ((1, 1024, 0, 5, 0, 2), 1, 2),
    (_A + (0, 1), 8, NONE),
    (_A + (0, 1), -4, 1),
    (_A + (5, 1), 3, 2),       # partition 5 of 2
    (_A + (0, 1), 3, 8),
]
HAND_KMAX = 2
W, L, N = FIT_ETA_WINDOW, FIT_ETA_LATER, FIT_ETA_NOW
# (code, dur, need, start, wait_min, members, hosts, now, ready, reserved), each job queried alone
HAND_ROWS = np.array([
    (N, 2, 1, 0, 0, 3, 3, 1, 1, 0),
    (L, 2, 1, 3, 15, 3, 2, 0, 1, 0),
    (W, 2, 1, -1, -1, 3, 0, 0, 0, 0),
    (L, 2, 1, 1, 5, 3, 1, 1, 1, 0),
    (L, 2, 2, 6, 30, 3, 2, 2, 2, 0),
    (W, 2, 2, -1, -1, 3, 0, 0, 0, 0),
    (W, 2, 2, -1, -1, 3, 2, 1, 0, 0),
    (L, 1, 2, 1, 5, 3, 2, 2, 2, 0),
    (W, 2, 1, -1, -1, 3, 0, 0, 0, 0),
    (W, 2, 1, -1, -1, 3, 0, 0, 0, 0),
    (FIT_ETA_PARTITION, 2, 1, -1, -1, 0, 0, 0, 0, 0),
    (L, 2, 1, 3, 15, 3, 2, 1, 1, 0),
], ETA_K_DTYPE)
HAND_NODES = np.array([[0, -1], [1, -1], [-1, -1], [0, -1], [1, 2], [-1, -1], [-1, -1], [2, 0], [-1, -1], [-1, -1],
                       [-1, -1], [1, -1]], np.int32)
# the same twelve as one queue: row 7 is unplaced (row 3 took n0's slot 1), row 10 rejected
HAND_Q_START = np.array([0, 3, -1, 1, 6, -1, -1, -1, -1, -1, -1, 3], np.int32)
HAND_Q_NODES = np.array([[0, -1], [1, -1], [-1, -1], [0, -1], [1, 2], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1],
                         [FIT_REJECTED, -1], [1, -1]], np.int32)
HAND_Q_CPU = np.array([[2, 0, 2, -1, -1, -1, -1, -1],
                       [0, 0, 0, 0, 0, 4, 2, 2],
                       [1, 1, 1, 1, 1, 8, 6, 6],
                       [4, 4, 4, 4, 4, 4, 4, 4]], np.int32)
# the minima trap: n1 leaves 3 cpus and n2 7 on [5, 6); minima from the start of n2's stretch
# (1 cpu at slots 0-4) would score n2 as leaving 0 and pick it
TRAP = ((1, 1024, 0, 5, 0, 1), 5, NONE)
TRAP_NODE = 1


def hand_case():
    nodes, tline, _, parts = wk.hand_case()
    jobs = wk.jobs_of([h[0] for h in HAND])
    nb = np.array([h[1] for h in HAND], np.int32)
    dl = np.array([h[2] for h in HAND], np.int32)
    return nodes, tline, jobs, parts, nb, dl


# ---- the random windows -------------------------------------------------------------------------
def draw_windows(jobs, H, slot_min, seed):
    """not_before from a list of edge values, 30 % uniform in [0, H]; deadline none for a third, else
    from + d, from + d - 1, uniform in [-2, H + 2] or from + d + a small slack."""
    r = np.random.default_rng(seed)
    j = jobs.j
    d = durs(jobs, slot_min).astype(np.int64)
    nb = r.choice([0, 0, 0, 1, 2, H // 4, H // 2, H - 1, H, H + 5, -3, -1], j).astype(np.int64)
    nb = np.where(r.random(j) < 0.3, r.integers(0, H + 1, j), nb)
    frm = np.clip(nb, 0, H)
    kind = r.integers(0, 6, j)  # 0, 1: none
    dl = np.full(j, NONE, np.int64)
    dl = np.where(kind == 2, frm + d, dl)
    dl = np.where(kind == 3, frm + d - 1, dl)
    dl = np.where(kind == 4, r.integers(-2, H + 3, j), dl)
    dl = np.where(kind == 5, frm + d + r.integers(1, 6, j), dl)
    return nb.astype(np.int32), dl.astype(np.int32)


WIN_CASES = [(8, 200, 3), (64, 300, 8), (1024, 300, 8)]  # (H, jobs, kmax) of pk.busy_case
SLOT_MIN = pk.SLOT_MIN


@functools.lru_cache(maxsize=None)
def win_case(H, j, kmax):
    """(jobs, not_before, deadline) of the case: pk.busy_case with the seeded window draw."""
    jobs = pk.busy_case(H, j, kmax)
    nb, dl = draw_windows(jobs, H, SLOT_MIN, 900 + H)
    nb.setflags(write=False)
    dl.setflags(write=False)
    return jobs, nb, dl


@functools.lru_cache(maxsize=None)
def reference(H, j, kmax):
    """(out, start, final timeline) of ref_place_tl_k_win on pk.start_timeline(H), computed once."""
    nodes, tline, parts = pk.cluster(H)
    jobs, nb, dl = win_case(H, j, kmax)
    res = ref_place_tl_k_win(pk.start_timeline(H), nodes.part_mask, parts, jobs, SLOT_MIN, kmax, nb, dl)
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def alone(H, j, kmax):
    """(rows, nodes) of ref_when_k_win, every job alone on pk.start_timeline(H)."""
    nodes, tline, parts = pk.cluster(H)
    jobs, nb, dl = win_case(H, j, kmax)
    res = ref_when_k_win(pk.start_timeline(H), nodes.part_mask, parts, jobs, SLOT_MIN, kmax, nb, dl)
    for a in res:
        a.setflags(write=False)
    return res

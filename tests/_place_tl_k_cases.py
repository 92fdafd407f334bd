"""Cases and the checker of fit_place_tl_k, shared by tests/test_place_tl_k.py and
tests/test_place_tl_k_gpu.py (not a test module).  ref_place_tl_k restates §2g in numpy over the dense
[n, H, 3] timeline: job after job, _when_k_cases.ref_when_k on the timeline as it stands, then the
subtraction on the job's nodes.  It shares nothing with the run-length walk of the kernels."""
import functools

import numpy as np

import _when_k_cases as wk
from fitgpu import FIT_ETA_LATER, FIT_ETA_NOW, FIT_REJECTED, synth

REJECT_CODES = (1, 2, 3, 4)  # FIT_ETA_PARTITION, LIMIT_TIME, LIMIT_CPUS, LIMIT_MEM


def ref_place_tl_k(tl, mask, parts, jobs, slot_min, kmax):
    """§2g: (out[J, kmax], start[J], final dense timeline).  tl is not changed."""
    tl = np.array(tl, np.int32, copy=True)
    J = jobs.j
    out = np.full((J, kmax), -1, np.int32)
    start = np.full(J, -1, np.int32)
    for q in range(J):
        one = wk.one_job(jobs, q)
        rows, nodes = wk.ref_when_k(tl, mask, parts, one, slot_min, kmax)
        code = int(rows["code"][0])
        if code in REJECT_CODES:
            out[q, 0] = FIT_REJECTED
        elif code in (FIT_ETA_NOW, FIT_ETA_LATER):
            need, s, d = int(rows["need"][0]), int(rows["start"][0]), int(rows["dur"][0])
            sel = nodes[0, :need]
            assert (sel >= 0).all()
            out[q, :need] = sel
            start[q] = s
            tl[sel, s:s + d] -= np.array([one.cpu[0], one.mem[0], one.gpu[0]], np.int32)[None, None, :]
    return out, start, tl


def alone_starts(tl, mask, parts, jobs, slot_min, kmax):
    """Every job judged alone on tl (fit_when_k's start, -1 if none)."""
    return wk.ref_when_k(tl, mask, parts, jobs, slot_min, kmax)[0]["start"]


# ---- generators ------------------------------------------------------------------------------------
def busy_jobs(j, H, slot_min, kmax, seed):      # contended: the 63/64/65-node components take 90 %
    r = np.random.default_rng(seed)
    cpu = r.choice([2, 4, 8, 16], j).astype(np.int32)
    mem = (cpu.astype(np.int64) * r.choice([512, 1024], j)).astype(np.int32)
    gpu = r.choice([0, 0, 0, 1], j).astype(np.int32)
    wall = r.integers(1, max(H * slot_min // 4, 1) + 1, j).astype(np.int32)
    part = r.choice([1, 2, 3, 4, 0], j, p=[.3, .3, .3, .05, .05]).astype(np.uint16)
    k = r.integers(0, kmax + 1, j).astype(np.uint16)
    return synth.Jobs(cpu, mem, gpu, wall, part, k)


def stairs(n=5, H=256):
    """One partition, cpu_free 0, mem_free 1 << 20, no GPUs, avail INF, slot_min 1; node x releases
    1 cpu at every slot of range(2 + x % 2, H, 2): 128 runs per node at load."""
    nodes = synth.Nodes(cpu_free=np.zeros(n, np.int32), mem_free=np.full(n, 1 << 20, np.int32),
                        gpu_free=np.zeros(n, np.int32), avail_min=np.full(n, wk.INF, np.int32),
                        part_mask=np.ones(n, np.uint32))
    off, slot = [0], []
    for x in range(n):
        slot += list(range(2 + x % 2, H, 2))
        off.append(len(slot))
    m = len(slot)
    tline = synth.Timeline(slots=H, slot_min=1, off=np.array(off, np.int32), slot=np.array(slot, np.int32),
                           cpu=np.ones(m, np.int32), mem=np.zeros(m, np.int32), gpu=np.zeros(m, np.int32))
    return nodes, tline, wk.open_parts(1)


def stair_jobs(j, seed, kmax=4):
    r = np.random.default_rng(seed)
    cpu = r.integers(1, 100, j).astype(np.int32)
    return synth.Jobs(cpu, np.full(j, 1024, np.int32), np.zeros(j, np.int32), r.integers(1, 41, j).astype(np.int32),
                      np.zeros(j, np.uint16), r.integers(1, kmax + 1, j).astype(np.uint16))


def ones(jobs, k=1):
    """The same jobs with nodes_k forced to k."""
    return synth.Jobs(jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.part, np.full(jobs.j, k, np.uint16))


# (H, jobs, kmax) of the busy_jobs cases, seed 5 * H + j + kmax, on wk.rand_cluster(H, 5, 7000 + H)
BUSY = [(8, 200, 3), (64, 300, 8), (1024, 300, 8), (1024, 300, 1)]
# the same of wk.rand_jobs, seed 31 * H + 7 * j + kmax: undeclared partitions, limit rejections, d == H + 1
RAND = [(1, 9, 2), (64, 65, 8), (1024, 120, 8)]
SLOT_MIN = 5


def busy_case(H, j, kmax):
    return busy_jobs(j, H, SLOT_MIN, kmax, 5 * H + j + kmax)


def rand_case(H, j, kmax):
    return wk.rand_jobs(j, H, SLOT_MIN, kmax, 31 * H + 7 * j + kmax)


# ---- the references, computed once and shared by the tests that need them ----------------------------
def pre_jobs(H):
    """test_when_k_gpu's warm-up queue: its reservations give the starting run lists their dips."""
    return wk.rand_jobs(300, H, SLOT_MIN, 1, 99 + H, valid_only=True)


@functools.lru_cache(maxsize=None)
def cluster(H):
    return wk.rand_cluster(H, SLOT_MIN, 7000 + H)


@functools.lru_cache(maxsize=None)
def start_timeline(H):
    """The dense timeline the random cases start from: rand_cluster as loaded, at H >= 64 after a
    fit_place_tl of pre_jobs(H) — by the C oracle here; the GPU tests check the engine's agrees."""
    from oracle import pyoracle as po
    nodes, tline, parts = cluster(H)
    if H >= 64:
        tl = po.ref_place_tl(nodes, tline, pre_jobs(H), parts)[3]
    else:
        tl = po.ref_build_timeline(nodes, tline)
    tl.setflags(write=False)
    return tl


@functools.lru_cache(maxsize=None)
def reference(kind, H, j, kmax):
    """(jobs, out, start, final timeline) of the case on start_timeline(H); kind 'busy' or 'rand'."""
    nodes, tline, parts = cluster(H)
    jobs = (busy_case if kind == "busy" else rand_case)(H, j, kmax)
    out, start, fin = ref_place_tl_k(start_timeline(H), nodes.part_mask, parts, jobs, SLOT_MIN, kmax)
    for a in (out, start, fin):
        a.setflags(write=False)
    return jobs, out, start, fin


@functools.lru_cache(maxsize=None)
def stairs_reference():
    nodes, tline, parts = stairs()
    from oracle import pyoracle as po
    tl0 = po.ref_build_timeline(nodes, tline)
    jobs = stair_jobs(120, 3)
    out, start, fin = ref_place_tl_k(tl0, nodes.part_mask, parts, jobs, tline.slot_min, 4)
    for a in (tl0, out, start, fin):
        a.setflags(write=False)
    return jobs, tl0, out, start, fin


# ---- the hand case -----------------------------------------------------------------------------------
# _when_k_cases.hand_case()'s cluster, kmax 3: H = 8, L = 5, mem 8192 everywhere, no GPUs.
# Partition 0 = n0, n1, n2; partition 1 = n3.  cpus per slot at load:
#   n0: 4 4 4 - - - - -      n1: 0 0 0 4 4 4 4 4      n2: 1 1 1 1 1 8 8 8      n3: 4 everywhere
# q0 (2 cpus, d 2, k 2): S_n0 = {0, 1}, S_n1 = {3..6}, S_n2 = {5, 6}: cnt reaches 2 first at s = 5; n1
#    leaves 2 cpus, n2 6 -> [1, 2] from 5.            n1: 0 0 0 4 4 2 2 4      n2: 1 1 1 1 1 6 6 8
# q1 (the same): S_n1 is still {3..6} (slots 5, 6 hold exactly 2), S_n2 = {5, 6}: 5 again; n1 now leaves
#    0 cpus, n2 4 -> [1, 2].                          n1: 0 0 0 4 4 0 0 4      n2: 1 1 1 1 1 4 4 8
# q2 (the same): alone on the loaded timeline it starts at 5.  Now S_n0 = {0, 1}, S_n1 = {3} (its only
#    window), S_n2 = {5, 6}: no slot has two nodes -> unplaced, nothing consumed.
# q3 (1 cpu, d 1, k 2): slot 0: n0 (4) and n2 (1) hold it, n1 does not: cnt(0) = 2; n2 leaves 0, n0 3
#    -> [2, 0] from 0.                                n0: 3 4 4 - ...          n2: 0 1 1 1 1 4 4 8
# q4 (the same): q3 took n2's last cpu of slot 0, so cnt(0) = 1 (n0); slot 1: n0 and n2 -> [2, 0]
#    from 1.                                          n0: 3 3 4 - ...          n2: 0 0 1 1 1 4 4 8
# q5 (2 cpus, d 2, k 1): n0 holds 3, 3 on slots 0, 1 -> node 0 from 0.       n0: 1 1 4 - ...
# q6: partition 5 of 2 -> FIT_REJECTED.   q7 (partition 1, k 2): one member -> unplaced.
# q8 (5 cpus, d 1, nodes_k 0 = 1): only n2's slot 7 (8 cpus) holds 5 -> node 2 from 7.  n2: 0 0 1 1 1 4 4 3
def hand_case():
    nodes, tline, _, parts = wk.hand_case()
    a, b = (2, 1024, 0, 10, 0, 2), (1, 1024, 0, 5, 0, 2)
    jobs = wk.jobs_of([a, a, a, b, b, (2, 1024, 0, 10, 0, 1), (1, 1024, 0, 5, 5, 1), (2, 1024, 0, 10, 1, 2),
                       (5, 1024, 0, 5, 0, 0)])
    return nodes, tline, jobs, parts


HAND_KMAX = 3
HAND_NODES = np.array([[1, 2, -1], [1, 2, -1], [-1, -1, -1], [2, 0, -1], [2, 0, -1], [0, -1, -1],
                       [FIT_REJECTED, -1, -1], [-1, -1, -1], [2, -1, -1]], np.int32)
HAND_START = np.array([5, 5, -1, 0, 1, 0, -1, -1, 7], np.int32)
HAND_CPU = np.array([[1, 1, 4, -1, -1, -1, -1, -1],
                     [0, 0, 0, 4, 4, 0, 0, 4],
                     [0, 0, 1, 1, 1, 4, 4, 3],
                     [4, 4, 4, 4, 4, 4, 4, 4]], np.int32)
# q0, q1, q3, q4, q5 and q8 are placed, q2 and q7 unplaced, q6 rejected
HAND_STATS = dict(jobs=9, placed=6, unplaced=2, rejected=1, engine=4)

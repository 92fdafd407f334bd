"""Cases and the checker of fit_when_k, shared by tests/test_when_k_gpu.py (not a
test module).  ref_when_k restates §2f in numpy over the dense [n, H, 3] timeline that
Engine.read_timeline returns; it shares nothing with the run-length walk of the kernels."""
import numpy as np

from fitgpu import (ETA_K_DTYPE, FIT_ETA_HORIZON, FIT_ETA_LATER, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM,
                    FIT_ETA_LIMIT_TIME, FIT_ETA_NO_NODES, FIT_ETA_NOW, FIT_ETA_PARTITION, synth)

INF = synth.INT32_MAX
JOB_FIELDS = ("cpu", "mem", "gpu", "wall", "part", "nodes_k")


def ref_when_k(tl, mask, parts, jobs, slot_min, kmax):
    """§2f, every job alone: ok[n, t] = the slot holds the demand (-1 holds nothing); a window of d
    slots that ends at t is feasible when the running count of ok slots ending at t is >= d;
    cnt(s) = members whose window [s, s + d) is feasible; start = the first s with cnt >= need; the
    nodes = the need smallest (score from the window minima minus the demand, node id)."""
    n, H, _ = tl.shape
    P, J = parts.p, jobs.j
    rows = np.zeros(J, ETA_K_DTYPE)
    rows["start"] = rows["wait_min"] = -1
    nodes = np.full((J, kmax), -1, np.int32)
    tl64 = tl.astype(np.int64)
    ids = np.arange(n)
    t = np.arange(H)
    sub_of = {}
    for q in range(J):
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        wall, p = int(jobs.wall[q]), int(jobs.part[q])
        need = max(int(jobs.nodes_k[q]), 1)
        d = max(1, -(-wall // slot_min))
        rows["dur"][q], rows["need"][q] = d, need
        if p >= P:
            rows["code"][q] = FIT_ETA_PARTITION
            continue
        if parts.max_time_min[p] >= 0 and wall > parts.max_time_min[p]:
            rows["code"][q] = FIT_ETA_LIMIT_TIME
            continue
        if parts.max_cpus_per_node[p] >= 0 and dem[0] > parts.max_cpus_per_node[p]:
            rows["code"][q] = FIT_ETA_LIMIT_CPUS
            continue
        if parts.max_mem_per_node[p] >= 0 and dem[1] > parts.max_mem_per_node[p]:
            rows["code"][q] = FIT_ETA_LIMIT_MEM
            continue
        if p not in sub_of:
            mem = ids[((mask.astype(np.int64) >> p) & 1) != 0]
            sub_of[p] = (mem, tl64[mem])
        mem, sub = sub_of[p]                                  # members, [m, H, 3]
        rows["members"][q] = len(mem)
        if len(mem) == 0:
            rows["code"][q] = FIT_ETA_NO_NODES
            continue
        rows["code"][q] = FIT_ETA_HORIZON
        if d > H:
            continue
        ok = (sub >= dem[None, None, :]).all(axis=2)          # [m, H]
        last_bad = np.maximum.accumulate(np.where(ok, -1, t[None, :]), axis=1)
        feas = ((t[None, :] - last_bad) >= d)[:, d - 1:]      # [m, H - d + 1]: feas[:, s] = window [s, s + d)
        cnt = feas.sum(axis=0)
        rows["hosts"][q] = feas.any(axis=1).sum()
        rows["now"][q] = cnt[0]
        hit = np.flatnonzero(cnt >= need)
        if hit.size == 0:
            continue
        s = int(hit[0])
        rows["start"][q], rows["ready"][q] = s, cnt[s]
        rows["wait_min"][q] = min(s * slot_min, INF)
        rows["code"][q] = FIT_ETA_LATER if s > 0 else FIT_ETA_NOW
        sel = feas[:, s]
        wmin = sub[sel, s:s + d].min(axis=1) - dem[None, :]   # [r, 3]
        score = (np.minimum(wmin[:, 2], 255) << 24) | (np.minimum(wmin[:, 0], 4095) << 12) | \
            np.minimum(wmin[:, 1] >> 10, 4095)
        order = np.lexsort((mem[sel], score))[:need]
        nodes[q, :need] = mem[sel][order]
    return rows, nodes


def one_job(jobs, q):
    return synth.Jobs(*(getattr(jobs, f)[q:q + 1] for f in JOB_FIELDS))


def jobs_of(rows):
    """(cpu, mem, gpu, wall, part, k) tuples -> synth.Jobs."""
    a = np.array(rows, np.int64).reshape(-1, 6)
    return synth.Jobs(a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32),
                      a[:, 3].astype(np.int32), a[:, 4].astype(np.uint16), a[:, 5].astype(np.uint16))


def open_parts(p):
    return synth.Partitions(np.full(p, -1, np.int32), np.full(p, -1, np.int32), np.full(p, -1, np.int32))


# ---- 1. the hand case ------------------------------------------------------------------------------
# H = 8, L = 5, mem 8192 everywhere, no GPUs.  Partition 0 = n0, n1, n2; partition 1 = n3.
#   n0: 4 cpus free, avail_min 15: slots 0-2 hold 4, the rest -1
#   n1: 0 cpus free, 4 released at slot 3: slots 3-7 hold 4
#   n2: 1 cpu free, 7 released at slot 5: slots 0-4 hold 1, 5-7 hold 8
#   n3: 4 cpus
# j0 (2 cpus, d 2, k 2): S_n0 = {0, 1}, S_n1 = {3..6}, S_n2 = {5, 6}: cnt reaches 2 first at s = 5
#    (the per-node earliest starts are 0, 3, 5 — their 2nd smallest, 3, is NOT a common start);
#    window minima minus the demand: n1 2 cpus, n2 6 cpus -> [1, 2].
# j1 (k 1): n0 at 0.   j2 (k 3): cnt never reaches 3; cnt(0) = 1.
# j3 (1 cpu, d 1, k 2): S_n0 = {0, 1, 2}, S_n1 = {3..7}, S_n2 = {0..7}: cnt(0) = 2; n2 leaves 0 cpus,
#    n0 3 -> [2, 0].
# j4 (partition 1, k 2): one member.   j5: partition 5 of 2.
def hand_case():
    nodes = synth.Nodes(cpu_free=np.array([4, 0, 1, 4], np.int32), mem_free=np.full(4, 8192, np.int32),
                        gpu_free=np.zeros(4, np.int32), avail_min=np.array([15, INF, INF, INF], np.int32),
                        part_mask=np.array([1, 1, 1, 2], np.uint32))
    tline = synth.Timeline(slots=8, slot_min=5, off=np.array([0, 0, 1, 2, 2], np.int32),
                           slot=np.array([3, 5], np.int32), cpu=np.array([4, 7], np.int32),
                           mem=np.zeros(2, np.int32), gpu=np.zeros(2, np.int32))
    jobs = jobs_of([(2, 1024, 0, 10, 0, 2), (2, 1024, 0, 10, 0, 1), (2, 1024, 0, 10, 0, 3), (1, 1024, 0, 5, 0, 2),
                    (2, 1024, 0, 10, 1, 2), (1, 1024, 0, 5, 5, 1)])
    return nodes, tline, jobs, open_parts(2)


# (code, dur, need, start, wait_min, members, hosts, now, ready, reserved)
HAND_ROWS = np.array([
    (FIT_ETA_LATER, 2, 2, 5, 25, 3, 3, 1, 2, 0),
    (FIT_ETA_NOW, 2, 1, 0, 0, 3, 3, 1, 1, 0),
    (FIT_ETA_HORIZON, 2, 3, -1, -1, 3, 3, 1, 0, 0),
    (FIT_ETA_NOW, 1, 2, 0, 0, 3, 3, 2, 2, 0),
    (FIT_ETA_HORIZON, 2, 2, -1, -1, 1, 1, 1, 0, 0),
    (FIT_ETA_PARTITION, 1, 1, -1, -1, 0, 0, 0, 0, 0),
], ETA_K_DTYPE)
HAND_NODES = np.array([[1, 2, -1], [0, -1, -1], [-1, -1, -1], [2, 0, -1], [-1, -1, -1], [-1, -1, -1]], np.int32)


# ---- 5. edges ----------------------------------------------------------------------------------------
# H = 8, L = 5, mem 8192, no GPUs.  Partition 0 = n0..n7, 4 cpus each; partition 1 = n8, n9:
#   n8: 0 cpus free, 4 released at slot 3: slots 3-7 hold 4 — a stretch that ends at the horizon
#   n9: 0 cpus free, 2 released at slot 2, avail_min 25: slots 2-4 hold 2, slots 5-7 read -1
def edge_case():
    nodes = synth.Nodes(cpu_free=np.array([4] * 8 + [0, 0], np.int32), mem_free=np.full(10, 8192, np.int32),
                        gpu_free=np.zeros(10, np.int32), avail_min=np.array([INF] * 9 + [25], np.int32),
                        part_mask=np.array([1] * 8 + [2, 2], np.uint32))
    off = np.array([0] * 9 + [1, 2], np.int32)
    tline = synth.Timeline(slots=8, slot_min=5, off=off, slot=np.array([3, 2], np.int32),
                           cpu=np.array([4, 2], np.int32), mem=np.zeros(2, np.int32), gpu=np.zeros(2, np.int32))
    jobs = jobs_of([
        (4, 1024, 0, 40, 0, 8),  # e0: k = 8 on exactly 8 members, d == H, need == ready
        (4, 1024, 0, 41, 0, 8),  # e1: d == H + 1
        (5, 1024, 0, 5, 0, 1),   # e2: more than any node ever has
        (0, 0, 0, 0, 1, 2),      # e3: all-zero demand: every slot that is not -1 holds it
        (2, 1024, 0, 25, 1, 1),  # e4: n8's stretch 3-7 is exactly d = 5 long and ends at the horizon
        (2, 1024, 0, 15, 1, 2),  # e5: n8 from {3, 4, 5}, n9 from {2} only: no common start
        (2, 1024, 0, 15, 1, 1),  # e6: n9's only window is its last 3 usable slots
        (2, 1024, 0, 10, 1, 2),  # e7: n8 {3..6}, n9 {2, 3}: common at 3, need == ready; n9 the tighter fit
        (1, 1024, 0, 5, 1, 3),   # e8: need 3 > 2 members
    ])
    return nodes, tline, jobs, open_parts(2)


EDGE_ROWS = np.array([
    (FIT_ETA_NOW, 8, 8, 0, 0, 8, 8, 8, 8, 0),
    (FIT_ETA_HORIZON, 9, 8, -1, -1, 8, 0, 0, 0, 0),
    (FIT_ETA_HORIZON, 1, 1, -1, -1, 8, 0, 0, 0, 0),
    (FIT_ETA_NOW, 1, 2, 0, 0, 2, 2, 2, 2, 0),
    (FIT_ETA_LATER, 5, 1, 3, 15, 2, 1, 0, 1, 0),
    (FIT_ETA_HORIZON, 3, 2, -1, -1, 2, 2, 0, 0, 0),
    (FIT_ETA_LATER, 3, 1, 2, 10, 2, 2, 0, 1, 0),
    (FIT_ETA_LATER, 2, 2, 3, 15, 2, 2, 0, 2, 0),
    (FIT_ETA_HORIZON, 1, 3, -1, -1, 2, 2, 0, 0, 0),
], ETA_K_DTYPE)
EDGE_NODES = np.full((9, 8), -1, np.int32)
EDGE_NODES[0] = np.arange(8)
EDGE_NODES[3, :2] = [8, 9]
EDGE_NODES[4, 0] = 8
EDGE_NODES[6, 0] = 9
EDGE_NODES[7, :2] = [9, 8]


# ---- 2. random timelines -------------------------------------------------------------------------
# Five components of 1, 63, 64, 65 and 600 nodes (partitions 0..4, one partition each, node ids
# interleaved), partition 5 declared without a node, partition 6 not declared.  Partition 0 limits
# the walltime, partition 1 the cpus and the memory.
COMP_SIZES = (1, 63, 64, 65, 600)
RUN_TARGETS = (1, 4, 5, 8, 9, 13)  # TL_HEAD = 4 header runs, four Seg per wait beyond them


def rand_cluster(H, slot_min, seed):
    """synth's node rows with the partition of each node set by hand, and release events that give
    the run lists 1, 4, 5, 8, 9 and 13 runs where the horizon has room for them."""
    n = sum(COMP_SIZES)
    r = np.random.default_rng(seed)
    nodes = synth.gen_nodes(synth.SEEDS["c5"], n, 1)
    nodes.cpu_free //= 8  # 2..32 cpus: the jobs below compete for them, so starts lie in the future too
    nodes.mem_free //= 8
    part = r.permutation(np.repeat(np.arange(len(COMP_SIZES)), COMP_SIZES))
    nodes.part_mask = (np.uint32(1) << part.astype(np.uint32)).astype(np.uint32)
    # avail_min cuts the horizon on a quarter of the nodes (0: never usable)
    nodes.avail_min = np.where(r.random(n) < 0.25, r.integers(0, H * slot_min + 1, n), INF).astype(np.int32)
    off, slot, rc, rm, rg = [0], [], [], [], []
    for x in range(n):
        u = min(int(nodes.avail_min[x]) // slot_min, H)  # usable slots
        tail = 1 if u < H else 0                          # the unusable tail is a run of its own
        want = RUN_TARGETS[x % len(RUN_TARGETS)]
        k = max(0, min(want - 1 - tail, u - 1))            # k releases at distinct slots in [1, u): k + 1 runs
        for s in sorted(r.choice(np.arange(1, max(u, 2)), k, replace=False).tolist() if k else []):
            slot.append(s)
            rc.append(int(r.integers(1, 9)))
            rm.append(int(r.integers(0, 3)) * 4096)
            rg.append(int(r.integers(0, 2)))
        off.append(len(slot))
    a = lambda v: np.array(v, np.int32)  # noqa: E731
    tline = synth.Timeline(slots=H, slot_min=slot_min, off=a(off), slot=a(slot), cpu=a(rc), mem=a(rm), gpu=a(rg))
    parts = synth.Partitions(np.array([H * slot_min // 2 + 1, -1, -1, -1, -1, -1], np.int32),
                             np.array([-1, 48, -1, -1, -1, -1], np.int32),
                             np.array([-1, 100000, -1, -1, -1, -1], np.int32))
    return nodes, tline, parts


def rand_jobs(j, H, slot_min, kmax, seed, valid_only=False):
    """Demands around rand_cluster's node sizes, walls of 0, one slot,
    d == H, d == H + 1 and anything between, nodes_k mixed in 0..kmax."""
    r = np.random.default_rng(seed)
    cpu = r.choice([0, 1, 2, 4, 8, 16, 32, 64, 300], j).astype(np.int32)
    mem = (np.maximum(cpu, 1).astype(np.int64) * r.choice([512, 1024, 4096], j)).astype(np.int32)
    gpu = r.choice([0, 0, 0, 1, 2, 4], j).astype(np.int32)
    wall = r.choice([0, 1, slot_min, H * slot_min, H * slot_min + 1, -1, -1, -1], j)
    short = r.integers(0, max(H * slot_min // 4, 1) + 1, j)
    wall = np.where(wall < 0, short, wall).astype(np.int32)
    part = r.integers(0, 5 if valid_only else 7, j).astype(np.uint16)
    # the large component takes half of the jobs: that is where k nodes at once are found
    part = np.where(r.random(j) < 0.5, 4, part).astype(np.uint16)
    k = r.integers(0, kmax + 1, j).astype(np.uint16)
    if valid_only:
        cpu = np.minimum(cpu, 16)
        wall = np.minimum(wall, H * slot_min // 2)
        k[:] = 1
    return synth.Jobs(cpu, mem, gpu, wall, part, k)


def run_counts(dense):
    return 1 + (dense[:, 1:, :] != dense[:, :-1, :]).any(axis=2).sum(axis=1)

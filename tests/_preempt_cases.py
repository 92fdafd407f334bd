"""fit_preempt's reference and inputs (not a test module): ref_preempt, a numpy int64 restatement of
DESIGN.md §2l over the raw columns — never taken from the engine — the packed generator and a
hand-written case with literal rows."""
import functools
from dataclasses import dataclass

import numpy as np

from fitgpu import EVICT_DTYPE, synth

INF = synth.INT32_MAX
I32MIN = -2**31
FITS, PARTITION, LIMIT_TIME, LIMIT_CPUS, LIMIT_MEM, NO_NODES, EVICT, NONE = range(8)


@dataclass
class Case:
    nodes: synth.Nodes
    victims: synth.Victims  # or None
    parts: synth.Partitions
    jobs: synth.Jobs
    prio: np.ndarray


def score(dc, dm, dg):
    """DESIGN.md §2's score of a residual, int64 in and out."""
    return (np.minimum(dg, 255) << 24) | (np.minimum(dc, 4095) << 12) | np.minimum(dm >> 10, 4095)


def ref_preempt(nodes, victims, parts, jobs, prio, stats=None, free=None):
    """Every job alone: the victim columns padded to the longest list, a cumulative sum, a
    first-true search per (job, node).  free: the current free columns (read_nodes()), default the
    loaded ones.  stats: a dict that collects, over the EVICT rows, how many tie at each level of the
    key, how many winners are not a fewest-victims node, and the entries a lane walks."""
    N, J, P = nodes.n, jobs.j, parts.p
    fc, fm, fg = (np.asarray(c, np.int64) for c in (free if free is not None else
                                                     (nodes.cpu_free, nodes.mem_free, nodes.gpu_free)))
    avail, mask = nodes.avail_min.astype(np.int64), nodes.part_mask.astype(np.int64)
    off = np.zeros(N + 1, np.int64) if victims is None else victims.off.astype(np.int64)
    ln = np.diff(off)
    W = int(ln.max()) if N else 0
    vp = np.full((N, W), np.iinfo(np.int64).max)  # the padding is outranked by no job
    S = np.zeros((N, W + 1, 3), np.int64)         # S[n, v, c]: column c over the first v entries
    if W:
        col = np.arange(W)[None, :]
        inside = col < ln[:, None]
        src = np.minimum(off[:-1, None] + col, max(len(victims.prio) - 1, 0))
        vp[inside] = victims.prio.astype(np.int64)[src][inside]
        amounts = np.stack([np.where(inside, np.asarray(a, np.int64)[src], 0) for a in (victims.cpu, victims.mem, victims.gpu)],
                           axis=2)
        S[:, 1:, :] = np.cumsum(amounts, axis=1)
    ar = np.arange(W + 1)[None, :]
    open_ = (fc >= 0) & (fm >= 0) & (fg >= 0)
    out = np.zeros(J, EVICT_DTYPE)
    out["node"] = -1
    for q in range(J):
        c, m, g, w, p, pr = (int(x[q]) for x in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.part, prio))
        if p >= P:
            out["code"][q] = PARTITION
        elif 0 <= parts.max_time_min[p] < w:
            out["code"][q] = LIMIT_TIME
        elif 0 <= parts.max_cpus_per_node[p] < c:
            out["code"][q] = LIMIT_CPUS
        elif 0 <= parts.max_mem_per_node[p] < m:
            out["code"][q] = LIMIT_MEM
        if out["code"][q]:
            continue
        member = ((mask >> p) & 1) != 0
        elig = member & (avail >= w) & open_
        ok = ((fc[:, None] + S[:, :, 0] >= c) & (fm[:, None] + S[:, :, 1] >= m) & (fg[:, None] + S[:, :, 2] >= g)
              & elig[:, None])
        L = (vp < pr).sum(1)  # the lists are sorted: the entries below the job's priority are a prefix
        low = ok & (ar <= L[:, None])
        has = low.any(1)
        v = np.where(has, low.argmax(1), -1)
        fit, able = has & (v == 0), has & (v >= 1)
        outranked = elig & ~has & (ok & (ar > L[:, None]) & (ar <= ln[:, None])).any(1)
        r = out[q]
        r["members"], r["fit"], r["able"], r["outranked"] = member.sum(), fit.sum(), able.sum(), outranked.sum()
        if stats is not None:  # a lane looks when it is short and the whole list would do; it stops at v or at entry L + 1
            looks = elig & ~fit & ok[np.arange(N), ln]
            stats["pairs"] = stats.get("pairs", 0) + int(member.sum())
            stats["walked"] = stats.get("walked", 0) + int(np.where(has, v, L + 1)[looks].sum())
        if r["members"] == 0:
            r["code"] = NO_NODES
        elif r["fit"] > 0:
            idx = np.flatnonzero(fit)
            sc = score(fc[idx] - c, fm[idx] - m, fg[idx] - g)
            r["code"], r["node"] = FITS, idx[np.lexsort((idx, sc))[0]]
        elif r["able"] > 0:
            idx = np.flatnonzero(able)
            vv = v[idx]
            top = vp[idx, vv - 1]
            res = [np.minimum(f[idx] + S[idx, vv, k], INF) - d for k, (f, d) in enumerate(((fc, c), (fm, m), (fg, g)))]
            sc = score(*res)
            best = np.lexsort((idx, sc, vv, top))[0]
            r["code"], r["node"], r["victims"], r["top_prio"] = EVICT, idx[best], vv[best], top[best]
            if stats is not None:
                t1 = top == top[best]
                t2 = t1 & (vv == vv[best])
                t3 = t2 & (sc == sc[best])
                for name, t in (("tie_top", t1), ("tie_top_v", t2), ("tie_top_v_score", t3)):
                    stats[name] = stats.get(name, 0) + int(t.sum() > 1)
                stats["not_fewest"] = stats.get("not_fewest", 0) + int(vv[best] > vv.min())
        else:
            r["code"] = NONE
    return out


def rich_enough(want, stats):
    """What every random case must hold on the REFERENCE's output, so that a comparison of nothing
    interesting fails."""
    assert (want["code"] == EVICT).sum() >= 20, np.unique(want["code"], return_counts=True)
    assert (want["code"] == NONE).any() and (want["outranked"] > 0).any()
    assert stats["tie_top"] > 0 and stats["tie_top_v"] > 0 and stats["tie_top_v_score"] > 0, stats
    assert stats["not_fewest"] > 0, stats


# ---- the packed generator -----------------------------------------------------------------------
# 5 partitions are declared: 0 limits the walltime, 1 the cpus, 2 the memory, 3 nothing, 4 has no
# node; jobs also name 5 and 6 (>= P).  Nodes sit in one partition of 0..3, 20 % also in its
# neighbour (two components of two partitions each), 5 % in none.  one_component: every node in
# partition 3, 20 % also in 2.
PARTS = synth.Partitions(np.array([500, -1, -1, -1, -1], np.int32), np.array([-1, 16, -1, -1, -1], np.int32),
                         np.array([-1, -1, 30000, -1, -1], np.int32))


@functools.lru_cache(maxsize=None)
def packed_case(n, j, seed=0, one_component=False):
    """Nodes of 16..128 cpus packed with victims of 4..64 cpus (synth.pack_victims) until no cpu is
    free: one to a dozen per node, so the lowest priority on a node varies.  About 2 % of the nodes
    stay empty — above 257 nodes about five of them, or every job would fit somewhere and no row would
    say EVICT.  On half of the nodes the priorities rise with the victims' size.  10 % of the nodes
    are copies of their left neighbour, victims included: full-key ties, the node id decides.  Then
    3 % get a negative column; 20 % have a finite avail_min.  Victim priorities from {-5, 0, 10, 10,
    100, 1000}, job priorities from {0, 10, 11, 100, 1001}.  Cached: the arrays are shared among the
    tests and never written."""
    r = np.random.default_rng(1000003 * n + 101 * j + seed)
    p = np.full(n, 3) if one_component else r.integers(0, 4, n)
    mask = (1 << p).astype(np.uint32)
    two = r.random(n) < 0.2
    mask[two] |= (1 << (p ^ 1)).astype(np.uint32)[two]
    mask[r.random(n) < 0.05] = 0
    cpu = r.choice([16, 32, 64, 128], n).astype(np.int32)
    mem = (cpu.astype(np.int64) * r.choice([2048, 4096], n)).astype(np.int32)
    gpu = r.choice([0, 0, 4, 8], n).astype(np.int32)
    avail = np.where(r.random(n) < 0.2, r.integers(0, 3000, n), INF).astype(np.int32)
    nodes, victims = synth.pack_victims(0x5EED0700 + seed, synth.Nodes(cpu, mem, gpu, avail, mask),
                                        cpus=[4, 8, 16, 32, 64], empty_pm=20 if n <= 257 else max(1, 5000 // n))
    lists = [list(zip(*(a[victims.off[x]:victims.off[x + 1]].tolist() for a in (victims.prio, victims.cpu, victims.mem,
                                                                                 victims.gpu)))) for x in range(n)]
    # on half of the nodes the smaller a victim, the lower its priority (filler jobs): a node of many
    # small low-priority victims then beats a node of one large high-priority victim
    for x in np.flatnonzero(r.random(n) < 0.5):
        amounts = sorted((e[1:] for e in lists[x]), key=lambda a: a[0])
        lists[x] = [(e[0], *a) for e, a in zip(lists[x], amounts)]
    for x in np.flatnonzero(r.random(n) < 0.1):
        if x > 0:
            for col in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask):
                col[x] = col[x - 1]
            lists[x] = lists[x - 1]
    victims = victims_of(lists)
    neg = r.random(n) < 0.03
    if n >= 8:
        neg[n // 2] = True  # at least one, whatever the draw
    for k in np.flatnonzero(neg):
        (nodes.cpu_free, nodes.mem_free, nodes.gpu_free)[r.integers(0, 3)][k] = -r.integers(1, 50)
    # 64 and 100 take several victims on every node that can hold them; 200 is more than any node holds
    jc = r.choice([1, 4, 8, 16, 32, 64, 100, 200], j).astype(np.int32)
    jm = (jc.astype(np.int64) * r.choice([0, 500, 1024, 4096], j)).astype(np.int32)
    jg = r.choice([0, 0, 0, 1, 2, 4], j).astype(np.int32)
    wall = r.choice([0, 60, 240, 600, 2000], j).astype(np.int32)
    part = r.choice([0, 1, 2, 3, 0, 1, 2, 3, 3, 3, 4, 5, 6], j).astype(np.uint16)
    jobs = synth.Jobs(jc, jm, jg, wall, part, np.ones(j, np.uint16))
    return Case(nodes, victims, PARTS, jobs, r.choice(synth.JOB_PRIO, j).astype(np.int32))


@functools.lru_cache(maxsize=None)
def packed_ref(n, j, seed=0, one_component=False):
    """(rows, stats) of packed_case, computed once."""
    c = packed_case(n, j, seed, one_component)
    stats = {}
    return ref_preempt(c.nodes, c.victims, c.parts, c.jobs, c.prio, stats), stats


# ---- the hand-written case ----------------------------------------------------------------------
def victims_of(lists):
    """synth.Victims from per-node lists of (prio, cpu, mem, gpu)."""
    off = np.cumsum([0] + [len(v) for v in lists]).astype(np.int32)
    flat = np.array([e for v in lists for e in v], np.int64).reshape(-1, 4)
    return synth.Victims(off, *(flat[:, k].astype(np.int32) for k in range(4)))


def hand_case():
    """6 nodes, 13 jobs, every code.  Partition 0 limits time 100, cpus 8, mem 10000; 1 nothing; 2 has
    no node.  The rows of HAND_ROWS are worked out by hand from DESIGN.md §2l."""
    parts = synth.Partitions(np.array([100, -1, -1], np.int32), np.array([8, -1, -1], np.int32),
                             np.array([10000, -1, -1], np.int32))
    nodes = synth.Nodes(np.array([2, 0, 0, 8, -1, 2], np.int32), np.array([8192, 4096, 0, 16384, 4096, 2048], np.int32),
                        np.array([0, 0, 0, 2, 0, 1], np.int32), np.array([INF, INF, INF, 50, INF, INF], np.int32),
                        np.array([1, 1, 1, 1, 1, 2], np.uint32))
    victims = victims_of([[(1, 2, 1024, 0), (5, 2, 1024, 0)], [(6, 6, 2048, 0)],
                          [(3, 2, 2048, 0), (3, 2, 2048, 0), (9, 8, 8192, 1)], [], [(0, 64, 65536, 0)], [(7, 6, 6144, 1)]])
    #        cpu   mem  gpu wall part prio
    rows = [(2, 1024, 0, 10, 0, 5), (6, 2048, 0, 60, 0, 5), (8, 8192, 0, 60, 0, 10), (4, 2048, 0, 60, 0, 4),
            (6, 4096, 0, 60, 0, 7), (1, 1, 0, 101, 0, 0), (9, 1, 0, 10, 0, 0), (1, 10001, 0, 10, 0, 0),
            (1, 1, 0, 10, 3, 0), (1, 1, 0, 10, 2, 0), (1, 1024, 1, 10, 1, 8), (8, 8192, 2, 10, 1, 8),
            (0, 0, 0, 60, 0, I32MIN)]
    a = np.array(rows, np.int64)
    jobs = synth.Jobs(*(a[:, k].astype(np.int32) for k in range(4)), a[:, 4].astype(np.uint16), np.ones(len(a), np.uint16))
    return Case(nodes, victims, parts, jobs, a[:, 5].astype(np.int32))


# code, node, victims, top_prio, members, fit, able, outranked
HAND_ROWS = [
    (FITS, 0, 0, 0, 5, 2, 1, 1),         # nodes 0 and 3 fit, node 0 the tighter; 2 needs one victim; 1 is held at 6 >= 5
    (NONE, -1, 0, 0, 5, 0, 0, 3),        # every list would do, but each stops at an entry >= 5 first
    (EVICT, 2, 3, 9, 5, 0, 1, 0),        # only node 2's whole list frees 8 cpus
    (EVICT, 0, 1, 1, 5, 0, 2, 1),        # node 0 (top 1) before node 2 (top 3, two victims); node 1 outranks
    (EVICT, 0, 2, 5, 5, 0, 2, 1),        # node 0 with TWO victims (top 5) before node 1 with one (top 6)
    (LIMIT_TIME, -1, 0, 0, 0, 0, 0, 0),
    (LIMIT_CPUS, -1, 0, 0, 0, 0, 0, 0),
    (LIMIT_MEM, -1, 0, 0, 0, 0, 0, 0),
    (PARTITION, -1, 0, 0, 0, 0, 0, 0),
    (NO_NODES, -1, 0, 0, 0, 0, 0, 0),
    (FITS, 5, 0, 0, 1, 1, 0, 0),
    (EVICT, 5, 1, 7, 1, 0, 1, 0),
    (FITS, 2, 0, 0, 5, 3, 0, 0),         # the all-zero demand at INT32_MIN: nodes 0, 1, 2 fit (3: walltime, 4: closed)
]

"""fit_preempt_tl's reference and inputs (not a test module): ref_preempt_tl, a numpy int64 restatement
of DESIGN.md §2n on the DENSE [n, H, 3] timeline — a cumulative sum over a node's entries of
amount x (t < end), an all-over-the-window test per prefix, first true; it shares nothing with the
run walk — the packed generator with ends, release events and a queue whose reservations dent the
timeline, and a hand-written case with literal rows."""
import functools
from dataclasses import dataclass

import numpy as np

import _preempt_cases as pc
from fitgpu import EVICT_DTYPE, synth
from _preempt_cases import EVICT, FITS, LIMIT_CPUS, LIMIT_MEM, LIMIT_TIME, NO_NODES, NONE, PARTITION  # noqa: F401

INF, I32MIN = pc.INF, pc.I32MIN


@dataclass
class CaseTL:
    nodes: synth.Nodes
    victims: synth.VictimsTL  # or None
    tline: synth.Timeline     # the release events the timeline is loaded from
    queue: synth.Jobs         # placed with place_tl (or held, hand case) before the query: the reservations
    parts: synth.Partitions
    jobs: synth.Jobs
    prio: np.ndarray


def dur(wall, slot_min):
    """d of §2b: max(1, ceil(wall / slot_min))."""
    return max(1, -(-int(wall) // int(slot_min)))


def victim_tables(n, victims, H, shift=0):
    """Per node, padded to the longest list: priorities vp [n, W] (the padding is outranked by no
    job), list lengths ln [n], and cum [n, W + 1, H, 3]: column c freed at slot t by the first v
    entries, every end read as max(end - shift, 0)."""
    off = np.zeros(n + 1, np.int64) if victims is None else victims.off.astype(np.int64)
    ln = np.diff(off)
    W = int(ln.max()) if n else 0
    vp = np.full((n, W), np.iinfo(np.int64).max)
    cum = np.zeros((n, W + 1, H, 3), np.int64)
    if W:
        col = np.arange(W)[None, :]
        inside = col < ln[:, None]
        src = np.minimum(off[:-1, None] + col, max(len(victims.prio) - 1, 0))
        vp[inside] = victims.prio.astype(np.int64)[src][inside]
        end = np.where(inside, np.maximum(victims.end.astype(np.int64)[src] - shift, 0), 0)
        live = np.arange(H)[None, None, :] < end[:, :, None]  # [n, W, H]: the entry still holds at slot t
        amounts = np.stack([np.where(inside, np.asarray(a, np.int64)[src], 0) for a in (victims.cpu, victims.mem, victims.gpu)],
                           axis=2)  # [n, W, 3]
        cum[:, 1:] = np.cumsum(amounts[:, :, None, :] * live[:, :, :, None], axis=1)
    return vp, ln, cum


def ref_preempt_tl(mask, T, victims, parts, jobs, prio, slot_min, shift=0, stats=None):
    """Every job alone on the dense timeline T [n, H, 3] (read_timeline()): rows of EVICT_DTYPE.
    stats: a dict that collects, over the EVICT rows, how many tie at each level of the key and in how
    many some able node's v differs from the slot-0 rule's (fit_preempt's rule on slot 0 alone)."""
    T = np.asarray(T, np.int64)
    N, H = T.shape[0], T.shape[1]
    J, P = jobs.j, parts.p
    mask = np.asarray(mask).astype(np.int64)
    vp, ln, cum = victim_tables(N, victims, H, shift)
    ar = np.arange(cum.shape[1])[None, :]
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
        dem = np.array([c, m, g], np.int64)
        d = dur(w, slot_min)
        member = ((mask >> p) & 1) != 0
        dd = min(d, H)
        win = T[:, :dd, :]                                   # [n, dd, 3]
        elig = member & (win >= 0).all(axis=(1, 2)) & (d <= H)
        tot = win[:, None, :, :] + cum[:, :, :dd, :]         # [n, W + 1, dd, 3]
        ok = (tot >= dem).all(axis=(2, 3)) & elig[:, None]   # [n, W + 1]
        L = (vp < pr).sum(1)
        low = ok & (ar <= L[:, None])
        has = low.any(1)
        v = np.where(has, low.argmax(1), -1)
        fit, able = has & (v == 0), has & (v >= 1)
        outranked = elig & ~has & (ok & (ar > L[:, None]) & (ar <= ln[:, None])).any(1)
        r = out[q]
        r["members"], r["fit"], r["able"], r["outranked"] = member.sum(), fit.sum(), able.sum(), outranked.sum()
        if r["members"] == 0:
            r["code"] = NO_NODES
        elif r["fit"] > 0:
            idx = np.flatnonzero(fit)
            res = win[idx].min(axis=1) - dem
            sc = pc.score(res[:, 0], res[:, 1], res[:, 2])
            r["code"], r["node"] = FITS, idx[np.lexsort((idx, sc))[0]]
        elif r["able"] > 0:
            idx = np.flatnonzero(able)
            vv = v[idx]
            top = vp[idx, vv - 1]
            res = np.minimum(tot[idx, vv], INF).min(axis=1) - dem  # [k, 3]
            sc = pc.score(res[:, 0], res[:, 1], res[:, 2])
            best = np.lexsort((idx, sc, vv, top))[0]
            r["code"], r["node"], r["victims"], r["top_prio"] = EVICT, idx[best], vv[best], top[best]
            if stats is not None:
                t1 = top == top[best]
                t2 = t1 & (vv == vv[best])
                t3 = t2 & (sc == sc[best])
                for name, t in (("tie_top", t1), ("tie_top_v", t2), ("tie_top_v_score", t3)):
                    stats[name] = stats.get(name, 0) + int(t.sum() > 1)
                ok0 = (tot[:, :, 0, :] >= dem).all(axis=2) & (ar <= L[:, None])  # the slot-0 rule
                v0 = ok0.argmax(1)
                stats["slot0_differs"] = stats.get("slot0_differs", 0) + int((v0[idx] != vv).any())
        else:
            r["code"] = NONE
    return out


def rich_enough(want, stats):
    """What every random case must hold on the REFERENCE's output, so that a comparison of nothing
    interesting fails."""
    assert (want["code"] == EVICT).sum() >= 20, np.unique(want["code"], return_counts=True)
    assert (want["code"] == NONE).any() and (want["outranked"] > 0).any()
    assert stats["tie_top"] > 0 and stats["tie_top_v"] > 0 and stats["tie_top_v_score"] > 0, stats
    assert stats["slot0_differs"] >= 3, stats


# ---- the packed generator -----------------------------------------------------------------------
H, SLOT_MIN = 64, 30
ENDS = (1, 2, 3, 8, 20, H, H)
# the seed of packed_tl_case for which the reference holds rich_enough, per shape (tests/test_preempt_tl.py
# asserts it on the CPU); a shape that is not listed takes seed 0 and is not asked to be rich
SEEDS = {(65, 65): 0, (257, 128): 0, (257, 257): 0}


@functools.lru_cache(maxsize=None)
def packed_tl_case(n, j, seed=None, one_component=False):
    """tests/_preempt_cases.packed_case's cluster, victims, partitions, jobs and priorities.  The
    victims get ends from ENDS (synth.gen_victim_ends), the timeline is loaded from their release
    events over H slots of SLOT_MIN minutes, and a queue of 2n jobs of 4..32 cpus and 2..20 slots is
    there to be placed with place_tl: the cluster is packed, so they reserve the slots behind the
    victims' ends — the dips a victim that ends early does not fill.  The jobs' walls {0, 60, 240, 600,
    2000} are windows of 1, 2, 8, 20 and 67 > H slots.  Cached and never written."""
    seed = SEEDS.get((n, j), 0) if seed is None else seed
    c = pc.packed_case(n, j, seed, one_component)
    vt, tline = synth.gen_victim_ends(0x7E0D + seed, c.victims, H, SLOT_MIN, ENDS)
    r = np.random.default_rng(7919 * n + 31 * j + seed)
    jq = 2 * n
    qc = r.choice([4, 8, 16, 32], jq).astype(np.int32)
    queue = synth.Jobs(qc, (qc.astype(np.int64) * r.choice([512, 1024, 2048], jq)).astype(np.int32),
                       r.choice([0, 0, 0, 1], jq).astype(np.int32), r.choice([60, 150, 300, 600], jq).astype(np.int32),
                       r.choice([0, 1, 2, 3], jq).astype(np.uint16), np.ones(jq, np.uint16))
    return CaseTL(c.nodes, vt, tline, queue, c.parts, c.jobs, c.prio)


def oracle_timeline(c):
    """The dense timeline after the queue's backfill, from the CPU oracle (bit-exact with place_tl,
    which the suite checks elsewhere); rows of nodes in no partition read -1, as read_timeline()'s."""
    from oracle import pyoracle as po
    T = po.ref_place_tl(c.nodes, c.tline, c.queue, c.parts)[3]
    T[c.nodes.part_mask == 0] = -1
    return T


@functools.lru_cache(maxsize=None)
def packed_tl_ref(n, j, seed=None, one_component=False):
    """(rows, stats, timeline) of packed_tl_case on the oracle's timeline, computed once."""
    c = packed_tl_case(n, j, seed, one_component)
    T = oracle_timeline(c)
    stats = {}
    return ref_preempt_tl(c.nodes.part_mask, T, c.victims, c.parts, c.jobs, c.prio, SLOT_MIN, 0, stats), stats, T


# ---- the hand-written case ----------------------------------------------------------------------
def victims_tl_of(lists):
    """synth.VictimsTL from per-node lists of (prio, end, cpu, mem, gpu)."""
    off = np.cumsum([0] + [len(v) for v in lists]).astype(np.int32)
    flat = np.array([e for v in lists for e in v], np.int64).reshape(-1, 5)
    return synth.VictimsTL(off, *(flat[:, k].astype(np.int32) for k in range(5)))


def jobs_of(rows):
    """synth.Jobs and priorities from (cpu, mem, gpu, wall, part, prio) rows."""
    a = np.array(rows, np.int64).reshape(-1, 6)
    return (synth.Jobs(*(a[:, k].astype(np.int32) for k in range(4)), a[:, 4].astype(np.uint16), np.ones(len(a), np.uint16)),
            a[:, 5].astype(np.int32))


HAND_H, HAND_SLOT_MIN = 8, 10
# the reservations of the hand case, held with hold_tl: (cpu, mem, gpu, wall) on node at start
HAND_HOLDS = [((4, 0, 0, 30), 0, 3), ((8, 0, 0, 40), 1, 2)]


def hand_case():
    """6 nodes of 4096 MiB, 14 jobs, every code; 8 slots of 10 minutes.  Partition 0 limits time 70,
    cpus 8, mem 10000; 1 nothing; 2 has no node.  cpus over the slots, after the two reservations:
      node 0  0 0 0 0 0 0 4 4   A (prio 1, 4 cpus) ends at 3 and B (prio 2, 4 cpus) at 8; A's cpus are reserved on [3, 6)
      node 1  0 0 0 0 0 0 8 8   C (prio 1, 8 cpus) ends at 2; its cpus are reserved on [2, 6)
      node 2  0 0 0 0 0 0 0 0   D (prio 0, 4 cpus) has end 0, E (prio 3, 4 cpus) ends at 8
      node 3  8 8 8 8 8 8 - -   partition 1 only; avail_min 60 closes slots 6 and 7
      node 4  - - - - - - - -   a negative cpu column
      node 5  0 0 0 0 0 0 0 0   F (prio 9, 8 cpus) ends at 8
    The rows of HAND_ROWS are worked out by hand from DESIGN.md §2n."""
    parts = synth.Partitions(np.array([70, -1, -1], np.int32), np.array([8, -1, -1], np.int32),
                             np.array([10000, -1, -1], np.int32))
    nodes = synth.Nodes(np.array([0, 0, 0, 8, -1, 0], np.int32), np.full(6, 4096, np.int32), np.zeros(6, np.int32),
                        np.array([INF, INF, INF, 60, INF, INF], np.int32), np.array([1, 1, 1, 2, 1, 1], np.uint32))
    victims = victims_tl_of([[(1, 3, 4, 0, 0), (2, 8, 4, 0, 0)], [(1, 2, 8, 0, 0)], [(0, 0, 4, 0, 0), (3, 8, 4, 0, 0)], [], [],
                             [(9, 8, 8, 0, 0)]])
    tline = synth.Timeline(HAND_H, HAND_SLOT_MIN, np.array([0, 1, 2, 2, 2, 2, 2], np.int32), np.array([3, 2], np.int32),
                           np.array([4, 8], np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32))
    h = np.array([d for d, _, _ in HAND_HOLDS], np.int64)
    queue = synth.Jobs(*(h[:, k].astype(np.int32) for k in range(4)), np.zeros(len(h), np.uint16), np.ones(len(h), np.uint16))
    #        cpu   mem  gpu wall part prio
    rows = [(4, 0, 0, 50, 0, 5), (4, 0, 0, 20, 0, 5), (8, 0, 0, 20, 0, 5), (8, 0, 0, 50, 0, 5), (4, 0, 0, 50, 0, 2),
            (1, 1, 0, 71, 0, 0), (9, 1, 0, 10, 0, 0), (1, 10001, 0, 10, 0, 0), (1, 1, 0, 10, 3, 0), (1, 1, 0, 10, 2, 0),
            (8, 1024, 0, 50, 1, 0), (8, 0, 0, 70, 1, 9), (0, 0, 0, 50, 0, I32MIN), (1, 0, 0, 90, 1, 5)]
    jobs, prio = jobs_of(rows)
    return CaseTL(nodes, victims, tline, queue, parts, jobs, prio)


def hand_timeline():
    """The hand case's dense timeline: the oracle's build from the release events, minus the holds."""
    from oracle import pyoracle as po
    c = hand_case()
    T = po.ref_build_timeline(c.nodes, c.tline)
    for (cpu, mem, gpu, wall), x, s in HAND_HOLDS:
        T[x, s:s + dur(wall, HAND_SLOT_MIN)] -= np.array([cpu, mem, gpu], np.int32)
    return T


HAND_CPUS = [[0, 0, 0, 0, 0, 0, 4, 4], [0, 0, 0, 0, 0, 0, 8, 8], [0] * 8, [8] * 6 + [-1] * 2, [-1] * 8, [0] * 8]

# code, node, victims, top_prio, members, fit, able, outranked
HAND_ROWS = [
    (EVICT, 0, 2, 2, 5, 0, 2, 1),        # 5 slots: A has ended at the dip [3, 5), so node 0 takes B too (slot 0 alone: v = 1);
                                         # node 2 takes D (frees nothing) and E (top 3); node 1: C ended, nothing frees it; 5 outranks
    (EVICT, 0, 1, 1, 5, 0, 3, 1),        # 2 slots, before the dips: A frees node 0, C node 1 (4 cpus to spare: the looser fit)
    (EVICT, 1, 1, 1, 5, 0, 2, 1),        # 8 cpus on 2 slots: C alone (top 1) before A and B (top 2); node 2's list holds 4
    (NONE, -1, 0, 0, 5, 0, 0, 1),        # 8 cpus on 5 slots: at the dip only B counts on node 0; F would do but outranks
    (NONE, -1, 0, 0, 5, 0, 0, 3),        # priority 2: B, E and F are not below it
    (LIMIT_TIME, -1, 0, 0, 0, 0, 0, 0),
    (LIMIT_CPUS, -1, 0, 0, 0, 0, 0, 0),
    (LIMIT_MEM, -1, 0, 0, 0, 0, 0, 0),
    (PARTITION, -1, 0, 0, 0, 0, 0, 0),
    (NO_NODES, -1, 0, 0, 0, 0, 0, 0),
    (FITS, 3, 0, 0, 1, 1, 0, 0),         # node 3 is open and free on [0, 5)
    (NONE, -1, 0, 0, 1, 0, 0, 0),        # 7 slots reach the closed slot 6: not eligible
    (FITS, 0, 0, 0, 5, 4, 0, 0),         # the all-zero demand at INT32_MIN: every open member fits, the lowest id wins
    (NONE, -1, 0, 0, 1, 0, 0, 0),        # 9 slots > H
]

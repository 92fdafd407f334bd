"""fit_preempt_tl_k's reference and inputs (not a test module): ref_preempt_tl_k, a numpy int64
restatement of DESIGN.md §2o on the DENSE [n, H, 3] timeline — _preempt_tl_cases.victim_tables'
cumulative sums, per prefix a test over the whole window, first true, then a lexsort on (top, v,
score, node id) and its first `need`; it shares nothing with the run walk and takes nothing from the
engine — the packed cases on two timelines (the full and the short queue) with a nodes_k column and
the conditions they must hold, and a hand-written case with literal rows."""
import functools

import numpy as np

import _preempt_cases as pc
import _preempt_tl_cases as tc
from _preempt_cases import EVICT, FITS, LIMIT_CPUS, LIMIT_MEM, LIMIT_TIME, NO_NODES, NONE, PARTITION  # noqa: F401
from _preempt_k_cases import K_DRAW, KMAX, NO_TOP, with_k  # noqa: F401
from fitgpu import EVICT_K_DTYPE, synth

INF, I32MIN = pc.INF, pc.I32MIN


def ref_preempt_tl_k(mask, T, victims, parts, jobs, prio, slot_min, kmax, shift=0, stats=None):
    """Every job alone on the dense timeline T [n, H, 3] (read_timeline()), every end read as
    max(end - shift, 0): (rows of EVICT_K_DTYPE, out_node[J, kmax], out_victims[J, kmax]).
    jobs.nodes_k None: every need is 1.  stats: a dict that counts, over the EVICT rows, what the
    richness conditions ask for."""
    T = np.asarray(T, np.int64)
    N, H = T.shape[0], T.shape[1]
    J, P = jobs.j, parts.p
    mask = np.asarray(mask).astype(np.int64)
    vp, ln, cum = tc.victim_tables(N, victims, H, shift)
    W = cum.shape[1] - 1
    ar = np.arange(W + 1)[None, :]
    nk = np.ones(J, np.int64) if jobs.nodes_k is None else np.asarray(jobs.nodes_k, np.int64)
    out = np.zeros(J, EVICT_K_DTYPE)
    out_node = np.full((J, kmax), -1, np.int32)
    out_vic = np.zeros((J, kmax), np.int32)
    for q in range(J):
        c, m, g, w, p, pr = (int(x[q]) for x in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.part, prio))
        r = out[q]
        need = r["need"] = max(int(nk[q]), 1)
        assert need <= kmax
        if p >= P:
            r["code"] = PARTITION
        elif 0 <= parts.max_time_min[p] < w:
            r["code"] = LIMIT_TIME
        elif 0 <= parts.max_cpus_per_node[p] < c:
            r["code"] = LIMIT_CPUS
        elif 0 <= parts.max_mem_per_node[p] < m:
            r["code"] = LIMIT_MEM
        if r["code"]:
            continue
        dem = np.array([c, m, g], np.int64)
        d = tc.dur(w, slot_min)
        member = ((mask >> p) & 1) != 0
        dd = min(d, H)
        win = T[:, :dd, :]                                   # [n, dd, 3]
        elig = member & (win >= 0).all(axis=(1, 2)) & (d <= H)
        tot = win[:, None, :, :] + cum[:, :, :dd, :]         # [n, W + 1, dd, 3]
        ok = (tot >= dem).all(axis=(2, 3)) & elig[:, None]   # [n, W + 1]: the prefix covers the whole window
        L = (vp < pr).sum(1)
        low = ok & (ar <= L[:, None])
        has = low.any(1)
        v = np.where(has, low.argmax(1), -1)                 # first true
        fit, able = int((has & (v == 0)).sum()), int((has & (v >= 1)).sum())
        outranked = elig & ~has & (ok & (ar > L[:, None]) & (ar <= ln[:, None])).any(1)
        r["members"], r["fit"], r["able"], r["outranked"] = member.sum(), fit, able, outranked.sum()
        if r["members"] == 0:
            r["code"] = NO_NODES
            continue
        if fit + able < need:
            r["code"] = NONE
            continue
        idx = np.flatnonzero(has)
        vv = v[idx]
        top = np.where(vv > 0, vp[idx, np.maximum(vv - 1, 0)] if W else NO_TOP, NO_TOP)
        res = np.minimum(tot[idx, vv], INF).min(axis=1) - dem  # [k, 3]: the window minima with the prefix gone
        sc = pc.score(res[:, 0], res[:, 1], res[:, 2])
        order = np.lexsort((idx, sc, vv, top))
        pick = order[:need]
        r["code"] = FITS if fit >= need else EVICT
        out_node[q, :need], out_vic[q, :need] = idx[pick], vv[pick]
        ev = vv[pick] > 0
        r["evict_nodes"], r["victims"] = ev.sum(), vv[pick].sum()
        r["top_prio"] = top[pick][ev].max() if ev.any() else 0
        if stats is not None and r["code"] == EVICT:
            stats["diff_top"] = stats.get("diff_top", 0) + int(len(set(top[pick][ev].tolist())) > 1)
            stats["not_fewest"] = stats.get("not_fewest", 0) + int(vv[pick].sum() > np.sort(vv)[:need].sum())
            if len(order) > need:  # the need-th and the (need + 1)-th key
                a, b = order[need - 1], order[need]
                t1 = top[a] == top[b]
                t2 = t1 and vv[a] == vv[b]
                t3 = t2 and sc[a] == sc[b]
                for name, t in (("tie_top", t1), ("tie_top_v", t2), ("tie_top_v_score", t3)):
                    stats[name] = stats.get(name, 0) + int(t)
            ok0 = (tot[:, :, 0, :] >= dem).all(axis=2) & (ar <= L[:, None])  # the slot-0 rule (fit_preempt's on slot 0)
            differs = int((ok0.argmax(1)[idx[pick]] != vv[pick]).any())
            stats["slot0_differs"] = stats.get("slot0_differs", 0) + differs
            stats["slot0_differs_k"] = stats.get("slot0_differs_k", 0) + (differs if need >= 2 else 0)
    return out, out_node, out_vic


# ---- the conditions of the packed cases, on the REFERENCE's output alone -------------------------
def rich_full(rows, stats, evict=20):
    """The full queue: so full that no row mixes fitting and evicting picks."""
    code, need, fit, able = rows["code"], rows["need"], rows["fit"], rows["able"]
    assert ((code == EVICT) & (need >= 2)).sum() >= evict, np.unique(code[need >= 2], return_counts=True)
    assert ((code == NONE) & (fit + able > 0)).any()
    assert stats.get("diff_top", 0) >= 1 and stats.get("not_fewest", 0) >= 1, stats
    assert stats.get("tie_top", 0) >= 1 and stats.get("tie_top_v", 0) >= 1 and stats.get("tie_top_v_score", 0) >= 1, stats
    assert stats.get("slot0_differs_k", 0) >= 2, stats


def rich_short(rows, stats, evict=20):
    """The short queue: some nodes still fit."""
    code, need, fit = rows["code"], rows["need"], rows["fit"]
    assert ((code == EVICT) & (need >= 2)).sum() >= evict, np.unique(code[need >= 2], return_counts=True)
    assert ((code == EVICT) & (fit > 0) & (fit < need)).any(), "no EVICT row mixes fitting and evicting picks"
    assert ((code == FITS) & (need >= 2)).any()
    assert stats.get("slot0_differs", 0) >= 1, stats
    assert stats.get("tie_top", 0) >= 1 and stats.get("tie_top_v", 0) >= 1, stats


def count_only(rows, stats, evict=10):
    """(65, 65): 12-17 EVICT rows with need >= 2 and no FITS row with need >= 2 at seeds 0-3 in either
    variant: the count at 10 and nothing else."""
    assert ((rows["code"] == EVICT) & (rows["need"] >= 2)).sum() >= evict


# (variant, n, j) -> the seeds of packed_tl_case at which the reference holds the variant's
# conditions (tests/test_preempt_tl_k.py asserts them on the CPU) and the conditions
SEEDS = {("full", 257, 128): ((0,), rich_full), ("full", 257, 257): ((0,), rich_full),
         ("short", 257, 128): ((0, 1), rich_short),
         ("full", 65, 65): ((0,), count_only), ("short", 65, 65): ((0,), count_only)}


@functools.lru_cache(maxsize=None)
def packed_tl_case_k(variant, n, j, seed=0, one_component=False):
    """_preempt_tl_cases.packed_tl_case with nodes_k drawn from K_DRAW.  variant "full": the whole
    queue of 2n jobs is placed before the query, as §2n's tests do; "short": only its first n // 8
    jobs, so some nodes still fit.  Cached and never written."""
    c = tc.packed_tl_case(n, j, seed, one_component)
    nk = np.random.default_rng(7 * n + j).choice(K_DRAW, j)
    queue = c.queue if variant == "full" else synth.Jobs(*(getattr(c.queue, f)[:n // 8] for f in (
        "cpu", "mem", "gpu", "wall", "part", "nodes_k")))
    return tc.CaseTL(c.nodes, c.victims, c.tline, queue, c.parts, with_k(c.jobs, nk), c.prio)


@functools.lru_cache(maxsize=None)
def packed_tl_ref_k(variant, n, j, seed=0, one_component=False, kmax=KMAX):
    """((rows, out_node, out_victims), stats, timeline) of packed_tl_case_k on the oracle's timeline,
    computed once."""
    c = packed_tl_case_k(variant, n, j, seed, one_component)
    T = tc.oracle_timeline(c)
    stats = {}
    return ref_preempt_tl_k(c.nodes.part_mask, T, c.victims, c.parts, c.jobs, c.prio, tc.SLOT_MIN, kmax, 0, stats), stats, T


# ---- the hand-written case ----------------------------------------------------------------------
def jobs_of_k(rows):
    """synth.Jobs and priorities from (cpu, mem, gpu, wall, part, prio, nodes_k) rows."""
    a = np.array(rows, np.int64).reshape(-1, 7)
    return (synth.Jobs(*(a[:, k].astype(np.int32) for k in range(4)), a[:, 4].astype(np.uint16), a[:, 6].astype(np.uint16)),
            a[:, 5].astype(np.int32))


def hand_case_k():
    """_preempt_tl_cases.hand_case's 6 nodes, victims, timeline and the two reservations under jobs
    with a nodes_k column.  8 slots of 10 minutes; partition 0 (nodes 0, 1, 2, 4, 5; 4 is closed by its
    negative cpu column) limits time 70, cpus 8, mem 10000; partition 1 is node 3; 2 has no node.
    cpus over the slots (tc.HAND_CPUS):
      node 0  0 0 0 0 0 0 4 4   A (prio 1, 4 cpus) ends at 3, B (prio 2, 4 cpus) at 8; [3, 6) is reserved
      node 1  0 0 0 0 0 0 8 8   C (prio 1, 8 cpus) ends at 2; [2, 6) is reserved
      node 2  0 0 0 0 0 0 0 0   D (prio 0, 4 cpus) has end 0, E (prio 3, 4 cpus) ends at 8
      node 3  8 8 8 8 8 8 - -   partition 1 only
      node 4  - - - - - - - -
      node 5  0 0 0 0 0 0 0 0   F (prio 9, 8 cpus) ends at 8
    The rows of HAND_ROWS_K are worked out by hand from DESIGN.md §2o."""
    h = tc.hand_case()
    #        cpu mem gpu wall part prio        nodes_k
    rows = [(0, 0, 0, 50, 0, I32MIN, 2),     # the all-zero demand: nodes 0, 1, 2, 5 fit
            (0, 0, 0, 50, 0, I32MIN, 0),     # nodes_k 0 is one node
            (4, 0, 0, 50, 0, 5, 2),          # 5 slots: node 0 needs A and B (the dip), node 2 D and E; node 1 nothing frees
            (4, 0, 0, 20, 0, 5, 3),          # 2 slots: A frees node 0, C node 1 (top 1 both), then node 2 with D, E (top 3)
            (4, 0, 0, 50, 0, 5, 3),          # fit + able = 2 = need - 1
            (4, 0, 0, 20, 0, 10, 4),         # every list is outranked: nodes 0, 1, 2 and 5 (F, top 9)
            (8, 1024, 0, 50, 1, 0, 2),       # partition 1 has one node, which fits: members < need
            (8, 1024, 0, 50, 1, 0, 1),
            (1, 1, 0, 71, 0, 0, 2), (9, 1, 0, 10, 0, 0, 3), (1, 10001, 0, 10, 0, 0, 4), (1, 1, 0, 10, 3, 0, 8),
            (1, 1, 0, 10, 2, 0, 2),
            (4, 0, 0, 70, 0, 5, 2),          # 7 slots reach the open slots 6, 7 of node 0: only the dip binds there
            (0, 0, 0, 50, 0, I32MIN, 5)]     # four fit, nothing can be freed at INT32_MIN
    jobs, prio = jobs_of_k(rows)
    return tc.CaseTL(h.nodes, h.victims, h.tline, h.queue, h.parts, jobs, prio)


def flat_hand_case_k():
    """Three nodes on an open timeline of 8 slots of 10 minutes without events or reservations: node 0
    has 4 cpus free, nodes 1 and 2 none; node 1's victim (prio 1, 4 cpus) ends at 8, node 2's two
    (prio 1, end 1, 4 cpus; prio 2, end 8, 4 cpus).  A job of 4 cpus on 2 slots at need 2 takes the
    fitting node 0 and evicts on node 1; at need 3 node 2 as well, with v = 2 where slot 0 alone says 1."""
    nodes = synth.Nodes(np.array([4, 0, 0], np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32),
                        np.full(3, INF, np.int32), np.ones(3, np.uint32))
    victims = tc.victims_tl_of([[], [(1, 8, 4, 0, 0)], [(1, 1, 4, 0, 0), (2, 8, 4, 0, 0)]])
    tline = synth.Timeline(8, 10, np.zeros(4, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs, prio = jobs_of_k([(4, 0, 0, 20, 0, 5, 2), (4, 0, 0, 20, 0, 5, 3), (4, 0, 0, 10, 0, 5, 3)])
    parts = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
    queue = synth.Jobs(*(np.zeros(0, np.int32) for _ in range(4)), np.zeros(0, np.uint16), np.zeros(0, np.uint16))
    return tc.CaseTL(nodes, victims, tline, queue, parts, jobs, prio)


# (code, need, evict_nodes, victims, top_prio, members, fit, able, outranked, reserved), picks, their v
FLAT_ROWS_K = [
    ((EVICT, 2, 1, 1, 1, 3, 1, 2, 0, 0), [0, 1], [0, 1]),        # a fitting and an evicting pick
    ((EVICT, 3, 2, 3, 2, 3, 1, 2, 0, 0), [0, 1, 2], [0, 1, 2]),  # node 2: its first victim has ended at slot 1, so v = 2
    ((EVICT, 3, 2, 2, 1, 3, 1, 2, 0, 0), [0, 1, 2], [0, 1, 1]),  # one slot: slot 0 is the window, v = 1 on node 2
]

HAND_ROWS_K = [
    # nodes 0, 1, 2, 5 fit with minima 0: the score and then the id decide
    ((FITS, 2, 0, 0, 0, 5, 4, 0, 0, 0), [0, 1], [0, 0]),
    ((FITS, 1, 0, 0, 0, 5, 4, 0, 0, 0), [0], [0]),
    # node 0 with A and B (top 2; the slot-0 rule says A alone), node 2 with D and E (top 3): the picks differ in top
    ((EVICT, 2, 2, 4, 3, 5, 0, 2, 1, 0), [0, 2], [2, 2]),
    # node 0 with A (top 1, residual 0) before node 1 with C (top 1, 4 cpus to spare), then node 2 (top 3, two victims)
    ((EVICT, 3, 3, 4, 3, 5, 0, 3, 1, 0), [0, 1, 2], [1, 1, 2]),
    ((NONE, 3, 0, 0, 0, 5, 0, 2, 1, 0), [], []),          # fit + able = need - 1; node 5 is outranked
    ((EVICT, 4, 4, 5, 9, 5, 0, 4, 0, 0), [0, 1, 2, 5], [1, 1, 2, 1]),
    ((NONE, 2, 0, 0, 0, 1, 1, 0, 0, 0), [], []),          # members < need
    ((FITS, 1, 0, 0, 0, 1, 1, 0, 0, 0), [3], [0]),
    ((LIMIT_TIME, 2, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((LIMIT_CPUS, 3, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((LIMIT_MEM, 4, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((PARTITION, 8, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((NO_NODES, 2, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    # 7 slots: on node 0 the runs [0, 3) and [3, 6) are short, A and B cover both, [6, 8) is free; node 2 as before
    ((EVICT, 2, 2, 4, 3, 5, 0, 2, 1, 0), [0, 2], [2, 2]),
    ((NONE, 5, 0, 0, 0, 5, 4, 0, 0, 0), [], []),
]


def hand_arrays(table=None, kmax=KMAX):
    """HAND_ROWS_K (or another table of the same form) as (rows, out_node, out_victims)."""
    table = HAND_ROWS_K if table is None else table
    rows = np.array([r for r, _, _ in table], np.int32).view(EVICT_K_DTYPE).reshape(-1)
    node = np.full((len(table), kmax), -1, np.int32)
    vic = np.zeros((len(table), kmax), np.int32)
    for q, (_, n, v) in enumerate(table):
        node[q, :len(n)], vic[q, :len(v)] = n, v
    return rows, node, vic

"""fit_preempt_k's reference and inputs (not a test module): ref_preempt_k, a numpy int64 restatement
of DESIGN.md §2m over the raw columns — never taken from the engine — the packed cases with a
nodes_k column, and a hand-written case with literal rows."""
import functools

import numpy as np

import _preempt_cases as pc
from _preempt_cases import EVICT, FITS, LIMIT_CPUS, LIMIT_MEM, LIMIT_TIME, NO_NODES, NONE, PARTITION  # noqa: F401
from fitgpu import EVICT_K_DTYPE, synth

INF, I32MIN = pc.INF, pc.I32MIN
NO_TOP = np.iinfo(np.int64).min  # the first key word of a node that fits now: below every priority
K_DRAW = (1, 2, 2, 3, 4, 8)
KMAX = 8


def ref_preempt_k(nodes, victims, parts, jobs, prio, kmax, stats=None, free=None):
    """Every job alone: §2l's per-(job, node) v through padded victim columns, a cumulative sum and
    a first-true search; then a lexsort on (top, v, score, node id) and its first `need`.  Returns
    (rows, out_node[J, kmax], out_victims[J, kmax]).  jobs.nodes_k None: every need is 1.  stats: a
    dict that counts, over the EVICT rows, what rich_enough_k asks for, and the offers that enter a
    list of kmax keys when the nodes come in id order."""
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
        amounts = np.stack([np.where(inside, np.asarray(a, np.int64)[src], 0)
                            for a in (victims.cpu, victims.mem, victims.gpu)], axis=2)
        S[:, 1:, :] = np.cumsum(amounts, axis=1)
    ar = np.arange(W + 1)[None, :]
    open_ = (fc >= 0) & (fm >= 0) & (fg >= 0)
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
        member = ((mask >> p) & 1) != 0
        elig = member & (avail >= w) & open_
        ok = ((fc[:, None] + S[:, :, 0] >= c) & (fm[:, None] + S[:, :, 1] >= m) & (fg[:, None] + S[:, :, 2] >= g)
              & elig[:, None])
        L = (vp < pr).sum(1)  # the lists are sorted: the entries below the job's priority are a prefix
        low = ok & (ar <= L[:, None])
        has = low.any(1)
        v = np.where(has, low.argmax(1), -1)
        fit, able = int((has & (v == 0)).sum()), int((has & (v >= 1)).sum())
        outranked = elig & ~has & (ok & (ar > L[:, None]) & (ar <= ln[:, None])).any(1)
        r["members"], r["fit"], r["able"], r["outranked"] = member.sum(), fit, able, outranked.sum()
        if r["members"] == 0:
            r["code"] = NO_NODES
            continue
        idx = np.flatnonzero(has)
        vv = v[idx]
        top = np.where(vv > 0, vp[idx, np.maximum(vv - 1, 0)] if W else NO_TOP, NO_TOP)
        res = [np.minimum(f[idx] + S[idx, vv, k], INF) - d for k, (f, d) in enumerate(((fc, c), (fm, m), (fg, g)))]
        sc = pc.score(*res)
        order = np.lexsort((idx, sc, vv, top))
        if stats is not None:  # keys in id order: one enters a lane's list when it is below the kmax-th smallest so far
            keys = list(zip(top.tolist(), vv.tolist(), sc.tolist(), idx.tolist()))
            kept = []
            for key in keys:
                if len(kept) < kmax or key < kept[-1]:
                    kept = sorted(kept + [key])[:kmax]
                    stats["entered"] = stats.get("entered", 0) + 1
            stats["pairs"] = stats.get("pairs", 0) + int(member.sum())
            stats["offers"] = stats.get("offers", 0) + len(keys)
        if fit + able < need:
            r["code"] = NONE
            continue
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
    return out, out_node, out_vic


def rich_enough_k(rows, stats, evict=20, full_tie=True):
    """What every random case must hold on the REFERENCE's output, so that a comparison of nothing
    interesting fails."""
    code, need, fit, able = rows["code"], rows["need"], rows["fit"], rows["able"]
    assert ((code == EVICT) & (need >= 2)).sum() >= evict, np.unique(code[need >= 2], return_counts=True)
    assert ((code == EVICT) & (fit > 0) & (fit < need)).any(), "no EVICT row mixes fitting and evicting picks"
    assert ((code == FITS) & (need >= 2)).any()
    assert ((code == NONE) & (fit + able > 0)).any()
    assert stats.get("diff_top", 0) > 0 and stats.get("not_fewest", 0) > 0, stats
    assert stats.get("tie_top", 0) > 0 and stats.get("tie_top_v", 0) > 0, stats
    if full_tie:
        assert stats.get("tie_top_v_score", 0) > 0, stats


def with_k(jobs, nodes_k):
    return synth.Jobs(jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.part,
                      None if nodes_k is None else np.asarray(nodes_k, np.uint16))


@functools.lru_cache(maxsize=None)
def packed_case_k(n, j, seed=0, one_component=False):
    """_preempt_cases.packed_case with nodes_k drawn from K_DRAW.  Cached and never written."""
    c = pc.packed_case(n, j, seed, one_component)
    nk = np.random.default_rng(7 * n + j).choice(K_DRAW, j)
    return pc.Case(c.nodes, c.victims, c.parts, with_k(c.jobs, nk), c.prio)


@functools.lru_cache(maxsize=None)
def packed_ref_k(n, j, seed=0, one_component=False, kmax=KMAX):
    """((rows, out_node, out_victims), stats) of packed_case_k, computed once."""
    c = packed_case_k(n, j, seed, one_component)
    stats = {}
    return ref_preempt_k(c.nodes, c.victims, c.parts, c.jobs, c.prio, kmax, stats), stats


# ---- the hand-written case ----------------------------------------------------------------------
def hand_case_k():
    """_preempt_cases.hand_case's 6 nodes, victims and partitions under 14 jobs with a nodes_k column.
    Partition 0 (nodes 0-4; 4 is closed by its negative cpu column) limits time 100, cpus 8, mem
    10000; partition 1 is node 5; 2 has no node.  Node 3 runs no job above 50 minutes.  The rows of
    HAND_ROWS_K are worked out by hand from DESIGN.md §2m."""
    h = pc.hand_case()
    #        cpu   mem  gpu wall part prio      nodes_k
    rows = [(2, 1024, 0, 10, 0, 5, 2), (2, 1024, 0, 10, 0, 5, 3), (4, 2048, 0, 60, 0, 4, 2), (4, 2048, 0, 60, 0, 4, 3),
            (1, 1024, 1, 10, 1, 8, 2), (2, 1024, 0, 10, 0, 5, 0), (6, 4096, 0, 60, 0, 7, 2), (0, 0, 0, 60, 0, I32MIN, 3),
            (1, 1, 0, 101, 0, 0, 2), (9, 1, 0, 10, 0, 0, 3), (1, 10001, 0, 10, 0, 0, 4), (1, 1, 0, 10, 3, 0, 8),
            (1, 1, 0, 10, 2, 0, 2), (0, 0, 0, 60, 0, I32MIN, 4)]
    a = np.array(rows, np.int64)
    jobs = synth.Jobs(*(a[:, k].astype(np.int32) for k in range(4)), a[:, 4].astype(np.uint16), a[:, 6].astype(np.uint16))
    return pc.Case(h.nodes, h.victims, h.parts, jobs, a[:, 5].astype(np.int32))


# (code, need, evict_nodes, victims, top_prio, members, fit, able, outranked, reserved), picks, their v
HAND_ROWS_K = [
    # nodes 0 and 3 fit, node 0 the tighter; node 2 needs one victim; node 1 is held at 6 >= 5
    ((FITS, 2, 0, 0, 0, 5, 2, 1, 1, 0), [0, 3], [0, 0]),
    # need 3 = fit + able: both fitting nodes first, then node 2 with one victim of priority 3
    ((EVICT, 3, 1, 1, 3, 5, 2, 1, 1, 0), [0, 3, 2], [0, 0, 1]),
    # node 0 frees 4 cpus with one victim (top 1), node 2 with two (top 3); node 1 outranks; 3 is too short-lived
    ((EVICT, 2, 2, 3, 3, 5, 0, 2, 1, 0), [0, 2], [1, 2]),
    ((NONE, 3, 0, 0, 0, 5, 0, 2, 1, 0), [], []),          # fit + able = need - 1
    ((NONE, 2, 0, 0, 0, 1, 1, 0, 0, 0), [], []),          # partition 1 has one node, which fits: members < need
    ((FITS, 1, 0, 0, 0, 5, 2, 1, 1, 0), [0], [0]),        # nodes_k 0 is one node
    # node 0 with TWO victims (top 5) before node 1 with one (top 6): not the fewest victims first
    ((EVICT, 2, 2, 3, 6, 5, 0, 2, 1, 0), [0, 1], [2, 1]),
    # the all-zero demand at INT32_MIN: nodes 0, 1, 2 fit (3: walltime, 4: closed), the emptiest first
    ((FITS, 3, 0, 0, 0, 5, 3, 0, 0, 0), [2, 1, 0], [0, 0, 0]),
    ((LIMIT_TIME, 2, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((LIMIT_CPUS, 3, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((LIMIT_MEM, 4, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((PARTITION, 8, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((NO_NODES, 2, 0, 0, 0, 0, 0, 0, 0, 0), [], []),
    ((NONE, 4, 0, 0, 0, 5, 3, 0, 0, 0), [], []),          # three fit, nothing can be freed at INT32_MIN
]


def hand_arrays(kmax=KMAX):
    """HAND_ROWS_K as (rows, out_node, out_victims)."""
    rows = np.array([r for r, _, _ in HAND_ROWS_K], np.int32).view(EVICT_K_DTYPE).reshape(-1)
    node = np.full((len(HAND_ROWS_K), kmax), -1, np.int32)
    vic = np.zeros((len(HAND_ROWS_K), kmax), np.int32)
    for q, (_, n, v) in enumerate(HAND_ROWS_K):
        node[q, :len(n)], vic[q, :len(v)] = n, v
    return rows, node, vic

"""Cases and the checker of fit_hold_tl, shared by tests/test_hold_tl.py and
tests/test_hold_tl_gpu.py (not a test module).  ref_hold_tl restates §2j in numpy over the dense
[n, H, 3] timeline: the int64 sum of every live window, one comparison, one subtraction of the held
rows.  The records it holds come from _unplace_tl_cases.reference (the restatement of §2g).  It
shares nothing with the kernels' run lists."""
import functools

import numpy as np

import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from fitgpu import synth

INT32_MAX = synth.INT32_MAX
HELD, REFUSED, SKIPPED = 1, 0, -1  # FIT_HOLD_* of include/fitgpu.h (tests/test_hold_tl.py compares them)


def ref_hold_tl(tl, jobs, node, start, slot_min, kmax, rows=None):
    """§2j: (dense timeline after, state[J], applied, refused).  tl is not changed; rows: the rows of
    the call, in that order (None: all, in index order); a row outside the call reads SKIPPED."""
    tl = np.array(tl, np.int32, copy=True)
    n, H, _ = tl.shape
    node = np.asarray(node, np.int32).reshape(-1, kmax)
    state = np.full(len(start), SKIPPED, np.int32)
    live = []
    for q in range(len(start)) if rows is None else rows:
        if start[q] < 0:
            continue
        need, s = max(int(jobs.nodes_k[q]), 1), int(start[q])
        d = max(1, -(-int(jobs.wall[q]) // slot_min))
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        live.append((int(q), node[q, :need].copy(), s, min(s + d, H), dem))
    S = np.zeros((n, H, 3), np.int64)
    for _, ids, s, e, dem in live:
        S[ids, s:e] += dem
    over = (S > tl.astype(np.int64)).any(axis=2)  # [n, H]; a slot that reads -1 is over: S >= 0
    held = np.zeros((n, H, 3), np.int64)
    applied = refused = 0
    for q, ids, s, e, dem in live:
        if over[ids, s:e].any():
            state[q] = REFUSED
            refused += 1
        else:
            state[q] = HELD
            applied += len(ids)
            held[ids, s:e] += dem
    out = tl.astype(np.int64) - held
    assert (out >= -1).all() and (out[tl == -1] == -1).all()  # nothing clamps, no -1 slot is touched
    return out.astype(np.int32), state, applied, refused


def shuffled(jobs, node, start, seed):
    """The same rows in a seeded random order: (perm, jobs', node', start')."""
    perm = np.random.default_rng(seed).permutation(len(start))
    return perm, uc.take(jobs, perm), np.ascontiguousarray(np.asarray(node)[perm]), np.ascontiguousarray(start[perm])


def replay_conditions(H, kmax):
    """The counts that keep a replay from being vacuous."""
    jobs, out, start, _ = uc.reference(H, kmax)
    c = uc.conditions(H, kmax)
    _, state, _, refused = ref_hold_tl(pk.start_timeline(H), jobs, out, start, pk.SLOT_MIN, kmax)
    return dict(held=int((state == HELD).sum()), multi=int(((state == HELD) & (jobs.nodes_k > 1)).sum()),
                skipped_unplaced=c["unplaced"], skipped_rejected=c["rejected"], refused=refused)


# ---- the refresh case -----------------------------------------------------------------------------------
# The records of uc.reference(H, kmax) held on the cluster as a resync finds it: in every component
# the node with the most recorded windows now carries another user's job that takes all its cpus for
# the whole horizon, and the next REFRESH_CUT busiest nodes are usable for a quarter of the horizon
# only (DRAIN with a deadline).  The warm-up queue is not on it: most records fit again.
REFRESH = [(64, 8), (256, 1)]
REFRESH_CUT = 6


@functools.lru_cache(maxsize=None)
def refresh_cluster(H, kmax):
    nodes, tline, parts = pk.cluster(H)
    jobs, out, start, _ = uc.reference(H, kmax)
    cnt = uc.windows_per_node(jobs, out, start, nodes.n)
    new = synth.Nodes(*(getattr(nodes, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min",
                                                           "part_mask")))
    taken = []
    for m in np.unique(nodes.part_mask):
        members = np.flatnonzero(nodes.part_mask == m)
        x = int(members[np.argmax(cnt[members])])
        new.cpu_free[x] = 0
        taken.append(x)
    rest = [int(x) for x in np.argsort(-cnt, kind="stable") if int(x) not in taken][:REFRESH_CUT]
    new.avail_min[rest] = np.minimum(new.avail_min[rest], (H // 4) * pk.SLOT_MIN)
    return new, tline, parts


@functools.lru_cache(maxsize=None)
def refresh_reference(H, kmax):
    """(timeline the refreshed cluster loads to, timeline after the hold, state, applied, refused)."""
    from oracle import pyoracle as po
    nodes, tline, _ = refresh_cluster(H, kmax)
    tl0 = po.ref_build_timeline(nodes, tline)
    jobs, out, start, _ = uc.reference(H, kmax)
    fin, state, applied, refused = ref_hold_tl(tl0, jobs, out, start, pk.SLOT_MIN, kmax)
    for a in (tl0, fin, state):
        a.setflags(write=False)
    return tl0, fin, state, applied, refused


# ---- the rule case ---------------------------------------------------------------------------------------
# 8 nodes, H = 64, slot_min 1, one partition, kmax 2.  Level 4 cpus, 8192 MiB, 2 gpus, except:
#   node 4 is usable for 40 slots (slots 40.. read -1), node 5 has INT32_MAX cpus, node 7 is in no partition.
# row  node(s)  start wall  demand             outcome
#  0   0        0     10    3 cpu              refused: slots 5..9 carry 3 + 2 > 4 with row 1
#  1   0        5     10    2 cpu              refused: the same slots; all parties of a conflict
#  2   0        20    5     1 cpu, 100, 1      held: the same node, other slots
#  3   1        0     8     4, 8192, 2         held: S == T exactly, the slots become 0
#  4   2, 3     0     4     3 cpu              refused through node 2 (slots 2, 3: 3 + 2 > 4 with row 5)
#  5   2        2     4     2 cpu              refused
#  6   3        0     2     2 cpu              refused: it fits node 3 alone, but row 4 still counts there
#  7   4        38    5     nothing            refused: a zero demand over the -1 slots 40..42
#  8   4        30    5     nothing            held: nothing changes
#  9   5        10    1     INT32_MAX cpu      refused \
# 10   5        10    1     INT32_MAX cpu      refused  } 3 * INT32_MAX > INT32_MAX: the sum does not wrap
# 11   5        10    1     INT32_MAX cpu      refused /
# 12   5        20    2     INT32_MAX cpu      held: slots 20, 21 become 0
# 13   6        60    100   1 cpu, 1, 1        held: the window is clipped at H, slots 60..63
# 14   (junk)   -1                             skipped whatever it holds
# 15   7        3     3     1 cpu              refused: a node in no partition reads -1 everywhere
# 16   6, 1     62    9     1 cpu              held: two nodes, clipped, beside row 13 (1 + 1 <= 4)
RULE_H, RULE_KMAX, RULE_SLOT_MIN = 64, 2, 1
RULE_STATE = np.array([REFUSED, REFUSED, HELD, HELD, REFUSED, REFUSED, REFUSED, REFUSED, HELD, REFUSED, REFUSED,
                       REFUSED, HELD, HELD, SKIPPED, REFUSED, HELD], np.int32)


def rule_cluster():
    n = 8
    cpu = np.full(n, 4, np.int32)
    cpu[5] = INT32_MAX
    avail = np.full(n, wk.INF, np.int32)
    avail[4] = 40
    mask = np.ones(n, np.uint32)
    mask[7] = 0
    nodes = synth.Nodes(cpu_free=cpu, mem_free=np.full(n, 8192, np.int32), gpu_free=np.full(n, 2, np.int32),
                        avail_min=avail, part_mask=mask)
    return nodes, uc.no_events(n, RULE_H, RULE_SLOT_MIN), wk.open_parts(1)


def rule_dense():
    """rule_cluster() as loaded, restated."""
    tl = np.empty((8, RULE_H, 3), np.int32)
    tl[:, :] = (4, 8192, 2)
    tl[5, :, 0] = INT32_MAX
    tl[4, 40:] = -1
    tl[7] = -1
    return tl


def rule_rows():
    M = INT32_MAX
    jobs = wk.jobs_of([(3, 0, 0, 10, 0, 1), (2, 0, 0, 10, 0, 1), (1, 100, 1, 5, 0, 1), (4, 8192, 2, 8, 0, 1),
                       (3, 0, 0, 4, 0, 2), (2, 0, 0, 4, 0, 1), (2, 0, 0, 2, 0, 1), (0, 0, 0, 5, 0, 1),
                       (0, 0, 0, 5, 0, 1), (M, 0, 0, 1, 0, 1), (M, 0, 0, 1, 0, 1), (M, 0, 0, 1, 0, 0),
                       (M, 0, 0, 2, 0, 1), (1, 1, 1, 100, 0, 1), (-7, -7, -7, -7, 0, 9), (1, 0, 0, 3, 0, 1),
                       (1, 0, 0, 9, 0, 2)])
    node = np.array([[0, -1], [0, 99], [0, -1], [1, -1], [2, 3], [2, -1], [3, -1], [4, -1], [4, -1], [5, -1],
                     [5, -1], [5, -1], [5, -1], [6, -1], [-9, 99], [7, -1], [6, 1]], np.int32)
    start = np.array([0, 5, 20, 0, 0, 2, 0, 38, 30, 10, 10, 10, 20, 60, -1, 3, 62], np.int32)
    return jobs, node, start


# ---- the seam --------------------------------------------------------------------------------------------
SEAM_CPU = 8


def seam_rows(n=64, j=16390, H=64):
    """j one-node rows of 1 cpu and one slot for SEAM_CPU-cpu nodes, spread so that no slot carries
    more than 5 of them — except two pairs of 5-cpu rows, each row of which fits alone: rows 3 and
    j - 2 on (node 1, slot 7), 16,385 rows apart, and rows 100 and 9,000 on (node 2, slot 9), inside
    one block of 16,384.  (jobs, node, start, the four rows.)"""
    q = np.arange(j)
    node = (q % (n - 4) + 4).astype(np.int32)       # nodes 4 .. n - 1: 60 nodes x 64 slots = 3,840 cells
    start = ((q // (n - 4)) % H).astype(np.int32)   # at most ceil(16390 / 3840) = 5 rows per cell
    cpu = np.ones(j, np.int32)
    pairs = [3, j - 2, 100, 9000]
    node[pairs] = [1, 1, 2, 2]
    start[pairs] = [7, 7, 9, 9]
    cpu[pairs] = 5
    jobs = synth.Jobs(cpu, np.zeros(j, np.int32), np.zeros(j, np.int32), np.ones(j, np.int32),
                      np.zeros(j, np.uint16), np.ones(j, np.uint16))
    return jobs, node, start, pairs

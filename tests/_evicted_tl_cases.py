"""fit_evicted_tl's reference and inputs (not a test module): ref_evicted_tl, a numpy int64 restatement
of DESIGN.md §2p on the DENSE [n, H, 3] timeline and the CSR of the lists — per row a saturating add
over the window, then a boolean delete per list; it shares nothing with the kernels — a hand-written
case with literal timelines and lists, the packed case's rows and the conditions a packed case must
hold on the reference alone, with the recorded seeds."""
import functools

import numpy as np

import _preempt_tl_cases as tc
from fitgpu import synth

INF = tc.INF
VCOLS = ("off", "prio", "end", "cpu", "mem", "gpu")


def list_lengths(victims, n, mask=None):
    """The lengths the library reads: a node in no partition has no list."""
    ln = np.diff(np.asarray(victims.off, np.int64)) if victims is not None else np.zeros(n, np.int64)
    return ln if mask is None else np.where(np.asarray(mask) != 0, ln, 0)


def ref_evicted_tl(T, victims, shift, rows, mask=None):
    """(T', victims') after the rows [m, 2] of (node id, position): every position refers to `victims`
    as given.  e' = max(end - shift, 0); per row T'[x, :e', c] = where(T == -1, -1, minimum(T + amount,
    INT32_MAX)), then the row's entry leaves its list; victims' has every end written as e' and the
    lists of nodes with mask 0 empty (mask None: every node is in a partition).  Raises ValueError on
    a row the library refuses: a node id outside [0, n), a position outside the node's list, a pair
    twice.  T and victims are not changed."""
    T = np.array(T, np.int64)
    n = T.shape[0]
    off = np.asarray(victims.off, np.int64)
    ln = list_lengths(victims, n, mask)
    e1 = np.maximum(np.asarray(victims.end, np.int64) - int(shift), 0)
    amount = np.stack([np.asarray(a, np.int64) for a in (victims.cpu, victims.mem, victims.gpu)], axis=1)
    gone = np.zeros(len(e1), bool)
    for x, p in np.asarray(rows, np.int64).reshape(-1, 2):
        if not 0 <= x < n:
            raise ValueError(f"node id {x} outside [0, {n})")
        if not 0 <= p < ln[x]:
            raise ValueError(f"position {p} outside node {x}'s list of {ln[x]}")
        if gone[off[x] + p]:
            raise ValueError(f"entry {p} of node {x} twice")
        gone[off[x] + p] = True
    owner = np.repeat(np.arange(n), np.diff(off))
    for k in np.flatnonzero(gone):
        w = T[owner[k], :e1[k]]  # [e', 3]
        T[owner[k], :e1[k]] = np.where(w == -1, -1, np.minimum(w + amount[k], INF))
    keep = ~gone & (ln[owner] > 0)
    noff = np.zeros(n + 1, np.int64)
    noff[1:] = np.cumsum(np.bincount(owner[keep], minlength=n))
    left = synth.VictimsTL(noff.astype(np.int32), np.asarray(victims.prio, np.int32)[keep], e1[keep].astype(np.int32),
                           *(amount[keep, c].astype(np.int32) for c in range(3)))
    return T.astype(np.int32), left


def unplace_rows(victims, shift, rows, slot_min, mask=None):
    """The defining relation's first half: fit_unplace_tl's rows (jobs, node, start) for the evicted
    entries with e' > 0."""
    off = np.asarray(victims.off, np.int64)
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    k = off[rows[:, 0]] + rows[:, 1]
    e1 = np.maximum(np.asarray(victims.end, np.int64)[k] - int(shift), 0)
    k, x, e1 = k[e1 > 0], rows[e1 > 0, 0], e1[e1 > 0]
    jobs = synth.Jobs(np.asarray(victims.cpu, np.int32)[k], np.asarray(victims.mem, np.int32)[k],
                      np.asarray(victims.gpu, np.int32)[k], (e1 * slot_min).astype(np.int32),
                      np.zeros(len(k), np.uint16), np.ones(len(k), np.uint16))
    return jobs, x.astype(np.int32), np.zeros(len(k), np.int32)


def same_victims(a, b):
    return all(np.array_equal(np.asarray(getattr(a, f), np.int32), np.asarray(getattr(b, f), np.int32)) for f in VCOLS)


def bytes_of(T, victims):
    return np.asarray(T, np.int32).tobytes(), tuple(np.asarray(getattr(victims, f), np.int32).tobytes() for f in VCOLS)


# ---- the hand-written case -----------------------------------------------------------------------
HAND_H, HAND_SHIFT = 8, 3
HAND_MASK = np.array([1, 1, 1, 1, 0, 1], np.uint32)
# (prio, end, cpu, mem, gpu) as loaded; with the shift of 3 the ends read 0, 2, 5, 3, 5 on node 0
HAND_LISTS = [
    [(1, 3, 1, 10, 0), (1, 5, 2, 20, 0), (2, 8, 4, 40, 1), (3, 6, 8, 80, 0), (4, 8, 16, 160, 0)],
    [(0, 4, 1, 1, 1), (5, 8, 2, 2, 0)],
    [],
    [(1, 8, 1, 0, 0), (2, 8, 1, 0, 0), (2, 7, 5, 6, 7)],
    [(1, 8, 1, 1, 1)],  # node 4 is in no partition: validated, never used, reads as empty
    [(7, 8, 10, INF, 0)],
]


def hand_timeline():
    """cpu / mem / gpu over the 8 slots.  Node 0 is closed at slot 4, node 3's gpu column at slot 1,
    node 4 is in no partition (all -1), node 5 sits 5 cpus below INT32_MAX and at INT32_MAX MiB."""
    T = np.zeros((6, HAND_H, 3), np.int64)
    T[0, :, 0], T[0, :, 1] = [0, 0, 1, 1, -1, 2, 2, 2], 100
    T[0, 4] = -1
    T[1, :, 0] = 3
    T[2, :, 0] = 7
    T[3, :, 1] = 10
    T[3, 1, 2] = -1
    T[4] = -1
    T[5, :, 0], T[5, :, 1] = INF - 5, INF
    return T


# call 1, in no particular order: node 0's first entry (a prefix of one; e' = 0, frees nothing) and
# its middle entry C over the closed slot 4; node 1's whole list; node 3's last entry; node 5's one.
HAND_ROWS_1 = [(3, 2), (0, 2), (1, 1), (5, 0), (0, 0), (1, 0)]
HAND_T1 = {  # node: (cpu, mem, gpu) rows after call 1, for the nodes it touches
    0: ([4, 4, 5, 5, -1, 2, 2, 2], [140, 140, 140, 140, -1, 100, 100, 100], [1, 1, 1, 1, -1, 0, 0, 0]),
    1: ([6, 5, 5, 5, 5, 3, 3, 3], [3, 2, 2, 2, 2, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]),
    3: ([5, 5, 5, 5, 0, 0, 0, 0], [16, 16, 16, 16, 10, 10, 10, 10], [7, -1, 7, 7, 0, 0, 0, 0]),
    5: ([INF] * 5 + [INF - 5] * 3, [INF] * 8, [0] * 8),
}
HAND_LISTS_1 = [[(1, 2, 2, 20, 0), (3, 3, 8, 80, 0), (4, 5, 16, 160, 0)], [], [], [(1, 5, 1, 0, 0), (2, 5, 1, 0, 0)], [],
                []]
# call 2 on that state (its ends are e' already: shift 0): the prefix B, D of node 0
HAND_ROWS_2 = [(0, 1), (0, 0)]
HAND_T2 = {0: ([14, 14, 13, 5, -1, 2, 2, 2], [240, 240, 220, 140, -1, 100, 100, 100], [1, 1, 1, 1, -1, 0, 0, 0])}
HAND_LISTS_2 = [[(4, 5, 16, 160, 0)], [], [], [(1, 5, 1, 0, 0), (2, 5, 1, 0, 0)], [], []]


def hand_expected(T, changed):
    out = np.array(T, np.int32)
    for x, cols in changed.items():
        out[x] = np.array(cols, np.int64).T
    return out


# ---- the packed cases ----------------------------------------------------------------------------
# The shift of a packed case: ENDS starts at 1, so an entry with e' = 0 takes an advance first.
PACKED_SHIFT = 2
# seed of packed_rows per (n, one_component) for which the reference holds rich_enough below
# (tests/test_evicted_tl.py asserts it on the CPU); a shape that is not listed takes seed 0 and is
# not asked to be rich
SEEDS = {(65, False): 0, (257, False): 0, (257, True): 0}
# relation 4: the seed for which some job's answer after unplace_tl alone differs from the true state's
DOUBLE_COUNT = (257, False, 0)


@functools.lru_cache(maxsize=None)
def packed_rows(n, one_component=False, seed=None, frac=0.3):
    """(case, rows): tc.packed_tl_case(n, 257) and about `frac` of its entries of nodes in a partition
    as (node, pos) rows, in shuffled order.  Cached and never written."""
    seed = SEEDS.get((n, one_component), 0) if seed is None else seed
    c = tc.packed_tl_case(n, 257, None, one_component)
    r = np.random.default_rng(0xE71C + 977 * n + seed)
    ln = list_lengths(c.victims, n, c.nodes.part_mask)
    node = np.repeat(np.arange(n), ln)
    pos = np.concatenate([np.arange(k) for k in ln] + [np.zeros(0, np.int64)]).astype(np.int64)
    pick = r.random(len(node)) < frac
    rows = np.stack([node[pick], pos[pick]], axis=1).astype(np.int32)
    r.shuffle(rows, axis=0)
    return c, rows


def advanced(T, a):
    """The dense timeline after fit_advance_tl(a) without tails: every column continues its slot
    H - 1 value."""
    T = np.asarray(T)
    H = T.shape[1]
    a = min(a, H)
    return np.concatenate([T[:, a:], np.repeat(T[:, H - 1:], a, axis=1)], axis=1) if a else T.copy()


def rich_enough(T, victims, shift, rows, mask):
    """What a packed case must hold on the REFERENCE's output alone, so that a comparison of nothing
    interesting fails."""
    rows = np.asarray(rows, np.int64)
    T2, left = ref_evicted_tl(T, victims, shift, rows, mask)
    assert len(rows) >= 20
    per = np.bincount(rows[:, 0], minlength=T.shape[0])
    assert per.max() >= 3
    ln = list_lengths(victims, T.shape[0], mask)
    off = np.asarray(victims.off, np.int64)
    middle = zero = shut = False
    for x in np.flatnonzero(per):
        gone = np.zeros(ln[x], bool)
        gone[rows[rows[:, 0] == x, 1]] = True
        g = np.flatnonzero(gone)
        middle |= any((~gone[:p]).any() and (~gone[p + 1:]).any() for p in g)
        e1 = np.maximum(np.asarray(victims.end, np.int64)[off[x] + g] - shift, 0)
        zero |= bool((e1 == 0).any())
        shut |= bool(len(e1) and (np.asarray(T)[x, :e1.max()] == -1).any())
    assert middle, "no removed middle entry with a survivor on each side"
    assert zero, "no evicted entry with e' = 0"
    assert shut, "no -1 slot inside an evicted window"
    assert (T2 != np.asarray(T)).any() and left.off[-1] == ln.sum() - len(rows)
    assert ((T2 == -1) == (np.asarray(T) == -1)).all()
    return T2, left


@functools.lru_cache(maxsize=None)
def double_count_case():
    """Relation 4 on the reference alone: (case, rows, T', victims', the rows fit_preempt_tl gives when
    the evicted entries were unplaced but stay in the lists, the rows on the true state)."""
    n, one_component, seed = DOUBLE_COUNT
    c, rows = packed_rows(n, one_component, seed)
    T1, v1 = ref_evicted_tl(tc.oracle_timeline(c), c.victims, 0, rows, c.nodes.part_mask)
    args = (c.parts, c.jobs, c.prio, tc.SLOT_MIN)
    return (c, rows, T1, v1, tc.ref_preempt_tl(c.nodes.part_mask, T1, c.victims, *args),
            tc.ref_preempt_tl(c.nodes.part_mask, T1, v1, *args))

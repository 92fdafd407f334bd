"""Cases and the checker of fit_set_tl, shared by tests/test_set_tl.py and
tests/test_set_tl_gpu.py (not a test module).  ref_set_tl restates §2q in numpy over the dense
[n, H, 3] timeline: a plain loop over the rows in index order with slice assignment.  It shares
nothing with the kernels' run lists, their grouping by node or their owner column."""
import functools

import numpy as np

import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from fitgpu import synth

INT32_MAX = synth.INT32_MAX
RANDOM_H = (16, 64, 100, 256)


def ref_set_tl(tl, node, frm, to, levels, mask=None):
    """§2q: (dense timeline after, applied, ignored).  tl is not changed.  mask: the loaded partition
    masks (None: every node is in a partition); a node with mask 0 has no run list, a live row on it
    writes nothing and is ignored.  A bad live row raises ValueError, as the library refuses the call."""
    tl = np.array(tl, np.int32, copy=True)
    n, H, _ = tl.shape
    levels = np.asarray(levels, np.int64).reshape(-1, 3)
    live = [q for q in range(len(node)) if frm[q] >= 0]
    for q in live:
        if not 0 <= node[q] < n or frm[q] >= H or to[q] <= frm[q] or (levels[q] < -1).any():
            raise ValueError(f"row {q}")
    applied = ignored = 0
    for q in live:
        if mask is not None and mask[node[q]] == 0:
            ignored += 1
            continue
        tl[node[q], frm[q]:min(int(to[q]), H)] = levels[q]
        applied += 1
    return tl, applied, ignored


def cols(rows):
    """(node, from, to, cpu, mem, gpu) tuples -> (node[m], frm[m], to[m], levels[m, 3]), int32."""
    a = np.array(rows, np.int64).reshape(-1, 6).astype(np.int32)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3:].copy()


def take(c, idx):
    return tuple(np.ascontiguousarray(a[idx]) for a in c)


def runs_as_rows(dense, nodes):
    """The run-length rows of the nodes' dense timelines: what a caller writes for a node whose target
    timeline it knows."""
    rows = []
    H = dense.shape[1]
    for x in nodes:
        cut = [0] + (1 + np.flatnonzero((dense[x, 1:] != dense[x, :-1]).any(axis=1))).tolist() + [H]
        rows += [(x, a, b, *dense[x, a].tolist()) for a, b in zip(cut[:-1], cut[1:])]
    return rows


def overlapping(node, frm, to, levels, H):
    """The live rows that overlap an EARLIER live row of the same node with a different level."""
    hit = []
    seen = {}
    for q in range(len(node)):
        if frm[q] < 0:
            continue
        a, b, lv = int(frm[q]), min(int(to[q]), H), tuple(levels[q].tolist())
        if any(a < pb and pa < b and plv != lv for pa, pb, plv in seen.get(int(node[q]), [])):
            hit.append(q)
        seen.setdefault(int(node[q]), []).append((a, b, lv))
    return hit


# ---- 1. the random case ------------------------------------------------------------------------------
# pk.cluster(H) puts every node in a partition, and §2q has a rule for the nodes that are in none: the
# random case runs on pk.cluster(H) with the masks of NO_PART cleared, after the same warm-up queue.
NO_PART = (3, 50, 200, 640)
HOT = 11          # the node with more than 64 live rows
QUIET = 17        # the node of the row that changes nothing: no other row names it


@functools.lru_cache(maxsize=None)
def cluster(H):
    nodes, tline, parts = pk.cluster(H)
    nodes = synth.Nodes(*(getattr(nodes, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min",
                                                              "part_mask")))
    nodes.part_mask[list(NO_PART)] = 0
    return nodes, tline, parts


@functools.lru_cache(maxsize=None)
def start_timeline(H):
    """cluster(H) as loaded, at H >= 64 after a fit_place_tl of pk.pre_jobs(H) (by the C oracle; the
    GPU test checks that the engine's agrees); a node in no partition reads -1."""
    from oracle import pyoracle as po
    nodes, tline, parts = cluster(H)
    tl = po.ref_place_tl(nodes, tline, pk.pre_jobs(H), parts)[3] if H >= 64 else po.ref_build_timeline(nodes, tline)
    tl = tl.copy()
    tl[nodes.part_mask == 0] = -1
    tl.setflags(write=False)
    return tl


@functools.lru_cache(maxsize=None)
def random_rows(H):
    """About 400 rows on start_timeline(H), shuffled with the seed 77 + H: the columns of cols()."""
    tl0 = start_timeline(H)
    n = tl0.shape[0]
    r = np.random.default_rng(77 + H)

    def level():
        v = [int(r.integers(0, 65)), int(r.integers(0, 9)) * 4096, int(r.integers(0, 5))]
        for c in range(3):
            if r.random() < 0.08:
                v[c] = -1
        return v

    rows = []
    # the hot node: one-slot rows over consecutive slots with alternating levels (min(H, 130) runs), then
    # 40 wider rows over them; every later round over the same slots overlaps with a different level
    for i in range(130):
        rows.append((HOT, i % H, i % H + 1, 10 + i % 2 + 2 * (i // H), 4096, i % 2))
    for _ in range(40):
        a = int(r.integers(0, H))
        rows.append((HOT, a, a + int(r.integers(1, 6)), *level()))
    # random windows on 52 nodes, about four rows each: wide windows, so that they overlap
    free = [x for x in range(n) if x not in (HOT, QUIET) + NO_PART]
    for x in r.choice(free, 52, replace=False).tolist():
        for _ in range(int(r.integers(2, 7))):
            a = int(r.integers(0, H))
            rows.append((x, a, a + int(r.integers(1, H + 1)), *level()))
    # the edges of a window
    e = r.choice(free, 12, replace=False).tolist()
    rows += [(e[0], 0, 1, 5, 5, 1), (e[1], H - 1, H, 6, 0, 0), (e[2], H - 1, INT32_MAX, 7, 1, 1),
             (e[3], 0, H, 8, 2, 2), (e[4], 0, H + 5, 9, 3, 3), (e[5], 0, INT32_MAX, -1, -1, -1),
             (e[6], H // 2, INT32_MAX, 3, -1, 3), (e[7], 0, H, -1, 4, 0), (e[8], 1, H + 1000, 1, 1, -1)]
    # nodes with long lists flattened (their run count falls), a long list drained
    long_ = [x for x in np.argsort(-wk.run_counts(tl0)).tolist() if x not in (HOT, QUIET) + NO_PART][:3]
    rows += [(long_[0], 0, H, 4, 8192, 1), (long_[1], 0, INT32_MAX, -1, -1, -1), (long_[2], 0, H, 0, 0, 0)]
    # the row that changes nothing: the first run of QUIET, written with the level it has
    end0 = int(np.flatnonzero(np.append((tl0[QUIET, 1:] != tl0[QUIET, :-1]).any(axis=1), True))[0]) + 1
    rows.append((QUIET, 0, end0, *tl0[QUIET, 0].tolist()))
    # nodes in no partition, and skipped rows that hold what would be refused in a live row
    rows += [(NO_PART[0], 0, H, 4, 4, 4), (NO_PART[1], 2 % H, INT32_MAX, -1, 0, 0), (NO_PART[0], H - 1, H, 1, 1, 1)]
    rows += [(-7, -1, 0, -9, -9, -9), (n + 5, -3, -8, 1, 1, 1), (HOT, -1, H, 1000, 1000, 1000), (0, INT32_MAX * -1, 5, 0, 0, 0)]
    c = cols([rows[i] for i in r.permutation(len(rows))])
    for a in c:
        a.setflags(write=False)
    return c


def random_conditions(H):
    """The counts that keep the random case from being vacuous (asserted in tests/test_set_tl.py)."""
    tl0 = start_timeline(H)
    mask = cluster(H)[0].part_mask
    node, frm, to, levels = random_rows(H)
    want, applied, ignored = ref_set_tl(tl0, node, frm, to, levels, mask)
    live = frm >= 0
    per_node = np.bincount(node[live], minlength=tl0.shape[0])
    r0, r1 = wk.run_counts(tl0), wk.run_counts(want)
    one_closed = ((levels == -1).sum(axis=1) == 1) & live
    q = int(np.flatnonzero(live & (node == QUIET))[0])
    same = ref_set_tl(tl0, *take((node, frm, to, levels), [q]), mask)[0].tobytes() == tl0.tobytes()
    return dict(rows=len(node), live=int(live.sum()), applied=applied, ignored=ignored,
                overlap=len(overlapping(node, frm, to, levels, H)), busiest=int(per_node.max()),
                from0=int((frm[live] == 0).sum()), from_last=int((frm[live] == H - 1).sum()),
                to_h=int((to[live] == H).sum()), to_beyond=int(((to[live] > H) & (to[live] < INT32_MAX)).sum()),
                to_max=int((to[live] == INT32_MAX).sum()), nothing=bool(same), quiet_rows=int((node[live] == QUIET).sum()),
                one_closed=int(one_closed.sum()), skipped=int((~live).sum()), longest=int(r1.max()),
                fell=int((r1 < r0).sum()), changed=int((want != tl0).any(axis=(1, 2)).sum()))


@functools.lru_cache(maxsize=None)
def random_reference(H):
    """(want, applied, ignored) of random_rows(H) on start_timeline(H), and what a pk.busy_case queue
    of 60 jobs places on `want` by the restatement of §2g: (queue, nodes, start, final)."""
    nodes, _, parts = cluster(H)
    want, applied, ignored = ref_set_tl(start_timeline(H), *random_rows(H), nodes.part_mask)
    kmax = 4
    queue = pk.busy_case(H, 60, kmax)
    rn, rs, rfin = pk.ref_place_tl_k(want, nodes.part_mask, parts, queue, pk.SLOT_MIN, kmax)
    for a in (want, rn, rs, rfin):
        a.setflags(write=False)
    return want, applied, ignored, (queue, kmax, rn, rs, rfin)


# ---- 2. the largest-index rule -----------------------------------------------------------------------
def crowd(n=40, H=64, seed=23):
    """300 rows with random overlapping windows and levels on node 7 and 30 rows on 30 other nodes, one
    each, so that the other nodes' rows commute with everything: (rows of node 7 in their order, the 30
    others)."""
    r = np.random.default_rng(seed)
    on7, others = [], []
    for _ in range(300):
        a = int(r.integers(0, H))
        on7.append((7, a, a + int(r.integers(1, 9)), int(r.integers(-1, 50)), int(r.choice([-1, 0, 1024, 2048])),
                    int(r.integers(-1, 4))))
    for x in range(30):
        a = int(r.integers(0, H))
        others.append((8 + x, a, a + int(r.integers(1, H)), int(r.integers(0, 50)), 2048, 1))
    return on7, others


def interleaved(on7, others, seed):
    """The rows of node 7 in their order with the others, permuted, at random places between them."""
    r = np.random.default_rng(seed)
    at = np.sort(r.integers(0, len(on7) + 1, len(others)))
    perm = r.permutation(len(others))
    rows, k = [], 0
    for i in range(len(on7) + 1):
        while k < len(others) and at[k] == i:
            rows.append(others[perm[k]])
            k += 1
        if i < len(on7):
            rows.append(on7[i])
    return cols(rows)


# ---- 7. the seam -------------------------------------------------------------------------------------
def seam_rows(n=64, m=16390, H=64):
    """m one-slot rows spread over nodes 4 .. n - 1, each cell written several times with the row's own
    level, and two pairs of overlapping windows: rows 3 and m - 2 on node 1, 16,385 rows apart (across
    the chunk boundary), rows 100 and 9,000 on node 2, inside one chunk.  (columns, the four rows.)"""
    q = np.arange(m)
    node = (q % (n - 4) + 4).astype(np.int32)
    frm = ((q // (n - 4)) % H).astype(np.int32)
    to = frm + 1
    levels = np.stack([100 + q % 1000, q % 7, q % 3], axis=1).astype(np.int32)
    pairs = [3, m - 2, 100, 9000]
    node[pairs] = [1, 1, 2, 2]
    frm[pairs] = [5, 8, 9, 2]
    to[pairs] = [20, 12, 30, 40]
    levels[pairs] = [[11, 1, 1], [22, 2, 2], [33, 3, 0], [44, 4, 1]]
    return (node, frm, to.astype(np.int32), levels), pairs


# ---- 5. two clusters that differ on some nodes -------------------------------------------------------
def two_clusters(n=24, H=32, L=5):
    """(X, Y, what differs): Y is X after nodes changed outside the plan.  slot_min L; partition 0 holds
    every node but node 5, partition 1 nodes 5 and 6, so that a job judged alone does not always land on
    the one large node.
      1 drained (avail_min 0)              2 resumed: avail_min 0 in X, a staircase of releases in Y
      3 avail_min shortened                4 avail_min lengthened
      5 totals raised above X's ceilings   6 totals lowered
    Every other node has the same row and the same release events in both."""
    r = np.random.default_rng(5)
    x = uc.flat_cluster(n, cpu=32, mem=65536, gpu=4)
    x.cpu_free[:] = r.integers(0, 7, n)  # nearly full now: the releases below decide when a job starts
    x.avail_min[[2, 3, 4]] = [0, 20 * L, 10 * L]
    x.part_mask[[5, 6]] = [2, 3]
    y = synth.Nodes(*(getattr(x, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min", "part_mask")))
    y.avail_min[[1, 2, 3, 4]] = [0, wk.INF, 6 * L, 25 * L]
    y.cpu_free[2], y.mem_free[2], y.gpu_free[2] = 2, 8192, 0
    y.cpu_free[5], y.mem_free[5], y.gpu_free[5] = 200, 1 << 20, 16
    y.cpu_free[6], y.mem_free[6], y.gpu_free[6] = 1, 1024, 0
    ev = {k: [(int(s), int(r.integers(6, 25)), int(r.integers(0, 2)) * 1024, int(r.integers(0, 2)))
              for s in sorted(r.choice(np.arange(1, H), 3, replace=False))] for k in range(7, n, 2)}
    evy = dict(ev)
    evy[2] = [(s, 3, 4096, 1) for s in range(2, 20, 3)]  # the staircase of releases

    def tline(events):
        off, flat = [0], []
        for k in range(n):
            flat += events.get(k, [])
            off.append(len(flat))
        a = np.array(flat, np.int64).reshape(-1, 4).astype(np.int32)
        return synth.Timeline(slots=H, slot_min=L, off=np.array(off, np.int32), slot=a[:, 0].copy(), cpu=a[:, 1].copy(),
                              mem=a[:, 2].copy(), gpu=a[:, 3].copy())
    return (x, tline(ev)), (y, tline(evy)), [1, 2, 3, 4, 5, 6]

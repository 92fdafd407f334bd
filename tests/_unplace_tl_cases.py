"""Cases and the checker of fit_unplace_tl, shared by tests/test_unplace_tl.py and
tests/test_unplace_tl_gpu.py (not a test module).  ref_unplace_tl restates §2h in numpy over the dense
[n, H, 3] timeline; the placements it hands back come from _place_tl_k_cases.ref_place_tl_k.  It
shares nothing with the kernels' run lists."""
import functools

import numpy as np

import _place_tl_k_cases as pk
import _when_k_cases as wk
from fitgpu import FIT_REJECTED, synth

INT32_MAX = synth.INT32_MAX


def ref_unplace_tl(tl, jobs, node, start, slot_min, kmax, rows=None):
    """§2h: (dense timeline after, windows applied).  tl is not changed; rows: the rows to take, in
    that order (None: all, in index order)."""
    tl = np.array(tl, np.int32, copy=True)
    node = np.asarray(node, np.int32).reshape(-1, kmax)
    applied = 0
    for q in range(len(start)) if rows is None else rows:
        if start[q] < 0:
            continue
        need, s = max(int(jobs.nodes_k[q]), 1), int(start[q])
        d = max(1, -(-int(jobs.wall[q]) // slot_min))
        v = tl[node[q, :need], s:s + d].astype(np.int64)  # the slice clips at H
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        tl[node[q, :need], s:s + d] = np.where(v == -1, -1, np.minimum(v + dem, INT32_MAX))
        applied += need
    return tl, applied


def take(jobs, rows):
    return synth.Jobs(*(np.ascontiguousarray(getattr(jobs, f)[rows]) for f in wk.JOB_FIELDS))


def concat(a, b):
    return synth.Jobs(*(np.concatenate([getattr(a, f), getattr(b, f)]) for f in wk.JOB_FIELDS))


# ---- the round-trip cases ----------------------------------------------------------------------------
# (H, kmax): a contended pk.busy_case queue followed by a pk.rand_case queue (undeclared partitions,
# limit rejections, d == H + 1) on pk.start_timeline(H) — rand_cluster after the warm-up queue, so the
# run lists already carry dips.  Five components of 1, 63, 64, 65 and 600 nodes.
ROUND_TRIP = [(64, 1), (64, 8), (256, 1), (256, 8)]
N_BUSY, N_RAND = 120, 60


def queue(H, kmax):
    return concat(pk.busy_case(H, N_BUSY, kmax), pk.rand_case(H, N_RAND, kmax))


@functools.lru_cache(maxsize=None)
def reference(H, kmax):
    """(jobs, nodes[J, kmax], start[J], timeline after the placement) of queue(H, kmax) on
    pk.start_timeline(H), by the restatement of §2g."""
    nodes, tline, parts = pk.cluster(H)
    jobs = queue(H, kmax)
    out, start, fin = pk.ref_place_tl_k(pk.start_timeline(H), nodes.part_mask, parts, jobs, pk.SLOT_MIN, kmax)
    for a in (out, start, fin):
        a.setflags(write=False)
    return jobs, out, start, fin


def second_jobs(H, kmax):
    """The queue placed after a partial unplace (test 2): another seed of the contended generator."""
    return pk.busy_case(H, 60, kmax)


def half(H, kmax):
    """A seeded random half of the placed rows of reference(H, kmax), shuffled."""
    _, _, start, _ = reference(H, kmax)
    placed = np.flatnonzero(start >= 0)
    r = np.random.default_rng(1000 * H + kmax)
    return r.permutation(placed)[:len(placed) // 2]


def windows_per_node(jobs, node, start, n):
    """How many windows of the live rows land on each node."""
    cnt = np.zeros(n, np.int64)
    for q in np.flatnonzero(start >= 0):
        cnt[node[q, :max(int(jobs.nodes_k[q]), 1)]] += 1
    return cnt


def conditions(H, kmax):
    """The counts that keep a round trip from being vacuous (asserted in tests/test_unplace_tl.py)."""
    jobs, out, start, _ = reference(H, kmax)
    placed = start >= 0
    rejected = out[:, 0] == FIT_REJECTED
    return dict(placed=int(placed.sum()), multi=int((placed & (jobs.nodes_k > 1)).sum()),
                unplaced=int((~placed & ~rejected).sum()), rejected=int(rejected.sum()),
                busiest=int(windows_per_node(jobs, out, start, pk.cluster(H)[0].n).max()))


# ---- many windows on one node (test 4) -----------------------------------------------------------------
def crowd(H=64, n=40, seed=11):
    """300 one-node rows on node 7, 30 rows on single-window nodes and 12 rows of 3 nodes that all
    name node 7 again, shuffled: (jobs, node[J, 3], start[J]); kmax 3.  Demands small enough that
    nothing saturates."""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(300):
        rows.append(([7, -1, -1], 1))
    for x in range(30):
        rows.append(([8 + x, -1, -1], 1))
    for i in range(12):
        rows.append(([int(v) for v in r.permutation([7, 1 + i % 6, 39 - i % 2])], 3))
    order = r.permutation(len(rows))
    node = np.array([rows[i][0] for i in order], np.int32)
    k = np.array([rows[i][1] for i in order], np.uint16)
    j = len(order)
    jobs = synth.Jobs(r.integers(0, 9, j).astype(np.int32), r.integers(0, 4096, j).astype(np.int32),
                      r.integers(0, 3, j).astype(np.int32), r.integers(0, H * 2 + 10, j).astype(np.int32),
                      np.zeros(j, np.uint16), k)
    start = r.integers(0, H, j).astype(np.int32)
    return jobs, node, start


def flat_cluster(n, cpu=4, mem=8192, gpu=2, avail=None, mask=None):
    """n nodes with the same free columns, one partition, no release events."""
    nodes = synth.Nodes(cpu_free=np.full(n, cpu, np.int32), mem_free=np.full(n, mem, np.int32),
                        gpu_free=np.full(n, gpu, np.int32),
                        avail_min=np.full(n, wk.INF, np.int32) if avail is None else np.asarray(avail, np.int32),
                        part_mask=np.ones(n, np.uint32) if mask is None else np.asarray(mask, np.uint32))
    return nodes


def no_events(n, H, slot_min):
    z = np.zeros(0, np.int32)
    return synth.Timeline(slots=H, slot_min=slot_min, off=np.zeros(n + 1, np.int32), slot=z, cpu=z, mem=z, gpu=z)

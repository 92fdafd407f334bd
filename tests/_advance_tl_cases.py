"""Cases and the checker of fit_advance_tl, shared by tests/test_advance_tl.py and
tests/test_advance_tl_gpu.py (not a test module).  ref_advance_tl restates §2i in numpy over the dense
[n, H, 3] timeline: a slice, a broadcast and the sticky -1 `where`.  It shares nothing with the
kernels' run lists."""
import numpy as np

import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from fitgpu import synth

BASES = [(64, 8), (256, 8), (64, 1)]  # (H, kmax) of uc.reference: its final timeline is a base timeline
CUTS = (1, 7, 32, 63)                 # the advances whose cut positions the conditions count, at (64, 8)


def ref_advance_tl(tl, a, tail):
    """§2i: the dense timeline after an advance by a >= 0 slots.  tail: [n, 3] (>= -1), or None: every
    column continues its slot H - 1 value.  tl is not changed."""
    tl = np.asarray(tl, np.int32)
    n, H, _ = tl.shape
    if a == 0:
        return tl.copy()
    ap = min(a, H)
    last = tl[:, H - 1, :]
    fill = np.where(last == -1, -1, last if tail is None else np.asarray(tail, np.int32).reshape(n, 3))
    out = np.empty_like(tl)
    out[:, :H - ap] = tl[:, ap:]
    out[:, H - ap:] = fill[:, None, :]
    return out


def base(H, kmax):
    """The final timeline of uc.reference(H, kmax): rand_cluster, the warm-up queue and a contended
    multi-node queue placed on it."""
    return uc.reference(H, kmax)[3]


def level_tail(H):
    """What the caller knows without the reservations: every node's level at the loaded horizon edge."""
    return pk.start_timeline(H)[:, H - 1]


def random_tail(tl, seed):
    """Per node and column one of: -1, 0, a value below the node's maximum, and values above
    everything the node held."""
    n = tl.shape[0]
    r = np.random.default_rng(seed)
    top = tl.max(axis=1).astype(np.int64)  # [n, 3]
    pick = r.integers(0, 5, (n, 3))
    val = np.select([pick == 0, pick == 1, pick == 2, pick == 3],
                    [-1, 0, np.maximum(top, 0) // 2, top + 1 + r.integers(0, 1000, (n, 3))], top + 100000)
    return val.astype(np.int32)


def rewrite_rows(jobs, start, a, H, slot_min):
    """INTEGRATION.md's row rewrite: the recorded placements as they read after an advance by a.
    A row's window [s, e), e = min(s + d, H), becomes [max(s - a', 0), e - a'); start' =
    max(start - a', 0), wall' = (e - a' - start') * slot_min; a row with e <= a' is dropped
    (start' = -1, which fit_unplace_tl skips).  Returns (jobs', start')."""
    ap = min(a, H)
    s = np.asarray(start, np.int64)
    d = np.maximum(1, -(-jobs.wall.astype(np.int64) // slot_min))
    e = np.minimum(s + d, H)
    live = (s >= 0) & (e > ap)
    s2 = np.where(live, np.maximum(s - ap, 0), -1)
    wall2 = np.where(live, (e - ap - s2) * slot_min, jobs.wall)
    out = synth.Jobs(jobs.cpu, jobs.mem, jobs.gpu, wall2.astype(np.int32), jobs.part, jobs.nodes_k)
    return out, s2.astype(np.int32)


def cut_counts(tl, a):
    """(nodes whose cut at slot a falls exactly on a run boundary, inside a run, nodes that lose at
    least one whole run), 1 <= a < H."""
    change = (tl[:, 1:] != tl[:, :-1]).any(axis=2)  # change[:, t - 1]: slot t starts a run
    on = change[:, a - 1]
    return int(on.sum()), int((~on).sum()), int(change[:, :a].any(axis=1).sum())


# ---- long lists ------------------------------------------------------------------------------------------
STAIR_FULL, STAIR_HALF = 3, 4  # the staircase nodes of staircase()


def staircase(H=256):
    """slot_min 1, one partition, 6 nodes: 0-2 flat (node 2 usable for 100 slots only), node 3 with a
    1-cpu release at every slot 1 .. H - 1 (H runs: a full slab row at the horizon limit of its
    size), node 4 with one at every second slot, node 5 flat."""
    n = 6
    nodes = uc.flat_cluster(n, cpu=4, mem=1 << 20, gpu=2, avail=[wk.INF, wk.INF, 100, wk.INF, wk.INF, wk.INF])
    off, slot = [0], []
    for x in range(n):
        if x == STAIR_FULL:
            slot += list(range(1, H))
        elif x == STAIR_HALF:
            slot += list(range(2, H, 2))
        off.append(len(slot))
    m = len(slot)
    tline = synth.Timeline(slots=H, slot_min=1, off=np.array(off, np.int32), slot=np.array(slot, np.int32),
                           cpu=np.ones(m, np.int32), mem=np.zeros(m, np.int32), gpu=np.zeros(m, np.int32))
    return nodes, tline, wk.open_parts(1)


def staircase_dense(H=256):
    """staircase() as loaded, restated: the release events summed up to each slot."""
    nodes, tline, _ = staircase(H)
    tl = np.empty((nodes.n, H, 3), np.int32)
    tl[:, :, 0] = nodes.cpu_free[:, None]
    tl[:, :, 1] = nodes.mem_free[:, None]
    tl[:, :, 2] = nodes.gpu_free[:, None]
    t = np.arange(H)
    tl[STAIR_FULL, :, 0] += t
    tl[STAIR_HALF, :, 0] += t // 2
    tl[2, 100:] = -1
    return tl

"""Cases and the checker of fit_free_tl, shared by tests/test_free_tl.py and
tests/test_free_tl_gpu.py (not a test module).  ref_free_tl restates §2k in numpy over the dense
[n, H, 3] timeline: a `where`, a sum and a max per partition.  It shares nothing with the kernels'
run lists.  The dense timelines come from the pure-numpy and C-oracle references of the other suites
(pk.start_timeline, ac.base, ac.staircase_dense, po.ref_build_timeline), never from the engine."""
import functools

import numpy as np

import _advance_tl_cases as ac
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from fitgpu import FREE_DTYPE, synth

SUMS, MAXS = ("cpu", "mem", "gpu"), ("max_cpu", "max_mem", "max_gpu")


def ref_free_tl(tl, part_mask, parts):
    """§2k: FREE_DTYPE rows [parts, H] of the dense timeline tl [n, H, 3] under the masks part_mask[n]."""
    tl = np.asarray(tl, np.int32)
    n, H, _ = tl.shape
    mask = np.asarray(part_mask).astype(np.int64)
    is_open = (tl >= 0).all(axis=2)                                   # [n, H]
    out = np.zeros((parts, H), FREE_DTYPE)
    for p in range(parts):
        sel = (is_open & (((mask >> p) & 1) != 0)[:, None])[:, :, None]  # [n, H, 1]
        s = np.where(sel, tl.astype(np.int64), 0).sum(axis=0)         # [H, 3]
        x = np.where(sel, tl, -1).max(axis=0, initial=-1)             # [H, 3]
        out["nodes"][p] = sel[:, :, 0].sum(axis=0)
        for c in range(3):
            out[SUMS[c]][p] = s[:, c]
            out[MAXS[c]][p] = x[:, c]
    return out


def as_loaded(nodes, tline):
    """The dense timeline of a load, by the C oracle."""
    from oracle import pyoracle as po
    return po.ref_build_timeline(nodes, tline)


def conditions(ref):
    """What keeps a profile from being vacuous: (rows without an open node, partitions whose open-node
    count differs between two slots, (partition, slot) pairs whose sums differ from the next slot's)."""
    nodes = ref["nodes"]
    sums = np.stack([ref[f] for f in SUMS], axis=2)
    return (int((nodes == 0).sum()), int((nodes.max(axis=1) != nodes.min(axis=1)).sum()),
            int((sums[:, 1:] != sums[:, :-1]).any(axis=2).sum()))


def deltas(nodes, jobs, out, start, slot_min, parts, H):
    """The placement identity of §2k: per (partition, slot) the sum of the demands of the placed
    windows that cover the slot on nodes with the partition's bit: int64 [parts, H, 3]."""
    d = np.zeros((parts, H, 3), np.int64)
    for q in np.flatnonzero(start >= 0):
        s = int(start[q])
        e = min(s + max(1, -(-int(jobs.wall[q]) // slot_min)), H)
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        for x in out[q, :max(int(jobs.nodes_k[q]), 1)]:
            for p in range(parts):
                if (int(nodes.part_mask[x]) >> p) & 1:
                    d[p, s:e] += dem
    return d


# ---- the hand case of the CPU test -----------------------------------------------------------------
# 6 nodes, H = 8, columns (cpu, mem, gpu); masks: n0 1, n1 1, n2 2, n3 3, n4 0, n5 1 << 31.
#   n0: (4, 100, 1) on slots 0-3, closed from slot 4 (past avail_min)
#   n1: (2, 50, 0) on slots 0-1, (6, 50, 2) from slot 2
#   n2: (8, 10, 0) everywhere
#   n3: (1, 1, 1) on slots 0-5, (1, 1, -1) on 6-7: closed there by the one negative column
#   n4: (9, 9, 9) everywhere, but in no partition
#   n5: (3, 3, 3) everywhere, partition 31 alone
def hand_case():
    tl = np.empty((6, 8, 3), np.int32)
    tl[0, :4], tl[0, 4:] = (4, 100, 1), -1
    tl[1, :2], tl[1, 2:] = (2, 50, 0), (6, 50, 2)
    tl[2] = (8, 10, 0)
    tl[3, :6], tl[3, 6:] = (1, 1, 1), (1, 1, -1)
    tl[4] = (9, 9, 9)
    tl[5] = (3, 3, 3)
    mask = np.array([1, 1, 2, 3, 0, 1 << 31], np.uint32)
    return tl, mask


def _rows(rows):
    return np.array(rows, FREE_DTYPE)


# (cpu, mem, gpu, nodes, max_cpu, max_mem, max_gpu) at slots 0 .. 7
HAND_ROWS = {
    0: _rows([(7, 151, 2, 3, 4, 100, 1)] * 2 + [(11, 151, 4, 3, 6, 100, 2)] * 2 + [(7, 51, 3, 2, 6, 50, 2)] * 2 +
             [(6, 50, 2, 1, 6, 50, 2)] * 2),
    1: _rows([(9, 11, 1, 2, 8, 10, 1)] * 6 + [(8, 10, 0, 1, 8, 10, 0)] * 2),
    2: _rows([(0, 0, 0, 0, -1, -1, -1)] * 8),
    31: _rows([(3, 3, 3, 1, 3, 3, 3)] * 8),
}


# ---- masks and closed columns by hand (GPU test 2) --------------------------------------------------
MASKS_H, MASKS_L = 16, 5


def masks_case():
    """n = 10, H = 16: masks 1, 2, 3, 1 << 31, 1 | 1 << 31 and 0; node 4 with gpu_free -5 (closed
    everywhere), node 5 with avail_min 0, node 6 cut mid-horizon, release events on nodes 0 and 2."""
    B = 1 << 31
    nodes = synth.Nodes(cpu_free=np.array([4, 6, 8, 2, 9, 9, 5, 7, 3, 11], np.int32),
                        mem_free=np.arange(10, dtype=np.int32) * 100 + 50,
                        gpu_free=np.array([1, 0, 2, 1, -5, 1, 1, 0, 4, 1], np.int32),
                        avail_min=np.array([wk.INF, wk.INF, wk.INF, wk.INF, wk.INF, 0, 7 * MASKS_L, wk.INF, wk.INF,
                                            wk.INF], np.int32),
                        part_mask=np.array([1, 2, 3, B, 1, 1, 1 | B, 0, B | 1, 2], np.uint32))
    off = np.array([0, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3], np.int32)
    tline = synth.Timeline(slots=MASKS_H, slot_min=MASKS_L, off=off, slot=np.array([3, 9, 5], np.int32),
                           cpu=np.array([2, 1, 4], np.int32), mem=np.array([0, 10, 0], np.int32),
                           gpu=np.array([0, 1, 0], np.int32))
    return nodes, tline, wk.open_parts(2)


# ---- chunk seams (GPU test 5) -------------------------------------------------------------------------
SEAM_N = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 5000)


def seam_cluster(n, spread=False):
    """n flat nodes, cpu_free[x] = x + 1.  spread: masks 1 << (x % 7), every 11th node in partition 7 too."""
    x = np.arange(n)
    mask = np.ones(n, np.uint32)
    if spread:
        mask = ((np.uint32(1) << (x % 7).astype(np.uint32)) | np.where(x % 11 == 0, 1 << 7, 0)).astype(np.uint32)
    return uc.flat_cluster(n, cpu=(x + 1).astype(np.int32), mem=8192, gpu=2, mask=mask)


# ---- lists on both sides of the header's four runs, built by hand (GPU test 3) -------------------------
def runs_cluster(H=64, counts=(1, 2, 3, 4, 5, 6, 8, 9, 16, 17, 33)):
    """One partition, slot_min 1: node x has counts[x] runs (a 1-cpu release at each of the first
    counts[x] - 1 slots from 1), so lists end on each side of TL_HEAD and of the powers of two the
    binary search of the long lists splits at."""
    n = len(counts)
    nodes = uc.flat_cluster(n, cpu=1, mem=64, gpu=0)
    off, slot = [0], []
    for k in counts:
        slot += list(range(1, k))
        off.append(len(slot))
    m = len(slot)
    tline = synth.Timeline(slots=H, slot_min=1, off=np.array(off, np.int32), slot=np.array(slot, np.int32),
                           cpu=np.ones(m, np.int32), mem=np.zeros(m, np.int32), gpu=np.zeros(m, np.int32))
    return nodes, tline, wk.open_parts(1)


@functools.lru_cache(maxsize=None)
def loaded_reference(H, parts):
    """(dense timeline, rows) of pk.cluster(H) as loaded."""
    nodes, tline, _ = pk.cluster(H)
    tl = as_loaded(nodes, tline)
    ref = ref_free_tl(tl, nodes.part_mask, parts)
    ref.setflags(write=False)
    return tl, ref


@functools.lru_cache(maxsize=None)
def base_reference(H, kmax, parts):
    """The rows of ac.base(H, kmax): pk.cluster(H) after the warm-up queue and a multi-node queue."""
    ref = ref_free_tl(ac.base(H, kmax), pk.cluster(H)[0].part_mask, parts)
    ref.setflags(write=False)
    return ref

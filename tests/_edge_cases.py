"""Placement inputs at the score caps and the int32 edges, shared by tests/test_edges.py (CPU: the
inputs do what they claim, and a wrong key would be noticed), tests/test_edges_gpu.py (the HIP engines
against the oracle) and tools/fuzz_sweep.py --edges.

The best-fit score is min(gpu_resid, 255) << 24 | min(cpu_resid, 4095) << 12 |
min(mem_resid >> 10, 4095).  The random cases of the rest of the suite keep every residual far below
its cap and every memory residual >= 1 GiB, so none of the three saturating minima, a score of 0, a
score of 0xFFFFFFFF or an int32 extreme ever reaches a kernel from them.  edge_case() draws from
exactly those corners; the family is seed % 4:

  0  caps      residuals straddle one cap while the more significant fields sit far above theirs;
               level (seed // 4) % 3: gpu around 255 / cpu around 4095 / memory around 4095 GiB
  1  zero      nodes of a handful of shapes, jobs demanding exactly those shapes: winners score 0
               (also with a residual below 1 GiB, and on nodes already filled to (0, 0, 0))
  2  extremes  node fields and demands from the ends of int32
  3  capped    every residual above every cap: each feasible key is 0xFFFFFFFF << 32 | position,
               one bit pattern short of "infeasible" in the high word, and the node id alone decides

Partition limits are unlimited; avail_min and wall come from AVAIL / WALL in every family.
"""
import numpy as np

from fitgpu import synth

INT32_MAX = 2**31 - 1
INT32_MIN = -2**31
AVAIL = np.array([INT32_MAX, INT32_MAX - 1, 100, 0, -1, INT32_MIN], np.int64)
AVAIL_P = [0.60, 0.10, 0.15, 0.05, 0.05, 0.05]
WALL = np.array([0, 1, 100, 101, INT32_MAX - 1, INT32_MAX], np.int64)
WALL_P = [0.30, 0.25, 0.20, 0.10, 0.075, 0.075]
NODE_X = np.array([INT32_MIN, -5, -1, 0, 1, 2**30, INT32_MAX - 1, INT32_MAX], np.int64)
NODE_XP = [0.05, 0.05, 0.05, 0.10, 0.10, 0.20, 0.20, 0.25]
DEMAND_X = np.array([0, 1, 2**30, 2**30 + 1, INT32_MAX - 1, INT32_MAX], np.int64)
DEMAND_XP = [0.30, 0.30, 0.15, 0.10, 0.075, 0.075]
RELEASE_X = np.array([0, 1, 2**30, INT32_MAX], np.int64)
MEM_CAP_MIB = 4095 << 10  # 4,193,280 MiB: the memory residual whose GiB count is the cap


def score(gr, cr, mr):
    """The SPEC §2 score of residuals (arrays or scalars, >= 0), as uint64."""
    gr, cr, mr = (np.asarray(a, np.int64) for a in (gr, cr, mr))
    return (np.minimum(gr, 255).astype(np.uint64) << np.uint64(24)) | \
           (np.minimum(cr, 4095).astype(np.uint64) << np.uint64(12)) | \
           np.minimum(mr >> 10, 4095).astype(np.uint64)


def _i32(a):
    return np.asarray(a, np.int64).astype(np.int32)


def _masks(r, n, p, disjoint):
    if disjoint:  # exactly one partition bit per node: the class engine's domain
        return (np.uint32(1) << r.integers(0, p, n).astype(np.uint32)).astype(np.uint32)
    mask = r.integers(0, 1 << p, n).astype(np.uint32)  # overlapping, some empty
    mask[r.random(n) < 0.05] = 0
    return mask


def _pick_shapes(r, shapes, j):
    """j demands drawn from the rows of `shapes` ([S, 3]: cpu, mem, gpu): few demand classes."""
    s = np.asarray(shapes, np.int64)[r.integers(0, len(shapes), j)]
    return s[:, 0], s[:, 1], s[:, 2]


def zero256_case(kmax=1):
    """256 identical nodes in one partition, 400 jobs that each fit one node exactly.

    The persistent engine plans a component of `len` rows as (engine.cpp, run_persistent's plan):
    ks = KS = 16 keys per (job, block-slice), slices = MAX_SLICES * KS / ks = 8,
    sub = max(MIN_SUB = 64, ceil(len / (SCAN_WAVES * slices))) = max(64, ceil(256 / 64)) = 64 rows per
    wave sub-slice, nslice = ceil(256 / (8 * 64)) = 1.  So waves 0..3 of the one scan block walk 64
    rows each, every one of score 0 for the first job: once a wave's list holds KS = 16 of them the
    candidate limit `K-th score - 1` wraps to 0xffffffff, and the 48 rows that follow in the same
    sub-slice are the spurious inserts the insertion network has to drop.  Each placed job turns one
    node into (0, 0, 0); after 256 jobs nothing fits."""
    n, j = 256, 400
    nodes = synth.Nodes(np.full(n, 12, np.int32), np.full(n, 6144, np.int32), np.full(n, 2, np.int32),
                        np.full(n, INT32_MAX, np.int32), np.ones(n, np.uint32))
    k = np.ones(j, np.uint16)
    if kmax > 1:
        k[1::3] = 2
    jobs = synth.Jobs(np.full(j, 12, np.int32), np.full(j, 6144, np.int32), np.full(j, 2, np.int32),
                      np.zeros(j, np.int32), np.zeros(j, np.uint16), k)
    parts = synth.Partitions(*(np.full(1, -1, np.int32) for _ in range(3)))
    return nodes, jobs, parts, kmax


def edge_case(seed, timeline=False, disjoint=False):
    """The same tuples as test_fuzz_gpu.random_case: (nodes, jobs, parts, kmax), or with
    timeline=True (nodes, timeline, jobs, parts).  Seed 1 without a timeline is zero256_case()."""
    fam, level = seed % 4, (seed // 4) % 3
    if seed == 1 and not timeline:
        return zero256_case(kmax=2)
    r = np.random.default_rng([seed, int(timeline), int(disjoint)])
    # a timeline case needs contention (jobs that start in a later slot): few nodes, many jobs
    n = int(r.integers(1, 121 if timeline else 701))
    j = int(r.integers(300, 1501)) if timeline else int(r.integers(1, 1501))
    p = int(r.integers(1, 5))
    kmax = 1 if timeline else int(r.choice([1, 2, 8]))
    if fam == 0 and level == 0 and not timeline:
        n = min(n, max(1, j // 3))  # nodes fill up, so the choice moves on to the capped ones
    if fam == 2:
        j = max(j, 60)  # enough jobs that some find a node and some do not

    slots = slot_min = 0
    if timeline:
        slots, slot_min = int(r.choice([16, 64, 1024])), int(r.choice([1, 5, 30]))

    if fam == 0:
        if level == 0:
            gpu = r.integers(250, 264, n)
            cpu = r.integers(4, 24, n)
            mem = r.integers(4000, 40000, n)
        elif level == 1:
            gpu = r.integers(5000, 6000, n)  # stays above 255 + every job's gpus
            cpu = r.integers(4090, 4112, n)
            mem = r.integers(1000, 8000, n)
        else:
            gpu = r.integers(5000, 6000, n)
            cpu = r.integers(25000, 26000, n)  # stays above 4095 + every job's cpus
            # A node below the cap beats every node above it and, never full, goes on winning.  So
            # every node starts above the cap, a few thousand MiB or more, and the winner (the lowest
            # id while all tie) sinks through it, slowly: two shapes in three ask for no memory.
            mem = MEM_CAP_MIB + np.where(r.random(n) < 0.5, r.integers(1, 4000, n), r.integers(4000, 60000, n))
        shapes = np.stack([r.integers(0, 12, 24), r.integers(0, 3000, 24), r.integers(0, 4, 24)], axis=1)
        if level == 2:
            shapes[r.random(24) < 0.67, 1] = 0
        jc, jm, jg = _pick_shapes(r, shapes, j)
    elif fam == 1:
        ns = int(r.integers(3, 7))
        shapes = np.stack([r.integers(1, 65, ns), r.integers(0, 9, ns) * 1024 + r.choice([0, 300, 1023], ns),
                           r.integers(0, 5, ns)], axis=1)
        if r.random() < 0.5:
            shapes[0] = 0  # nodes with nothing free, jobs that ask for nothing
        # twins of a shape whose memory differs by less than 1 GiB: a score of 0 with a residual
        twins = shapes.copy()
        twins[:, 1] = (twins[:, 1] >> 10 << 10) + r.choice([0, 300, 1023], ns)
        node_shapes = np.concatenate([shapes, twins])
        pick = node_shapes[r.integers(0, len(node_shapes), n)]
        cpu, mem, gpu = pick[:, 0], pick[:, 1], pick[:, 2]
        jc, jm, jg = _pick_shapes(r, shapes, j)
    elif fam == 2:
        cpu, mem, gpu = (r.choice(NODE_X, n, p=NODE_XP) for _ in range(3))
        shapes = r.choice(DEMAND_X, (48, 3), p=DEMAND_XP)
        jc, jm, jg = _pick_shapes(r, shapes, j)
    else:
        cpu, mem, gpu = np.full(n, 10**6), np.full(n, INT32_MAX), np.full(n, 10**4)
        jc, jm, jg = (r.integers(0, 3, j) for _ in range(3))

    avail = r.choice(AVAIL, n, p=AVAIL_P)
    mask = _masks(r, n, p, disjoint)
    parts = synth.Partitions(*(np.full(p, -1, np.int32) for _ in range(3)))
    if timeline:
        span = slots * slot_min
        wall = r.choice(np.concatenate([WALL, [span, span + 1]]), j,
                        p=[0.25, 0.25, 0.15, 0.10, 0.06, 0.06, 0.08, 0.05])
    else:
        wall = r.choice(WALL, j, p=WALL_P)
    nodes_k = np.ones(j, np.uint16) if timeline else r.integers(1, kmax + 1, j).astype(np.uint16)
    jobs = synth.Jobs(_i32(jc), _i32(jm), _i32(jg), _i32(wall), r.integers(0, p, j).astype(np.uint16), nodes_k)
    if not timeline:
        return synth.Nodes(_i32(cpu), _i32(mem), _i32(gpu), _i32(avail), mask), jobs, parts, kmax

    # release events: 0-3 per node, sorted slots in [-2, slots + 4) as in the fuzz
    lifted = fam in (0, 3)
    ev = r.integers(1 if lifted else 0, 4, n)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(ev)
    e = int(off[-1])
    slot = np.concatenate([np.sort(r.integers(-2, slots + 4, k)) for k in ev]) if e else np.zeros(0, np.int64)
    if fam == 1:  # what a finished job of one of the shapes gives back
        rc, rm, rg = _pick_shapes(r, shapes, e)
    elif fam == 2:
        rc, rm, rg = (r.choice(RELEASE_X, e) for _ in range(3))
    else:
        rc, rm, rg = r.integers(0, 3, e), r.integers(0, 2048, e), r.integers(0, 2, e)
    if lifted:
        # The caps family and the all-capped family have room for every job at once, so nothing
        # would ever wait.  Here a node starts almost empty and its first release, in slot >= 1,
        # lifts it to the family's values: every job that asks for anything starts in a later slot,
        # at a residual on or beyond the caps.
        first = off[:-1]
        lift = r.integers(1, max(2, slots // 2), n)
        slot = np.maximum(slot, np.repeat(lift, ev))  # (still sorted within a node)
        slot[first] = lift
        rc[first], rm[first], rg[first] = cpu, mem, gpu
        cpu, mem, gpu = r.integers(0, 2, n), r.integers(0, 1500, n), np.zeros(n, np.int64)
    tl = synth.Timeline(slots, slot_min, off, _i32(slot), _i32(rc), _i32(rm), _i32(rg))
    return synth.Nodes(_i32(cpu), _i32(mem), _i32(gpu), _i32(avail), mask), tl, jobs, parts

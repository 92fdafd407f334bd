"""fit_preempt_k on the GPU against ref_preempt_k (tests/_preempt_k_cases.py, a numpy int64
restatement of DESIGN.md §2m): rows, out_node and out_victims compared field for field through the
host and the device entry point, on shapes that cross every wave, tile, slice and chunk edge of
k_prek_walk, at every list capacity the walk is built for, list lengths around the walk's four-entry
loads, int32 edge values, the three relations of §2m (fit_preempt at need 1, the oracle's placement
of a FITS row, fit_place on the raised table of an EVICT row), and the state and argument errors."""
import ctypes as C

import numpy as np
import pytest

import _preempt_cases as pc
import _preempt_k_cases as pk
import fitgpu
from _devarray import DevArray
from fitgpu import EVICT_K_DTYPE, Engine, FitError, _lib, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INF, I32MIN = synth.INT32_MAX, -2**31
ONE_PART = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
VCOLS = ("off", "prio", "cpu", "mem", "gpu")
JCOLS = ("cpu", "mem", "gpu", "wall", "part")


def preempt_k_both(e, jobs, prio, kmax=pk.KMAX):
    """Engine.preempt_k through host pointers and through device pointers: the same rows and picks.
    The device outputs start from a pattern, so an entry the call leaves unwritten shows."""
    rows, node, vic = e.preempt_k(jobs, prio, kmax)
    assert node.shape == vic.shape == (jobs.j, kmax)
    cols = [DevArray(getattr(jobs, f)) for f in JCOLS]
    nk = None if jobs.nodes_k is None else DevArray(np.asarray(jobs.nodes_k, np.uint16))
    out = DevArray(np.full(jobs.j * 10, -7, np.int32).view(EVICT_K_DTYPE))
    dn, dv = DevArray(np.full((jobs.j, kmax), -7, np.int32)), DevArray(np.full((jobs.j, kmax), -7, np.int32))
    ms = e.preempt_k_device(*cols, nk, DevArray(np.asarray(prio, np.int32)), out, dn, dv, kmax=kmax)
    assert ms > 0 and e.preempt_k_ms() == ms
    assert np.array_equal(rows, out.numpy()), "host and device entry points differ in the rows"
    assert np.array_equal(node, dn.numpy()) and np.array_equal(vic, dv.numpy()), "... in the picks"
    return rows, node, vic


def assert_same(got, want):
    (rows, node, vic), (wrows, wnode, wvic) = got, want
    for f in EVICT_K_DTYPE.names:
        bad = np.flatnonzero(rows[f] != wrows[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {rows[bad[0]]}, want {wrows[bad[0]]}"
    for name, a, b in (("out_node", node, wnode), ("out_victims", vic, wvic)):
        bad = np.flatnonzero((a != b).any(1))
        assert bad.size == 0, f"{name}: {bad.size} jobs differ, first {bad[0]}: got {a[bad[0]]}, want {b[bad[0]]}"


def load(e, c, device=False):
    e.load_nodes(c.nodes)
    e.load_partitions(c.parts)
    if device and c.victims is not None:
        e.load_victims_device(*(DevArray(getattr(c.victims, f)) for f in VCOLS))
    else:
        e.load_victims(c.victims)


def jobs_of(rows):
    """synth.Jobs and priorities from (cpu, mem, gpu, wall, part, prio, nodes_k) rows."""
    a = np.array(rows, np.int64).reshape(-1, 7)
    return (synth.Jobs(*(a[:, k].astype(np.int32) for k in range(4)), a[:, 4].astype(np.uint16), a[:, 6].astype(np.uint16)),
            a[:, 5].astype(np.int32))


def plain_nodes(cpu, mask=None):
    """Nodes with the given free cpus, nothing else free and no walltime bound, in partition 0."""
    n = len(cpu)
    return synth.Nodes(np.asarray(cpu, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32),
                       np.ones(n, np.uint32) if mask is None else np.asarray(mask, np.uint32))


def check(e, c, kmax=pk.KMAX, device=False):
    """Load the case, run both entry points, compare with the reference; returns the rows and picks."""
    load(e, c, device)
    got = preempt_k_both(e, c.jobs, c.prio, kmax)
    assert_same(got, pk.ref_preempt_k(c.nodes, c.victims, c.parts, c.jobs, c.prio, kmax))
    return got


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


# ---- 1. the hand-written and the packed random cases ---------------------------------------------
def test_hand_written_case_gives_the_literal_rows(engine):
    c = pk.hand_case_k()
    load(engine, c)
    got = preempt_k_both(engine, c.jobs, c.prio)
    assert_same(got, pk.hand_arrays())
    load(engine, c, device=True)
    assert_same(preempt_k_both(engine, c.jobs, c.prio), got)


# (65, 65): seed 5 with the count at 10, see tests/test_preempt_k.py
@pytest.mark.parametrize("one_component", [False, True])
@pytest.mark.parametrize("n,j,seed,evict,full_tie", [(65, 65, 5, 10, False), (257, 128, 0, 20, True), (1000, 300, 0, 20, True)])
def test_packed_random_cases(engine, n, j, seed, evict, full_tie, one_component):
    c = pk.packed_case_k(n, j, seed, one_component)
    want, stats = pk.packed_ref_k(n, j, seed, one_component)
    pk.rich_enough_k(want[0], stats, evict, full_tie)  # on the reference alone: a comparison of nothing interesting fails
    load(engine, c, device=one_component)
    assert_same(preempt_k_both(engine, c.jobs, c.prio), want)


# ---- 2. shapes at the seams ---------------------------------------------------------------------
# n: the wave sub-slices (8 waves share a slice's rows), the four-row loads and the 256-row node slices;
# J: the 64-job tiles, and above 256 jobs on several components the component-ordered job list.
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000])
def test_shapes_at_the_seams(engine, n):
    evict = picks = 0
    for one_component in (False, True):
        for i, j in enumerate((1, 63, 64, 65, 257)):
            c = pk.packed_case_k(n, j, 0, one_component)
            want, _ = pk.packed_ref_k(n, j, 0, one_component)
            load(engine, c, device=i == 0)  # the table depends on j through the generator's seed: load each
            assert_same(preempt_k_both(engine, c.jobs, c.prio), want)
            evict += int(((want[0]["code"] == pk.EVICT) & (want[0]["need"] >= 2)).sum())
            picks += int((want[1] >= 0).sum())
    if n >= 63:
        assert evict >= 20 and picks >= 200, (evict, picks)
    elif n >= 7:
        assert evict > 0 and picks > 0, (evict, picks)


@pytest.mark.parametrize("kmax", [1, 2, 3, 4, 5, 8])
def test_every_list_capacity(engine, kmax):
    """The walk keeps 1, 2, 4 or 8 keys and stores kmax of them: every kmax that selects another kernel
    or another store count, with nodes_k up to it."""
    c = pk.packed_case_k(257, 128)
    nk = np.minimum(np.asarray(c.jobs.nodes_k), kmax)
    c = pc.Case(c.nodes, c.victims, c.parts, pk.with_k(c.jobs, nk), c.prio)
    rows, node, _ = check(engine, c, kmax)
    assert ((rows["code"] == pk.EVICT) & (rows["need"] == kmax)).any() and node.shape[1] == kmax


def test_picks_across_node_slices(engine):
    """5,000 nodes of one component under 64 jobs: one job tile, so the rows are cut into about twenty
    slices of some 250.  Nodes 1100, 1101 and 1102 are emptied: a job of up to three nodes finds all its
    picks in one slice, whose list alone must hold them; a wider job takes these three and then nodes
    thousands of ids away."""
    c = pk.packed_case_k(5000, 64, 0, True)
    cols = [a.copy() for a in (c.nodes.cpu_free, c.nodes.mem_free, c.nodes.gpu_free, c.nodes.avail_min, c.nodes.part_mask)]
    for col, val in zip(cols, (128, 1 << 20, 8, INF, 3 << 2)):  # in both partitions of the component
        col[1100:1103] = val
    c = pc.Case(synth.Nodes(*cols), c.victims, c.parts, c.jobs, c.prio)
    want = pk.ref_preempt_k(c.nodes, c.victims, c.parts, c.jobs, c.prio, pk.KMAX)
    rows, node, _ = want
    multi = np.flatnonzero(np.isin(rows["code"], (pk.FITS, pk.EVICT)) & (rows["need"] >= 2))
    span = np.array([node[q, :rows["need"][q]].max() - node[q, :rows["need"][q]].min() for q in multi])
    assert (span >= 2500).sum() >= 3 and (span <= 2).sum() >= 3, span
    assert ((rows["code"] == pk.EVICT) & (rows["fit"] == 3)).any()
    load(engine, c)
    assert_same(preempt_k_both(engine, c.jobs, c.prio), want)


def test_a_batch_above_one_chunk_of_positions(engine):
    """16,800 jobs: the walk and the final run twice, the second time over 416 positions of the
    component-ordered job list.  Every job is judged alone, so the 700-job case repeated 24 times has
    the reference's rows and picks repeated 24 times."""
    c = pk.packed_case_k(257, 700)
    want, _ = pk.packed_ref_k(257, 700)
    reps = 24
    jobs = synth.Jobs(*(np.tile(getattr(c.jobs, f), reps) for f in JCOLS + ("nodes_k",)))
    assert jobs.j > 16384 and len(np.unique(c.jobs.part)) > 2
    load(engine, c)
    got = preempt_k_both(engine, jobs, np.tile(c.prio, reps))
    assert_same(got, (np.tile(want[0], reps), np.tile(want[1], (reps, 1)), np.tile(want[2], (reps, 1))))


# ---- 3. need at its edges -----------------------------------------------------------------------
def edge_table():
    """Seven nodes: 0 and 1 have 4 cpus free, 2 and 3 a victim of priority 1 that holds 4, 4 one of
    priority 100, 5 nothing at all, 6 is in no partition.  members 6; for a job of 4 cpus at priority
    50: fit 2, able 2, outranked 1; at priority 200: able 3."""
    nodes = plain_nodes([4, 4, 0, 0, 0, 0, 4], [1, 1, 1, 1, 1, 1, 0])
    return nodes, pc.victims_of([[], [], [(1, 4, 0, 0)], [(1, 4, 0, 0)], [(100, 4, 0, 0)], [], [(1, 4, 0, 0)]])


def test_need_at_fit_at_fit_plus_able_and_at_members(engine):
    nodes, v = edge_table()
    #                  cpu mem gpu wall part prio need
    jobs, prio = jobs_of([(4, 0, 0, 0, 0, 50, 2),    # need == fit: FITS at the boundary
                          (4, 0, 0, 0, 0, 50, 3),    # one more: the first eviction
                          (4, 0, 0, 0, 0, 50, 4),    # need == fit + able exactly
                          (4, 0, 0, 0, 0, 50, 5),    # one more: NONE, with fit + able = need - 1
                          (4, 0, 0, 0, 0, 200, 5),   # node 4 can be freed too: need == fit + able
                          (4, 0, 0, 0, 0, 200, 6),   # need == members, but node 5 has nothing to free
                          (0, 0, 0, 0, 0, 0, 6),     # the all-zero demand: need == members == fit
                          (0, 0, 0, 0, 0, 0, 7)])    # members < need
    rows, node, vic = check(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    want = [((pk.FITS, 2, 0, 0, 0, 6, 2, 2, 1, 0), [0, 1], [0, 0]),
            ((pk.EVICT, 3, 1, 1, 1, 6, 2, 2, 1, 0), [0, 1, 2], [0, 0, 1]),
            ((pk.EVICT, 4, 2, 2, 1, 6, 2, 2, 1, 0), [0, 1, 2, 3], [0, 0, 1, 1]),
            ((pk.NONE, 5, 0, 0, 0, 6, 2, 2, 1, 0), [], []),
            ((pk.EVICT, 5, 3, 3, 100, 6, 2, 3, 0, 0), [0, 1, 2, 3, 4], [0, 0, 1, 1, 1]),
            ((pk.NONE, 6, 0, 0, 0, 6, 2, 3, 0, 0), [], []),
            ((pk.FITS, 6, 0, 0, 0, 6, 6, 0, 0, 0), [2, 3, 4, 5, 0, 1], [0] * 6),  # the emptiest first
            ((pk.NONE, 7, 0, 0, 0, 6, 6, 0, 0, 0), [], [])]
    for q, (r, n, x) in enumerate(want):
        assert tuple(int(a) for a in rows[q]) == r, (q, rows[q])
        assert node[q].tolist() == n + [-1] * (8 - len(n)) and vic[q].tolist() == x + [0] * (8 - len(x)), (q, node[q], vic[q])


@pytest.mark.parametrize("nodes_k", [1, 0, None])
def test_need_one_at_kmax_eight_leaves_the_other_entries_empty(engine, nodes_k):
    c = pk.packed_case_k(257, 128)
    jobs = pk.with_k(c.jobs, None if nodes_k is None else np.full(c.jobs.j, nodes_k))
    rows, node, vic = check(engine, pc.Case(c.nodes, c.victims, c.parts, jobs, c.prio))
    assert (rows["need"] == 1).all() and (node[:, 1:] == -1).all() and not vic[:, 1:].any()
    assert (rows["code"] == pk.EVICT).sum() >= 20 and (node[:, 0] >= 0).sum() >= 40


def test_eight_copies_of_one_node_pick_the_lowest_ids(engine):
    nodes = plain_nodes([2] * 8)
    v = pc.victims_of([[(1, 2, 0, 0), (2, 4, 0, 0)]] * 8)
    jobs, prio = jobs_of([(8, 0, 0, 0, 0, 9, 3), (4, 0, 0, 0, 0, 9, 8), (2, 0, 0, 0, 0, 9, 3)])
    rows, node, vic = check(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    assert tuple(int(a) for a in rows[0]) == (pk.EVICT, 3, 3, 6, 2, 8, 0, 8, 0, 0)
    assert node[0].tolist() == [0, 1, 2] + [-1] * 5 and vic[0].tolist() == [2, 2, 2] + [0] * 5
    assert node[1].tolist() == list(range(8)) and vic[1].tolist() == [1] * 8 and rows[1]["victims"] == 8
    assert rows[2]["code"] == pk.FITS and node[2].tolist() == [0, 1, 2] + [-1] * 5


LENS = (0, 1, 63, 64, 65, 300)


def test_list_lengths_on_need_nodes_at_once(engine):
    """Partition p has three nodes without a free cpu whose lists have LENS[p] entries of priorities 0,
    1, 2, ..., all of them holding nothing but the last, which holds 8 cpus: only the whole list frees
    enough, on all three picks at once.  A job at the priority of the last entry finds them outranked."""
    P = len(LENS)
    lists = [[(i, 8 if i == ln - 1 else 0, 0, 0) for i in range(ln)] for ln in LENS for _ in range(3)]
    nodes = plain_nodes([0] * (3 * P), [1 << p for p in range(P) for _ in range(3)])
    parts = synth.Partitions(*(np.full(P, -1, np.int32) for _ in range(3)))
    jobs, prio = jobs_of([(8, 0, 0, 0, p, pr, 3) for p in range(P) for pr in (LENS[p], LENS[p] - 1)])
    rows, node, vic = check(engine, pc.Case(nodes, pc.victims_of(lists), parts, jobs, prio))
    for p, ln in enumerate(LENS):
        hi, lo = rows[2 * p], rows[2 * p + 1]
        if ln == 0:
            assert tuple(int(a) for a in hi) == tuple(int(a) for a in lo) == (pk.NONE, 3, 0, 0, 0, 3, 0, 0, 0, 0)
            continue
        assert tuple(int(a) for a in hi) == (pk.EVICT, 3, 3, 3 * ln, ln - 1, 3, 0, 3, 0, 0), (ln, hi)
        assert node[2 * p, :3].tolist() == [3 * p, 3 * p + 1, 3 * p + 2] and vic[2 * p, :3].tolist() == [ln] * 3
        assert tuple(int(a) for a in lo) == (pk.NONE, 3, 0, 0, 0, 3, 0, 0, 3, 0), (ln, lo)


# ---- 4. edge values -----------------------------------------------------------------------------
def test_priorities_at_the_int32_ends(engine):
    nodes = plain_nodes([0, 0, 0])
    v = pc.victims_of([[(I32MIN, 4, 0, 0), (INF, 4, 0, 0)], [(INF, 8, 0, 0)], [(I32MIN, 2, 0, 0), (I32MIN + 1, 2, 0, 0)]])
    jobs, prio = jobs_of([(4, 0, 0, 0, 0, I32MIN, 2), (4, 0, 0, 0, 0, I32MIN + 1, 2), (4, 0, 0, 0, 0, I32MIN + 2, 2),
                          (4, 0, 0, 0, 0, INF, 2), (4, 0, 0, 0, 0, INF, 3), (2, 0, 0, 0, 0, I32MIN + 1, 2)])
    rows, node, vic = check(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    got = [tuple(int(a) for a in r) for r in rows]
    assert got[0] == (pk.NONE, 2, 0, 0, 0, 3, 0, 0, 3, 0)                 # a job at INT32_MIN evicts nothing
    assert got[1] == (pk.NONE, 2, 0, 0, 0, 3, 0, 1, 2, 0)                 # one above: node 0 alone
    assert got[2] == (pk.EVICT, 2, 2, 3, I32MIN + 1, 3, 0, 2, 1, 0)       # node 0 (top INT32_MIN) before node 2
    assert node[2, :2].tolist() == [0, 2] and vic[2, :2].tolist() == [1, 2]
    assert got[3] == got[2]                                               # INT32_MAX does not evict INT32_MAX
    assert got[4] == (pk.NONE, 3, 0, 0, 0, 3, 0, 2, 1, 0)
    assert got[5] == (pk.EVICT, 2, 2, 2, I32MIN, 3, 0, 2, 1, 0) and node[5, :2].tolist() == [2, 0]  # a top of INT32_MIN; node 2 the tighter


def test_sums_are_exact_the_residual_is_clamped_and_the_zero_demand_fits(engine):
    """Nodes 0 and 2: INT32_MAX free cpus and three victims of INT32_MAX cpus and 1 MiB each; node 1 the
    same free cpus, its victims hold no cpu.  A job of INT32_MAX - 5 cpus and 3 MiB needs all three
    victims on each: the sum on node 0 is 4 (2^31 - 1), its residual min(sum, INT32_MAX) - demand = 5, as
    node 1's: the ids decide.  A sum that wrapped would not fit; an unclamped residual would lose."""
    nodes = synth.Nodes(np.full(3, INF, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32), np.full(3, INF, np.int32),
                        np.ones(3, np.uint32))
    v = pc.victims_of([[(1, INF, 1, 0)] * 3, [(1, 0, 1, 0)] * 3, [(1, INF, 1, 0)] * 3])
    jobs, prio = jobs_of([(INF - 5, 3, 0, 0, 0, 2, 2), (INF, 2, 0, 0, 0, 2, 3), (INF, 0, 0, 0, 0, 2, 3), (0, 0, 0, 0, 0, 0, 2)])
    rows, node, vic = check(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    assert tuple(int(a) for a in rows[0]) == (pk.EVICT, 2, 2, 6, 1, 3, 0, 3, 0, 0)
    assert node[0, :2].tolist() == [0, 1] and vic[0, :2].tolist() == [3, 3]
    assert tuple(int(a) for a in rows[1]) == (pk.EVICT, 3, 3, 6, 1, 3, 0, 3, 0, 0) and vic[1, :3].tolist() == [2, 2, 2]
    assert tuple(int(a) for a in rows[2]) == (pk.FITS, 3, 0, 0, 0, 3, 3, 0, 0, 0) and node[2, :3].tolist() == [0, 1, 2]
    assert tuple(int(a) for a in rows[3]) == (pk.FITS, 2, 0, 0, 0, 3, 3, 0, 0, 0) and node[3, :2].tolist() == [0, 1]


# ---- 5. the relations of §2m --------------------------------------------------------------------
@pytest.mark.parametrize("kmax", [1, 8])
def test_at_need_one_the_row_is_fit_preempts(engine, kmax):
    c = pc.packed_case(1000, 300)
    load(engine, c)
    want = engine.preempt(c.jobs, c.prio)
    rows, node, vic = preempt_k_both(engine, c.jobs, c.prio, kmax)
    for f in ("code", "victims", "top_prio", "members", "fit", "able", "outranked"):
        assert np.array_equal(rows[f], want[f]), f
    assert np.array_equal(node[:, 0], want["node"]) and np.array_equal(vic[:, 0], want["victims"])
    assert (want["code"] == pk.EVICT).sum() >= 20 and (want["code"] == pk.FITS).any() and (want["code"] == pk.NONE).any()


def one_job(jobs, q):
    return synth.Jobs(*(getattr(jobs, f)[q:q + 1].copy() for f in JCOLS + ("nodes_k",)))


def test_a_fits_rows_picks_are_the_oracles_placement(engine):
    c = pk.packed_case_k(1000, 300, 0, True)
    want, _ = pk.packed_ref_k(1000, 300, 0, True)
    load(engine, c)
    rows, node, vic = preempt_k_both(engine, c.jobs, c.prio)
    fits = np.flatnonzero((rows["code"] == pk.FITS) & (rows["need"] >= 2))
    assert len(fits) >= 10
    for q in fits[:: max(1, len(fits) // 10)][:10]:
        ref, _, _ = po.ref_place(c.nodes, one_job(c.jobs, q), c.parts, pk.KMAX)
        assert node[q].tolist() == ref[0].tolist() and ref[0, 0] >= 0, (q, rows[q], node[q], ref)
    assert_same((rows, node, vic), want)


@pytest.mark.auto_engine
def test_evicting_the_prefixes_places_the_job_on_the_picks_and_one_less_does_not():
    c = pk.packed_case_k(257, 128)
    want, _ = pk.packed_ref_k(257, 128)
    v = c.victims
    with Engine(device=0) as e:  # its own context: the engine choice is read when it is created
        load(e, c)
        rows, node, vic = e.preempt_k(c.jobs, c.prio, pk.KMAX)
        assert_same((rows, node, vic), want)
        ev = np.flatnonzero((rows["code"] == pk.EVICT) & (rows["need"] >= 2))
        picked = list(ev[:: max(1, len(ev) // 6)][:6])
        picked += [q for q in ev if 0 < rows["fit"][q]][:2]           # a fitting pick among the evicting ones
        picked += [q for q in ev if rows["evict_nodes"][q] >= 2][:2]  # several nodes to free
        assert len(picked) >= 8
        base = e.read_nodes()
        for q in picked:
            need = int(rows["need"][q])
            for less, placed in ((0, True), (1, False)):
                cols = [col.copy() for col in base]
                for i in range(need):
                    x, take = int(node[q, i]), int(vic[q, i]) - (less if i == need - 1 else 0)
                    sl = slice(v.off[x], v.off[x] + take)
                    for col, amt in zip(cols, (v.cpu, v.mem, v.gpu)):
                        col[x] = min(int(col[x]) + int(amt[sl].astype(np.int64).sum()), INF)
                e.load_nodes(synth.Nodes(*cols, c.nodes.avail_min, c.nodes.part_mask))
                out, _ = e.place(one_job(c.jobs, q), pk.KMAX)
                if placed:  # exactly the picks fit: the placement's set is theirs
                    assert sorted(out[0, :need].tolist()) == sorted(node[q, :need].tolist()), (q, rows[q], out, node[q])
                    assert (out[0, need:] == -1).all()
                else:
                    assert out[0, 0] == fitgpu.FIT_UNPLACED, (q, rows[q], out)
        load(e, c)  # the original table and its victims again
        again = e.preempt_k(c.jobs, c.prio, pk.KMAX)
        assert all(np.array_equal(a, b) for a, b in zip(again, (rows, node, vic)))


def test_members_and_fit_are_fit_explains(engine):
    c = pk.packed_case_k(1000, 300)
    load(engine, c)
    rows, _, _ = preempt_k_both(engine, c.jobs, c.prio)
    why = engine.explain(c.jobs)
    assert np.array_equal(rows["members"], why["members"]) and np.array_equal(rows["fit"], why["fit"])
    assert np.array_equal(rows["need"], why["need"])
    early = np.isin(rows["code"], (1, 2, 3, 4, 5)) | np.isin(why["code"], (1, 2, 3, 4, 5))
    assert early.any() and np.array_equal(rows["code"][early], why["code"][early])  # FIT_PRE_1..5 are FIT_WHY_1..5
    assert np.array_equal(rows["code"] == pk.FITS, why["code"] == fitgpu.FIT_WHY_FITS)
    assert (rows["fit"] > 0).any() and (why["code"] == fitgpu.FIT_WHY_RESOURCES).any()


# ---- 6. read-only -------------------------------------------------------------------------------
def test_preempt_k_changes_nothing(engine):
    c = pk.packed_case_k(1000, 300)
    load(engine, c)
    before = engine.read_nodes()
    first = preempt_k_both(engine, c.jobs, c.prio)
    after = engine.read_nodes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), "preempt_k changed the node table"
    assert all(np.array_equal(a, b) for a, b in zip(after, (c.nodes.cpu_free, c.nodes.mem_free, c.nodes.gpu_free)))
    second = preempt_k_both(engine, c.jobs, c.prio)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), "a second call differs"
    one = pk.with_k(c.jobs, np.ones(c.jobs.j))  # and fit_preempt sees the same victims before and after
    assert np.array_equal(engine.preempt(one, c.prio), pc.ref_preempt(c.nodes, c.victims, c.parts, one, c.prio))


# ---- 7. state and argument errors ---------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


NULLS = (None,) * 7


def test_state_errors_and_the_ms_diagnostic():
    c = pk.hand_case_k()
    L = _lib.lib()
    ms = C.c_double()
    with Engine(device=0) as e:
        assert _code(lambda: e.preempt_k(c.jobs, c.prio)) == _lib.FIT_E_STATE       # before load_nodes
        e.load_nodes(c.nodes)
        e.load_partitions(c.parts)
        assert _code(lambda: e.preempt_k(c.jobs, c.prio)) == _lib.FIT_E_STATE       # before load_victims
        assert b"fit_load_victims" in L.fit_last_error()
        assert L.fit_preempt_k(e._h, 0, *NULLS, 8, None, None, None) == _lib.FIT_E_STATE
        e.load_victims(c.victims)
        assert L.fit_preempt_k_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE            # no fit_preempt_k_device yet
        got = e.preempt_k(c.jobs, c.prio)
        assert_same(got, pk.hand_arrays())
        assert L.fit_preempt_k_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE            # the host entry point is none
        for fn in (L.fit_preempt_k, L.fit_preempt_k_device):
            assert fn(e._h, 0, *NULLS, 8, None, None, None) == 0                    # j == 0, whatever the pointers
            assert fn(e._h, 1, *NULLS, 8, None, None, None) == _lib.FIT_E_INVAL
            assert fn(e._h, -1, *NULLS, 8, None, None, None) == _lib.FIT_E_INVAL
            assert fn(e._h, 0, *NULLS, 0, None, None, None) == _lib.FIT_E_INVAL     # kmax, even without a job
            assert fn(e._h, 0, *NULLS, 9, None, None, None) == _lib.FIT_E_INVAL
        assert b"kmax" in L.fit_last_error()
        assert L.fit_preempt_k_ms(e._h, None) == _lib.FIT_E_INVAL
        e.place(pk.with_k(c.jobs, np.ones(c.jobs.j)))                               # fit_place leaves the victims alone
        assert len(e.preempt_k(c.jobs, c.prio)[0]) == c.jobs.j
        e.load_nodes(c.nodes)                                                       # drops them: node ids change
        assert _code(lambda: e.preempt_k(c.jobs, c.prio)) == _lib.FIT_E_STATE
        e.load_victims(c.victims)
        assert_same(preempt_k_both(e, c.jobs, c.prio), got)
        assert L.fit_preempt_k_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_victims(None)                                                        # every list empty
        none = preempt_k_both(e, c.jobs, c.prio)
        assert not none[0]["able"].any() and not (none[0]["code"] == pk.EVICT).any() and not none[2].any()
        assert_same(none, pk.ref_preempt_k(c.nodes, None, c.parts, c.jobs, c.prio, pk.KMAX))


def test_no_preemption_while_a_timeline_is_loaded():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    prio = np.zeros(16, np.int32)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_victims(None)
        assert len(e.preempt_k(jobs, prio)[0]) == 16
        e.load_timeline(tline)
        assert _code(lambda: e.preempt_k(jobs, prio)) == _lib.FIT_E_STATE
        e.load_nodes(nodes)  # drops the timeline and the victims
        e.load_victims(None)
        assert len(e.preempt_k(jobs, prio)[0]) == 16


def test_a_sharded_context_answers_state():
    nodes, jobs, parts = synth.make_config("c2", 64, 16)
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.preempt_k(jobs, np.zeros(16, np.int32))) == _lib.FIT_E_STATE


def test_every_invalid_argument_fails_the_whole_call(engine):
    c = pk.hand_case_k()
    load(engine, c)
    good = preempt_k_both(engine, c.jobs, c.prio)

    def device(jobs, kmax):
        cols = [DevArray(getattr(jobs, g)) for g in JCOLS] + [DevArray(np.asarray(jobs.nodes_k, np.uint16)), DevArray(c.prio)]
        outs = [DevArray(np.zeros(jobs.j, EVICT_K_DTYPE))] + [DevArray(np.zeros((jobs.j, max(kmax, 1)), np.int32)) for _ in range(2)]
        return _code(lambda: engine.preempt_k_device(*cols, *outs, kmax=kmax))

    for kmax in (0, 9, -1):
        assert _code(lambda: engine.preempt_k(c.jobs, c.prio, kmax)) == _lib.FIT_E_INVAL
        assert device(c.jobs, kmax) == _lib.FIT_E_INVAL
    for kmax in (1, 4, 7):  # the batch's largest nodes_k is 8
        assert _code(lambda: engine.preempt_k(c.jobs, c.prio, kmax)) == _lib.FIT_E_INVAL
        assert device(c.jobs, kmax) == _lib.FIT_E_INVAL
    assert b"nodes_k" in _lib.lib().fit_last_error()
    for f in ("cpu", "mem", "gpu", "wall"):
        bad = synth.Jobs(*(getattr(c.jobs, g).copy() for g in JCOLS + ("nodes_k",)))
        getattr(bad, f)[8] = -1
        assert _code(lambda: engine.preempt_k(bad, c.prio)) == _lib.FIT_E_INVAL
        assert device(bad, pk.KMAX) == _lib.FIT_E_INVAL
    with pytest.raises(ValueError):
        engine.preempt_k(c.jobs, c.prio[:-1])
    assert_same(preempt_k_both(engine, c.jobs, c.prio), good)
    assert_same(good, pk.hand_arrays())

"""fit_preempt_tl_k on the GPU against ref_preempt_tl_k (tests/_preempt_tl_k_cases.py, a numpy int64
restatement of DESIGN.md §2o on the dense timeline): rows, out_node and out_victims compared field for
field through the host and the device entry point, on timelines WITH reservations (the full and the
short queue), on shapes that cross every wave, tile, slice and chunk edge of k_ptlk_walk, at every list
capacity the walk is built for, need at its thresholds, run counts, list lengths, ends and windows
around the loads' seams, int32 edge values, the six relations of §2o and the state errors."""
import ctypes as C

import numpy as np
import pytest

import _preempt_cases as pc
import _preempt_k_cases as pk
import _preempt_tl_cases as tc
import _preempt_tl_k_cases as tk
import fitgpu
from _devarray import DevArray
from fitgpu import EVICT_K_DTYPE, Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu

INF, I32MIN = tc.INF, tc.I32MIN
KMAX = tk.KMAX
ONE_PART = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
VCOLS = ("off", "prio", "end", "cpu", "mem", "gpu")
JCOLS = ("cpu", "mem", "gpu", "wall", "part")
F, E, N = tk.FITS, tk.EVICT, tk.NONE


def preempt_both(e, jobs, prio, kmax=KMAX):
    """Engine.preempt_tl_k through host pointers and through device pointers: the same rows and picks.
    The device outputs start from a pattern, so an entry the call leaves unwritten shows."""
    rows, node, vic = e.preempt_tl_k(jobs, prio, kmax)
    assert node.shape == vic.shape == (jobs.j, kmax)
    cols = [DevArray(getattr(jobs, f)) for f in JCOLS]
    nk = None if jobs.nodes_k is None else DevArray(np.asarray(jobs.nodes_k, np.uint16))
    out = DevArray(np.full(jobs.j * 10, -7, np.int32).view(EVICT_K_DTYPE))
    dn, dv = DevArray(np.full((jobs.j, kmax), -7, np.int32)), DevArray(np.full((jobs.j, kmax), -7, np.int32))
    ms = e.preempt_tl_k_device(*cols, nk, DevArray(np.asarray(prio, np.int32)), out, dn, dv, kmax=kmax)
    assert ms > 0 and e.preempt_tl_k_ms() == ms
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


def take(jobs, idx):
    return synth.Jobs(*(np.array(getattr(jobs, f)[idx]) for f in JCOLS),
                      None if jobs.nodes_k is None else np.array(jobs.nodes_k[idx]))  # copies: the cases are shared


def no_jobs():
    return synth.Jobs(*(np.zeros(0, np.int32) for _ in range(4)), np.zeros(0, np.uint16), np.zeros(0, np.uint16))


def load(e, c, device=False, place=True, hold=None):
    """Node table, partitions, the timeline from the release events, the reservations (the queue
    through place_tl, or `hold` = (nodes, starts) through hold_tl), then the victims."""
    e.load_nodes(c.nodes)
    e.load_partitions(c.parts)
    e.load_timeline(c.tline)
    if hold is not None:
        state, _, refused = e.hold_tl(c.queue, np.asarray(hold[0], np.int32), np.asarray(hold[1], np.int32))
        assert refused == 0 and (state == fitgpu.FIT_HOLD_HELD).all()
    elif place and c.queue.j:
        e.place_tl(c.queue)
    if device and c.victims is not None:
        e.load_victims_tl_device(*(DevArray(getattr(c.victims, f)) for f in VCOLS))
    else:
        e.load_victims_tl(c.victims)


def ref(e, c, jobs=None, prio=None, kmax=KMAX, shift=0):
    """The reference on what read_timeline() returns now."""
    jobs, prio = (c.jobs, c.prio) if jobs is None else (jobs, prio)
    return tk.ref_preempt_tl_k(c.nodes.part_mask, e.read_timeline(), c.victims, c.parts, jobs, prio, c.tline.slot_min,
                               kmax, shift)


def check(e, c, kmax=KMAX, **kw):
    """Load the case, run both entry points, compare with the reference; returns the rows and picks."""
    load(e, c, **kw)
    got = preempt_both(e, c.jobs, c.prio, kmax)
    assert_same(got, ref(e, c, kmax=kmax))
    return got


def tup(r):
    return tuple(int(x) for x in r)


HAND_HOLD = ([x for _, x, _ in tc.HAND_HOLDS], [s for _, _, s in tc.HAND_HOLDS])


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


# ---- 1. the hand-written and the packed random cases, with reservations --------------------------
def test_hand_written_cases_give_the_literal_rows(engine):
    c = tk.hand_case_k()
    load(engine, c, hold=HAND_HOLD)
    assert engine.read_timeline()[:, :, 0].tolist() == tc.HAND_CPUS
    got = preempt_both(engine, c.jobs, c.prio)
    assert_same(got, tk.hand_arrays())
    load(engine, c, device=True, hold=HAND_HOLD)
    assert_same(preempt_both(engine, c.jobs, c.prio), got)
    assert_same(check(engine, tk.flat_hand_case_k()), tk.hand_arrays(tk.FLAT_ROWS_K))


PACKED = [(variant, n, j, seed) for (variant, n, j), (seeds, _) in sorted(tk.SEEDS.items()) for seed in seeds]


@pytest.mark.parametrize("variant,n,j,seed", PACKED)
def test_packed_random_cases_on_both_timelines(engine, variant, n, j, seed):
    c = tk.packed_tl_case_k(variant, n, j, seed)
    want, stats, T = tk.packed_tl_ref_k(variant, n, j, seed)
    tk.SEEDS[(variant, n, j)][1](want[0], stats)  # on the reference alone: a comparison of nothing interesting fails
    load(engine, c, device=seed == 1 or j == 257)
    member = c.nodes.part_mask != 0
    assert np.array_equal(engine.read_timeline()[member], T[member]), "place_tl left another timeline than the oracle"
    got = preempt_both(engine, c.jobs, c.prio)
    assert_same(got, want)
    assert_same(got, ref(engine, c))


@pytest.mark.parametrize("variant", ["full", "short"])
def test_packed_random_case_on_one_component(engine, variant):
    c = tk.packed_tl_case_k(variant, 257, 128, 0, True)
    want, _, T = tk.packed_tl_ref_k(variant, 257, 128, 0, True)
    rows = want[0]
    assert len(np.unique(np.asarray(c.jobs.part)[rows["members"] > 0])) == 2  # the two partitions of the one component
    assert (rows["code"] == E).any() and (rows["code"] == N).any()
    load(engine, c)
    member = c.nodes.part_mask != 0
    assert np.array_equal(engine.read_timeline()[member], T[member]), "place_tl left another timeline than the oracle"
    assert_same(preempt_both(engine, c.jobs, c.prio), want)


# ---- 2. shapes at the seams ----------------------------------------------------------------------
# n: the wave sub-slices (8 waves share a slice's positions) and the node slices; J: the 64-job tiles,
# and above 256 jobs on several components the component-ordered job list.  One table per (n,
# components): every job is judged alone, so the first J jobs have the first J rows of the reference.
SEAM_J = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("one_component", [False, True])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 63, 64, 65, 257])
def test_shapes_at_the_seams(engine, n, one_component):
    c = tk.packed_tl_case_k("full", n, 257, 0, one_component)
    assert tc.H == 64
    load(engine, c, device=n == 65)
    want = ref(engine, c)
    rows = want[0]
    if n >= 63:
        assert (rows["code"] == E).sum() >= 20 and (rows["code"] == N).any() and (want[1] >= 0).sum() >= 40
    for j in SEAM_J:
        got = preempt_both(engine, take(c.jobs, slice(0, j)), c.prio[:j])
        assert_same(got, tuple(a[:j] for a in want))


@pytest.mark.parametrize("kmax", [1, 2, 3, 4, 5, 8])
def test_every_list_capacity(engine, kmax):
    """The walk keeps 1, 2, 4 or 8 keys and stores kmax of them: every kmax that selects another kernel
    or another store count, with nodes_k up to it."""
    c = tk.packed_tl_case_k("short", 257, 128)
    nk = np.minimum(np.asarray(c.jobs.nodes_k), kmax)
    c = tc.CaseTL(c.nodes, c.victims, c.tline, c.queue, c.parts, tk.with_k(c.jobs, nk), c.prio)
    rows, node, _ = check(engine, c, kmax)
    assert (np.isin(rows["code"], (F, E)) & (rows["need"] == kmax)).any() and node.shape[1] == kmax
    assert (rows["code"] == E).sum() >= 20


def sliced_case(n=5000, j=64):
    """5,000 nodes of one partition on 8 slots of 10 minutes, none with a free cpu at slot 0 but nodes
    1100, 1101 and 1102 (64 cpus): one release of 4 cpus per node, lists of 1 .. 3 victims of 4 .. 16
    cpus with ends 1, 4 or 8.  Only the nodes from 4000 on hold a victim of priority 0, so a job above
    three nodes takes the three emptied ones and then nodes thousands of ids away."""
    r = np.random.default_rng(5000)
    cpu = np.zeros(n, np.int32)
    cpu[1100:1103] = 64
    nodes = synth.Nodes(cpu, np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32), np.ones(n, np.uint32))
    lists = []
    for x in range(n):
        k = int(r.integers(1, 4))
        pr = np.sort(r.integers(0 if x >= 4000 else 1, 4, k))
        lists.append([(int(p), int(r.choice([1, 4, 8])), int(r.choice([4, 8, 16])), 0, 0) for p in pr])
    lists[1100] = lists[1101] = lists[1102] = []
    tline = synth.Timeline(8, 10, np.arange(n + 1, dtype=np.int32), r.integers(1, 8, n).astype(np.int32),
                           np.full(n, 4, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    rows = [(int(r.choice([4, 8, 16, 64])), 0, 0, int(r.choice([10, 40, 80])), 0, int(r.integers(1, 5)), int(k))
            for k in np.random.default_rng(7 * n + j).choice(tk.K_DRAW, j)]
    jobs, prio = tk.jobs_of_k(rows)
    return tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, no_jobs(), ONE_PART, jobs, prio)


def test_picks_across_node_slices(engine):
    """One job tile, so the positions are cut into node slices: a job of up to three nodes finds all
    its picks in one slice, whose list alone must hold them; a wider job takes these three and then
    nodes thousands of ids away."""
    c = sliced_case()
    load(engine, c)
    want = ref(engine, c)
    rows, node, _ = want
    multi = np.flatnonzero(np.isin(rows["code"], (F, E)) & (rows["need"] >= 2))
    span = np.array([node[q, :rows["need"][q]].max() - node[q, :rows["need"][q]].min() for q in multi])
    assert (span >= 2500).sum() >= 3 and (span <= 2).sum() >= 3, span
    assert ((rows["code"] == E) & (rows["fit"] == 3)).any()
    assert_same(preempt_both(engine, c.jobs, c.prio), want)


def test_a_batch_above_one_chunk_of_positions(engine):
    """16,800 jobs on 65 nodes: the walk and the final run twice, the second time over 416 positions of
    the component-ordered job list.  Every job is judged alone, so the 700-job case repeated 24 times
    has the reference's rows and picks repeated 24 times."""
    c = tk.packed_tl_case_k("full", 65, 700)
    reps = 24
    jobs = synth.Jobs(*(np.tile(getattr(c.jobs, f), reps) for f in JCOLS + ("nodes_k",)))
    assert jobs.j == 16800 > 16384 and len(np.unique(c.jobs.part)) > 2
    load(engine, c)
    want = ref(engine, c)
    assert ((want[0]["code"] == E) & (want[0]["need"] >= 2)).sum() >= 20
    got = preempt_both(engine, jobs, np.tile(c.prio, reps))
    assert_same(got, (np.tile(want[0], reps), np.tile(want[1], (reps, 1)), np.tile(want[2], (reps, 1))))


# ---- 3. need at its edges -----------------------------------------------------------------------
def flat_case(cpu, lists, rows, Hh=4, slot_min=10, mask=None):
    """n nodes of `cpu` free cpus on an open timeline of Hh slots without events."""
    n = len(lists)
    nodes = synth.Nodes(np.asarray(cpu, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32),
                        np.ones(n, np.uint32) if mask is None else np.asarray(mask, np.uint32))
    tline = synth.Timeline(Hh, slot_min, np.zeros(n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs, prio = tk.jobs_of_k(rows)
    return tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, no_jobs(), ONE_PART, jobs, prio)


def test_need_at_fit_at_fit_plus_able_and_at_members(engine):
    """Seven nodes: 0 and 1 have 4 cpus free, 2 and 3 a victim of priority 1 that holds 4 until the
    horizon, 4 one of priority 100, 5 nothing at all, 6 is in no partition.  members 6; for a job of
    4 cpus at priority 50: fit 2, able 2, outranked 1; at priority 200: able 3."""
    v1, v100 = [(1, 4, 4, 0, 0)], [(100, 4, 4, 0, 0)]
    #         cpu mem gpu wall part prio need
    c = flat_case([4, 4, 0, 0, 0, 0, 4], [[], [], v1, v1, v100, [], v1],
                  [(4, 0, 0, 40, 0, 50, 2),    # need == fit: FITS at the boundary
                   (4, 0, 0, 40, 0, 50, 3),    # one more: the first eviction
                   (4, 0, 0, 40, 0, 50, 4),    # need == fit + able exactly
                   (4, 0, 0, 40, 0, 50, 5),    # one more: NONE, with fit + able = need - 1
                   (4, 0, 0, 40, 0, 200, 5),   # node 4 can be freed too: need == fit + able
                   (4, 0, 0, 40, 0, 200, 6),   # need == members, but node 5 has nothing to free
                   (0, 0, 0, 40, 0, 0, 6),     # the all-zero demand: need == members == fit
                   (0, 0, 0, 40, 0, 0, 7)],    # members < need
                  mask=[1, 1, 1, 1, 1, 1, 0])
    rows, node, vic = check(engine, c)
    want = [((F, 2, 0, 0, 0, 6, 2, 2, 1, 0), [0, 1], [0, 0]),
            ((E, 3, 1, 1, 1, 6, 2, 2, 1, 0), [0, 1, 2], [0, 0, 1]),
            ((E, 4, 2, 2, 1, 6, 2, 2, 1, 0), [0, 1, 2, 3], [0, 0, 1, 1]),
            ((N, 5, 0, 0, 0, 6, 2, 2, 1, 0), [], []),
            ((E, 5, 3, 3, 100, 6, 2, 3, 0, 0), [0, 1, 2, 3, 4], [0, 0, 1, 1, 1]),
            ((N, 6, 0, 0, 0, 6, 2, 3, 0, 0), [], []),
            ((F, 6, 0, 0, 0, 6, 6, 0, 0, 0), [2, 3, 4, 5, 0, 1], [0] * 6),  # the emptiest first
            ((N, 7, 0, 0, 0, 6, 6, 0, 0, 0), [], [])]
    for q, (r, n, x) in enumerate(want):
        assert tup(rows[q]) == r, (q, rows[q])
        assert node[q].tolist() == n + [-1] * (8 - len(n)) and vic[q].tolist() == x + [0] * (8 - len(x)), (q, node[q], vic[q])


@pytest.mark.parametrize("nodes_k", [1, 0, None])
def test_need_one_at_kmax_eight_is_fit_preempt_tls_row(engine, nodes_k):
    """Relation 1: with every need 1 the row, out_node[0] and out_victims[0] are fit_preempt_tl's."""
    c = tk.packed_tl_case_k("full", 257, 128)
    jobs = tk.with_k(c.jobs, None if nodes_k is None else np.full(c.jobs.j, nodes_k))
    c = tc.CaseTL(c.nodes, c.victims, c.tline, c.queue, c.parts, jobs, c.prio)
    rows, node, vic = check(engine, c)
    assert (rows["need"] == 1).all() and (node[:, 1:] == -1).all() and not vic[:, 1:].any() and not rows["reserved"].any()
    one = engine.preempt_tl(jobs, c.prio)
    for f in ("code", "victims", "top_prio", "members", "fit", "able", "outranked"):
        assert np.array_equal(rows[f], one[f]), f
    assert np.array_equal(node[:, 0], one["node"]) and np.array_equal(vic[:, 0], one["victims"])
    assert np.array_equal(rows["evict_nodes"], (one["victims"] > 0).astype(np.int32))
    assert (rows["code"] == E).sum() >= 20 and (rows["code"] == N).any()
    k1 = preempt_both(engine, jobs, c.prio, 1)
    assert np.array_equal(k1[0], rows) and np.array_equal(k1[1], node[:, :1]) and np.array_equal(k1[2], vic[:, :1])


def test_eight_copies_of_one_node_pick_the_lowest_ids(engine):
    c = flat_case([2] * 8, [[(1, 4, 2, 0, 0), (2, 4, 4, 0, 0)]] * 8,
                  [(8, 0, 0, 40, 0, 9, 3), (4, 0, 0, 40, 0, 9, 8), (2, 0, 0, 40, 0, 9, 3)])
    rows, node, vic = check(engine, c)
    assert tup(rows[0]) == (E, 3, 3, 6, 2, 8, 0, 8, 0, 0)
    assert node[0].tolist() == [0, 1, 2] + [-1] * 5 and vic[0].tolist() == [2, 2, 2] + [0] * 5
    assert node[1].tolist() == list(range(8)) and vic[1].tolist() == [1] * 8 and rows[1]["victims"] == 8
    assert rows[2]["code"] == F and node[2].tolist() == [0, 1, 2] + [-1] * 5


# ---- 4. runs, list lengths and ends around the loads and the window ------------------------------
RUNS = (1, 4, 5, 8, 9, 13)
LENS = (0, 1, 3, 4, 5, 8, 9, 64, 65)
WIN = 16  # the window of the jobs below, in slots


def test_runs_lists_and_ends_at_every_seam_on_pairs_of_nodes(engine):
    """§2n's per-node grid with every node duplicated once, at need 2.  Two nodes (2i, 2i + 1) per
    (runs, list length, end of the last entry): R runs inside the 16-slot window (a release of one cpu
    at each of the slots 1 .. R - 1), a list of which only the last entry holds the 16 cpus a job
    wants, ending at 0, 1, d - 1, d, d + 1 or H.  Free never reaches 16, so every run is short and the
    node can be freed exactly when the last entry's end is >= d.  Twins have the same key but the id:
    the picks of every row are a pair."""
    Hh, sm = 64, 10
    ends = (0, 1, WIN - 1, WIN, WIN + 1, Hh)
    combos = [(r, ln, en) for r in RUNS for ln in LENS for en in ends for _ in range(2)]
    n = len(combos)
    lists, ev_off, ev_slot = [], [0], []
    for r, ln, en in combos:
        lists.append([(i, en if i == ln - 1 else 1 + i % 3, 16 if i == ln - 1 else i % 2, 0, 0) for i in range(ln)])
        ev_slot += list(range(1, r))
        ev_off.append(len(ev_slot))
    ne = len(ev_slot)
    nodes = synth.Nodes(np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32),
                        np.ones(n, np.uint32))
    tline = synth.Timeline(Hh, sm, np.array(ev_off, np.int32), np.array(ev_slot, np.int32), np.ones(ne, np.int32),
                           np.zeros(ne, np.int32), np.zeros(ne, np.int32))
    prios = sorted({p for ln in LENS if ln for p in (ln - 1, ln)} | {I32MIN, INF})
    rows = [(16, 0, 0, WIN * sm, 0, p, 2) for p in prios]
    rows += [(16, 0, 0, w, 0, INF, 2) for w in (0, sm, sm + 1, (WIN - 1) * sm, (WIN + 1) * sm, Hh * sm, Hh * sm + 1)]
    rows += [(3, 0, 0, WIN * sm, 0, INF, 2), (0, 0, 0, WIN * sm, 0, 0, 2)]
    jobs, prio = tk.jobs_of_k(rows)
    c = tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, no_jobs(), ONE_PART, jobs, prio)
    load(engine, c)
    T = engine.read_timeline()
    per = 2 * len(LENS) * len(ends)
    for x, (r, _, _) in enumerate(combos[::per]):
        cpus = T[x * per, :WIN, 0]
        assert len(np.unique(cpus)) == r, (r, cpus)  # r runs inside the window
    got = preempt_both(engine, jobs, prio)
    assert_same(got, ref(engine, c))
    rws, node, vic = got
    picked = np.isin(rws["code"], (F, E))
    assert picked.sum() >= len(prios) + 6 - 1
    assert (node[picked, 0] % 2 == 0).all() and (node[picked, 1] == node[picked, 0] + 1).all()  # the pair
    assert (vic[picked, 0] == vic[picked, 1]).all()
    r = rws[len(prios) - 1]  # 16 cpus on 16 slots at INT32_MAX: lists whose last entry ends at d, d + 1 or H
    able = sum(1 for _, ln, en in combos if ln and en >= WIN)
    assert tup(r) == (E, 2, 2, 2, 0, n, 0, able, 0, 0), r  # the one-entry lists: the fewest victims at the lowest top
    r = rws[0]  # at INT32_MIN every such node is held
    assert (r["code"], r["able"], r["outranked"]) == (N, 0, able), r
    r = rws[len(prios) + 6]  # H + 1 slots: no node is eligible
    assert (r["code"], r["members"], r["able"], r["outranked"]) == (N, n, 0, 0), r


def small_case(Hh, slot_min, seed, n=48, j=40):
    """A small random cluster on a horizon of Hh slots: up to 14 releases per node, lists of 0 .. 9
    entries with ends at 0, 1, d - 1, d, d + 1 and Hh for the windows d the jobs use, one reservation
    window per node (held where it fits): the dips; jobs of 1 .. 3 nodes."""
    r = np.random.default_rng(seed)
    ds = sorted({1, min(2, Hh), max(Hh // 2, 1), Hh, Hh + 1})
    ends = sorted({min(max(v, 0), Hh) for d in ds for v in (0, 1, d - 1, d, d + 1, Hh)})
    nodes = synth.Nodes(r.integers(0, 6, n).astype(np.int32), np.full(n, 8192, np.int32), r.integers(0, 2, n).astype(np.int32),
                        np.where(r.random(n) < 0.2, r.integers(0, Hh * slot_min + 1, n), INF).astype(np.int32),
                        np.where(r.random(n) < 0.1, 0, 1 + (r.random(n) < 0.3)).astype(np.uint32))
    cnt = r.integers(0, 15, n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    slot = np.concatenate([np.sort(r.integers(0, Hh, k)) for k in cnt] + [np.zeros(0, np.int64)]).astype(np.int32)
    ne = len(slot)
    tline = synth.Timeline(Hh, slot_min, off, slot, r.integers(0, 4, ne).astype(np.int32),
                           r.integers(0, 1024, ne).astype(np.int32), np.zeros(ne, np.int32))
    lists = [sorted(((int(r.integers(0, 6)), int(r.choice(ends)), int(r.integers(0, 9)), int(r.integers(0, 2048)),
                      int(r.integers(0, 2))) for _ in range(r.integers(0, 10))), key=lambda e: e[0]) for _ in range(n)]
    qs = r.integers(0, Hh, n)
    qd = 1 + r.integers(0, np.maximum(Hh - qs, 1))
    queue = synth.Jobs(r.integers(1, 4, n).astype(np.int32), r.integers(0, 2048, n).astype(np.int32), np.zeros(n, np.int32),
                       (qd * slot_min).astype(np.int32), np.zeros(n, np.uint16), np.ones(n, np.uint16))
    rows = [(int(r.integers(0, 13)), int(r.integers(0, 3000)), int(r.integers(0, 2)), int((r.choice(ds) - 1) * slot_min + 1),
             int(r.integers(0, 3)), int(r.integers(0, 7)), int(r.integers(1, 4))) for _ in range(j)]
    jobs, prio = tk.jobs_of_k(rows)
    parts = synth.Partitions(np.full(2, -1, np.int32), np.full(2, -1, np.int32), np.full(2, -1, np.int32))
    return tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, queue, parts, jobs, prio), qs.astype(np.int32)


@pytest.mark.parametrize("Hh,slot_min", [(1, 7), (64, 5), (1024, 3)])
def test_horizons_and_windows_of_1_h_and_h_plus_1(engine, Hh, slot_min):
    c, starts = small_case(Hh, slot_min, 100 + Hh)
    e = engine
    e.load_nodes(c.nodes)
    e.load_partitions(c.parts)
    e.load_timeline(c.tline)
    state, held, _ = e.hold_tl(c.queue, np.arange(c.nodes.n, dtype=np.int32), starts)
    assert Hh == 1 or held > 0
    e.load_victims_tl(c.victims)
    d = np.array([tc.dur(w, slot_min) for w in c.jobs.wall])
    assert {1, Hh, Hh + 1} <= set(d.tolist())
    want = ref(e, c, kmax=4)
    assert_same(preempt_both(e, c.jobs, c.prio, 4), want)
    rows = want[0]
    assert (rows["able"] > 0).any() and (rows["outranked"] > 0).any() and (rows["code"] == N).any()
    assert (rows["need"] >= 2).sum() >= 10 and (Hh == 1 or ((rows["code"] == E) & (rows["need"] >= 2)).any())


# ---- 5. edge values ------------------------------------------------------------------------------
def test_priorities_at_the_int32_ends(engine):
    c = flat_case([0, 0, 0], [[(I32MIN, 4, 4, 0, 0), (INF, 4, 4, 0, 0)], [(INF, 4, 8, 0, 0)],
                              [(I32MIN, 4, 2, 0, 0), (I32MIN + 1, 4, 2, 0, 0)]],
                  [(4, 0, 0, 40, 0, I32MIN, 2), (4, 0, 0, 40, 0, I32MIN + 1, 2), (4, 0, 0, 40, 0, I32MIN + 2, 2),
                   (4, 0, 0, 40, 0, INF, 2), (4, 0, 0, 40, 0, INF, 3), (2, 0, 0, 40, 0, I32MIN + 1, 2)])
    rows, node, vic = check(engine, c)
    got = [tup(r) for r in rows]
    assert got[0] == (N, 2, 0, 0, 0, 3, 0, 0, 3, 0)                 # a job at INT32_MIN evicts nothing
    assert got[1] == (N, 2, 0, 0, 0, 3, 0, 1, 2, 0)                 # one above: node 0 alone
    assert got[2] == (E, 2, 2, 3, I32MIN + 1, 3, 0, 2, 1, 0)        # node 0 (top INT32_MIN) before node 2
    assert node[2, :2].tolist() == [0, 2] and vic[2, :2].tolist() == [1, 2]
    assert got[3] == got[2]                                         # INT32_MAX does not evict INT32_MAX
    assert got[4] == (N, 3, 0, 0, 0, 3, 0, 2, 1, 0)
    assert got[5] == (E, 2, 2, 2, I32MIN, 3, 0, 2, 1, 0) and node[5, :2].tolist() == [2, 0]  # node 2 the tighter


def test_sums_are_exact_the_residual_is_clamped_and_the_zero_demand_fits(engine):
    """Nodes 0 and 2: INT32_MAX free cpus and three victims of INT32_MAX cpus and 1 MiB each; node 1 the
    same free cpus, its victims hold no cpu.  A job of INT32_MAX - 5 cpus and 3 MiB needs all three
    victims on each: the residual is min(sum, INT32_MAX) - demand = 5 everywhere, the ids decide.  A
    sum that wrapped would not fit; an unclamped residual would lose."""
    c = flat_case([INF] * 3, [[(1, 4, INF, 1, 0)] * 3, [(1, 4, 0, 1, 0)] * 3, [(1, 4, INF, 1, 0)] * 3],
                  [(INF - 5, 3, 0, 40, 0, 2, 2), (INF, 2, 0, 40, 0, 2, 3), (INF, 0, 0, 40, 0, 2, 3), (0, 0, 0, 40, 0, 0, 2)])
    rows, node, vic = check(engine, c)
    assert tup(rows[0]) == (E, 2, 2, 6, 1, 3, 0, 3, 0, 0)
    assert node[0, :2].tolist() == [0, 1] and vic[0, :2].tolist() == [3, 3]
    assert tup(rows[1]) == (E, 3, 3, 6, 1, 3, 0, 3, 0, 0) and vic[1, :3].tolist() == [2, 2, 2]
    assert tup(rows[2]) == (F, 3, 0, 0, 0, 3, 3, 0, 0, 0) and node[2, :3].tolist() == [0, 1, 2]
    assert tup(rows[3]) == (F, 2, 0, 0, 0, 3, 3, 0, 0, 0) and node[3, :2].tolist() == [0, 1]


def test_an_entry_with_end_0_frees_nothing_and_keeps_its_place(engine):
    two = [(1, 0, 4, 0, 0), (2, 4, 4, 0, 0)]
    c = flat_case([0, 0], [two, two], [(4, 0, 0, 40, 0, 5, 2), (0, 0, 0, 40, 0, 5, 2), (4, 0, 0, 40, 0, 2, 2)])
    rows, node, vic = check(engine, c)
    assert tup(rows[0]) == (E, 2, 2, 4, 2, 2, 0, 2, 0, 0) and vic[0, :2].tolist() == [2, 2]
    assert tup(rows[1]) == (F, 2, 0, 0, 0, 2, 2, 0, 0, 0)
    assert tup(rows[2]) == (N, 2, 0, 0, 0, 2, 0, 0, 2, 0)


# ---- 6. relations --------------------------------------------------------------------------------
def test_members_fit_need_and_a_fits_rows_nodes_are_fit_when_ks(engine):
    """Relation 2, on the short queue where some nodes still fit."""
    c = tk.packed_tl_case_k("short", 257, 128, 1)
    load(engine, c)
    (rows, node, vic), (eta, enode) = preempt_both(engine, c.jobs, c.prio), engine.when_k(c.jobs, KMAX)
    assert_same((rows, node, vic), ref(engine, c))
    for a, b in (("members", "members"), ("fit", "now"), ("need", "need")):
        assert np.array_equal(rows[a], eta[b]), (a, b)
    fits = rows["code"] == F
    assert (fits & (rows["need"] >= 2)).sum() >= 5 and (rows["code"] == E).any()
    assert np.array_equal(fits, eta["code"] == fitgpu.FIT_ETA_NOW) and not eta["start"][fits].any()
    assert np.array_equal(node[fits], enode[fits])
    early = np.isin(rows["code"], (1, 2, 3, 4, 5))
    assert early.any() and np.array_equal(rows["code"][early], eta["code"][early])
    assert not rows["members"][np.isin(rows["code"], (1, 2, 3, 4))].any()  # codes 1-4 carry only code and need


def test_without_reservations_a_second_context_answers_fit_preempt_k_alike(engine):
    """Relation 3: no release events, slot_min = 1, walls in [1, H], every end H — the timeline is the
    node table on every open slot, and a second context without a timeline answers fit_preempt_k with
    the same rows and picks."""
    base = pk.packed_case_k(257, 128)
    n, Hh = base.nodes.n, tc.H
    r = np.random.default_rng(5)
    v = base.victims
    vt = synth.VictimsTL(v.off, v.prio, np.full(len(v.prio), Hh, np.int32), v.cpu, v.mem, v.gpu)
    empty = synth.Timeline(Hh, 1, np.zeros(n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs = take(base.jobs, slice(None))
    jobs.wall = r.integers(1, Hh + 1, jobs.j).astype(np.int32)
    nd = base.nodes
    nodes = synth.Nodes(nd.cpu_free, nd.mem_free, nd.gpu_free, r.integers(0, 2 * Hh, n).astype(np.int32), nd.part_mask)
    c = tc.CaseTL(nodes, vt, empty, no_jobs(), base.parts, jobs, base.prio)
    got = check(engine, c)
    with Engine(device=0) as e2:
        e2.load_nodes(nodes)
        e2.load_partitions(base.parts)
        e2.load_victims(v)
        assert_same(got, e2.preempt_k(jobs, base.prio, KMAX))
    assert ((got[0]["code"] == E) & (got[0]["need"] >= 2)).sum() >= 10 and (got[0]["code"] == F).any()


def test_unplacing_the_prefixes_starts_the_job_now_on_the_picks_and_one_less_does_not(engine):
    """Relation 4, on a sample of the EVICT rows."""
    c = tk.packed_tl_case_k("short", 257, 128)
    load(engine, c)
    rows, node, vic = engine.preempt_tl_k(c.jobs, c.prio, KMAX)
    v = c.victims
    ev = np.flatnonzero((rows["code"] == E) & (rows["need"] >= 2))
    picked = list(ev[:: max(1, len(ev) // 5)][:5])
    picked += [q for q in ev if 0 < rows["fit"][q]][:2]           # a fitting pick among the evicting ones
    picked += [q for q in ev if rows["evict_nodes"][q] >= 2][:2]  # several nodes to free
    assert len(picked) >= 8
    before = engine.read_timeline()
    for q in picked:
        need = int(rows["need"][q])
        one = take(c.jobs, slice(q, q + 1))
        for less in (0, 1):
            idx, nds, walls = [], [], []
            for i in range(need):
                x, cnt = int(node[q, i]), int(vic[q, i])
                ids = np.arange(v.off[x], v.off[x] + cnt)
                if less and i == need - 1:
                    ids = ids[:-1]  # entry v - 1 of the last pick left out
                ids = ids[v.end[ids] > 0]  # an entry with end 0 frees nothing
                # unplace_tl leaves a closed slot closed and hold_tl refuses a window that reaches one: hand
                # back the open part of [0, end) only, which is the same timeline, so hold_tl can take it again
                shut = np.flatnonzero(before[x, :, 0] < 0)
                u = int(shut[0]) if len(shut) else tc.H
                idx += ids.tolist()
                nds += [x] * len(ids)
                walls += (np.minimum(v.end[ids], u) * tc.SLOT_MIN).tolist()
            idx = np.array(idx, np.int64)
            back = synth.Jobs(v.cpu[idx], v.mem[idx], v.gpu[idx], np.array(walls, np.int32), np.zeros(len(idx), np.uint16),
                              np.ones(len(idx), np.uint16))
            nd, start = np.array(nds, np.int32), np.zeros(len(idx), np.int32)
            if len(idx):
                assert engine.unplace_tl(back, nd, start) == len(idx)
            eta, enode = engine.when_k(one, KMAX)
            if less:
                assert eta["now"][0] == need - 1 and eta["code"][0] != fitgpu.FIT_ETA_NOW, (q, rows[q], eta)
            else:
                assert (eta["code"][0], eta["now"][0], eta["start"][0]) == (fitgpu.FIT_ETA_NOW, need, 0), (q, rows[q], eta)
                assert sorted(enode[0, :need].tolist()) == sorted(node[q, :need].tolist()), (q, enode, node[q])
            if len(idx):
                state, held, refused = engine.hold_tl(back, nd, start)  # take them back
                assert held == len(idx) and refused == 0
        assert engine.read_timeline().tobytes() == before.tobytes()


@pytest.mark.parametrize("a", [1, 8, tc.H])
def test_after_advance_tl_every_end_reads_a_slots_earlier(engine, a):
    """Relation 5."""
    c = tk.packed_tl_case_k("full", 65, 65)
    load(engine, c)
    first = engine.preempt_tl_k(c.jobs, c.prio, KMAX)
    engine.advance_tl(a)
    got = preempt_both(engine, c.jobs, c.prio)
    assert_same(got, ref(engine, c, shift=a))
    if a < tc.H:
        assert not np.array_equal(got[0], first[0]) and (got[0]["code"] == E).any()
        engine.advance_tl(8)  # the shifts add up ...
        assert_same(preempt_both(engine, c.jobs, c.prio), ref(engine, c, shift=a + 8))
        engine.advance_tl(tc.H)  # ... and saturate at H
    after = preempt_both(engine, c.jobs, c.prio)
    assert_same(after, ref(engine, c, shift=tc.H))
    assert not after[0]["able"].any() and not after[0]["outranked"].any()  # every end reads 0: nothing can be freed
    engine.load_victims_tl(c.victims)  # a new load starts from shift 0 again
    assert_same(preempt_both(engine, c.jobs, c.prio), ref(engine, c))


def test_preempt_tl_k_changes_nothing(engine):
    """Relation 6."""
    c = tk.packed_tl_case_k("full", 257, 128)
    load(engine, c)
    before = engine.read_timeline()
    first = preempt_both(engine, c.jobs, c.prio)
    assert engine.read_timeline().tobytes() == before.tobytes(), "preempt_tl_k changed the timeline"
    second = preempt_both(engine, c.jobs, c.prio)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), "a second call differs"


# ---- 7. state and argument errors ----------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


NULLS = (None,) * 7


def test_state_errors_and_the_ms_diagnostic():
    c = tk.hand_case_k()
    hold = (np.array(HAND_HOLD[0], np.int32), np.array(HAND_HOLD[1], np.int32))
    L = _lib.lib()
    ms = C.c_double()
    with Engine(device=0) as e:
        assert _code(lambda: e.preempt_tl_k(c.jobs, c.prio)) == _lib.FIT_E_STATE    # before load_nodes
        e.load_nodes(c.nodes)
        e.load_partitions(c.parts)
        assert _code(lambda: e.preempt_tl_k(c.jobs, c.prio)) == _lib.FIT_E_STATE    # without a timeline
        e.load_victims(None)                                                        # fit_load_victims' lists are not these
        e.load_timeline(c.tline)
        assert _code(lambda: e.preempt_tl_k(c.jobs, c.prio)) == _lib.FIT_E_STATE    # before load_victims_tl
        assert b"fit_load_victims_tl" in L.fit_last_error()
        assert L.fit_preempt_tl_k(e._h, 0, *NULLS, 8, None, None, None) == _lib.FIT_E_STATE
        assert _code(lambda: e.preempt_k(c.jobs, c.prio)) == _lib.FIT_E_STATE       # fit_preempt_k still refuses a timeline
        e.load_victims_tl(c.victims)
        assert _code(lambda: e.preempt_k(c.jobs, c.prio)) == _lib.FIT_E_STATE
        assert L.fit_preempt_tl_k_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE         # no fit_preempt_tl_k_device yet
        state, _, refused = e.hold_tl(c.queue, *hold)                               # fit_hold_tl leaves the lists alone
        assert refused == 0
        got = e.preempt_tl_k(c.jobs, c.prio, KMAX)
        assert_same(got, tk.hand_arrays())
        assert L.fit_preempt_tl_k_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE         # the host entry point is none
        for fn in (L.fit_preempt_tl_k, L.fit_preempt_tl_k_device):
            assert fn(e._h, 0, *NULLS, 8, None, None, None) == 0                    # j == 0, whatever the pointers
            assert fn(e._h, 1, *NULLS, 8, None, None, None) == _lib.FIT_E_INVAL
            assert fn(e._h, -1, *NULLS, 8, None, None, None) == _lib.FIT_E_INVAL
            assert fn(e._h, 0, *NULLS, 0, None, None, None) == _lib.FIT_E_INVAL     # kmax, even without a job
            assert fn(e._h, 0, *NULLS, 9, None, None, None) == _lib.FIT_E_INVAL
        assert b"kmax" in L.fit_last_error()
        assert L.fit_preempt_tl_k_ms(e._h, None) == _lib.FIT_E_INVAL
        assert e.unplace_tl(c.queue, *hold) == 2                                    # fit_unplace_tl and fit_place_tl too
        e.place_tl(take(c.jobs, slice(7, 8)))
        assert len(e.preempt_tl_k(c.jobs, c.prio, KMAX)[0]) == c.jobs.j
        e.load_timeline(c.tline)                                                    # drops them: their ends are its slots
        assert _code(lambda: e.preempt_tl_k(c.jobs, c.prio)) == _lib.FIT_E_STATE
        e.load_victims_tl(c.victims)
        e.hold_tl(c.queue, *hold)
        assert_same(preempt_both(e, c.jobs, c.prio), got)
        assert L.fit_preempt_tl_k_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_victims_tl(None)                                                     # every list empty
        none = preempt_both(e, c.jobs, c.prio)
        assert not none[0]["able"].any() and not (none[0]["code"] == E).any() and not none[2].any()
        assert_same(none, tk.ref_preempt_tl_k(c.nodes.part_mask, e.read_timeline(), None, c.parts, c.jobs, c.prio,
                                              tc.HAND_SLOT_MIN, KMAX))
        e.load_victims_tl(c.victims)
        e.load_nodes(c.nodes)                                                       # drops the timeline and the lists
        e.load_timeline(c.tline)
        assert _code(lambda: e.preempt_tl_k(c.jobs, c.prio)) == _lib.FIT_E_STATE


def test_a_sharded_context_answers_state():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    prio = np.zeros(16, np.int32)
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        assert _code(lambda: e.preempt_tl_k(jobs, prio)) == _lib.FIT_E_STATE


def test_a_rejected_victim_list_leaves_the_loaded_ones_answering(engine):
    c = tk.hand_case_k()
    load(engine, c, hold=HAND_HOLD)
    good = preempt_both(engine, c.jobs, c.prio)
    assert_same(good, tk.hand_arrays())
    v = c.victims
    for f, i, val in (("end", 0, -1), ("end", len(v.end) - 1, tc.HAND_H + 1), ("cpu", 2, -1), ("prio", 1, 0)):
        cols = {g: getattr(v, g).copy() for g in VCOLS}
        cols[f][i] = val
        assert _code(lambda: engine.load_victims_tl(synth.VictimsTL(*(cols[g] for g in VCOLS)))) == _lib.FIT_E_INVAL
        assert _code(lambda: engine.load_victims_tl_device(*(DevArray(cols[g]) for g in VCOLS))) == _lib.FIT_E_INVAL
        assert_same(engine.preempt_tl_k(c.jobs, c.prio, KMAX), good)


def test_every_invalid_argument_fails_the_whole_call(engine):
    c = tk.hand_case_k()
    load(engine, c, hold=HAND_HOLD)
    good = preempt_both(engine, c.jobs, c.prio)

    def device(jobs, kmax):
        cols = [DevArray(getattr(jobs, g)) for g in JCOLS] + [DevArray(np.asarray(jobs.nodes_k, np.uint16)), DevArray(c.prio)]
        outs = [DevArray(np.zeros(jobs.j, EVICT_K_DTYPE))] + [DevArray(np.zeros((jobs.j, max(kmax, 1)), np.int32)) for _ in range(2)]
        return _code(lambda: engine.preempt_tl_k_device(*cols, *outs, kmax=kmax))

    for kmax in (0, 9, -1):
        assert _code(lambda: engine.preempt_tl_k(c.jobs, c.prio, kmax)) == _lib.FIT_E_INVAL
        assert device(c.jobs, kmax) == _lib.FIT_E_INVAL
    for kmax in (1, 4, 7):  # the batch's largest nodes_k is 8
        assert _code(lambda: engine.preempt_tl_k(c.jobs, c.prio, kmax)) == _lib.FIT_E_INVAL
        assert device(c.jobs, kmax) == _lib.FIT_E_INVAL
    assert b"nodes_k" in _lib.lib().fit_last_error()
    for f in ("cpu", "mem", "gpu", "wall"):
        bad = take(c.jobs, slice(None))
        getattr(bad, f)[8] = -1
        assert _code(lambda: engine.preempt_tl_k(bad, c.prio)) == _lib.FIT_E_INVAL
        assert device(bad, KMAX) == _lib.FIT_E_INVAL
    with pytest.raises(ValueError):
        engine.preempt_tl_k(c.jobs, c.prio[:-1])
    assert_same(preempt_both(engine, c.jobs, c.prio), good)
    assert_same(good, tk.hand_arrays())

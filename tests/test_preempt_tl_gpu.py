"""fit_preempt_tl on the GPU against ref_preempt_tl (tests/_preempt_tl_cases.py, a numpy int64
restatement of DESIGN.md §2n on the dense timeline): rows compared field for field through the host
and the device entry point, on timelines WITH reservations, on shapes that cross every wave, tile and
slice edge of k_ptl_walk, run counts around TL_HEAD and the four-run loads, list lengths around the
four-entry loads, ends around the window's edge, int32 edge values, what fit_when, fit_preempt,
fit_unplace_tl and fit_advance_tl confirm, and the state errors."""
import ctypes as C

import numpy as np
import pytest

import _preempt_cases as pc
import _preempt_tl_cases as tc
import fitgpu
from _devarray import DevArray
from fitgpu import EVICT_DTYPE, Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu

INF, I32MIN = tc.INF, tc.I32MIN
ONE_PART = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
VCOLS = ("off", "prio", "end", "cpu", "mem", "gpu")
JCOLS = ("cpu", "mem", "gpu", "wall", "part", "nodes_k")


def preempt_both(e, jobs, prio):
    """Engine.preempt_tl through host pointers and through device pointers: the same rows."""
    host = e.preempt_tl(jobs, prio)
    cols = [DevArray(getattr(jobs, f)) for f in JCOLS[:5]] + [DevArray(np.asarray(prio, np.int32))]
    out = DevArray(np.full(jobs.j * 8, -7, np.int32).view(EVICT_DTYPE))
    ms = e.preempt_tl_device(*cols, out)
    assert ms > 0 and e.preempt_tl_ms() == ms
    assert np.array_equal(host, out.numpy()), "host and device entry points differ"
    return host


def assert_rows(got, want):
    for f in EVICT_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def take(jobs, idx):
    return synth.Jobs(*(np.array(getattr(jobs, f)[idx]) for f in JCOLS))  # copies: the cases are shared


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


def ref(e, c, jobs=None, prio=None, shift=0, stats=None):
    """The reference on what read_timeline() returns now."""
    jobs, prio = (c.jobs, c.prio) if jobs is None else (jobs, prio)
    return tc.ref_preempt_tl(c.nodes.part_mask, e.read_timeline(), c.victims, c.parts, jobs, prio, c.tline.slot_min,
                             shift, stats)


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


# ---- 1. the packed random cases, with reservations -----------------------------------------------
@pytest.mark.parametrize("n,j,device", [(65, 65, False), (257, 128, True)])
def test_packed_random_cases(engine, n, j, device):
    c = tc.packed_tl_case(n, j)
    want, stats, T = tc.packed_tl_ref(n, j)
    tc.rich_enough(want, stats)  # on the reference alone: a comparison of nothing interesting fails
    load(engine, c, device)
    member = c.nodes.part_mask != 0
    assert np.array_equal(engine.read_timeline()[member], T[member]), "place_tl left another timeline than the oracle"
    got = preempt_both(engine, c.jobs, c.prio)
    assert_rows(got, want)
    assert_rows(got, ref(engine, c))


def test_hand_written_case_gives_the_literal_rows(engine):
    c = tc.hand_case()
    hold = ([x for _, x, _ in tc.HAND_HOLDS], [s for _, _, s in tc.HAND_HOLDS])
    load(engine, c, hold=hold)
    assert engine.read_timeline()[:, :, 0].tolist() == tc.HAND_CPUS
    got = preempt_both(engine, c.jobs, c.prio)
    for q, want in enumerate(tc.HAND_ROWS):
        assert tuple(int(x) for x in got[q]) == want, (q, got[q], want)
    load(engine, c, device=True, hold=hold)
    assert np.array_equal(preempt_both(engine, c.jobs, c.prio), got)


# ---- 2. shapes at the seams ----------------------------------------------------------------------
# n: the wave sub-slices (8 waves share a slice's positions) and the node slices; J: the 64-job tiles,
# and above 256 jobs on several components the component-ordered job list.  One table per (n,
# components): every job is judged alone, so the first J jobs have the first J rows of the reference.
SEAM_J = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("one_component", [False, True])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_shapes_at_the_seams(engine, n, one_component):
    c = tc.packed_tl_case(n, 257, None, one_component)
    load(engine, c, device=n == 65)
    want = ref(engine, c)
    if n >= 63:
        assert (want["code"] == tc.EVICT).sum() >= 20 and (want["code"] == tc.NONE).any()
    for j in SEAM_J:
        assert_rows(preempt_both(engine, take(c.jobs, slice(0, j)), c.prio[:j]), want[:j])


def test_a_batch_above_one_chunk_of_positions(engine):
    """16,962 jobs on 65 nodes: the walk and the final run twice, the second time over 578 positions of
    the component-ordered job list.  The 257-job case repeated 66 times has the reference's rows
    repeated 66 times."""
    c = tc.packed_tl_case(65, 257)
    reps = 66
    jobs = synth.Jobs(*(np.tile(getattr(c.jobs, f), reps) for f in JCOLS))
    assert jobs.j > 16384 and len(np.unique(c.jobs.part)) > 2
    load(engine, c)
    assert_rows(preempt_both(engine, jobs, np.tile(c.prio, reps)), np.tile(ref(engine, c), reps))


# ---- 3. runs, list lengths and ends around the loads and the window ------------------------------
RUNS = (1, 4, 5, 8, 9, 13)
LENS = (0, 1, 3, 4, 5, 8, 9, 64, 65)
WIN = 16  # the window of the jobs below, in slots


def test_runs_lists_and_ends_at_every_seam(engine):
    """One node per (runs, list length, end of the last entry): R runs inside the 16-slot window (a
    release of one cpu at each of the slots 1 .. R - 1: TL_HEAD and the four-per-wait seam), a list of
    which only the last entry holds the 16 cpus a job wants, ending at 0, 1, d - 1, d, d + 1 or H.
    Free never reaches 16, so every run is short and the node can be freed exactly when the last
    entry's end is >= d.  The other entries hold 0 or 1 cpus and end at slots 1 .. 3."""
    Hh, sm = 64, 10
    ends = (0, 1, WIN - 1, WIN, WIN + 1, Hh)
    combos = [(r, ln, en) for r in RUNS for ln in LENS for en in ends]
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
    rows = [(16, 0, 0, WIN * sm, 0, p) for p in prios]
    rows += [(16, 0, 0, w, 0, INF) for w in (0, sm, sm + 1, (WIN - 1) * sm, (WIN + 1) * sm, Hh * sm, Hh * sm + 1)]
    rows += [(3, 0, 0, WIN * sm, 0, INF), (0, 0, 0, WIN * sm, 0, 0)]
    jobs, prio = tc.jobs_of(rows)
    c = tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, take(jobs, slice(0, 0)), ONE_PART, jobs, prio)
    load(engine, c)
    T = engine.read_timeline()
    for x, (r, _, _) in enumerate(combos[:: len(LENS) * len(ends)]):
        cpus = T[x * len(LENS) * len(ends), :WIN, 0]
        assert len(np.unique(cpus)) == r, (r, cpus)  # r runs inside the window
    got = preempt_both(engine, jobs, prio)
    assert_rows(got, ref(engine, c))
    r = got[len(prios) - 1]  # 16 cpus on 16 slots at INT32_MAX: lists whose last entry ends at d, d + 1 or H
    able = sum(1 for _, ln, en in combos if ln and en >= WIN)
    assert (r["code"], r["members"], r["fit"], r["able"], r["outranked"]) == (tc.EVICT, n, 0, able, 0), r
    assert (r["victims"], r["top_prio"]) == (1, 0)  # the one-entry lists: the fewest victims at the lowest top
    r = got[0]  # at INT32_MIN every such node is held
    assert (r["code"], r["able"], r["outranked"]) == (tc.NONE, 0, able), r
    r = got[len(prios) + 6]  # H + 1 slots: no node is eligible
    assert (r["code"], r["members"], r["able"], r["outranked"]) == (tc.NONE, n, 0, 0), r


def small_case(Hh, slot_min, seed, n=48, j=40):
    """A small random cluster on a horizon of Hh slots: up to 14 releases per node, lists of 0 .. 9
    entries with ends at 0, 1, d - 1, d, d + 1 and Hh for the windows d the jobs use, and one
    reservation window per node (held where it fits): the dips."""
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
             int(r.integers(0, 3)), int(r.integers(0, 7))) for _ in range(j)]
    jobs, prio = tc.jobs_of(rows)
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
    want = ref(e, c)
    assert_rows(preempt_both(e, c.jobs, c.prio), want)
    # on one slot some node of 48 always fits: there the nodes that can be freed show in the counters only
    assert (want["able"] > 0).any() and (want["outranked"] > 0).any() and (want["code"] == tc.NONE).any()
    assert Hh == 1 or (want["code"] == tc.EVICT).any()


# ---- 4. edge values ------------------------------------------------------------------------------
def flat_case(cpu, lists, rows, Hh=4, slot_min=10):
    """n nodes of `cpu` free cpus on an open timeline of Hh slots without events."""
    n = len(lists)
    nodes = synth.Nodes(np.asarray(cpu, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32),
                        np.ones(n, np.uint32))
    tline = synth.Timeline(Hh, slot_min, np.zeros(n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs, prio = tc.jobs_of(rows)
    return tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, take(jobs, slice(0, 0)), ONE_PART, jobs, prio)


def test_priorities_at_the_int32_ends(engine):
    c = flat_case([0, 0], [[(I32MIN, 4, 4, 0, 0), (INF, 4, 4, 0, 0)], [(INF, 4, 8, 0, 0)]],
                  [(4, 0, 0, 40, 0, I32MIN), (4, 0, 0, 40, 0, I32MIN + 1), (8, 0, 0, 40, 0, INF), (4, 0, 0, 40, 0, INF),
                   (9, 0, 0, 40, 0, INF)])
    load(engine, c)
    got = preempt_both(engine, c.jobs, c.prio)
    assert_rows(got, ref(engine, c))
    rows = [tuple(int(x) for x in r) for r in got]
    assert rows[0] == (tc.NONE, -1, 0, 0, 2, 0, 0, 2)        # a job at INT32_MIN evicts nothing
    assert rows[1] == (tc.EVICT, 0, 1, I32MIN, 2, 0, 1, 1)   # one above: the INT32_MIN victim goes
    assert rows[2] == (tc.NONE, -1, 0, 0, 2, 0, 0, 2)        # an INT32_MAX job does not evict an INT32_MAX victim
    assert rows[3] == (tc.EVICT, 0, 1, I32MIN, 2, 0, 1, 1)
    assert rows[4] == (tc.NONE, -1, 0, 0, 2, 0, 0, 0)        # no list frees 9 cpus: neither able nor outranked


def test_sums_are_exact_and_the_residual_is_clamped(engine):
    """Node 0: INT32_MAX free cpus and three victims of INT32_MAX cpus and 1 MiB each; node 1 the same
    free cpus, its victims hold no cpu.  A job of INT32_MAX - 5 cpus and 3 MiB needs all three on
    either: node 0's residual is min(sum, INT32_MAX) - demand = 5, node 1's as well: the lower id wins.
    A sum that wrapped would not fit; an unclamped residual would lose."""
    c = flat_case([INF, INF], [[(1, 4, INF, 1, 0)] * 3, [(1, 4, 0, 1, 0)] * 3],
                  [(INF - 5, 3, 0, 40, 0, 2), (INF, 2, 0, 40, 0, 2), (INF, 0, 0, 40, 0, 2), (0, 0, 0, 40, 0, 0)])
    load(engine, c)
    got = preempt_both(engine, c.jobs, c.prio)
    assert_rows(got, ref(engine, c))
    rows = [tuple(int(x) for x in r) for r in got]
    assert rows[0] == (tc.EVICT, 0, 3, 1, 2, 0, 2, 0)
    assert rows[1] == (tc.EVICT, 0, 2, 1, 2, 0, 2, 0)
    assert rows[2] == (tc.FITS, 0, 0, 0, 2, 2, 0, 0)
    assert rows[3] == (tc.FITS, 0, 0, 0, 2, 2, 0, 0)  # the all-zero demand


def test_an_entry_with_end_0_frees_nothing_and_keeps_its_place(engine):
    c = flat_case([0], [[(1, 0, 4, 0, 0), (2, 4, 4, 0, 0)]], [(4, 0, 0, 40, 0, 5), (0, 0, 0, 40, 0, 5), (4, 0, 0, 40, 0, 2)])
    load(engine, c)
    got = preempt_both(engine, c.jobs, c.prio)
    assert tuple(int(x) for x in got[0]) == (tc.EVICT, 0, 2, 2, 1, 0, 1, 0)
    assert tuple(int(x) for x in got[1]) == (tc.FITS, 0, 0, 0, 1, 1, 0, 0)
    assert tuple(int(x) for x in got[2]) == (tc.NONE, -1, 0, 0, 1, 0, 0, 1)


# ---- 5. relations --------------------------------------------------------------------------------
def test_members_fit_and_a_fits_rows_node_are_fit_whens(engine):
    """With an eighth of the queue placed some nodes still fit: members and fit are fit_when's members
    and now, a FITS row's node is fit_when's node."""
    c = tc.packed_tl_case(257, 257)
    k = c.queue.j // 8
    c = tc.CaseTL(c.nodes, c.victims, c.tline, take(c.queue, slice(0, k)), c.parts, c.jobs, c.prio)
    load(engine, c)
    got, eta = preempt_both(engine, c.jobs, c.prio), engine.when(c.jobs)
    assert_rows(got, ref(engine, c))
    assert np.array_equal(got["members"], eta["members"]) and np.array_equal(got["fit"], eta["now"])
    fits = got["code"] == tc.FITS
    assert fits.sum() >= 5 and (got["code"] == tc.EVICT).any()
    assert np.array_equal(fits, (eta["code"] == fitgpu.FIT_ETA_NOW))
    assert np.array_equal(got["node"][fits], eta["node"][fits])
    early = np.isin(got["code"], (1, 2, 3, 4, 5))
    assert early.any() and np.array_equal(got["code"][early], eta["code"][early])


def second_context_rows(c, jobs, prio):
    with Engine(device=0) as e2:
        e2.load_nodes(c.nodes)
        e2.load_partitions(c.parts)
        v = c.victims
        e2.load_victims(synth.Victims(v.off, v.prio, v.cpu, v.mem, v.gpu))
        return e2.preempt(jobs, prio)


def test_without_reservations_the_rows_are_fit_preempts(engine):
    """(a) no release events, slot_min = 1, walls in [1, H], every end H: the timeline is the node
    table on every open slot.  (b) the victims are exactly the release events and nothing is placed:
    the timeline never decreases in t, slot 0 binds.  A second context without a timeline answers
    fit_preempt with the same rows."""
    base = tc.packed_tl_case(257, 128)
    n, Hh = base.nodes.n, tc.H
    r = np.random.default_rng(5)
    # (a)
    v = base.victims
    va = synth.VictimsTL(v.off, v.prio, np.full(len(v.prio), Hh, np.int32), v.cpu, v.mem, v.gpu)
    empty = synth.Timeline(Hh, 1, np.zeros(n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs = take(base.jobs, slice(None))
    jobs.wall = r.integers(1, Hh + 1, jobs.j).astype(np.int32)
    nodes = take_nodes_with_avail(base.nodes, r.integers(0, 2 * Hh, n))
    ca = tc.CaseTL(nodes, va, empty, take(base.queue, slice(0, 0)), base.parts, jobs, base.prio)
    load(engine, ca)
    got = preempt_both(engine, jobs, base.prio)
    assert_rows(got, second_context_rows(ca, jobs, base.prio))
    assert (got["code"] == tc.EVICT).sum() >= 20
    # (b) walls that are whole slots, so that avail_min >= wall says what the timeline's closed slots say
    jobs = take(base.jobs, slice(None))
    jobs.wall = (tc.SLOT_MIN * r.choice([1, 2, 8, 20], jobs.j)).astype(np.int32)
    cb = tc.CaseTL(base.nodes, base.victims, base.tline, base.queue, base.parts, jobs, base.prio)
    load(engine, cb, place=False)
    got = preempt_both(engine, jobs, base.prio)
    assert_rows(got, second_context_rows(cb, jobs, base.prio))
    assert (got["code"] == tc.EVICT).sum() >= 20 and (got["victims"] >= 2).any()
    engine.place_tl(cb.queue)  # and with the reservations they are not
    assert not np.array_equal(preempt_both(engine, jobs, base.prio), got)


def take_nodes_with_avail(nodes, avail):
    return synth.Nodes(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, np.asarray(avail, np.int32), nodes.part_mask)


def test_unplacing_the_prefix_starts_the_job_now_and_one_less_does_not(engine):
    c = tc.packed_tl_case(257, 128)
    load(engine, c)
    got = engine.preempt_tl(c.jobs, c.prio)
    v = c.victims
    ev = np.flatnonzero(got["code"] == tc.EVICT)
    many = [q for q in ev if got["victims"][q] >= 2]
    picked = list(ev[:: max(1, len(ev) // 6)][:6]) + many[:3]
    assert len(picked) >= 6 and many
    before = engine.read_timeline()
    for q in picked:
        x, k = int(got["node"][q]), int(got["victims"][q])
        one = take(c.jobs, slice(q, q + 1))
        # unplace_tl leaves a closed slot closed, hold_tl refuses a window that reaches one: hand back
        # the open part of [0, end) only, which is the same timeline, so that hold_tl can take it again
        shut = np.flatnonzero(before[x, :, 0] < 0)
        u = int(shut[0]) if len(shut) else tc.H
        for cnt, now in ((k, 1), (k - 1, 0)):
            idx = np.arange(v.off[x], v.off[x] + cnt)
            idx = idx[v.end[idx] > 0]  # an entry with end 0 frees nothing
            rows = synth.Jobs(v.cpu[idx], v.mem[idx], v.gpu[idx], (np.minimum(v.end[idx], u) * tc.SLOT_MIN).astype(np.int32),
                              np.zeros(len(idx), np.uint16), np.ones(len(idx), np.uint16))
            node, start = np.full(len(idx), x, np.int32), np.zeros(len(idx), np.int32)
            if len(idx):
                assert engine.unplace_tl(rows, node, start) == len(idx)
            eta = engine.when(one)[0]
            assert eta["now"] == now, (q, got[q], cnt, eta)
            if now:
                assert (eta["code"], eta["node"], eta["start"]) == (fitgpu.FIT_ETA_NOW, x, 0), (q, got[q], eta)
            if len(idx):
                state, held, refused = engine.hold_tl(rows, node, start)  # take them back
                assert held == len(idx) and refused == 0
        assert engine.read_timeline().tobytes() == before.tobytes()


@pytest.mark.parametrize("a", [1, 8, tc.H])
def test_after_advance_tl_every_end_reads_a_slots_earlier(engine, a):
    c = tc.packed_tl_case(65, 65)
    load(engine, c)
    first = engine.preempt_tl(c.jobs, c.prio)
    engine.advance_tl(a)
    got = preempt_both(engine, c.jobs, c.prio)
    assert_rows(got, ref(engine, c, shift=a))
    if a < tc.H:
        assert not np.array_equal(got, first) and (got["code"] == tc.EVICT).any()
        engine.advance_tl(8)  # the shifts add up ...
        assert_rows(preempt_both(engine, c.jobs, c.prio), ref(engine, c, shift=a + 8))
        engine.advance_tl(tc.H)  # ... and saturate at H
    after = preempt_both(engine, c.jobs, c.prio)
    assert_rows(after, ref(engine, c, shift=tc.H))
    assert not after["able"].any() and not after["outranked"].any()  # every end reads 0: nothing can be freed
    engine.load_victims_tl(c.victims)  # a new load starts from shift 0 again
    assert_rows(preempt_both(engine, c.jobs, c.prio), ref(engine, c))


def test_preempt_tl_changes_nothing(engine):
    c = tc.packed_tl_case(257, 128)
    load(engine, c)
    before = engine.read_timeline()
    first = preempt_both(engine, c.jobs, c.prio)
    assert engine.read_timeline().tobytes() == before.tobytes(), "preempt_tl changed the timeline"
    assert preempt_both(engine, c.jobs, c.prio).tobytes() == first.tobytes(), "a second call differs"


# ---- 6. state and argument errors ----------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_state_errors():
    c = tc.hand_case()
    hold = (np.array([x for _, x, _ in tc.HAND_HOLDS], np.int32), np.array([s for _, _, s in tc.HAND_HOLDS], np.int32))
    L = _lib.lib()
    ms = C.c_double()
    none7 = (None,) * 7
    with Engine(device=0) as e:
        assert _code(lambda: e.preempt_tl(c.jobs, c.prio)) == _lib.FIT_E_STATE    # before load_nodes
        assert L.fit_load_victims_tl(e._h, *none7[:6]) == _lib.FIT_E_STATE
        assert L.fit_load_victims_tl_device(e._h, None, 0, *none7[:5]) == _lib.FIT_E_STATE
        e.load_nodes(c.nodes)
        e.load_partitions(c.parts)
        assert _code(lambda: e.preempt_tl(c.jobs, c.prio)) == _lib.FIT_E_STATE    # without a timeline
        assert _code(lambda: e.load_victims_tl(c.victims)) == _lib.FIT_E_STATE
        assert L.fit_load_victims_tl_device(e._h, None, 0, *none7[:5]) == _lib.FIT_E_STATE
        e.load_victims(None)                                                      # fit_load_victims' lists are not these
        e.load_timeline(c.tline)
        assert _code(lambda: e.preempt_tl(c.jobs, c.prio)) == _lib.FIT_E_STATE    # before load_victims_tl
        assert b"fit_load_victims_tl" in L.fit_last_error()
        assert L.fit_preempt_tl(e._h, 0, *none7) == _lib.FIT_E_STATE
        assert _code(lambda: e.preempt(c.jobs, c.prio)) == _lib.FIT_E_STATE       # fit_preempt still refuses a timeline
        e.load_victims_tl(c.victims)
        assert _code(lambda: e.preempt(c.jobs, c.prio)) == _lib.FIT_E_STATE
        assert L.fit_preempt_tl_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE         # no fit_preempt_tl_device yet
        state, _, refused = e.hold_tl(c.queue, *hold)                             # fit_hold_tl leaves the lists alone
        assert refused == 0
        got = e.preempt_tl(c.jobs, c.prio)
        assert [tuple(int(x) for x in r) for r in got] == tc.HAND_ROWS
        assert L.fit_preempt_tl_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE         # the host entry point is none
        assert L.fit_preempt_tl(e._h, 0, *none7) == 0
        assert L.fit_preempt_tl_device(e._h, 0, *none7) == 0
        assert L.fit_preempt_tl(e._h, 1, *none7) == _lib.FIT_E_INVAL
        assert L.fit_preempt_tl(e._h, -1, *none7) == _lib.FIT_E_INVAL
        assert e.unplace_tl(c.queue, *hold) == 2                                  # fit_unplace_tl and fit_place_tl too
        e.place_tl(take(c.jobs, slice(10, 11)))
        assert len(e.preempt_tl(c.jobs, c.prio)) == c.jobs.j
        e.load_timeline(c.tline)                                                  # drops them: their ends are its slots
        assert _code(lambda: e.preempt_tl(c.jobs, c.prio)) == _lib.FIT_E_STATE
        e.load_victims_tl(c.victims)
        e.hold_tl(c.queue, *hold)
        assert np.array_equal(preempt_both(e, c.jobs, c.prio), got)
        assert L.fit_preempt_tl_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_victims_tl(None)                                                   # every list empty
        none = preempt_both(e, c.jobs, c.prio)
        assert not none["able"].any() and not none["outranked"].any() and not (none["code"] == tc.EVICT).any()
        assert_rows(none, tc.ref_preempt_tl(c.nodes.part_mask, e.read_timeline(), None, c.parts, c.jobs, c.prio,
                                            tc.HAND_SLOT_MIN))
        e.load_victims_tl_device(None, None, None, None, None, None)
        assert np.array_equal(e.preempt_tl(c.jobs, c.prio), none)
        e.load_victims_tl(c.victims)
        e.load_nodes(c.nodes)                                                     # drops the timeline and the lists
        e.load_timeline(c.tline)
        assert _code(lambda: e.preempt_tl(c.jobs, c.prio)) == _lib.FIT_E_STATE


def test_a_sharded_context_holds_no_victims():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    prio = np.zeros(16, np.int32)
    L = _lib.lib()
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        assert _code(lambda: e.load_victims_tl(None)) == _lib.FIT_E_STATE
        assert L.fit_load_victims_tl_device(e._h, None, 0, None, None, None, None, None) == _lib.FIT_E_STATE
        assert _code(lambda: e.preempt_tl(jobs, prio)) == _lib.FIT_E_STATE


def test_every_invalid_victim_list_fails_as_a_whole_and_keeps_the_loaded_ones(engine):
    c = tc.hand_case()
    hold = ([x for _, x, _ in tc.HAND_HOLDS], [s for _, _, s in tc.HAND_HOLDS])
    load(engine, c, hold=hold)
    good = preempt_both(engine, c.jobs, c.prio)
    assert [tuple(int(x) for x in r) for r in good] == tc.HAND_ROWS
    L = _lib.lib()
    v = c.victims
    n, nv = c.nodes.n, len(v.prio)

    def variant(**kw):
        cols = {f: getattr(v, f).copy() for f in VCOLS}
        for f, (i, val) in kw.items():
            cols[f][i] = val
        return cols

    def host(cols):
        return L.fit_load_victims_tl(engine._h, *(C.c_void_p(cols[f].ctypes.data) if cols[f] is not None else None
                                                  for f in VCOLS))

    def device(cols, n_vic=None):
        dev = {f: DevArray(cols[f]) if cols[f] is not None else None for f in VCOLS}
        return L.fit_load_victims_tl_device(engine._h, C.c_void_p(dev["off"].data_ptr()) if dev["off"] else None,
                                            nv if n_vic is None else n_vic,
                                            *(C.c_void_p(dev[f].data_ptr()) if dev[f] else None for f in VCOLS[1:]))

    assert host(variant()) == 0 and device(variant()) == 0  # the harness itself loads the good lists
    bad = [variant(off=(0, 1)),                      # vic_off[0] != 0
           variant(off=(3, 1)),                      # a decreasing vic_off
           variant(cpu=(2, -1)), variant(mem=(0, -1)), variant(gpu=(nv - 1, -1)),  # a negative amount
           variant(end=(0, -1)), variant(end=(nv - 1, tc.HAND_H + 1)),             # an end outside [0, H]
           variant(prio=(1, 0)),                     # node 0: priorities 1, 0 decrease
           variant(prio=(3, 5))]                     # node 2: 5, 3 decrease at its last entry
    for f in VCOLS[1:]:                              # a NULL column when there are entries
        cols = variant()
        cols[f] = None
        bad.append(cols)
    for cols in bad:
        for fn in (host, device):
            assert fn(cols) == _lib.FIT_E_INVAL, cols
            assert np.array_equal(engine.preempt_tl(c.jobs, c.prio), good), "a rejected load changed the loaded lists"
    assert device(variant(), n_vic=nv - 1) == _lib.FIT_E_INVAL  # vic_off does not end at n_vic
    assert device(variant(), n_vic=-1) == _lib.FIT_E_INVAL
    assert device(variant(off=(n, nv + 1))) == _lib.FIT_E_INVAL  # ends past the entries
    assert L.fit_load_victims_tl_device(engine._h, None, 3, None, None, None, None, None) == _lib.FIT_E_INVAL
    assert np.array_equal(preempt_both(engine, c.jobs, c.prio), good)
    ok = variant(end=(0, tc.HAND_H))  # an end at the horizon is inside
    assert host(ok) == 0 and device(ok) == 0
    with pytest.raises(ValueError):
        engine.load_victims_tl(synth.VictimsTL(v.off[:-1], v.prio, v.end, v.cpu, v.mem, v.gpu))  # off needs n + 1 entries


def test_every_invalid_job_fails_the_whole_call(engine):
    c = tc.hand_case()
    hold = ([x for _, x, _ in tc.HAND_HOLDS], [s for _, _, s in tc.HAND_HOLDS])
    load(engine, c, hold=hold)
    for f in ("cpu", "mem", "gpu", "wall"):
        bad = take(c.jobs, slice(None))
        getattr(bad, f)[5] = -1
        assert _code(lambda: engine.preempt_tl(bad, c.prio)) == _lib.FIT_E_INVAL
        cols = [DevArray(getattr(bad, g)) for g in JCOLS[:5]] + [DevArray(c.prio)]
        out = DevArray(np.zeros(c.jobs.j, EVICT_DTYPE))
        assert _code(lambda: engine.preempt_tl_device(*cols, out)) == _lib.FIT_E_INVAL
    with pytest.raises(ValueError):
        engine.preempt_tl(c.jobs, c.prio[:-1])
    assert [tuple(int(x) for x in r) for r in preempt_both(engine, c.jobs, c.prio)] == tc.HAND_ROWS

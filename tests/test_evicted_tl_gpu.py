"""fit_evicted_tl and fit_read_victims_tl on the GPU against ref_evicted_tl (tests/_evicted_tl_cases.py, a
numpy int64 restatement of DESIGN.md §2p): after every call read_timeline() and read_victims_tl() are
compared with the reference byte for byte, through the host and the device entry point, on timelines
WITH reservations, on shapes that cross the wave and block edges of the check and of the in-place
compaction, horizons of 1 to 1,024 slots, int32 edge values, closed slots, 20,000 rows with the launch
seam inside one node's rows, the relations of §2p and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import _evicted_tl_cases as ec
import _preempt_tl_cases as tc
import fitgpu
from _devarray import DevArray
from fitgpu import EVICT_DTYPE, EVICT_K_DTYPE, Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu

INF = tc.INF
JCOLS = ("cpu", "mem", "gpu", "wall", "part", "nodes_k")
ONE_PART = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
NO_ROWS = np.zeros((0, 2), np.int32)


@pytest.fixture(scope="module")
def engines():
    with Engine(device=0) as a, Engine(device=0) as b, Engine(device=0) as c:
        yield a, b, c


def setup(e, c, a=0, tail=None, victims=None):
    """Node table, partitions, the timeline from the release events, the queue's reservations, the
    victims, then the clock moved by a slots."""
    e.load_nodes(c.nodes)
    e.load_partitions(c.parts)
    e.load_timeline(c.tline)
    if c.queue.j:
        e.place_tl(c.queue)
    e.load_victims_tl(c.victims if victims is None else victims)
    if a:
        e.advance_tl(a, tail)


def state(e):
    return ec.bytes_of(e.read_timeline(), e.read_victims_tl())


def evict_host(e, rows):
    rows = np.asarray(rows, np.int32).reshape(-1, 2)
    e.evicted_tl(rows[:, 0], rows[:, 1])


def evict_device(e, rows):
    rows = np.asarray(rows, np.int32).reshape(-1, 2)
    ms = e.evicted_tl_device(DevArray(rows[:, 0]), DevArray(rows[:, 1]))
    if len(rows):
        assert ms > 0 and e.evicted_tl_ms() == ms
    return ms


def check_call(engines, c, rows, a=0, tail=None, shuffled=None):
    """The same state in two contexts; `rows` through the host entry point of the first and (sorted,
    unless `shuffled` gives another order) through the device entry point of the second; both against
    the reference on what read_timeline() returned before, byte for byte.  Returns (T', victims')."""
    e1, e2 = engines[:2]
    rows = np.asarray(rows, np.int32).reshape(-1, 2)
    for e in (e1, e2):
        setup(e, c, a, tail)
    T0 = e1.read_timeline()
    assert e2.read_timeline().tobytes() == T0.tobytes()
    want = ec.ref_evicted_tl(T0, c.victims, a, rows, c.nodes.part_mask)
    evict_host(e1, rows)
    evict_device(e2, rows[np.lexsort((rows[:, 1], rows[:, 0]))] if shuffled is None else shuffled)
    for e in (e1, e2):
        assert e.read_timeline().tobytes() == want[0].tobytes(), "the timeline differs from the reference"
        got = e.read_victims_tl()
        for f in ec.VCOLS:
            assert np.array_equal(getattr(got, f), getattr(want[1], f)), f"the lists differ from the reference in {f}"
    return want


def assert_rows(got, want, dtype=EVICT_DTYPE):
    for f in dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def take(jobs, idx):
    return synth.Jobs(*(np.array(getattr(jobs, f)[idx]) for f in JCOLS))


def with_k(jobs, seed=3):
    k = np.random.default_rng(seed).choice([1, 1, 2, 3, 4, 8], jobs.j).astype(np.uint16)
    return synth.Jobs(jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.part, k)


# ---- 1. the packed cases: advance, evict, and the defining relation ------------------------------
@pytest.mark.parametrize("n,one_component", sorted(ec.SEEDS))
def test_packed_cases_after_an_advance_and_the_defining_relation(engines, n, one_component):
    c, rows = ec.packed_rows(n, one_component)
    a = ec.PACKED_SHIFT
    # on the reference alone, before any comparison: a comparison of nothing interesting fails
    ec.rich_enough(ec.advanced(tc.oracle_timeline(c), a), c.victims, a, rows, c.nodes.part_mask)
    e1, e2, e3 = engines
    T1, v1 = check_call(engines, c, rows, a, shuffled=rows)  # relation 5; the device call takes them shuffled too
    setup(e2, c, a)
    evict_device(e2, rows[np.lexsort((rows[:, 1], rows[:, 0]))])  # sorted rows give the same bytes
    assert state(e2) == state(e1)
    # relation 1: a second context that was told the old way, and in full
    setup(e3, c, a)
    jobs, node, start = ec.unplace_rows(c.victims, a, rows, c.tline.slot_min)
    assert jobs.j < len(rows), "no evicted entry with e' = 0"
    assert e3.unplace_tl(jobs, node, start) == jobs.j
    e3.load_victims_tl(v1)
    assert e3.read_timeline().tobytes() == T1.tobytes()
    jk = with_k(c.jobs)
    for e in (e1, e2):
        assert_rows(e.preempt_tl(c.jobs, c.prio), e3.preempt_tl(c.jobs, c.prio))
        got, want = e.preempt_tl_k(jk, c.prio, 8), e3.preempt_tl_k(jk, c.prio, 8)
        assert_rows(got[0], want[0], EVICT_K_DTYPE)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(e.when(c.jobs), e3.when(c.jobs))
        wk, wn = e.when_k(jk, 8)
        wk3, wn3 = e3.when_k(jk, 8)
        assert np.array_equal(wk, wk3) and np.array_equal(wn, wn3)
    # and against the reference on the true state: the lists' ends are e' now, the shift stays a
    assert_rows(e1.preempt_tl(c.jobs, c.prio),
                tc.ref_preempt_tl(c.nodes.part_mask, T1, v1, c.parts, c.jobs, c.prio, c.tline.slot_min))
    # relation 7: the read-back loads into a context with the same timeline and answers the same
    back = e1.read_victims_tl()
    assert ec.same_victims(back, v1)
    e3.load_victims_tl(back)
    assert_rows(e3.preempt_tl(c.jobs, c.prio), e1.preempt_tl(c.jobs, c.prio))
    # place_tl_k leaves the same timeline and the same placements behind on both
    q = take(jk, slice(0, 64))
    p1, p3 = e1.place_tl_k(q, 8), e3.place_tl_k(q, 8)
    assert np.array_equal(p1[0], p3[0]) and np.array_equal(p1[1], p3[1])
    assert e1.read_timeline().tobytes() == e3.read_timeline().tobytes()


# ---- 2. shapes at the seams ----------------------------------------------------------------------
@pytest.mark.parametrize("one_component", [False, True])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_shapes_at_the_seams(engines, n, one_component):
    c, rows = ec.packed_rows(n, one_component, 0, 0.5)
    if n >= 63:
        assert len(rows) >= 20
    check_call(engines, c, rows)
    check_call(engines, c, rows[:1] if len(rows) else rows)


LENS = (0, 1, 63, 64, 65, 128, 129, 300, 5)


@functools.lru_cache(maxsize=None)
def long_lists_case(lens=LENS, Hh=64, seed=11, amounts=64):
    """One node per list length on an open timeline (node 2 closes at slot 40, the last node is in no
    partition): random amounts, ends anywhere in [0, H], priorities in order.  Cached, never written."""
    r = np.random.default_rng(seed)
    n = len(lens)
    lists = [sorted(((int(r.integers(0, 6)), int(r.integers(0, Hh + 1)), int(r.integers(0, amounts)),
                      int(r.integers(0, 4096)), int(r.integers(0, 3))) for _ in range(ln)), key=lambda e: e[0])
             for ln in lens]
    mask = np.ones(n, np.uint32)
    avail = np.full(n, INF, np.int32)
    mask[n - 1], avail[2] = 0, 40 * 10
    nodes = synth.Nodes(r.integers(0, 8, n).astype(np.int32), np.full(n, 1024, np.int32), np.zeros(n, np.int32), avail,
                        mask)
    tline = synth.Timeline(Hh, 10, np.zeros(n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs, prio = tc.jobs_of([(8, 0, 0, 40, 0, 9)])
    return tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, take(jobs, slice(0, 0)), ONE_PART, jobs, prio)


def picks(ln, kind):
    return {"first": [0], "last": [ln - 1], "all": list(range(ln)), "every other": list(range(0, ln, 2)),
            "62-65": [p for p in (62, 63, 64, 65) if p < ln], "none": []}[kind] if ln else []


@pytest.mark.parametrize("kind", ["first", "last", "all", "every other", "62-65", "none"])
def test_list_lengths_at_the_compactions_block_edges(engines, kind):
    c = long_lists_case()
    ln = ec.list_lengths(c.victims, c.nodes.n, c.nodes.part_mask)
    assert ln.tolist() == [0, 1, 63, 64, 65, 128, 129, 300, 0] and np.diff(c.victims.off)[8] == 5
    rows = np.array([(x, p) for x in range(c.nodes.n) for p in picks(int(ln[x]), kind)], np.int32).reshape(-1, 2)
    assert (len(rows) == 0) == (kind == "none")
    T1, v1 = check_call(engines, c, rows)
    if kind == "all":
        assert v1.off[-1] == 0
    if kind != "none":
        assert (T1[2, 40:] == -1).all() and (T1[2, :40] >= 0).all() and (T1[8] == -1).all()
        # a second call on the shortened lists: positions refer to the lists as they are now
        e1, e2 = engines[:2]
        left = ec.list_lengths(v1, c.nodes.n)
        rows2 = np.array([(x, p) for x in range(c.nodes.n) for p in picks(int(left[x]), "every other")],
                         np.int32).reshape(-1, 2)
        want = ec.ref_evicted_tl(T1, v1, 0, rows2)
        evict_host(e1, rows2)
        evict_device(e2, rows2)
        for e in (e1, e2):
            assert state(e) == ec.bytes_of(*want)


@pytest.mark.parametrize("Hh", [1, 64, 1024])
def test_horizons_with_ends_0_1_and_h(engines, Hh):
    r = np.random.default_rng(200 + Hh)
    n, slot_min = 48, 3
    nodes = synth.Nodes(r.integers(0, 6, n).astype(np.int32), np.full(n, 8192, np.int32),
                        r.integers(0, 2, n).astype(np.int32),
                        np.where(r.random(n) < 0.3, r.integers(0, Hh * slot_min + 1, n), INF).astype(np.int32),
                        np.where(r.random(n) < 0.1, 0, 1).astype(np.uint32))
    cnt = r.integers(0, 15, n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    slot = np.concatenate([np.sort(r.integers(0, Hh, k)) for k in cnt] + [np.zeros(0, np.int64)]).astype(np.int32)
    tline = synth.Timeline(Hh, slot_min, off, slot, r.integers(0, 4, len(slot)).astype(np.int32),
                           r.integers(0, 1024, len(slot)).astype(np.int32), np.zeros(len(slot), np.int32))
    ends = sorted({0, 1, Hh // 2, Hh - 1, Hh} & set(range(Hh + 1)))
    lists = [sorted(((int(r.integers(0, 6)), int(r.choice(ends)), int(r.integers(0, 9)), int(r.integers(0, 2048)),
                      int(r.integers(0, 2))) for _ in range(r.integers(0, 10))), key=lambda e: e[0]) for _ in range(n)]
    jobs, prio = tc.jobs_of([(1, 0, 0, 1, 0, 9)])
    c = tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, take(jobs, slice(0, 0)), ONE_PART, jobs, prio)
    ln = ec.list_lengths(c.victims, n, nodes.part_mask)
    rows = np.array([(x, p) for x in range(n) for p in range(ln[x]) if r.random() < 0.5], np.int32)
    k = c.victims.off[rows[:, 0]] + rows[:, 1]
    assert {0, Hh} <= set(c.victims.end[k].tolist()) and len(rows) >= 20
    for a in (0, 1):
        T1, _ = check_call(engines, c, rows, a)
    assert Hh == 1 or (T1 == -1).any()


def test_saturation_and_closed_slots(engines):
    """Node 0: INT32_MAX - 5 free cpus and INT32_MAX MiB, entries of INT32_MAX and of 10 cpus; node 1:
    closed from slot 2 on with an entry over the whole horizon; node 2: zero free, amounts at INT32_MAX."""
    lists = [[(1, 4, INF, INF, 0), (2, 3, 10, 1, 1)], [(1, 4, 7, 7, 7)], [(1, 2, INF, INF, INF), (1, 4, INF, 0, 1)]]
    nodes = synth.Nodes(np.array([INF - 5, 1, 0], np.int32), np.array([INF, 1, 0], np.int32), np.zeros(3, np.int32),
                        np.array([INF, 20, INF], np.int32), np.ones(3, np.uint32))
    tline = synth.Timeline(4, 10, np.zeros(4, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    jobs, prio = tc.jobs_of([(1, 0, 0, 1, 0, 9)])
    c = tc.CaseTL(nodes, tc.victims_tl_of(lists), tline, take(jobs, slice(0, 0)), ONE_PART, jobs, prio)
    T1, v1 = check_call(engines, c, [(0, 1), (1, 0), (2, 0), (2, 1), (0, 0)])
    assert T1[0, :, 0].tolist() == [INF] * 4 and T1[0, :, 2].tolist() == [1, 1, 1, 0]
    assert T1[1].tolist() == [[8, 8, 7]] * 2 + [[-1, -1, -1]] * 2
    assert T1[2].tolist() == [[INF, INF, INF]] * 2 + [[INF, 0, 1]] * 2 and v1.off[-1] == 0


@pytest.mark.parametrize("chunk", [None, "7"])
def test_20000_rows_and_the_launch_seam_inside_a_nodes_rows(engines, monkeypatch, chunk):
    c = long_lists_case(tuple(int(v) for v in 80 + np.random.default_rng(1).integers(0, 41, 257)), 64, 13, 4)
    ln = ec.list_lengths(c.victims, 257, c.nodes.part_mask)
    r = np.random.default_rng(2)
    every = np.array([(x, p) for x in range(257) for p in range(ln[x])], np.int32)
    rows = every[r.permutation(len(every))[:20000]]
    assert len(rows) == 20000 and np.bincount(rows[:, 0]).max() >= 64
    if chunk:
        monkeypatch.setenv("FIT_UTL_CHUNK", chunk)
    check_call(engines, c, rows, shuffled=rows)
    if chunk:  # a bad row in a late chunk: the marks of every chunk before it are taken back
        e1 = engines[0]
        setup(e1, c)
        before = state(e1)
        bad = np.concatenate([rows[:500], rows[3:4]])
        assert code(lambda: evict_host(e1, bad)) == _lib.FIT_E_INVAL and state(e1) == before
        evict_host(e1, rows)
        T0 = np.frombuffer(before[0], np.int32).reshape(257, 64, 3)
        assert state(e1) == ec.bytes_of(*ec.ref_evicted_tl(T0, c.victims, 0, rows, c.nodes.part_mask))


# ---- 3. the loop closes --------------------------------------------------------------------------
def test_the_loop_closes_on_one_node(engines):
    e = engines[0]
    c = tc.packed_tl_case(257, 128)
    setup(e, c)
    got = e.preempt_tl(c.jobs, c.prio)
    ev = np.flatnonzero(got["code"] == tc.EVICT)
    many = [q for q in ev if got["victims"][q] >= 2]
    assert len(ev) >= 20 and many
    for q in list(ev[:: max(1, len(ev) // 3)][:3]) + many[:2]:
        x, k = int(got["node"][q]), int(got["victims"][q])
        one = take(c.jobs, slice(q, q + 1))
        setup(e, c)
        evict_host(e, [(x, p) for p in range(k)])
        r = e.preempt_tl(one, c.prio[q:q + 1])[0]
        assert (r["code"], r["node"], r["fit"], r["victims"]) == (tc.FITS, x, 1, 0), (q, got[q], r)
        setup(e, c)  # a fresh copy, one entry fewer
        evict_host(e, [(x, p) for p in range(k - 1)])
        r = e.preempt_tl(one, c.prio[q:q + 1])[0]
        assert r["code"] != tc.FITS and r["fit"] == 0, (q, got[q], r)


def test_the_loop_closes_on_several_nodes(engines):
    e = engines[0]
    c = tc.packed_tl_case(257, 128)
    jk = with_k(c.jobs, 5)
    setup(e, c)
    rows, node, vic = e.preempt_tl_k(jk, c.prio, 8)
    ev = [q for q in np.flatnonzero(rows["code"] == tc.EVICT) if rows["need"][q] >= 2]
    assert len(ev) >= 3
    for q in ev[:: max(1, len(ev) // 3)][:3]:
        need = int(rows["need"][q])
        one = take(jk, slice(q, q + 1))
        setup(e, c)
        evict_device(e, [(int(node[q, i]), p) for i in range(need) for p in range(int(vic[q, i]))])
        r, rn, rv = e.preempt_tl_k(one, c.prio[q:q + 1], 8)
        assert r[0]["code"] == tc.FITS and r[0]["victims"] == 0 and not rv.any(), (q, rows[q], r[0])
        assert set(rn[0, :need].tolist()) == set(node[q, :need].tolist())
        pn, ps, _ = e.place_tl_k(one, 8)
        assert ps[0] == 0 and set(pn[0, :need].tolist()) == set(node[q, :need].tolist()) and (pn[0, need:] == -1).all()


# ---- 4. the double count the old recipe produced -------------------------------------------------
def test_unplacing_alone_counts_the_evicted_entries_twice(engines):
    e1, e2 = engines[:2]
    c, rows, T1, v1, wrong, true = ec.double_count_case()
    differ = np.flatnonzero([tuple(a) != tuple(b) for a, b in zip(wrong.tolist(), true.tolist())])
    assert differ.size > 0, "the recorded case has no job whose answer the double count changes"  # reference alone
    setup(e1, c)
    jobs, node, start = ec.unplace_rows(c.victims, 0, rows, c.tline.slot_min)
    e1.unplace_tl(jobs, node, start)  # INTEGRATION.md item 11 as it was: the entries stay in the lists
    assert e1.read_timeline().tobytes() == T1.tobytes()
    got = e1.preempt_tl(c.jobs, c.prio)
    assert_rows(got, wrong)
    assert any(tuple(got[q].tolist()) != tuple(true[q].tolist()) for q in differ)
    setup(e2, c)
    evict_host(e2, rows)
    assert_rows(e2.preempt_tl(c.jobs, c.prio), true)


# ---- 5. evict and advance commute ----------------------------------------------------------------
@pytest.mark.parametrize("a", [1, 8, tc.H])
def test_evict_and_advance_commute_with_explicit_tails(engines, a):
    e1, e2 = engines[:2]
    c, rows = ec.packed_rows(65)
    tail = np.random.default_rng(a).integers(-1, 50, (c.nodes.n, 3)).astype(np.int32)
    setup(e1, c, a, tail)
    evict_host(e1, rows)
    setup(e2, c)
    evict_host(e2, rows)
    mid = e2.read_victims_tl()
    e2.advance_tl(a, tail)
    assert state(e1) == state(e2)
    after = e2.read_victims_tl()
    assert np.array_equal(after.end, np.maximum(mid.end - a, 0)) and np.array_equal(after.off, mid.off)


# ---- 6. untouched lists ---------------------------------------------------------------------------
def test_untouched_lists_read_back_as_loaded(engines):
    e = engines[0]
    c, _ = ec.packed_rows(257)
    setup(e, c)
    T = e.read_timeline()
    assert (c.nodes.part_mask == 0).any()
    assert state(e) == ec.bytes_of(*ec.ref_evicted_tl(T, c.victims, 0, NO_ROWS, c.nodes.part_mask))
    got = e.read_victims_tl()
    member = np.repeat(c.nodes.part_mask != 0, np.diff(c.victims.off))
    assert np.array_equal(got.end, c.victims.end[member]) and len(got.end) < len(c.victims.end)
    evict_host(e, NO_ROWS)
    assert evict_device(e, NO_ROWS) == 0.0
    assert state(e) == ec.bytes_of(*ec.ref_evicted_tl(T, c.victims, 0, NO_ROWS, c.nodes.part_mask))
    e.advance_tl(3)
    assert ec.same_victims(e.read_victims_tl(), ec.ref_evicted_tl(T, c.victims, 3, NO_ROWS, c.nodes.part_mask)[1])
    e.advance_tl(tc.H)
    assert not e.read_victims_tl().end.any()
    e.load_victims_tl(None)
    assert not e.read_victims_tl().off.any()
    # sizing: off alone with cap 0; columns stay unwritten when cap is short
    e.load_victims_tl(c.victims)
    L = _lib.lib()
    off = np.full(c.nodes.n + 1, -7, np.int32)
    assert L.fit_read_victims_tl(e._h, C.c_void_p(off.ctypes.data), 0, None, None, None, None, None) == 0
    nv = int(off[-1])
    assert off[0] == 0 and nv == len(got.end)
    cols = [np.full(nv, -7, np.int32) for _ in range(5)]
    ptrs = [C.c_void_p(a.ctypes.data) for a in cols]
    assert L.fit_read_victims_tl(e._h, C.c_void_p(off.ctypes.data), nv - 1, *ptrs) == 0
    assert all((a == -7).all() for a in cols)
    assert L.fit_read_victims_tl(e._h, C.c_void_p(off.ctypes.data), nv, *ptrs[:4], None) == 0
    assert all((a == -7).all() for a in cols)
    assert L.fit_read_victims_tl(e._h, C.c_void_p(off.ctypes.data), nv, *ptrs) == 0
    assert np.array_equal(cols[1], got.end) and np.array_equal(cols[0], got.prio)
    assert L.fit_read_victims_tl(e._h, None, nv, *ptrs) == _lib.FIT_E_INVAL


# ---- 7. refusals ---------------------------------------------------------------------------------
def code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


@pytest.mark.parametrize("chunk", [None, "4"])
def test_every_refusal_leaves_everything_byte_identical(engines, monkeypatch, chunk):
    e = engines[0]
    c, rows = ec.packed_rows(65)
    if chunk:
        monkeypatch.setenv("FIT_UTL_CHUNK", chunk)
    setup(e, c, 2)
    before = state(e)
    ln = ec.list_lengths(c.victims, 65, c.nodes.part_mask)
    full = int(np.flatnonzero(ln >= 2)[0])
    out = int(np.flatnonzero(c.nodes.part_mask == 0)[0])
    assert np.diff(c.victims.off)[out] > 0  # it was loaded with entries: validated, never used
    good = rows[:9]
    bads = [(-1, 0), (65, 0), (INF, 0), (full, -1), (full, int(ln[full])), (full, INF), (out, 0), tuple(good[2]),
            tuple(good[8])]
    L = _lib.lib()
    for bad in bads:
        for where in (0, 5, len(good)):  # first, in the second chunk of 4, last
            batch = np.concatenate([good[:where], np.array([bad], np.int32), good[where:]])
            assert code(lambda: evict_host(e, batch)) == _lib.FIT_E_INVAL, (bad, where)
            assert b"position" in L.fit_last_error()
            assert state(e) == before, (bad, where, "host")
            assert code(lambda: evict_device(e, batch)) == _lib.FIT_E_INVAL, (bad, where)
            assert state(e) == before, (bad, where, "device")
    p = C.c_void_p(np.zeros(1, np.int32).ctypes.data)
    for fn in (L.fit_evicted_tl, L.fit_evicted_tl_device):
        assert fn(e._h, -1, p, p) == _lib.FIT_E_INVAL
        assert fn(e._h, 1, None, p) == _lib.FIT_E_INVAL and fn(e._h, 1, p, None) == _lib.FIT_E_INVAL
        assert fn(e._h, 0, None, None) == 0
    with pytest.raises(ValueError):
        e.evicted_tl(np.zeros(2, np.int32), np.zeros(3, np.int32))
    assert state(e) == before
    # the marks of the refused calls are gone: the good rows go through, and only once
    T0 = np.frombuffer(before[0], np.int32).reshape(65, tc.H, 3)
    evict_host(e, good)
    assert state(e) == ec.bytes_of(*ec.ref_evicted_tl(T0, c.victims, 2, good, c.nodes.part_mask))


def test_state_errors():
    c = tc.hand_case()
    L = _lib.lib()
    ms = C.c_double()
    z = np.zeros(1, np.int32)
    p = C.c_void_p(z.ctypes.data)
    off = np.zeros(c.nodes.n + 1, np.int32)
    po = C.c_void_p(off.ctypes.data)

    def refused(e):
        assert code(lambda: e.evicted_tl(z, z)) == _lib.FIT_E_STATE
        assert code(lambda: e.read_victims_tl()) == _lib.FIT_E_STATE
        assert L.fit_evicted_tl(e._h, 0, None, None) == _lib.FIT_E_STATE
        assert L.fit_evicted_tl_device(e._h, 1, p, p) == _lib.FIT_E_STATE
        assert L.fit_read_victims_tl(e._h, po, 0, None, None, None, None, None) == _lib.FIT_E_STATE

    with Engine(device=0) as e:
        refused(e)                                                  # before load_nodes
        e.load_nodes(c.nodes)
        e.load_partitions(c.parts)
        refused(e)                                                  # without a timeline
        e.load_timeline(c.tline)
        refused(e)                                                  # before load_victims_tl
        assert b"fit_load_victims_tl" in L.fit_last_error()
        e.load_victims_tl(c.victims)
        before = state(e)
        assert L.fit_evicted_tl_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE  # no call with rows yet
        assert L.fit_evicted_tl_device(e._h, 0, None, None) == 0
        assert L.fit_evicted_tl_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE
        assert state(e) == before
        evict_device(e, [(0, 0)])
        assert L.fit_evicted_tl_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        assert e.read_victims_tl().off.tolist() == [0, 1, 2, 4, 4, 4, 5]
        e.load_timeline(c.tline)                                    # drops the lists
        refused(e)
        e.load_victims_tl(c.victims)
        assert state(e) == before                                   # a new load has every entry again
        e.load_nodes(c.nodes)                                       # drops the timeline and the lists
        refused(e)
        e.load_timeline(c.tline)
        refused(e)
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        refused(e)

"""fit_hold_tl on the GPU against a numpy restatement of DESIGN.md §2j (_hold_tl_cases.ref_hold_tl,
over the dense [n, H, 3] timeline), bit for bit: replays of fit_place_tl_k / fit_place_tl after a
reload and what the engines place afterwards, a refreshed cluster on which some records no longer
fit, the hand-built rule case, many windows on one node, long run lists and window edges, the
headers after a hold, hold -> advance -> unplace, freedom of order, conflicts far apart in one call,
errors that leave the timeline and out_state alone, and the device entry point."""
import ctypes as C
import functools

import numpy as np
import pytest

import fitgpu
import _advance_tl_cases as ac
import _hold_tl_cases as hc
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from _devarray import DevArray
from fitgpu import Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu
INT32_MAX = hc.INT32_MAX


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


def fresh_random(e, H):
    """rand_cluster(H) loaded and the warm-up queue placed: the timeline the shared references start
    from (pk.start_timeline), its run lists already carrying dips."""
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    assert np.array_equal(e.read_timeline(), pk.start_timeline(H))


def same_table(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def hold_and_check(e, tl0, jobs, node, start, slot_min, kmax):
    """One hold_tl against the restatement, bit for bit; returns the restatement's answer."""
    want, wstate, wapplied, wrefused = hc.ref_hold_tl(tl0, jobs, node, start, slot_min, kmax)
    state, applied, refused = e.hold_tl(jobs, node, start, kmax)
    assert np.array_equal(state, wstate), np.flatnonzero(state != wstate)[:8]
    assert (applied, refused) == (wapplied, wrefused)
    got = e.read_timeline()
    assert got.tobytes() == want.tobytes(), np.argwhere((got != want).any(axis=(1, 2)))[:5]
    return want, wstate, wapplied, wrefused


@functools.lru_cache(maxsize=None)
def suffix(H, kmax, one):
    """What the restatement of §2g places after the replay: uc.second_jobs on the final timeline of
    uc.reference(H, kmax) (one: every job one node, fit_place_tl's queue)."""
    nodes, _, parts = pk.cluster(H)
    second = pk.ones(uc.second_jobs(H, kmax)) if one else uc.second_jobs(H, kmax)
    return (second,) + pk.ref_place_tl_k(uc.reference(H, kmax)[3], nodes.part_mask, parts, second, pk.SLOT_MIN,
                                         1 if one else kmax)


# ---- 1. replay -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_replay(engine, H, kmax):
    e = engine
    jobs, wnodes, wstart, wfin = uc.reference(H, kmax)
    fresh_random(e, H)
    table = e.read_nodes()
    nodes, start, _ = e.place_tl_k(jobs, kmax)
    fin = e.read_timeline()
    assert np.array_equal(nodes, wnodes) and np.array_equal(start, wstart) and np.array_equal(fin, wfin)
    for consumer in ("place_tl_k", "place_tl"):
        fresh_random(e, H)  # the reload: the plan is gone
        state, applied, refused = e.hold_tl(jobs, nodes, start, kmax)  # verbatim: unplaced and rejected rows included
        assert np.array_equal(state, np.where(start >= 0, hc.HELD, hc.SKIPPED))
        assert applied == np.maximum(jobs.nodes_k[start >= 0], 1).sum() and refused == 0
        assert e.read_timeline().tobytes() == fin.tobytes(), "the timeline after the placement is not restored"
        assert same_table(table, e.read_nodes()), "the node table changed"
        assert e.hold_tl_ms() > 0
        # the headers: a stale cnt or head[] changes what the queue's suffix gets now
        if consumer == "place_tl_k":
            second, rn, rs, rfin = suffix(H, kmax, False)
            gn, gs, st = e.place_tl_k(second, kmax)
            assert np.array_equal(gn, rn) and np.array_equal(gs, rs)
        else:
            second, rn, rs, rfin = suffix(H, kmax, True)
            gn, gs, st = e.place_tl(second)
            assert np.array_equal(gs, rs) and np.array_equal(gn[gs >= 0], rn[gs >= 0, 0])
        assert st["placed"] >= 20
        assert np.array_equal(e.read_timeline(), rfin)
    if kmax == 1:  # the persistent engine's records go back the same way
        fresh_random(e, H)
        n1, s1, _ = e.place_tl(jobs)
        assert np.array_equal(s1, wstart) and np.array_equal(n1[s1 >= 0], wnodes[s1 >= 0, 0])
        fresh_random(e, H)
        state, applied, refused = e.hold_tl(jobs, n1, s1)
        assert np.array_equal(state, np.where(s1 >= 0, hc.HELD, hc.SKIPPED)) and refused == 0
        assert applied == (s1 >= 0).sum() and e.read_timeline().tobytes() == fin.tobytes()


# ---- 2. the refreshed cluster --------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", hc.REFRESH)
def test_refresh(engine, H, kmax):
    e = engine
    jobs, out, start, _ = uc.reference(H, kmax)
    tl0, wfin, wstate, wapplied, wrefused = hc.refresh_reference(H, kmax)
    load(e, *hc.refresh_cluster(H, kmax))
    assert np.array_equal(e.read_timeline(), tl0)
    state, applied, refused = e.hold_tl(jobs, out, start, kmax)
    assert np.array_equal(state, wstate) and (applied, refused) == (wapplied, wrefused)
    assert e.read_timeline().tobytes() == wfin.tobytes()
    # the inverse: unplacing exactly the held rows restores the timeline the hold found
    held = np.flatnonzero(state == hc.HELD)
    assert e.unplace_tl(uc.take(jobs, held), out[held], start[held], kmax) == applied
    assert e.read_timeline().tobytes() == tl0.tobytes()
    # and hold of the rows just unplaced restores the timeline before the unplace
    state2, applied2, refused2 = e.hold_tl(uc.take(jobs, held), out[held], start[held], kmax)
    assert (state2 == hc.HELD).all() and (applied2, refused2) == (applied, 0)
    assert e.read_timeline().tobytes() == wfin.tobytes()


def test_order_and_split(engine):
    e = engine
    H, kmax = hc.REFRESH[0]
    jobs, out, start, _ = uc.reference(H, kmax)
    tl0, wfin, wstate, wapplied, wrefused = hc.refresh_reference(H, kmax)
    perm, pj, pn, ps = hc.shuffled(jobs, out, start, 5 * H + kmax)
    load(e, *hc.refresh_cluster(H, kmax))
    state, applied, refused = e.hold_tl(pj, pn, ps, kmax)
    assert np.array_equal(state, wstate[perm]) and (applied, refused) == (wapplied, wrefused)
    assert e.read_timeline().tobytes() == wfin.tobytes()
    # two calls give what one gives when neither refuses a row
    held = np.random.default_rng(H).permutation(np.flatnonzero(wstate == hc.HELD))
    a, b = held[:len(held) // 3], held[len(held) // 3:]
    load(e, *hc.refresh_cluster(H, kmax))
    s1, n1, r1 = e.hold_tl(uc.take(jobs, a), out[a], start[a], kmax)
    mid = e.read_timeline()
    s2, n2, r2 = e.hold_tl(uc.take(jobs, b), out[b], start[b], kmax)
    assert (s1 == hc.HELD).all() and (s2 == hc.HELD).all() and r1 == r2 == 0 and n1 + n2 == wapplied
    assert mid.tobytes() != tl0.tobytes() and e.read_timeline().tobytes() == wfin.tobytes()


# ---- 3. the rule case ------------------------------------------------------------------------------------
def test_rule_case(engine):
    e = engine
    load(e, *hc.rule_cluster())
    tl0 = e.read_timeline()
    assert np.array_equal(tl0, hc.rule_dense())
    jobs, node, start = hc.rule_rows()
    _, state, applied, refused = hold_and_check(e, tl0, jobs, node, start, hc.RULE_SLOT_MIN, hc.RULE_KMAX)
    assert state.tolist() == hc.RULE_STATE.tolist() and (applied, refused) == (7, 10)
    perm, pj, pn, ps = hc.shuffled(jobs, node, start, 3)
    load(e, *hc.rule_cluster())
    hold_and_check(e, tl0, pj, pn, ps, hc.RULE_SLOT_MIN, hc.RULE_KMAX)


# ---- 4. many windows on one node in one call ------------------------------------------------------------
@pytest.mark.parametrize("cpu7,all_held", [(4000, True), (800, False)])
def test_many_windows_on_one_node(engine, cpu7, all_held):
    """uc.crowd(): 312 windows on node 7.  At 4,000 cpus everything is held; at 800 cpus node 7 is over
    on its crowded slots and every window that covers one is refused — the 3-node rows with it."""
    e = engine
    H, n = 64, 40
    nodes = uc.flat_cluster(n, cpu=4000, mem=2000000, gpu=1000)
    nodes.cpu_free[7] = cpu7
    load(e, nodes, uc.no_events(n, H, 1), wk.open_parts(1))
    tl0 = e.read_timeline()
    jobs, node, start = uc.crowd(H, n)
    want, state, applied, refused = hold_and_check(e, tl0, jobs, node, start, 1, 3)
    if all_held:
        assert refused == 0 and applied == 300 + 30 + 36 and wk.run_counts(want)[7] > 32
    else:
        on7 = (node[:, 0] == 7) | ((jobs.nodes_k == 3) & (node == 7).any(axis=1))
        assert refused >= 20 and (state[~on7] == hc.HELD).all() and (state[on7] == hc.HELD).sum() >= 20
        assert ((state == hc.REFUSED) & (jobs.nodes_k == 3)).any()


# ---- 5. long lists and edges -----------------------------------------------------------------------------
def test_long_lists_and_edges(engine):
    """pk.stairs(): 128 runs per node (beyond one wave's lanes and beyond TL_HEAD), slot_min 1, H 256;
    node x holds (s - x % 2) // 2 cpus at slot s."""
    e = engine
    nodes, tline, parts = pk.stairs()
    H = tline.slots
    load(e, nodes, tline, parts)
    tl0 = e.read_timeline()
    assert (wk.run_counts(tl0) == 128).all()
    rows = [(1, 0, 1, 0, 7),        # a window from slot 0 (no cpu there: a zero cpu demand)
            (1, 2, 1, 0, 7),
            (0, 100, 1, 1, 1),      # the first slot of run 50
            (0, 201, 1, 5, 0),      # the last slot of run 100, beyond one wave's lanes
            (2, 250, 6, 1, 1),      # a window to H
            (3, 250, 100, 2, 2),    # start + d > H: clipped
            (4, 0, 256, 0, 9),      # the whole horizon
            (0, 0, 1000, 0, 1),     # the whole horizon, clipped
            (1, 130, 70, 4, 4),     # from inside run 64 to inside run 99: two splits
            (2, 0, 10, 3, 0),       # refused: slots 0..7 hold fewer than 3 cpus
            (3, 64, 64, 31, 0)]     # held exactly at its first slot: (64 - 1) // 2 = 31
    a = np.array(rows, np.int64)    # (node, start, wall, cpu, mem)
    jobs = synth.Jobs(a[:, 3].astype(np.int32), a[:, 4].astype(np.int32), np.zeros(len(a), np.int32),
                      a[:, 2].astype(np.int32), np.zeros(len(a), np.uint16), np.ones(len(a), np.uint16))
    node, start = a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)
    want, state, applied, refused = hold_and_check(e, tl0, jobs, node, start, 1, 1)
    assert state.tolist() == [1] * 9 + [0, 1] and want[3, 64, 0] == 0
    assert (wk.run_counts(want) >= 128).all() and wk.run_counts(want)[1] > 128
    # the lists are canonical and the headers current: the engines go on from them exactly
    queue = pk.stair_jobs(40, 17)
    rn, rs, rfin = pk.ref_place_tl_k(want, nodes.part_mask, parts, queue, 1, 4)
    gn, gs, st = e.place_tl_k(queue, 4)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and st["placed"] >= 10
    assert np.array_equal(e.read_timeline(), rfin)


# ---- 6. the headers after a hold ---------------------------------------------------------------------------
def test_consumers_answer_as_on_a_timeline_loaded_dense_equal():
    """Records that start at slot 0 are running jobs: holding them on the idle cluster gives the dense
    timeline that the cluster loads to with those jobs running (their demand off the node table, a
    release event at their end).  One context gets there by fit_hold_tl, the other by the load; every
    consumer of the headers — ceilings, cnt, head[] — must answer the same on both."""
    n, H, L, kmax = 24, 32, 5, 4
    r = np.random.default_rng(16)
    idle = uc.flat_cluster(n, cpu=64, mem=65536, gpu=8)
    parts = wk.open_parts(1)
    running = []
    for i in range(n + 30):  # one job on every node, so that none is idle, then 30 of 1 to 4 nodes
        rows = [i] if i < n else sorted(r.choice(n, int(r.integers(1, kmax + 1)), replace=False).tolist())
        rem = [1, L, L + 1, H * L, H * L + 70][i] if i < 5 else int(r.integers(1, H * L))
        running.append((rows, rem, int(r.integers(1, 9)), int(r.integers(0, 2048)), int(r.integers(0, 2))))
    busy = synth.Nodes(*(getattr(idle, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min",
                                                            "part_mask")))
    node = np.full((len(running), kmax), -1, np.int32)
    for i, (rows, rem, c, m, g) in enumerate(running):
        node[i, :len(rows)] = rows
        busy.cpu_free[rows] -= c
        busy.mem_free[rows] -= m
        busy.gpu_free[rows] -= g
    assert (busy.cpu_free >= 0).all() and (busy.gpu_free >= 0).all()
    recs = wk.jobs_of([(c, m, g, rem, 0, len(rows)) for rows, rem, c, m, g in running])
    j = 120
    queue = synth.Jobs(r.choice([1, 8, 30, 50, 60, 64], j).astype(np.int32), r.integers(0, 40000, j).astype(np.int32),
                       r.choice([0, 1, 7, 8], j).astype(np.int32), r.integers(1, H * L // 2, j).astype(np.int32),
                       np.zeros(j, np.uint16), r.integers(1, kmax + 1, j).astype(np.uint16))
    with Engine(device=0) as a, Engine(device=0) as b:
        def setup():
            load(a, idle, uc.no_events(n, H, L), parts)
            state, applied, refused = a.hold_tl(recs, node, np.zeros(len(running), np.int32), kmax)
            assert (state == hc.HELD).all() and refused == 0
            load(b, busy, fitgpu.release_events(n, running, H, L), parts)
            assert a.read_timeline().tobytes() == b.read_timeline().tobytes()

        setup()
        wa, wb = a.when(pk.ones(queue)), b.when(pk.ones(queue))
        assert wa.tobytes() == wb.tobytes() and len(set(wa["start"].tolist())) >= 4
        (ka, na), (kb, nb) = a.when_k(queue, kmax), b.when_k(queue, kmax)
        assert ka.tobytes() == kb.tobytes() and np.array_equal(na, nb)
        (gna, gsa, sa), (gnb, gsb, sb) = a.place_tl_k(queue, kmax), b.place_tl_k(queue, kmax)
        assert np.array_equal(gna, gnb) and np.array_equal(gsa, gsb) and sa["placed"] == sb["placed"] >= 20
        assert a.read_timeline().tobytes() == b.read_timeline().tobytes()
        setup()
        (gna, gsa, sa), (gnb, gsb, sb) = a.place_tl(pk.ones(queue)), b.place_tl(pk.ones(queue))
        assert np.array_equal(gna, gnb) and np.array_equal(gsa, gsb) and sa["placed"] == sb["placed"] >= 20
        assert a.read_timeline().tobytes() == b.read_timeline().tobytes()


def test_hold_advance_unplace(engine):
    """The plan put back, the clock moved, the rewritten records handed back: the advanced empty plan."""
    e = engine
    H, kmax = 64, 8
    jobs, out, start, fin = uc.reference(H, kmax)
    tail = ac.level_tail(H)
    for a in (1, 7, 16):  # 137, 97 and 33 of the 152 records outlive the advance
        fresh_random(e, H)
        state, applied, refused = e.hold_tl(jobs, out, start, kmax)
        assert refused == 0 and e.read_timeline().tobytes() == fin.tobytes()
        e.advance_tl(a, tail)
        j2, s2 = ac.rewrite_rows(jobs, start, a, H, pk.SLOT_MIN)
        assert (s2 >= 0).sum() >= 20
        e.unplace_tl(j2, out, s2, kmax)
        assert e.read_timeline().tobytes() == ac.ref_advance_tl(pk.start_timeline(H), a, tail).tobytes(), a


# ---- 7. conflicts far apart in one call ------------------------------------------------------------------
def test_seam(engine):
    """16,390 rows; rows 3 and 16,388 conflict on one node, 16,385 rows apart, and rows 100 and 9,000
    on another inside one block of 16,384: the judging is per call."""
    e = engine
    n, H = 64, 64
    jobs, node, start, pairs = hc.seam_rows(n, 16390, H)
    load(e, uc.flat_cluster(n, cpu=hc.SEAM_CPU), uc.no_events(n, H, 1), wk.open_parts(1))
    tl0 = e.read_timeline()
    _, state, applied, refused = hold_and_check(e, tl0, jobs, node, start, 1, 1)
    assert refused == 4 and (state[pairs] == hc.REFUSED).all() and applied == 16386


# ---- 8. errors leave the timeline and out_state unchanged ---------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_errors_and_state():
    n, H, L, kmax = 6, 16, 5, 3
    nodes, tline, parts = uc.flat_cluster(n), uc.no_events(n, H, L), wk.open_parts(1)
    good = wk.jobs_of([(1, 10, 0, 10, 0, 1), (2, 20, 1, 20, 0, 2), (1, 1, 1, 500, 0, 3), (3, 3, 0, 5, 0, 0),
                       (1, 10, 0, 10, 0, 1)])
    gnode = np.array([[0, 999, -5], [1, 2, 999], [3, 4, 5], [5, -1, -1], [-5, 77, 77]], np.int32)  # i >= need: ignored
    gstart = np.array([0, 3, 15, 7, -1], np.int32)  # the last row is skipped whatever it holds
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    L_ = _lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    with Engine(device=0) as e:
        assert _code(lambda: e.hold_tl(good, gnode, gstart, kmax)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.hold_tl(good, gnode, gstart, kmax)) == STATE  # no timeline loaded
        ms = C.c_double()
        assert L_.fit_hold_tl_ms(e._h, C.byref(ms)) == STATE  # before the first call
        e.load_timeline(tline)
        assert L_.fit_hold_tl_ms(e._h, C.byref(ms)) == STATE
        before = e.read_timeline()

        def with_bad(row, node_row, start):
            jobs = uc.concat(good, wk.jobs_of([row]))
            return jobs, np.vstack([gnode, np.array([node_row], np.int32)]), np.append(gstart, np.int32(start))

        bad = {
            "node id = n": ((1, 1, 1, 5, 0, 1), [n, -1, -1], 0),
            "node id -5 in a live row": ((1, 1, 1, 5, 0, 2), [0, -5, -1], 0),
            "start = H": ((1, 1, 1, 5, 0, 1), [0, -1, -1], H),
            "a duplicate node": ((1, 1, 1, 5, 0, 3), [2, 4, 2], 0),
            "negative cpu": ((-1, 1, 1, 5, 0, 1), [0, -1, -1], 0),
            "negative mem": ((1, -1, 1, 5, 0, 1), [0, -1, -1], 0),
            "negative gpu": ((1, 1, -1, 5, 0, 1), [0, -1, -1], 0),
            "need > kmax": ((1, 1, 1, 5, 0, 4), [0, 1, 2], 0),
        }
        for what, (row, node_row, start) in bad.items():
            jobs, node, st = with_bad(row, node_row, start)
            cols = [np.ascontiguousarray(a) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.nodes_k, node, st)]
            state = np.full(6, 77, np.int32)
            applied, refused = C.c_int64(-5), C.c_int64(-6)
            assert L_.fit_hold_tl(e._h, 6, *[p(c) for c in cols[:5]], kmax, p(cols[5]), p(cols[6]), p(state),
                                  C.byref(applied), C.byref(refused)) == INVAL, what
            assert (state == 77).all() and (applied.value, refused.value) == (-5, -6), what
            assert e.read_timeline().tobytes() == before.tobytes(), what
            dev = [DevArray(c) for c in cols]
            dstate = DevArray(state)
            assert _code(lambda: e.hold_tl_device(*dev, dstate, kmax)) == INVAL, what
            assert (dstate.numpy() == 77).all(), what
            assert e.read_timeline().tobytes() == before.tobytes(), what
        for k in (0, -1, 9):
            assert _code(lambda: e.hold_tl(good, gnode, gstart, k)) == INVAL, k
        cols = [np.ascontiguousarray(a) for a in (good.cpu, good.mem, good.gpu, good.wall)]
        state = np.full(5, 77, np.int32)
        applied, refused = C.c_int64(-1), C.c_int64(-1)
        for fn in (L_.fit_hold_tl, L_.fit_hold_tl_device):
            none = (None,) * 5
            assert fn(e._h, 0, *none, 1, None, None, None, None, None) == 0  # j == 0 whatever the pointers
            assert fn(e._h, 0, *none, 1, None, None, None, C.byref(applied), C.byref(refused)) == 0
            assert (applied.value, refused.value) == (0, 0)
            assert fn(e._h, -1, *none, 1, None, None, None, None, None) == INVAL
            assert fn(e._h, 5, *none, 1, None, None, None, None, None) == INVAL
        args = [p(c) for c in cols] + [None, kmax]
        assert L_.fit_hold_tl(e._h, 5, *args, None, p(gstart), p(state), None, None) == INVAL  # NULL nodes
        assert L_.fit_hold_tl(e._h, 5, *args, p(gnode), None, p(state), None, None) == INVAL  # NULL starts
        assert L_.fit_hold_tl(e._h, 5, *args, p(gnode), p(gstart), None, None, None) == INVAL  # NULL out_state
        assert e.read_timeline().tobytes() == before.tobytes() and (state == 77).all()
        assert L_.fit_hold_tl_ms(e._h, C.byref(ms)) == STATE  # no call has succeeded yet
        # the good batch alone is exact, the counts NULL and nodes_k NULL (= all 1) included
        want, wstate, wapplied, _ = hold_and_check(e, before, good, gnode, gstart, L, kmax)
        assert wapplied == 7 and wstate.tolist() == [1, 1, 1, 1, -1]
        assert L_.fit_hold_tl_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        all1 = pk.ones(good)
        want1, wstate1, _, _ = hc.ref_hold_tl(want, all1, gnode, gstart, L, kmax)
        assert L_.fit_hold_tl(e._h, 5, *args, p(gnode), p(gstart), p(state), None, None) == 0
        assert np.array_equal(e.read_timeline(), want1) and np.array_equal(state, wstate1)
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.hold_tl(good, gnode, gstart, kmax)) == STATE
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        load(e, nodes, tline, parts)
        assert _code(lambda: e.hold_tl(good, gnode, gstart, kmax)) == STATE


# ---- 9. the device entry point ----------------------------------------------------------------------------
def test_device_entry(engine):
    e = engine
    H, kmax = hc.REFRESH[0]
    jobs, out, start, _ = uc.reference(H, kmax)
    tl0, wfin, wstate, wapplied, wrefused = hc.refresh_reference(H, kmax)
    load(e, *hc.refresh_cluster(H, kmax))
    dev = [DevArray(np.ascontiguousarray(a)) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.nodes_k, out, start)]
    dstate = DevArray(np.full(len(start), 77, np.int32))
    assert e.hold_tl_device(*dev, dstate, kmax) == (wapplied, wrefused)
    assert np.array_equal(dstate.numpy(), wstate)
    assert e.read_timeline().tobytes() == wfin.tobytes()
    assert e.hold_tl_ms() > 0
    # nodes_k NULL on device columns: every row one node
    load(e, *hc.refresh_cluster(H, kmax))
    want, wstate1, wapplied1, wrefused1 = hc.ref_hold_tl(tl0, pk.ones(jobs), out, start, pk.SLOT_MIN, kmax)
    dev[4] = None
    assert e.hold_tl_device(*dev, dstate, kmax) == (wapplied1, wrefused1)
    assert np.array_equal(dstate.numpy(), wstate1) and np.array_equal(e.read_timeline(), want)

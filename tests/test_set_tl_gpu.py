"""fit_set_tl on the GPU against a numpy restatement of DESIGN.md §2q (_set_tl_cases.ref_set_tl, over
the dense [n, H, 3] timeline), bit for bit: random rows and what the engines place afterwards, the
largest-index rule under every order the grouping may leave, long run lists and window edges, the slab
row filled to the horizon limit, every consumer of the headers on two contexts, the composition with
advance / unplace / hold / the victims' lists, overlaps across the chunk seam, errors that leave the
timeline alone, and the device entry point."""
import ctypes as C

import numpy as np
import pytest

import fitgpu
import _advance_tl_cases as ac
import _evicted_tl_cases as ec
import _hold_tl_cases as hc
import _place_tl_k_cases as pk
import _preempt_tl_cases as tc
import _set_tl_cases as sc
import _unplace_tl_cases as uc
import _when_k_cases as wk
from _devarray import DevArray
from fitgpu import Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu
INT32_MAX = sc.INT32_MAX


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


def same_table(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def set_and_check(e, tl0, c, mask=None):
    """One set_tl against the restatement, bit for bit; returns the restatement's timeline."""
    want, wapplied, wignored = sc.ref_set_tl(tl0, *c, mask)
    assert e.set_tl(*c) == (wapplied, wignored)
    got = e.read_timeline()
    assert got.tobytes() == want.tobytes(), np.argwhere((got != want).any(axis=(1, 2)))[:5]
    return want


# ---- 1. random rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", sc.RANDOM_H)
def test_random_rows(engine, H):
    e = engine
    nodes, tline, parts = sc.cluster(H)
    load(e, nodes, tline, parts)
    if H >= 64:
        e.place_tl(pk.pre_jobs(H))
    tl0 = e.read_timeline()
    assert np.array_equal(tl0, sc.start_timeline(H))
    table = e.read_nodes()
    want, wapplied, wignored, (queue, kmax, rn, rs, rfin) = sc.random_reference(H)
    assert e.set_tl(*sc.random_rows(H)) == (wapplied, wignored)
    got = e.read_timeline()
    assert got.tobytes() == want.tobytes(), np.argwhere((got != want).any(axis=(1, 2)))[:5]
    assert same_table(table, e.read_nodes()), "the node table changed"
    assert e.set_tl_ms() > 0
    # the lists are canonical and the headers current: the engine goes on from them exactly
    gn, gs, st = e.place_tl_k(queue, kmax)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and st["placed"] >= 5
    assert np.array_equal(e.read_timeline(), rfin)


# ---- 2. the largest-index rule ---------------------------------------------------------------------------
def test_largest_index_rule(engine, monkeypatch):
    e = engine
    n, H = 40, 64
    nodes, tline, parts = uc.flat_cluster(n, cpu=64, mem=65536, gpu=8), uc.no_events(n, H, 1), wk.open_parts(1)
    on7, others = sc.crowd(n, H)
    seen = set()
    for seed in (1, 2, 3):  # three orders of the other nodes' rows between node 7's
        c = sc.interleaved(on7, others, seed)
        load(e, nodes, tline, parts)
        tl0 = e.read_timeline()
        want = set_and_check(e, tl0, c)
        seen.add(want.tobytes())
        assert wk.run_counts(want)[7] >= 16
    assert len(seen) == 1
    # node 7's rows the other way round give another timeline: the order is what decides
    load(e, nodes, tline, parts)
    assert set_and_check(e, tl0, sc.cols(on7[::-1] + others)).tobytes() not in seen
    for chunk in ("7", "1"):  # the launch seam between any two rows
        monkeypatch.setenv("FIT_UTL_CHUNK", chunk)
        load(e, nodes, tline, parts)
        assert e.set_tl(*c) == (330, 0)
        assert e.read_timeline().tobytes() in seen, chunk
    monkeypatch.delenv("FIT_UTL_CHUNK")


# ---- 3. long lists and edges -----------------------------------------------------------------------------
def test_long_lists_and_edges(engine):
    """pk.stairs(): 128 runs per node (beyond one wave's lanes and beyond TL_HEAD), slot_min 1, H 256;
    node x holds (s - x % 2) // 2 cpus at slot s, so run r of node 0 is the slots 2r, 2r + 1."""
    e = engine
    nodes, tline, parts = pk.stairs()
    H = tline.slots
    load(e, nodes, tline, parts)
    tl0 = e.read_timeline()
    assert (wk.run_counts(tl0) == 128).all()
    M = 1 << 20
    rows = [(0, 101, 129, 7, M, 0),         # from inside run 50 to inside run 64: both split
            (0, 129, 201, -1, M, 0),        # from inside run 64 to inside run 100, one column closed
            (0, 201, 202, 3, 3, 3),         # the last slot of run 100
            (1, 101, 103, 9, 9, 9),         # a window equal to one run of node 1 (runs start at odd slots)
            (2, 6, 8, 2, M, 0),             # run 3 takes run 2's level: two runs join into one
            (3, 0, H, 5, 5, 5),             # the whole horizon: 128 runs become one
            (4, 250, H + 100, 1, 1, 1),     # `to` clipped
            (4, 0, 1, 0, M, 0),             # a row that changes nothing
            (1, 255, INT32_MAX, -1, -1, -1)]
    want = set_and_check(e, tl0, sc.cols(rows))
    rc = wk.run_counts(want)
    assert rc.tolist() == [128 - 50 + 3, 128, 127, 1, 128 - 3 + 1] and (want[1, 101:103] == 9).all()
    # the lists are canonical and the headers current: the engines go on from them exactly
    queue = pk.stair_jobs(40, 17)
    rn, rs, rfin = pk.ref_place_tl_k(want, nodes.part_mask, parts, queue, 1, 4)
    gn, gs, st = e.place_tl_k(queue, 4)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and st["placed"] >= 10
    assert np.array_equal(e.read_timeline(), rfin)


# ---- 4. the slab row full ----------------------------------------------------------------------------------
def test_slab_row_full(engine):
    e = engine
    n, H = 8, 1024
    nodes, tline, parts = uc.flat_cluster(n, cpu=16, mem=1 << 16, gpu=2), uc.no_events(n, H, 1), wk.open_parts(1)
    load(e, nodes, tline, parts)
    tl0 = e.read_timeline()
    r = np.random.default_rng(4)
    full = [(0, s, s + 1, 10 + s % 2, 100, s % 2) for s in r.permutation(H).tolist()]
    half = [(1, s, s + 2, 20 + (s // 2) % 2, 200, 1) for s in r.permutation(np.arange(0, H, 2)).tolist()]
    want = set_and_check(e, tl0, sc.cols(full + half))
    assert wk.run_counts(want).tolist() == [H, H // 2] + [1] * (n - 2)
    back = set_and_check(e, want, sc.cols([(0, 0, H, 10, 100, 0)]))
    assert wk.run_counts(back)[0] == 1
    # every consumer of cnt and head[] sees the 1,024 runs gone: a job of 11 cpus fits nowhere on node 0
    jobs = wk.jobs_of([(11, 100, 0, 5, 0, 1), (10, 100, 0, H, 0, 1), (21, 200, 1, 2, 0, 1)])
    rows, picks = e.when_k(jobs, 1)
    wrows, wpicks = wk.ref_when_k(back, nodes.part_mask, parts, jobs, 1, 1)
    assert rows.tobytes() == wrows.tobytes() and np.array_equal(picks, wpicks)


# ---- 5. two contexts, every header consumer ------------------------------------------------------------------
def test_consumers_answer_as_on_a_timeline_loaded_dense_equal():
    """Cluster Y is cluster X after six nodes changed outside the plan (sc.two_clusters).  Context A
    loads X and gets fit_set_tl of the run-length rows of Y's dense timeline for those nodes; context B
    loads Y.  Every consumer of the headers — ceilings, cnt, head[] — must answer the same on both."""
    n, H, L, kmax = 24, 32, 5, 4
    (x, tx), (y, ty), differ = sc.two_clusters(n, H, L)
    parts = wk.open_parts(2)
    r = np.random.default_rng(21)
    j = 120
    queue = synth.Jobs(r.choice([1, 5, 9, 14, 24, 40, 100, 150], j).astype(np.int32), r.integers(0, 40000, j).astype(np.int32),
                       r.choice([0, 1, 3, 4, 9], j).astype(np.int32), r.integers(1, H * L // 2, j).astype(np.int32),
                       np.zeros(j, np.uint16), r.integers(1, kmax + 1, j).astype(np.uint16))
    queue.part[:] = np.where(queue.cpu >= 100, 1, r.choice([0, 0, 0, 1], j))  # partition 1: nodes 5 and 6
    lists = [sorted((int(r.integers(1, 9)), int(r.integers(0, H + 1)), int(r.integers(3, 17)), int(r.integers(0, 4096)),
                     int(r.integers(0, 2))) for _ in range(int(r.integers(0, 4)))) for _ in range(n)]  # by priority
    victims = tc.victims_tl_of(lists)
    prio = r.integers(0, 12, j).astype(np.int32)
    with Engine(device=0) as a, Engine(device=0) as b:
        def setup():
            load(a, x, tx, parts)
            load(b, y, ty, parts)
            target = b.read_timeline()
            changed = np.flatnonzero((a.read_timeline() != target).any(axis=(1, 2))).tolist()
            assert changed == differ
            rows = sc.runs_as_rows(target, differ)
            assert a.set_tl(*sc.cols(rows)) == (len(rows), 0) and len(rows) >= 12
            assert a.read_timeline().tobytes() == target.tobytes()
            assert same_table(a.read_nodes(), (x.cpu_free, x.mem_free, x.gpu_free)), "the node table changed"
            return target

        target = setup()
        wa, wb = a.when(pk.ones(queue)), b.when(pk.ones(queue))
        assert wa.tobytes() == wb.tobytes() and len(set(wa["start"].tolist())) >= 4
        raised = (queue.cpu >= 100)  # only node 5, raised above every ceiling X was loaded with, holds these
        assert (wa["node"][raised] == 5).any() and (wa["node"][raised & (wa["start"] >= 0)] == 5).all()
        (ka, na), (kb, nb) = a.when_k(queue, kmax), b.when_k(queue, kmax)
        assert ka.tobytes() == kb.tobytes() and np.array_equal(na, nb)
        fa, fb = a.free_tl(2), b.free_tl(2)
        assert fa.tobytes() == fb.tobytes() and fa["max_cpu"].max() == 200 and len(set(fa["nodes"].ravel().tolist())) >= 3
        a.load_victims_tl(victims)
        b.load_victims_tl(victims)
        pa, pb = a.preempt_tl(pk.ones(queue), prio), b.preempt_tl(pk.ones(queue), prio)
        assert pa.tobytes() == pb.tobytes() and (pa["code"] == tc.EVICT).sum() >= 3
        closed0 = np.flatnonzero((target[:, 0] == -1).any(axis=1))
        assert len(closed0) >= 1 and not np.isin(pa["node"], closed0).any()  # §2n: no eviction opens a closed node
        (gna, gsa, sa), (gnb, gsb, sb) = a.place_tl_k(queue, kmax), b.place_tl_k(queue, kmax)
        assert np.array_equal(gna, gnb) and np.array_equal(gsa, gsb) and sa["placed"] == sb["placed"] >= 20
        assert ((gna == 5).any(axis=1) & raised).any(), "no job was placed on the node whose level was raised"
        assert a.read_timeline().tobytes() == b.read_timeline().tobytes()
        setup()
        (gna, gsa, sa), (gnb, gsb, sb) = a.place_tl(pk.ones(queue)), b.place_tl(pk.ones(queue))
        assert np.array_equal(gna, gnb) and np.array_equal(gsa, gsb) and sa["placed"] == sb["placed"] >= 20
        assert (gna[raised & (gsa >= 0)] == 5).any()
        assert a.read_timeline().tobytes() == b.read_timeline().tobytes()


# ---- 6. composition ------------------------------------------------------------------------------------------
def fresh_random(e, H):
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    assert np.array_equal(e.read_timeline(), pk.start_timeline(H))


def test_close_advance_reopen_advance(engine):
    e = engine
    H = 64
    fresh_random(e, H)
    tl = pk.start_timeline(H)
    tail = ac.random_tail(tl, 9)
    open_ = np.flatnonzero((tl[:, H - 1] >= 0).all(axis=1))[:6].tolist()
    tail[open_] = [[50, 4096, 2]] * len(open_)
    close = sc.cols([(x, 0, INT32_MAX, -1, -1, -1) for x in open_[:3]] + [(open_[3], 10, H, -1, 5, 5),
                                                                          (open_[4], 0, H - 1, -1, -1, -1)])
    tl = set_and_check(e, tl, close)
    e.advance_tl(7, tail)
    tl = ac.ref_advance_tl(tl, 7, tail)
    assert e.read_timeline().tobytes() == tl.tobytes()
    # a column closed through slot H - 1 stays closed whatever the tail says; one closed short of it does not
    assert (tl[open_[:3]] == -1).all() and (tl[open_[3], 3:, 0] == -1).all() and (tl[open_[3], H - 7:, 1] == 4096).all()
    assert (tl[open_[4], H - 7:, 0] == 50).all() and (tl[open_[4], :H - 8] == -1).all()
    reopen = sc.cols([(open_[0], 0, H, 8, 8192, 1), (open_[0], 20, H, 12, 8192, 1), (open_[1], H - 1, H, 1, 1, 1),
                      (open_[3], 0, INT32_MAX, 3, 5, 5)])
    tl = set_and_check(e, tl, reopen)
    e.advance_tl(5, tail)
    tl = ac.ref_advance_tl(tl, 5, tail)
    assert e.read_timeline().tobytes() == tl.tobytes()
    assert (tl[open_[0], H - 5:] == [50, 4096, 2]).all() and (tl[open_[1], H - 5:] == [50, 4096, 2]).all()
    assert (tl[open_[1], :H - 6] == -1).all() and (tl[open_[1], H - 6] == 1).all() and (tl[open_[2]] == -1).all()


def test_a_row_short_of_the_horizon_commutes_with_advance(engine):
    e = engine
    H, a = 64, 9
    tl0 = pk.start_timeline(H)
    tail = ac.level_tail(H)
    rows = [(5, 0, 5, -1, -1, -1), (6, 3, 9, 1, 1, 1), (7, 4, 30, 2, -1, 2), (8, 20, H - 1, -1, -1, -1),
            (9, 9, 10, 4, 4, 4), (7, 8, 12, 6, 6, 6), (10, 0, H - 1, 0, 0, 0)]
    moved = [(x, max(f - a, 0), t - a, c, m, g) for x, f, t, c, m, g in rows if t > a]
    assert len(moved) == len(rows) - 2
    fresh_random(e, H)
    e.set_tl(*sc.cols(rows))
    e.advance_tl(a, tail)
    one = e.read_timeline()
    fresh_random(e, H)
    e.advance_tl(a, tail)
    e.set_tl(*sc.cols(moved))
    two = e.read_timeline()
    assert one.tobytes() == two.tobytes()
    assert one.tobytes() == ac.ref_advance_tl(sc.ref_set_tl(tl0, *sc.cols(rows))[0], a, tail).tobytes()
    assert one.tobytes() != ac.ref_advance_tl(tl0, a, tail).tobytes()


def test_unplace_and_hold_over_a_closed_window(engine):
    e = engine
    H, kmax = 64, 8
    jobs, out, start, fin = uc.reference(H, kmax)
    fresh_random(e, H)
    e.place_tl_k(jobs, kmax)
    assert e.read_timeline().tobytes() == fin.tobytes()
    busy = np.argsort(-uc.windows_per_node(jobs, out, start, fin.shape[0]))[:4].tolist()  # nodes that carry records
    close = sc.cols([(x, 0, INT32_MAX, -1, -1, -1) for x in busy[:3]] + [(busy[3], 0, H, 5, -1, 5)])
    tl = set_and_check(e, fin, close)
    # handing every record back adds nothing to a closed slot (§2h: -1 stays -1)
    tl, wapplied = uc.ref_unplace_tl(tl, jobs, out, start, pk.SLOT_MIN, kmax)
    assert e.unplace_tl(jobs, out, start, kmax) == wapplied
    assert e.read_timeline().tobytes() == tl.tobytes() and (tl[busy[:3]] == -1).all() and (tl[busy[3], :, 1] == -1).all()
    # a hold over a closed slot refuses, one beside it holds
    want, wstate, wapp, wref = hc.ref_hold_tl(tl, jobs, out, start, pk.SLOT_MIN, kmax)
    state, app, ref = e.hold_tl(jobs, out, start, kmax)
    assert np.array_equal(state, wstate) and (app, ref) == (wapp, wref) and ref >= 3 and app >= 20
    on_closed = np.array([start[q] >= 0 and np.isin(out[q, :max(int(jobs.nodes_k[q]), 1)], busy).any()
                          for q in range(jobs.j)])
    assert (state[on_closed] == hc.REFUSED).all() and on_closed.sum() >= 3
    assert e.read_timeline().tobytes() == want.tobytes()
    # reopen first, then hand back: the base level, then the refused records are held again
    base = pk.start_timeline(H)
    tl = set_and_check(e, want, sc.cols(sc.runs_as_rows(base, busy)))
    again = np.where(on_closed, start, -1).astype(np.int32)
    want2, wstate2, wapp2, wref2 = hc.ref_hold_tl(tl, jobs, out, again, pk.SLOT_MIN, kmax)
    state2, app2, ref2 = e.hold_tl(jobs, out, again, kmax)
    assert np.array_equal(state2, wstate2) and (app2, ref2) == (wapp2, wref2) and ref2 == 0
    assert e.read_timeline().tobytes() == want2.tobytes() == fin.tobytes()


def test_the_victims_lists_and_their_shift_stay(engine):
    e = engine
    c = tc.packed_tl_case(65, 65)
    load(e, c.nodes, c.tline, c.parts)
    e.place_tl(c.queue)
    e.load_victims_tl(c.victims)
    e.advance_tl(3)
    T = e.read_timeline()
    lists = e.read_victims_tl()
    before = e.preempt_tl(c.jobs, c.prio)
    named = [int(x) for x in np.unique(before["node"][before["code"] == tc.EVICT])[:4]]
    assert len(named) >= 2
    rows = [(named[0], 0, INT32_MAX, -1, -1, -1), (named[1], 0, 1, 0, 0, 0)] + \
           [(int(x), 2, 9, 64, 1 << 18, 8) for x in range(10, 20)]
    T2 = set_and_check(e, T, sc.cols(rows), c.nodes.part_mask)
    assert ec.same_victims(e.read_victims_tl(), lists)
    after = e.preempt_tl(c.jobs, c.prio)
    want = tc.ref_preempt_tl(c.nodes.part_mask, T2, c.victims, c.parts, c.jobs, c.prio, c.tline.slot_min, 3)
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    assert not (after["node"] == named[0]).any()  # closed at slot 0: no eviction opens it


# ---- 7. the seam ---------------------------------------------------------------------------------------------
def test_seam(engine):
    """16,390 rows; rows 3 and 16,388 overlap on node 1 across the chunk boundary, rows 100 and 9,000 on
    node 2 inside one chunk: in both pairs the later row wins."""
    e = engine
    n, H = 64, 64
    c, pairs = sc.seam_rows(n, 16390, H)
    load(e, uc.flat_cluster(n, cpu=8), uc.no_events(n, H, 1), wk.open_parts(1))
    tl0 = e.read_timeline()
    want = set_and_check(e, tl0, c)
    assert want[1, 5:8, 0].tolist() == [11] * 3 and want[1, 8:12, 0].tolist() == [22] * 4 and want[1, 12, 0] == 11
    assert want[2, 2:40, 0].tolist() == [44] * 38 and (want[4:, :, 0] >= 100).all()


# ---- 8. errors leave the timeline unchanged ------------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_errors_and_state(monkeypatch):
    n, H, L = 6, 16, 5
    nodes, tline, parts = uc.flat_cluster(n, mask=[1, 1, 1, 0, 1, 1]), uc.no_events(n, H, L), wk.open_parts(1)
    good = [(0, 0, 4, 1, 1, 1), (1, 3, INT32_MAX, -1, 2, 2), (3, 0, H, 9, 9, 9), (2, 15, 16, 0, 0, 0),
            (-5, -1, -7, -9, -9, -9), (99, -2, 0, 0, 0, 0), (4, 2, 100, 3, 3, -1)]  # rows 4 and 5 are skipped
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    L_ = _lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    gc = sc.cols(good)
    with Engine(device=0) as e:
        assert _code(lambda: e.set_tl(*gc)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.set_tl(*gc)) == STATE  # no timeline loaded
        ms = C.c_double()
        assert L_.fit_set_tl_ms(e._h, C.byref(ms)) == STATE
        e.load_timeline(tline)
        assert L_.fit_set_tl_ms(e._h, C.byref(ms)) == STATE  # before the first call
        before = e.read_timeline()
        probe = wk.jobs_of([(1, 1, 1, 5, 0, 1), (4, 8192, 2, 30, 0, 1), (3, 3, 3, 80, 0, 1)])
        when0 = e.when(probe)
        bad = {
            "node id = n": (n, 0, 1, 0, 0, 0),
            "node id -1 in a live row": (-1, 0, 1, 0, 0, 0),
            "from = H": (0, H, H + 1, 0, 0, 0),
            "to = from": (0, 5, 5, 0, 0, 0),
            "to < from": (0, 5, 2, 0, 0, 0),
            "to = 0 at from = 0": (0, 0, 0, 0, 0, 0),
            "cpu -2": (0, 0, 1, -2, 0, 0),
            "mem -2": (0, 0, 1, 0, -2, 0),
            "gpu INT32_MIN": (0, 0, 1, 0, 0, -INT32_MAX - 1),
            "a bad row on a node in no partition": (3, 0, 1, -2, 0, 0),
        }
        for chunk in (None, "4"):  # "4": the bad row is the last row of a late chunk
            if chunk:
                monkeypatch.setenv("FIT_UTL_CHUNK", chunk)
            for what, row in bad.items():
                node, frm, to, lv = sc.cols(good + [row])
                cols = [node, frm, to] + [np.ascontiguousarray(lv[:, k]) for k in range(3)]
                applied, ignored = C.c_int64(-5), C.c_int64(-6)
                assert L_.fit_set_tl(e._h, 8, *[p(c) for c in cols], C.byref(applied), C.byref(ignored)) == INVAL, what
                assert (applied.value, ignored.value) == (-5, -6), what
                assert e.read_timeline().tobytes() == before.tobytes(), what
                dev = [DevArray(c) for c in cols]
                assert _code(lambda: e.set_tl_device(*dev)) == INVAL, what
                assert e.read_timeline().tobytes() == before.tobytes(), what
                assert e.when(probe).tobytes() == when0.tobytes(), what
        monkeypatch.delenv("FIT_UTL_CHUNK")
        applied, ignored = C.c_int64(-1), C.c_int64(-1)
        cols = [gc[0], gc[1], gc[2]] + [np.ascontiguousarray(gc[3][:, k]) for k in range(3)]
        for fn in (L_.fit_set_tl, L_.fit_set_tl_device):
            none = (None,) * 6
            assert fn(e._h, 0, *none, None, None) == 0  # m == 0 whatever the pointers
            assert fn(e._h, 0, *none, C.byref(applied), C.byref(ignored)) == 0
            assert (applied.value, ignored.value) == (0, 0)
            assert fn(e._h, -1, *none, None, None) == INVAL
            assert fn(e._h, 7, *none, None, None) == INVAL
        for k in range(6):  # one NULL column
            args = [p(c) for c in cols]
            args[k] = None
            assert L_.fit_set_tl(e._h, 7, *args, None, None) == INVAL, k
        assert e.read_timeline().tobytes() == before.tobytes()
        # skipped rows alone: a success that writes nothing and is no "call with a live row"
        assert e.set_tl(*sc.cols(good[4:6])) == (0, 0)
        assert L_.fit_set_tl_ms(e._h, C.byref(ms)) == STATE
        assert e.read_timeline().tobytes() == before.tobytes()
        # the good batch is exact, the counts NULL included; the node in no partition is counted and unchanged
        want, wapplied, wignored = sc.ref_set_tl(before, *gc, nodes.part_mask)
        assert (wapplied, wignored) == (4, 1) and e.set_tl(*gc) == (4, 1)
        assert e.read_timeline().tobytes() == want.tobytes() and (want[3] == -1).all()
        assert L_.fit_set_tl_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        assert L_.fit_set_tl(e._h, 7, *[p(c) for c in cols], None, None) == 0  # a call repeated gives what one gives
        assert e.read_timeline().tobytes() == want.tobytes()
        assert e.set_tl(*sc.cols([(3, 0, 1, 1, 1, 1)])) == (0, 1)  # ignored rows alone
        assert e.read_timeline().tobytes() == want.tobytes()
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.set_tl(*gc)) == STATE
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        load(e, nodes, tline, parts)
        assert _code(lambda: e.set_tl(*gc)) == STATE


# ---- 9. the device entry point -------------------------------------------------------------------------------
def test_device_entry(engine):
    e = engine
    H = 64
    nodes, tline, parts = sc.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    want, wapplied, wignored, _ = sc.random_reference(H)
    node, frm, to, lv = sc.random_rows(H)
    dev = [DevArray(np.ascontiguousarray(a)) for a in (node, frm, to, lv[:, 0], lv[:, 1], lv[:, 2])]
    assert e.set_tl_device(*dev) == (wapplied, wignored)
    assert e.read_timeline().tobytes() == want.tobytes()
    assert e.set_tl_ms() > 0

"""fit_when_k_win / fit_place_tl_k_win on the GPU against the numpy restatement of DESIGN.md §2r
(_win_tl_cases, over the dense [n, H, 3] timeline): the hand table and the minima trap, exact rows,
nodes, starts, counts and final timelines on windowed queues over components below, at and above a
wave, open windows against the unwindowed calls byte for byte, the block edges of the bounded start
scan, long run lists, the consequences of §2r, the launch seam, state and argument errors.  Every
case runs through the host and the device entry point, and both must agree."""
import ctypes as C

import numpy as np
import pytest

import _place_tl_k_cases as pk
import _when_k_cases as wk
import _win_tl_cases as wc
from _devarray import DevArray
from fitgpu import FIT_REJECTED, Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu
COLS = ("cpu", "mem", "gpu", "wall", "part")


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


def dev(a):
    return None if a is None else DevArray(np.ascontiguousarray(a, np.int32))


def when_both(e, jobs, kmax, nb, dl):
    """fit_when_k_win through host and device pointers: the same rows and nodes."""
    rows, nodes = e.when_k_win(jobs, nb, dl, kmax)
    cols = [DevArray(getattr(jobs, f)) for f in COLS]
    dr = DevArray(np.full((jobs.j, 10), -7, np.int32))
    dn = DevArray(np.full((jobs.j, kmax), -7, np.int32))
    ms = e.when_k_win_device(*cols, DevArray(jobs.nodes_k), dev(nb), dev(dl), dr, dn, kmax)
    assert ms > 0
    assert rows.tobytes() == dr.numpy().tobytes(), "host and device entry points differ (rows)"
    assert np.array_equal(nodes, dn.numpy()), "host and device entry points differ (nodes)"
    return rows, nodes


def place_both(e, fresh, jobs, kmax, nb, dl):
    """fit_place_tl_k_win through host pointers and, after fresh() has loaded the timeline again,
    through device pointers: the same nodes, starts, counts and final timeline."""
    fresh()
    nodes, start, st = e.place_tl_k_win(jobs, nb, dl, kmax)
    fin = e.read_timeline()
    fresh()
    cols = [DevArray(getattr(jobs, f)) for f in COLS]
    dn = DevArray(np.full((jobs.j, kmax), -7, np.int32))
    ds = DevArray(np.full(jobs.j, -7, np.int32))
    dst = e.place_tl_k_win_device(*cols, DevArray(jobs.nodes_k), dev(nb), dev(dl), dn, ds, kmax)
    assert np.array_equal(nodes, dn.numpy()), "host and device entry points differ (nodes)"
    assert np.array_equal(start, ds.numpy()), "host and device entry points differ (starts)"
    assert fin.tobytes() == e.read_timeline().tobytes(), "host and device entry points differ (timeline)"
    for s in (st, dst):
        assert s["ms_device"] > 0 and s["ms_total"] > 0
        assert {k: s[k] for k in ("jobs", "placed", "unplaced", "rejected", "engine")} == wc.stats_of(nodes, start)
        assert all(s[f] == 0 for f in ("rounds", "evals", "useful_evals", "stops_rescan", "stops_dirty", "ms_scan",
                                       "ms_commit", "ms_exchange", "shard_mode", "reserved", "ms_arb_wait"))
    return nodes, start, st, fin


def assert_rows(got, want, jobs, nb, dl):
    (rows, nodes), (wrows, wnodes) = got, want
    bad = np.flatnonzero((rows != wrows) | (nodes != wnodes).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[0]}: got {rows[bad[0]]} {nodes[bad[0]]}, want " \
                          f"{wrows[bad[0]]} {wnodes[bad[0]]}, job {[getattr(jobs, f)[bad[0]] for f in wk.JOB_FIELDS]} " \
                          f"window {None if nb is None else nb[bad[0]]} {None if dl is None else dl[bad[0]]}"


def assert_same(got, want, jobs, nb, dl):
    (nodes, start, fin), (wnodes, wstart, wfin) = got, want
    bad = np.flatnonzero((nodes != wnodes).any(axis=1) | (start != wstart))
    assert bad.size == 0, f"{bad.size} jobs differ, first {bad[0]}: got {nodes[bad[0]]} from {start[bad[0]]}, want " \
                          f"{wnodes[bad[0]]} from {wstart[bad[0]]}, job {[getattr(jobs, f)[bad[0]] for f in wk.JOB_FIELDS]} " \
                          f"window {None if nb is None else nb[bad[0]]} {None if dl is None else dl[bad[0]]}"
    assert np.array_equal(fin, wfin), f"final timelines differ on nodes {np.flatnonzero((fin != wfin).any(axis=(1, 2)))[:8]}"


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


def fresh_random(e, H):
    """pk.cluster(H) loaded, at H >= 64 after the warm-up queue: the timeline the shared references
    start from."""
    nodes, tline, parts = pk.cluster(H)

    def fresh():
        load(e, nodes, tline, parts)
        if H >= 64:
            e.place_tl(pk.pre_jobs(H))
    fresh()
    assert np.array_equal(e.read_timeline(), pk.start_timeline(H))
    return fresh


# ---- 1. the hand table and the minima trap ---------------------------------------------------------
def test_hand_table(engine):
    nodes, tline, jobs, parts, nb, dl = wc.hand_case()
    fresh = lambda: load(engine, nodes, tline, parts)  # noqa: E731
    fresh()
    rows, nd = when_both(engine, jobs, wc.HAND_KMAX, nb, dl)
    assert rows.tolist() == wc.HAND_ROWS.tolist()  # the table worked out by hand in _win_tl_cases.py
    assert nd.tolist() == wc.HAND_NODES.tolist()
    got, start, st, fin = place_both(engine, fresh, jobs, wc.HAND_KMAX, nb, dl)
    assert start.tolist() == wc.HAND_Q_START.tolist()
    assert got.tolist() == wc.HAND_Q_NODES.tolist()
    assert fin[:, :, 0].tolist() == wc.HAND_Q_CPU.tolist()
    assert (st["placed"], st["unplaced"], st["rejected"], st["components"]) == (5, 6, 1, 2)


def test_minima_trap(engine):
    """The stretch of n2 begins at slot 0 with 1 cpu; from slot 5 it holds 8.  A score from minima
    that start at the stretch's begin instead of at `from` picks n2."""
    nodes, tline, _, parts, _, _ = wc.hand_case()
    job, nb, dl = wc.TRAP
    one = wk.jobs_of([job])
    fresh = lambda: load(engine, nodes, tline, parts)  # noqa: E731
    fresh()
    rows, nd = when_both(engine, one, 1, np.array([nb], np.int32), np.array([dl], np.int32))
    assert (rows["start"][0], nd[0, 0]) == (5, wc.TRAP_NODE)
    got, start, _, fin = place_both(engine, fresh, one, 1, np.array([nb], np.int32), None)
    assert (start[0], got[0, 0]) == (5, wc.TRAP_NODE) and fin[1, 5, 0] == 3 and fin[2, 5, 0] == 8


# ---- 2. exact against the restatement ----------------------------------------------------------------
# The cluster's components have 1, 63, 64, 65 and 600 nodes.  tests/test_win_tl.py asserts that the
# window draw moves starts and unplaces jobs.
@pytest.mark.parametrize("H,j,kmax", wc.WIN_CASES)
def test_exact_against_the_restatement(engine, H, j, kmax):
    fresh = fresh_random(engine, H)
    jobs, nb, dl = wc.win_case(H, j, kmax)
    table = engine.read_nodes()
    got = when_both(engine, jobs, kmax, nb, dl)
    assert_rows(got, wc.alone(H, j, kmax), jobs, nb, dl)
    # the query leaves the timeline and the node table as they were
    assert engine.read_timeline().tobytes() == pk.start_timeline(H).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(table, engine.read_nodes()))
    nodes, start, st, fin = place_both(engine, fresh, jobs, kmax, nb, dl)
    assert_same((nodes, start, fin), wc.reference(H, j, kmax), jobs, nb, dl)
    print(f"H {H} j {j} kmax {kmax}: placed/rejected/unplaced {st['placed']}/{st['rejected']}/{st['unplaced']}, "
          f"WINDOW rows {(got[0]['code'] == 8).sum()}")


# ---- 3. open windows are the unwindowed calls, byte for byte -------------------------------------------
def test_open_windows_are_byte_identical(engine):
    H, j, kmax = 64, 300, 8
    fresh = fresh_random(engine, H)
    jobs = pk.busy_case(H, j, kmax)
    r = np.random.default_rng(1)
    wrows, wnodes = engine.when_k(jobs, kmax)
    wn, ws, wst = engine.place_tl_k(jobs, kmax)
    wfin = engine.read_timeline()
    assert np.array_equal(wn, pk.reference("busy", H, j, kmax)[1])
    for nb, dl in ((None, None), (np.zeros(j, np.int32), np.full(j, wc.NONE, np.int32)),
                   (r.integers(-9, 1, j), None), (None, np.full(j, H, np.int32)),
                   (r.integers(-9, 1, j), r.choice([H, H + 1, wc.NONE], j))):
        fresh()
        rows, nodes = when_both(engine, jobs, kmax, nb, dl)
        assert rows.tobytes() == wrows.tobytes() and nodes.tobytes() == wnodes.tobytes()
        gn, gs, gst, gfin = place_both(engine, fresh, jobs, kmax, nb, dl)
        assert gn.tobytes() == wn.tobytes() and gs.tobytes() == ws.tobytes() and gfin.tobytes() == wfin.tobytes()
        assert all(gst[k] == wst[k] for k in ("jobs", "placed", "unplaced", "rejected", "components", "engine"))


# ---- 4. the block edges of the bounded start scan -------------------------------------------------------
def edge_jobs(H):
    """Single jobs on the 600-node component (partition 4) and on the 64-node one (2): every `from`
    around a 64-slot block edge and at the horizon's end, with every `until` that leaves A one slot,
    empty, or cut at a block edge."""
    rows, nb, dl = [], [], []
    for cpu, wall, k in ((2, 5, 1), (4, 13, 4), (8, 70 * pk.SLOT_MIN, 2), (32, 5, 8), (24, 13, 6)):
        d = max(1, -(-wall // pk.SLOT_MIN))
        for frm in (63, 64, 65, 127, 128, H - d, H - d + 1, H):
            for until in (frm + d, frm + d - 1, 64, 65, 129, wc.NONE):
                for part in (4, 2):
                    rows.append((cpu, cpu * 512, 0, wall, part, k))
                    nb.append(frm)
                    dl.append(until)
    return wk.jobs_of(rows), np.array(nb, np.int32), np.array(dl, np.int32)


def test_block_edges_of_the_start_scan(engine):
    H, kmax = 1024, 8
    fresh = fresh_random(engine, H)
    nodes, tline, parts = pk.cluster(H)
    jobs, nb, dl = edge_jobs(H)
    want = wc.ref_when_k_win(pk.start_timeline(H), nodes.part_mask, parts, jobs, pk.SLOT_MIN, kmax, nb, dl)
    codes = want[0]["code"]
    assert (codes == 8).sum() >= 50 and (codes == 6).sum() >= 50, np.bincount(codes)
    assert (want[0]["start"] == nb).sum() >= 30 and (want[0]["start"] > nb).sum() >= 5
    assert_rows(when_both(engine, jobs, kmax, nb, dl), want, jobs, nb, dl)
    wq = wc.ref_place_tl_k_win(pk.start_timeline(H), nodes.part_mask, parts, jobs, pk.SLOT_MIN, kmax, nb, dl)
    got = place_both(engine, fresh, jobs, kmax, nb, dl)
    assert_same((got[0], got[1], got[3]), wq, jobs, nb, dl)


# ---- 5. long run lists -----------------------------------------------------------------------------------
def test_long_run_lists(engine):
    """pk.stairs(): 128 runs per node, a run every two slots, so run i begins near slot 2 i.  `from`
    falls inside the header copy (runs 0-3), on the edges of the four-Seg loads behind it and deep in
    the slab; the deadlines cut the one long feasible stretch of a node short."""
    nodes, tline, parts = pk.stairs()
    jobs, tl0, _, _, _ = pk.stairs_reference()
    r = np.random.default_rng(11)
    j = jobs.j
    d = wc.durs(jobs, tline.slot_min).astype(np.int64)
    nb = r.choice([0, 1, 2, 3, 5, 7, 8, 9, 10, 15, 16, 17, 18, 100, 101, 200, 250], j)
    # a job of c cpus is feasible from about slot 2 c on: half of the deadlines sit just behind it
    near = np.maximum(nb, 2 * jobs.cpu.astype(np.int64)) + d + r.integers(-1, 6, j)
    dl = np.where(r.random(j) < 0.5, near, r.choice([wc.NONE, 256, 128, 64], j))
    nb, dl = nb.astype(np.int32), dl.astype(np.int32)
    fresh = lambda: load(engine, nodes, tline, parts)  # noqa: E731
    fresh()
    assert np.array_equal(engine.read_timeline(), tl0)
    want = wc.ref_when_k_win(tl0, nodes.part_mask, parts, jobs, tline.slot_min, 4, nb, dl)
    assert ((want[0]["start"] >= 0) & (dl < 256)).sum() >= 20 and (want[0]["code"] == 8).sum() >= 10
    assert_rows(when_both(engine, jobs, 4, nb, dl), want, jobs, nb, dl)
    wq = wc.ref_place_tl_k_win(tl0, nodes.part_mask, parts, jobs, tline.slot_min, 4, nb, dl)
    assert (wq[1] >= 0).sum() >= 30 and (wk.run_counts(wq[2]) > 128).all()
    got = place_both(engine, fresh, jobs, 4, nb, dl)
    assert_same((got[0], got[1], got[3]), wq, jobs, nb, dl)


# ---- 6. the consequences of §2r ----------------------------------------------------------------------------
def test_consequences(engine):
    H, j, kmax = 64, 300, 8
    fresh = fresh_random(engine, H)
    nodes, tline, parts = pk.cluster(H)
    jobs, nb, dl = wc.win_case(H, j, kmax)
    frm, until, d = np.clip(nb, 0, H), np.clip(dl, 0, H), wc.durs(jobs, wc.SLOT_MIN)
    # 2. job 0 of a placement is the query's answer on the timeline as loaded
    placed = 0
    for q in range(60, 72):
        one = wk.one_job(jobs, q)
        fresh()
        rows, want = engine.when_k_win(one, nb[q:q + 1], dl[q:q + 1], kmax)
        got, start, st = engine.place_tl_k_win(one, nb[q:q + 1], dl[q:q + 1], kmax)
        assert start[0] == rows["start"][0] and np.array_equal(got, want), (q, rows, got, want)
        placed += st["placed"]
    assert placed >= 4
    # 4. an unwindowed start inside A is the windowed answer, nodes included
    fresh()
    urows, unodes = engine.when_k(jobs, kmax)
    rows, wnodes = engine.when_k_win(jobs, nb, dl, kmax)
    s0 = urows["start"]
    inside = (s0 >= 0) & (frm <= s0) & (s0 + d <= until)
    assert inside.sum() >= 50
    assert np.array_equal(rows["start"][inside], s0[inside]) and np.array_equal(wnodes[inside], unodes[inside])
    # 3. every placed job starts inside its window
    got, start, st = engine.place_tl_k_win(jobs, nb, dl, kmax)
    p = start >= 0
    assert st["placed"] == p.sum() >= 100
    assert (frm[p] <= start[p]).all() and (start[p] + d[p] <= until[p]).all()
    fin = engine.read_timeline()
    # 5. unplacing the outputs restores the timeline bit for bit
    assert engine.unplace_tl(jobs, got, start, kmax) == np.maximum(jobs.nodes_k[p], 1).sum()
    assert engine.read_timeline().tobytes() == pk.start_timeline(H).tobytes()
    # 6. after a reload every row holds again
    fresh()
    state, applied, refused = engine.hold_tl(jobs, got, start, kmax)
    assert refused == 0 and (state[p] == _lib.FIT_HOLD_HELD).all() and (state[~p] == _lib.FIT_HOLD_SKIPPED).all()
    assert engine.read_timeline().tobytes() == fin.tobytes()


# ---- 7. the launch seam --------------------------------------------------------------------------------------
def test_chunk_seam(engine, monkeypatch):
    """FIT_PTLK_CHUNK (test-only, read at call time) cuts every component's job list into launches of
    64 jobs and of one: the run lists in HBM carry the state over the seam."""
    H, j, kmax = 64, 300, 8
    fresh = fresh_random(engine, H)
    jobs, nb, dl = wc.win_case(H, j, kmax)
    assert np.bincount(jobs.part).max() > 64
    for chunk in ("64", "1"):
        monkeypatch.setenv("FIT_PTLK_CHUNK", chunk)
        nodes, start, st, fin = place_both(engine, fresh, jobs, kmax, nb, dl)
        assert_same((nodes, start, fin), wc.reference(H, j, kmax), jobs, nb, dl)


# ---- 8. errors and state ---------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_errors_and_state():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    jobs.nodes_k[:] = np.arange(16) % 4
    nb = (np.arange(16, dtype=np.int32) % 5) - 1
    dl = np.where(np.arange(16) % 3 == 0, wc.NONE, tline.slots - 2).astype(np.int32)
    L = _lib.lib()
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    none = (None,) * 6
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    with Engine(device=0) as e:
        assert _code(lambda: e.place_tl_k_win(jobs, nb, dl, 3)) == STATE  # before load_nodes
        assert _code(lambda: e.when_k_win(jobs, nb, dl, 3)) == STATE
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.place_tl_k_win(jobs, nb, dl, 3)) == STATE  # no timeline loaded
        assert _code(lambda: e.when_k_win(jobs, nb, dl, 3)) == STATE
        e.load_timeline(tline)
        table = e.read_nodes()
        before = e.read_timeline()

        def unchanged():
            assert e.read_timeline().tobytes() == before.tobytes()

        ms = C.c_double()
        assert L.fit_when_k_win_ms(e._h, C.byref(ms)) == STATE  # no fit_when_k_win_device yet
        st = _lib.FitStats(jobs=7, engine=9)
        for fn in (L.fit_place_tl_k_win, L.fit_place_tl_k_win_device):
            assert fn(e._h, 0, *none, 1, None, None, None, None, None) == 0  # j == 0 whatever the pointers are
            st.jobs, st.engine = 7, 9
            assert fn(e._h, 0, *none, 1, None, None, None, None, C.byref(st)) == 0 and (st.jobs, st.engine) == (0, 0)
            assert fn(e._h, 1, *none, 1, None, None, None, None, None) == INVAL
            assert fn(e._h, -1, *none, 1, None, None, None, None, None) == INVAL
        for fn in (L.fit_when_k_win, L.fit_when_k_win_device):
            assert fn(e._h, 0, *none, 1, None, None, None, None) == 0
            assert fn(e._h, 1, *none, 1, None, None, None, None) == INVAL
            assert fn(e._h, -1, *none, 1, None, None, None, None) == INVAL
        for kmax in (0, -1, 9):
            assert _code(lambda: e.place_tl_k_win(jobs, nb, dl, kmax)) == INVAL, kmax
            assert _code(lambda: e.when_k_win(jobs, nb, dl, kmax)) == INVAL, kmax
        assert _code(lambda: e.place_tl_k_win(jobs, nb, dl, 2)) == INVAL  # a job of 3 nodes, kmax 2
        assert _code(lambda: e.when_k_win(jobs, nb, dl, 2)) == INVAL
        unchanged()
        for f in ("cpu", "mem", "gpu", "wall"):
            bad = synth.Jobs(*(getattr(jobs, g).copy() for g in wk.JOB_FIELDS))
            getattr(bad, f)[11] = -1  # behind jobs that would have been placed
            assert _code(lambda: e.place_tl_k_win(bad, nb, dl, 3)) == INVAL, f
            assert _code(lambda: e.when_k_win(bad, nb, dl, 3)) == INVAL, f
            unchanged()
        cols = [np.ascontiguousarray(getattr(jobs, f)) for f in wk.JOB_FIELDS]
        nd, ss = np.zeros((16, 3), np.int32), np.zeros(16, np.int32)
        win = (p(nb), p(dl))
        assert L.fit_place_tl_k_win(e._h, 16, *[p(c) for c in cols], 3, *win, None, p(ss), None) == INVAL  # NULL nodes
        assert L.fit_place_tl_k_win(e._h, 16, *[p(c) for c in cols], 3, *win, p(nd), None, None) == INVAL  # NULL starts
        unchanged()
        # no value of a window column is an error; the next valid call is exact, stats NULL included
        wild = np.array([-2**31, 2**31 - 1, -1, 0] * 4, np.int32)
        rows, _ = e.when_k_win(jobs, wild, wild[::-1].copy(), 3)
        assert set(rows["code"].tolist()) <= {0, 1, 2, 3, 4, 5, 6, 7, 8}
        unchanged()
        want = wc.ref_place_tl_k_win(before, nodes.part_mask, parts, jobs, tline.slot_min, 3, nb, dl)
        assert L.fit_place_tl_k_win(e._h, 16, *[p(c) for c in cols], 3, *win, p(nd), p(ss), None) == 0
        assert np.array_equal(nd, want[0]) and np.array_equal(ss, want[1]) and (ss >= 0).sum() >= 5
        assert np.array_equal(e.read_timeline(), want[2])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(table, e.read_nodes())), "the node table changed"
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.place_tl_k_win(jobs, nb, dl, 3)) == STATE
        assert _code(lambda: e.when_k_win(jobs, nb, dl, 3)) == STATE

"""fit_place_tl_k on the GPU against a numpy restatement of DESIGN.md §2g (_place_tl_k_cases.
ref_place_tl_k, over the dense [n, H, 3] timeline): the hand case, exact nodes, starts and final
timelines on contended queues over components below, at and above a wave, long run lists, k = 1 =
fit_place_tl, job 0 = fit_when_k, the launch seam, state and argument errors.  Every case runs through
the host and the device entry point, each on a freshly loaded timeline, and both must agree."""
import ctypes as C

import numpy as np
import pytest

import _place_tl_k_cases as pk
import _when_k_cases as wk
from _devarray import DevArray
from fitgpu import FIT_REJECTED, Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu
COLS = ("cpu", "mem", "gpu", "wall", "part")


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


def place_both(e, fresh, jobs, kmax, null_k=False):
    """fit_place_tl_k through host pointers and, after fresh() has loaded the timeline again, through
    device pointers: the same nodes, starts, counts and final timeline.  null_k: nodes_k passed as
    NULL (= all 1) to both.  Returns (nodes, start, stats, final timeline)."""
    fresh()
    if null_k:
        cols = [np.ascontiguousarray(getattr(jobs, f)) for f in COLS]
        nodes = np.full((jobs.j, kmax), -7, np.int32)
        start = np.full(jobs.j, -7, np.int32)
        st = _lib.FitStats()
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        rc = _lib.lib().fit_place_tl_k(e._h, jobs.j, *[p(c) for c in cols], None, kmax, p(nodes), p(start), C.byref(st))
        assert rc == 0, rc
        st = st.as_dict()
    else:
        nodes, start, st = e.place_tl_k(jobs, kmax)
    fin = e.read_timeline()
    fresh()
    cols = [DevArray(getattr(jobs, f)) for f in COLS]
    dk = None if null_k else DevArray(jobs.nodes_k)
    dn = DevArray(np.full((jobs.j, kmax), -7, np.int32))
    ds = DevArray(np.full(jobs.j, -7, np.int32))
    dst = e.place_tl_k_device(*cols, dk, dn, ds, kmax)
    assert np.array_equal(nodes, dn.numpy()), "host and device entry points differ (nodes)"
    assert np.array_equal(start, ds.numpy()), "host and device entry points differ (starts)"
    assert fin.tobytes() == e.read_timeline().tobytes(), "host and device entry points differ (timeline)"
    for s in (st, dst):
        assert s["engine"] == 4 and s["jobs"] == jobs.j and s["ms_device"] > 0 and s["ms_total"] > 0
        assert s["placed"] + s["unplaced"] + s["rejected"] == s["jobs"]
        assert s["placed"] == (start >= 0).sum() and s["rejected"] == (nodes[:, 0] == FIT_REJECTED).sum()
        assert all(s[f] == 0 for f in ("rounds", "evals", "useful_evals", "stops_rescan", "stops_dirty", "ms_scan",
                                       "ms_commit", "ms_exchange", "shard_mode", "reserved", "ms_arb_wait"))
    return nodes, start, st, fin


def assert_same(got, want, jobs):
    (nodes, start, fin), (wnodes, wstart, wfin) = got, want
    bad = np.flatnonzero((nodes != wnodes).any(axis=1) | (start != wstart))
    assert bad.size == 0, f"{bad.size} jobs differ, first {bad[0]}: got {nodes[bad[0]]} from {start[bad[0]]}, " \
                          f"want {wnodes[bad[0]]} from {wstart[bad[0]]}, job {[getattr(jobs, f)[bad[0]] for f in wk.JOB_FIELDS]}"
    assert np.array_equal(fin, wfin), f"final timelines differ on nodes {np.flatnonzero((fin != wfin).any(axis=(1, 2)))[:8]}"


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


def fresh_random(e, H):
    """rand_cluster(H) loaded, at H >= 64 after test_when_k_gpu's warm-up queue, so that the starting
    lists already carry dips; the engine's timeline is the one the shared references start from."""
    nodes, tline, parts = pk.cluster(H)

    def fresh():
        load(e, nodes, tline, parts)
        if H >= 64:
            e.place_tl(pk.pre_jobs(H))
    fresh()
    assert np.array_equal(e.read_timeline(), pk.start_timeline(H))
    return fresh


# ---- 1. the hand case -----------------------------------------------------------------------------
def test_hand_case(engine):
    nodes, tline, jobs, parts = pk.hand_case()
    got, start, st, fin = place_both(engine, lambda: load(engine, nodes, tline, parts), jobs, pk.HAND_KMAX)
    assert got.tolist() == pk.HAND_NODES.tolist()  # the table worked out by hand in _place_tl_k_cases.py
    assert start.tolist() == pk.HAND_START.tolist()
    assert fin[:, :, 0].tolist() == pk.HAND_CPU.tolist()
    assert {k: st[k] for k in pk.HAND_STATS} == pk.HAND_STATS and st["components"] == 2


# ---- 2. exact against the restatement ----------------------------------------------------------------
# The cluster's components have 1, 63, 64, 65 and 600 nodes: below, at and above a wave, and below a
# 1,024-thread pass.  busy: contended queues (tests/test_place_tl_k.py asserts they are); rand:
# undeclared partitions, limit rejections, d == H + 1; the smallest case is H = 1 with 9 jobs.
@pytest.mark.parametrize("kind,H,j,kmax", [("busy",) + c for c in pk.BUSY] + [("rand",) + c for c in pk.RAND])
def test_exact_against_the_restatement(engine, kind, H, j, kmax):
    fresh = fresh_random(engine, H)
    jobs, wnodes, wstart, wfin = pk.reference(kind, H, j, kmax)
    nodes, start, st, fin = place_both(engine, fresh, jobs, kmax)
    assert_same((nodes, start, fin), (wnodes, wstart, wfin), jobs)
    counts = (st["placed"], st["rejected"], st["unplaced"])
    print(f"{kind} H {H} j {j} kmax {kmax}: placed/rejected/unplaced {counts}")
    if kind == "rand":
        assert all(c > 0 for c in counts), counts


# ---- 3. long run lists --------------------------------------------------------------------------------
def test_long_run_lists(engine):
    """128 runs per node at load, 134-146 after: the reservations split runs beyond index 64 of a
    list — tl_reserve_any's second 64-lane pass, lists wholly in the slab."""
    nodes, tline, parts = pk.stairs()
    jobs, tl0, wnodes, wstart, wfin = pk.stairs_reference()
    fresh = lambda: load(engine, nodes, tline, parts)  # noqa: E731
    fresh()
    assert np.array_equal(engine.read_timeline(), tl0)
    nodes_, start, st, fin = place_both(engine, fresh, jobs, 4)
    assert_same((nodes_, start, fin), (wnodes, wstart, wfin), jobs)
    assert (wk.run_counts(fin) > 128).all() and st["unplaced"] >= 20


# ---- 4. k = 1 is fit_place_tl ---------------------------------------------------------------------------
def test_k1_equals_place_tl():
    nodes, tline, jobs, parts = synth.make_c5(500, 1500)
    _, _, more, _ = synth.make_c5(500, 300, shard=9)
    with Engine(device=0) as e:
        fresh = lambda: load(e, nodes, tline, parts)  # noqa: E731
        fresh()
        node, start, st = e.place_tl(jobs)
        fin = e.read_timeline()
        node2, start2, _ = e.place_tl(more)
        fin2 = e.read_timeline()
        assert st["placed"] > 1000 and (start > 0).any() and (node == FIT_REJECTED).any()
        for k, null_k in ((1, False), (0, False), (1, True)):
            gn, gs, gst, gfin = place_both(e, fresh, pk.ones(jobs, k), 1, null_k=null_k)
            assert np.array_equal(gn[:, 0], node) and np.array_equal(gs, start), (k, null_k)
            assert gfin.tobytes() == fin.tobytes(), (k, null_k)
            assert (gst["placed"], gst["unplaced"], gst["rejected"]) == (st["placed"], st["unplaced"], st["rejected"])
            # the canonical state: the k = 1 engine goes on from it exactly as from its own
            n2, s2, _ = e.place_tl(more)
            assert np.array_equal(n2, node2) and np.array_equal(s2, start2), (k, null_k)
            assert e.read_timeline().tobytes() == fin2.tobytes(), (k, null_k)


# ---- 5. job 0 is fit_when_k ------------------------------------------------------------------------------
def test_job0_is_when_k(engine):
    H, j, kmax = pk.BUSY[1]
    fresh = fresh_random(engine, H)
    nodes, tline, parts = pk.cluster(H)
    jobs = pk.busy_case(H, j, kmax)
    tl0 = pk.start_timeline(H)
    placed = 0
    for q in range(20):
        one = wk.one_job(jobs, q)
        fresh()
        rows, want = engine.when_k(one, kmax)
        got, start, st = engine.place_tl_k(one, kmax)
        assert start[0] == rows["start"][0] and np.array_equal(got, want), (q, rows, got, want)
        _, _, wfin = pk.ref_place_tl_k(tl0, nodes.part_mask, parts, one, pk.SLOT_MIN, kmax)
        fin = engine.read_timeline()
        assert np.array_equal(fin, wfin), q
        after = engine.when_k(one, kmax)  # reflects the reservation
        ref = wk.ref_when_k(wfin, nodes.part_mask, parts, one, pk.SLOT_MIN, kmax)
        assert np.array_equal(after[0], ref[0]) and np.array_equal(after[1], ref[1]), q
        placed += st["placed"]
    assert placed >= 15


# ---- 6. the launch seam -------------------------------------------------------------------------------
def test_chunk_seam(engine, monkeypatch):
    """FIT_PTLK_CHUNK (test-only, read at call time) cuts every component's job list into launches of
    64 jobs: the run lists in HBM carry the state over the seam."""
    H, j, kmax = pk.BUSY[1]
    fresh = fresh_random(engine, H)
    jobs, wnodes, wstart, wfin = pk.reference("busy", H, j, kmax)
    assert np.bincount(jobs.part).max() > 64  # a component's list spans several launches
    monkeypatch.setenv("FIT_PTLK_CHUNK", "64")
    nodes, start, st, fin = place_both(engine, fresh, jobs, kmax)
    assert_same((nodes, start, fin), (wnodes, wstart, wfin), jobs)
    monkeypatch.setenv("FIT_PTLK_CHUNK", "1")
    nodes, start, st, fin = place_both(engine, fresh, jobs, kmax)
    assert_same((nodes, start, fin), (wnodes, wstart, wfin), jobs)


# ---- 7. errors and state --------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_errors_and_state():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    jobs.nodes_k[:] = np.arange(16) % 4
    L = _lib.lib()
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    none = (None,) * 6
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    with Engine(device=0) as e:
        assert _code(lambda: e.place_tl_k(jobs, 3)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.place_tl_k(jobs, 3)) == STATE  # no timeline loaded
        e.load_timeline(tline)
        table = e.read_nodes()
        before = e.read_timeline()
        dense0 = before.copy()

        def unchanged():
            assert e.read_timeline().tobytes() == before.tobytes()

        st = _lib.FitStats(jobs=7, engine=9)
        for fn in (L.fit_place_tl_k, L.fit_place_tl_k_device):
            assert fn(e._h, 0, *none, 1, None, None, None) == 0  # j == 0 whatever the pointers are
            st.jobs, st.engine = 7, 9
            assert fn(e._h, 0, *none, 1, None, None, C.byref(st)) == 0 and (st.jobs, st.engine) == (0, 0)
            assert fn(e._h, 1, *none, 1, None, None, None) == INVAL
            assert fn(e._h, -1, *none, 1, None, None, None) == INVAL
        for kmax in (0, -1, 9):
            assert _code(lambda: e.place_tl_k(jobs, kmax)) == INVAL, kmax
        assert _code(lambda: e.place_tl_k(jobs, 2)) == INVAL  # a job of 3 nodes, kmax 2
        unchanged()
        for f in ("cpu", "mem", "gpu", "wall"):
            bad = synth.Jobs(*(getattr(jobs, g).copy() for g in wk.JOB_FIELDS))
            getattr(bad, f)[11] = -1  # behind jobs that would have been placed
            assert _code(lambda: e.place_tl_k(bad, 3)) == INVAL, f
            unchanged()
        cols = [np.ascontiguousarray(getattr(jobs, f)) for f in wk.JOB_FIELDS]
        nd, ss = np.zeros((16, 3), np.int32), np.zeros(16, np.int32)
        assert L.fit_place_tl_k(e._h, 16, *[p(c) for c in cols], 3, None, p(ss), None) == INVAL  # NULL nodes
        assert L.fit_place_tl_k(e._h, 16, *[p(c) for c in cols], 3, p(nd), None, None) == INVAL  # NULL starts
        unchanged()
        # the next valid call is exact, stats NULL included
        want = pk.ref_place_tl_k(dense0, nodes.part_mask, parts, jobs, tline.slot_min, 3)
        assert L.fit_place_tl_k(e._h, 16, *[p(c) for c in cols], 3, p(nd), p(ss), None) == 0
        assert np.array_equal(nd, want[0]) and np.array_equal(ss, want[1]) and (ss >= 0).sum() >= 5
        assert np.array_equal(e.read_timeline(), want[2])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(table, e.read_nodes())), "the node table changed"
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.place_tl_k(jobs, 3)) == STATE

"""fit_unplace_tl on the GPU against a numpy restatement of DESIGN.md §2h (_unplace_tl_cases.
ref_unplace_tl, over the dense [n, H, 3] timeline): round trips of fit_place_tl_k / fit_place_tl,
partial unplacing and what the engines place afterwards, long run lists and window edges, many
windows on one node, the header ceilings, a running job that ends early, -1 and saturation, errors
that leave the timeline alone, the launch seam and the device entry point."""
import ctypes as C

import numpy as np
import pytest

import fitgpu
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from _devarray import DevArray
from fitgpu import FIT_ETA_NOW, Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu
INT32_MAX = uc.INT32_MAX


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


def need_sum(jobs, start):
    return int(np.maximum(jobs.nodes_k[start >= 0], 1).sum())


def same_table(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. round trip ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_round_trip(engine, H, kmax):
    e = engine
    jobs, wnodes, wstart, wfin = uc.reference(H, kmax)
    fresh_random(e, H)
    tl0, table = e.read_timeline(), e.read_nodes()
    nodes, start, _ = e.place_tl_k(jobs, kmax)
    assert np.array_equal(nodes, wnodes) and np.array_equal(start, wstart)
    assert np.array_equal(e.read_timeline(), wfin)
    applied = e.unplace_tl(jobs, nodes, start, kmax)  # verbatim: unplaced and rejected rows included
    assert applied == need_sum(jobs, start)
    assert e.read_timeline().tobytes() == tl0.tobytes(), "the timeline as loaded is not restored"
    assert same_table(table, e.read_nodes()), "the node table changed"
    assert e.unplace_tl_ms() > 0
    # the headers: a stale cnt, head[] or ceiling changes what the same queue gets now
    nodes2, start2, _ = e.place_tl_k(jobs, kmax)
    assert np.array_equal(nodes2, nodes) and np.array_equal(start2, start)
    assert np.array_equal(e.read_timeline(), wfin)
    if kmax == 1:  # the persistent engine reads the same headers
        fresh_random(e, H)
        n1, s1, _ = e.place_tl(jobs)
        assert np.array_equal(s1, wstart) and np.array_equal(n1[s1 >= 0], wnodes[s1 >= 0, 0])
        assert e.unplace_tl(jobs, n1, s1) == (s1 >= 0).sum()
        assert e.read_timeline().tobytes() == tl0.tobytes()
        n2, s2, _ = e.place_tl(jobs)
        assert np.array_equal(n2, n1) and np.array_equal(s2, s1)
        assert np.array_equal(e.read_timeline(), wfin)


# ---- 2. partial ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_partial_then_place(H, kmax):
    nodes, tline, parts = pk.cluster(H)
    jobs, wnodes, wstart, wfin = uc.reference(H, kmax)
    rows = uc.half(H, kmax)
    want, wapplied = uc.ref_unplace_tl(wfin, jobs, wnodes, wstart, pk.SLOT_MIN, kmax, rows)
    second = uc.second_jobs(H, kmax)
    for consumer in ("place_tl_k", "place_tl"):
        with Engine(device=0) as e:  # a fresh context brought to the same state
            fresh_random(e, H)
            out, start, _ = e.place_tl_k(jobs, kmax)
            assert np.array_equal(out, wnodes) and np.array_equal(start, wstart)
            assert e.unplace_tl(uc.take(jobs, rows), out[rows], start[rows], kmax) == wapplied
            assert np.array_equal(e.read_timeline(), want)
            if consumer == "place_tl_k":
                rn, rs, rfin = pk.ref_place_tl_k(want, nodes.part_mask, parts, second, pk.SLOT_MIN, kmax)
                gn, gs, st = e.place_tl_k(second, kmax)
                assert np.array_equal(gn, rn) and np.array_equal(gs, rs)
            else:
                one = pk.ones(second)
                rn, rs, rfin = pk.ref_place_tl_k(want, nodes.part_mask, parts, one, pk.SLOT_MIN, 1)
                gn, gs, st = e.place_tl(one)
                assert np.array_equal(gs, rs) and np.array_equal(gn[gs >= 0], rn[gs >= 0, 0])
            assert st["placed"] >= 20
            assert np.array_equal(e.read_timeline(), rfin)


# ---- 3. long lists and edges -----------------------------------------------------------------------------
def test_long_lists_and_edges(engine):
    """pk.stairs(): 128 runs per node (beyond one wave's lanes and beyond TL_HEAD), slot_min 1, H 256.
    Node 1's runs are [0, 3), [3, 5), ..., [255, 256); node 0's [0, 2), [2, 4), ..."""
    e = engine
    nodes, tline, parts = pk.stairs()
    H = tline.slots
    load(e, nodes, tline, parts)
    tl = e.read_timeline()
    assert (wk.run_counts(tl) == 128).all()

    def step(rows, want_runs_node1):
        nonlocal tl
        a = np.array(rows, np.int64)  # (node, start, wall, cpu, mem)
        jobs = synth.Jobs(a[:, 3].astype(np.int32), a[:, 4].astype(np.int32), np.zeros(len(a), np.int32),
                          a[:, 2].astype(np.int32), np.zeros(len(a), np.uint16), np.ones(len(a), np.uint16))
        node, start = a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)
        tl, applied = uc.ref_unplace_tl(tl, jobs, node, start, 1, 1)
        assert e.unplace_tl(jobs, node, start) == applied == len(a)
        got = e.read_timeline()
        assert np.array_equal(got, tl)
        assert wk.run_counts(got)[1] == want_runs_node1

    step([(1, 0, 1, 3, 7), (1, 2, 1, 3, 7)], 130)  # a window from slot 0; the run [0, 3) is now 3 runs
    step([(1, 1, 1, 3, 7)], 128)                   # both ends on run boundaries: the count drops by 2
    step([(1, 1, 1, 2, 0)], 130)                   # inside one run: it rises by 2
    step([(0, 100, 1, 1, 1),     # the first slot of run 50
          (0, 201, 1, 5, 0),     # the last slot of run 100, beyond one wave's lanes
          (2, 250, 6, 1, 1),     # a window to H
          (3, 250, 100, 2, 2),   # start + d > H: clipped
          (4, 0, 256, 9, 9),     # the whole horizon
          (0, 0, 1000, 1, 0),    # the whole horizon, clipped
          (1, 130, 70, 4, 4)], 132)  # from inside run 64 to inside run 99: two splits
    runs = wk.run_counts(tl)  # node 0: two splits of one side each; node 3: 250 is inside its run [249, 251)
    assert runs[0] == 130 and runs[2] == 128 and runs[3] == 129 and runs[4] == 128
    # the lists are canonical and the headers current: the engines go on from them exactly
    jobs = pk.stair_jobs(40, 17)
    rn, rs, rfin = pk.ref_place_tl_k(tl, nodes.part_mask, parts, jobs, 1, 4)
    gn, gs, st = e.place_tl_k(jobs, 4)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and st["placed"] >= 10
    assert np.array_equal(e.read_timeline(), rfin)


# ---- 4. many windows on one node in one call ------------------------------------------------------------
def test_many_windows_on_one_node(engine):
    e = engine
    H, n = 64, 40
    load(e, uc.flat_cluster(n), uc.no_events(n, H, 1), wk.open_parts(1))
    tl0 = e.read_timeline()
    jobs, node, start = uc.crowd(H, n)
    want, applied = uc.ref_unplace_tl(tl0, jobs, node, start, 1, 3)
    assert e.unplace_tl(jobs, node, start, 3) == applied == 300 + 30 + 36
    assert np.array_equal(e.read_timeline(), want)
    assert wk.run_counts(want)[7] > 32


# ---- 5. the ceilings rise -------------------------------------------------------------------------------
def test_ceilings_rise():
    """A flat node with 4 cpus, then 4 cpus handed back on [0, 8) that were never reserved: a job of
    8 cpus fits at slot 0 — for every consumer that rejects a node by its header ceiling."""
    nodes, tline, parts = uc.flat_cluster(1, cpu=4), uc.no_events(1, 16, 5), wk.open_parts(1)
    back = wk.jobs_of([(4, 0, 0, 40, 0, 1)])
    job = wk.jobs_of([(8, 1024, 0, 40, 0, 1)])
    z = np.zeros(1, np.int32)
    with Engine(device=0) as e:
        def setup():
            load(e, nodes, tline, parts)
            assert e.when(job)["code"][0] != FIT_ETA_NOW  # 8 cpus do not fit the node as loaded
            assert e.unplace_tl(back, z, z) == 1
            tl = e.read_timeline()
            assert (tl[0, :8, 0] == 8).all() and (tl[0, 8:, 0] == 4).all()

        setup()
        row = e.when(job)
        assert row["code"][0] == FIT_ETA_NOW and row["node"][0] == 0 and row["start"][0] == 0
        rows, nk = e.when_k(job, 1)
        assert rows["code"][0] == FIT_ETA_NOW and nk[0, 0] == 0 and rows["start"][0] == 0
        gn, gs, _ = e.place_tl_k(job, 1)
        assert gn[0, 0] == 0 and gs[0] == 0
        setup()
        gn, gs, _ = e.place_tl(job)
        assert gn[0] == 0 and gs[0] == 0


# ---- 6. a running job ends early ---------------------------------------------------------------------------
def test_running_job_ends_early(engine):
    """12 running jobs as fit_release_events sees them; job i unplaced with start 0 and wall =
    rem_min.  The result is the timeline of a cluster on which job i does not run: its demand free in
    the node table and no release event of it."""
    e = engine
    n, H, L, kmax = 10, 32, 5, 4
    r = np.random.default_rng(6)
    running = []
    for i in range(12):
        rows = sorted(r.choice(n, int(r.integers(1, kmax + 1)), replace=False).tolist())
        rem = [0, 1, L, L + 1, H * L, H * L + 70][i] if i < 6 else int(r.integers(0, H * L))
        running.append((rows, rem, int(r.integers(0, 5)), int(r.integers(0, 2048)), int(r.integers(0, 2))))
    nodes = uc.flat_cluster(n, cpu=8, mem=16384, gpu=2)
    parts = wk.open_parts(1)
    for i, (rows, rem, c, m, g) in enumerate(running):
        load(e, nodes, fitgpu.release_events(n, running, H, L), parts)
        table = e.read_nodes()
        node = np.full((1, kmax), -1, np.int32)
        node[0, :len(rows)] = rows
        one = wk.jobs_of([(c, m, g, rem, 0, len(rows))])
        assert e.unplace_tl(one, node, np.zeros(1, np.int32), kmax) == len(rows)
        got = e.read_timeline()
        assert same_table(table, e.read_nodes())
        without = synth.Nodes(*(getattr(nodes, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min",
                                                                   "part_mask")))
        without.cpu_free[rows] += c
        without.mem_free[rows] += m
        without.gpu_free[rows] += g
        load(e, without, fitgpu.release_events(n, running[:i] + running[i + 1:], H, L), parts)
        assert np.array_equal(got, e.read_timeline()), i


# ---- 7. -1 and saturation -------------------------------------------------------------------------------
def test_minus_one_and_saturation(engine):
    e = engine
    H, L = 16, 5
    nodes = synth.Nodes(cpu_free=np.array([4, -3, INT32_MAX - 1, 4], np.int32),
                        mem_free=np.full(4, 1000, np.int32), gpu_free=np.full(4, 1, np.int32),
                        avail_min=np.array([5 * L, wk.INF, wk.INF, wk.INF], np.int32),
                        part_mask=np.array([1, 1, 1, 0], np.uint32))
    load(e, nodes, uc.no_events(4, H, L), wk.open_parts(1))
    tl0 = e.read_timeline()
    assert (tl0[0, 5:] == -1).all() and (tl0[1, :, 0] == -1).all() and (tl0[3] == -1).all()
    jobs = wk.jobs_of([(5, 10, 1, 5 * L, 0, 4)])  # slots [3, 8) of all four nodes
    node = np.array([[0, 1, 2, 3]], np.int32)
    start = np.array([3], np.int32)
    want, _ = uc.ref_unplace_tl(tl0, jobs, node, start, L, 4)
    assert e.unplace_tl(jobs, node, start, 4) == 4  # the node in no partition counts as a window
    got = e.read_timeline()
    assert np.array_equal(got, want)
    assert got[0, 3:5].tolist() == [[9, 1010, 2]] * 2 and (got[0, 5:] == -1).all()  # slots >= U stay -1
    assert (got[1, :, 0] == -1).all() and got[1, 3:8, 1:].tolist() == [[1010, 2]] * 5  # the other columns rise
    assert (got[2, 3:8, 0] == INT32_MAX).all() and got[2, 2, 0] == INT32_MAX - 1 and got[2, 8, 0] == INT32_MAX - 1
    assert (got[3] == -1).all()
    # twice more: saturated values stay, in one call of two rows
    two = uc.concat(jobs, jobs)
    want2, _ = uc.ref_unplace_tl(want, two, np.vstack([node, node]), np.array([3, 3], np.int32), L, 4)
    assert e.unplace_tl(two, np.vstack([node, node]), np.array([3, 3], np.int32), 4) == 8
    got = e.read_timeline()
    assert np.array_equal(got, want2) and (got[2, 3:8, 0] == INT32_MAX).all() and got[0, 3, 0] == 19


# ---- 8. errors leave the timeline unchanged ----------------------------------------------------------------
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
        assert _code(lambda: e.unplace_tl(good, gnode, gstart, kmax)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.unplace_tl(good, gnode, gstart, kmax)) == STATE  # no timeline loaded
        ms = C.c_double()
        assert L_.fit_unplace_tl_ms(e._h, C.byref(ms)) == STATE
        e.load_timeline(tline)
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
            assert _code(lambda: e.unplace_tl(jobs, node, st, kmax)) == INVAL, what
            assert e.read_timeline().tobytes() == before.tobytes(), what
            dev = [DevArray(np.ascontiguousarray(a)) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.nodes_k,
                                                               node, st)]
            assert _code(lambda: e.unplace_tl_device(*dev, kmax)) == INVAL, what
            assert e.read_timeline().tobytes() == before.tobytes(), what
        for k in (0, -1, 9):
            assert _code(lambda: e.unplace_tl(good, gnode, gstart, k)) == INVAL, k
        cols = [np.ascontiguousarray(a) for a in (good.cpu, good.mem, good.gpu, good.wall)]
        applied = C.c_int64(-1)
        for fn in (L_.fit_unplace_tl, L_.fit_unplace_tl_device):
            assert fn(e._h, 0, None, None, None, None, None, 1, None, None, None) == 0  # j == 0 whatever the pointers
            assert fn(e._h, 0, None, None, None, None, None, 1, None, None, C.byref(applied)) == 0 and applied.value == 0
            assert fn(e._h, -1, None, None, None, None, None, 1, None, None, None) == INVAL
            assert fn(e._h, 5, None, None, None, None, None, 1, None, None, None) == INVAL
        assert L_.fit_unplace_tl(e._h, 5, *[p(c) for c in cols], None, kmax, None, p(gstart), None) == INVAL  # NULL nodes
        assert L_.fit_unplace_tl(e._h, 5, *[p(c) for c in cols], None, kmax, p(gnode), None, None) == INVAL  # NULL starts
        assert e.read_timeline().tobytes() == before.tobytes()
        # the good batch alone is exact, applied NULL and nodes_k NULL (= all 1) included
        want, wapplied = uc.ref_unplace_tl(before, good, gnode, gstart, L, kmax)
        assert e.unplace_tl(good, gnode, gstart, kmax) == wapplied == 7
        assert np.array_equal(e.read_timeline(), want)
        all1 = pk.ones(good)
        want1, _ = uc.ref_unplace_tl(want, all1, gnode, gstart, L, kmax)
        assert L_.fit_unplace_tl(e._h, 5, *[p(c) for c in cols], None, kmax, p(gnode), p(gstart), None) == 0
        assert np.array_equal(e.read_timeline(), want1)
        assert L_.fit_unplace_tl_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.unplace_tl(good, gnode, gstart, kmax)) == STATE
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        load(e, nodes, tline, parts)
        assert _code(lambda: e.unplace_tl(good, gnode, gstart, kmax)) == STATE


# ---- 9. the launch seam ------------------------------------------------------------------------------------
def test_chunk_seam(engine, monkeypatch):
    """FIT_UTL_CHUNK (test-only, read at call time) cuts a 50-row call into launch sequences of 7 rows;
    node 2 has windows in every one of them."""
    e = engine
    n, H, kmax = 12, 64, 3
    r = np.random.default_rng(9)
    node = np.full((50, kmax), -1, np.int32)
    k = r.integers(1, kmax + 1, 50).astype(np.uint16)
    for q in range(50):
        node[q, :k[q]] = r.choice(np.delete(np.arange(n), 2), k[q], replace=False)
        if q % 3 == 0 or q == 49:
            node[q, 0] = 2
    start = r.integers(0, H, 50).astype(np.int32)
    start[1::10] = -1  # skipped rows between the live ones
    jobs = synth.Jobs(r.integers(0, 9, 50).astype(np.int32), r.integers(0, 99, 50).astype(np.int32),
                      r.integers(0, 2, 50).astype(np.int32), r.integers(0, 3 * H, 50).astype(np.int32),
                      np.zeros(50, np.uint16), k)
    assert all((node[a:a + 7, 0] == 2).any() for a in range(0, 50, 7)) and (start < 0).any()
    got = []
    for chunk in (None, "7", "1"):
        if chunk:
            monkeypatch.setenv("FIT_UTL_CHUNK", chunk)
        load(e, uc.flat_cluster(n), uc.no_events(n, H, 2), wk.open_parts(1))
        tl0 = e.read_timeline()
        applied = e.unplace_tl(jobs, node, start, kmax)
        got.append((applied, e.read_timeline()))
    want, wapplied = uc.ref_unplace_tl(tl0, jobs, node, start, 2, kmax)
    for applied, tl in got:
        assert applied == wapplied and np.array_equal(tl, want)


# ---- 10. the device entry point ----------------------------------------------------------------------------
def test_device_entry(engine):
    e = engine
    H, kmax = 64, 8
    jobs, wnodes, wstart, wfin = uc.reference(H, kmax)
    rows = uc.half(H, kmax)
    fresh_random(e, H)
    e.place_tl_k(jobs, kmax)
    sub = uc.take(jobs, rows)
    host_applied = e.unplace_tl(sub, wnodes[rows], wstart[rows], kmax)
    host = e.read_timeline()
    fresh_random(e, H)
    e.place_tl_k(jobs, kmax)
    dev = [DevArray(np.ascontiguousarray(a)) for a in (sub.cpu, sub.mem, sub.gpu, sub.wall, sub.nodes_k,
                                                       wnodes[rows], wstart[rows])]
    assert e.unplace_tl_device(*dev, kmax) == host_applied
    assert e.read_timeline().tobytes() == host.tobytes()
    assert e.unplace_tl_ms() > 0
    # nodes_k NULL on device columns: every row one node
    fresh_random(e, H)
    one = pk.ones(sub)
    want, _ = uc.ref_unplace_tl(pk.start_timeline(H), one, wnodes[rows], wstart[rows], pk.SLOT_MIN, kmax)
    dev[4] = None
    assert e.unplace_tl_device(*dev, kmax) == len(rows)
    assert np.array_equal(e.read_timeline(), want)

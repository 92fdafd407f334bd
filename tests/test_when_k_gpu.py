"""fit_when_k on the GPU against a numpy restatement of DESIGN.md §2f (_when_k_cases.ref_when_k, over
the dense [n, H, 3] timeline): the hand case, exact rows and node lists on shapes that cross every
wave, workgroup, slice and run-batch edge of the kernels after reservations, need == 1 = fit_when,
a flat timeline = fit_place, edges, read-only, state and argument errors.  Every case runs through
the host and the device entry point and rows and nodes must be identical."""
import ctypes as C

import numpy as np
import pytest

import _when_k_cases as wk
import fitgpu
from _devarray import DevArray
from fitgpu import (ETA_K_DTYPE, FIT_ETA_HORIZON, FIT_ETA_LATER, FIT_ETA_NOW, FIT_ETA_PARTITION, FIT_ETA_LIMIT_TIME,
                    FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM, Engine, FitError, _lib, synth)

pytestmark = pytest.mark.gpu

REJECT_CODES = (FIT_ETA_PARTITION, FIT_ETA_LIMIT_TIME, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM)


def when_k_both(e, jobs, kmax, null_k=False):
    """Engine.when_k through host pointers and through device pointers: the same rows and nodes.
    null_k: nodes_k passed as NULL (= all 1) to both."""
    if null_k:
        cols = [np.ascontiguousarray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")]
        rows = np.zeros(jobs.j, ETA_K_DTYPE)
        nodes = np.full((jobs.j, kmax), -7, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        rc = _lib.lib().fit_when_k(e._h, jobs.j, *[p(c) for c in cols], None, kmax, p(rows), p(nodes))
        assert rc == 0, rc
    else:
        rows, nodes = e.when_k(jobs, kmax)
    cols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")]
    dk = None if null_k else DevArray(jobs.nodes_k)
    out = DevArray(np.full(jobs.j * 10, -7, np.int32).view(ETA_K_DTYPE))
    dn = DevArray(np.full((jobs.j, kmax), -7, np.int32))
    ms = e.when_k_device(*cols, dk, out, dn, kmax)
    assert ms > 0
    assert np.array_equal(rows, out.numpy()), "host and device entry points differ (rows)"
    assert np.array_equal(nodes, dn.numpy()), "host and device entry points differ (nodes)"
    return rows, nodes


def assert_same(got, want):
    (rows, nodes), (wrows, wnodes) = got, want
    for f in ETA_K_DTYPE.names:
        bad = np.flatnonzero(rows[f] != wrows[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {rows[bad[0]]}, want {wrows[bad[0]]}"
    bad = np.flatnonzero((nodes != wnodes).any(axis=1))
    assert bad.size == 0, f"nodes: {bad.size} jobs differ, first {bad[0]}: got {nodes[bad[0]]}, " \
                          f"want {wnodes[bad[0]]}, row {rows[bad[0]]}"


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


# ---- 1. the hand case -----------------------------------------------------------------------------
def test_hand_case(engine):
    nodes, tline, jobs, parts = wk.hand_case()
    load(engine, nodes, tline, parts)
    got = when_k_both(engine, jobs, 3)
    assert_same(got, (wk.HAND_ROWS, wk.HAND_NODES))  # the rows worked out by hand in _when_k_cases.py
    assert_same(got, wk.ref_when_k(engine.read_timeline(), nodes.part_mask, parts, jobs, tline.slot_min, 3))
    # j0 is the case that rules out combining per-node earliest starts: they are 0, 3 and 5, the 2nd
    # smallest is 3, and no two nodes are free together before slot 5
    assert got[0]["start"][0] == 5 and got[1][0].tolist() == [1, 2, -1]
    eta = engine.when(jobs)  # j1, need 1: fit_when's row
    assert (eta["start"][1], eta["node"][1]) == (got[0]["start"][1], got[1][1, 0]) == (0, 0)
    assert fitgpu.when_k_message(got[0][0]) == \
        "earliest start in 25 min (slot 5) on 2 of 2/3 nodes, 1 free now"
    assert fitgpu.when_k_message(got[0][3]) == "can start now on 2 of 2/3 nodes"
    assert fitgpu.when_k_message(got[0][2]) == "no start inside the horizon for 3 nodes at once: 3/3 nodes can run it"


# ---- 2. random timelines against the restatement ----------------------------------------------------
# (H, jobs, kmax): horizons 1, 8, 64, 1,024 (one to sixteen 64-slot steps of the prefix sum, a
# partial last step); 1, 64, 65 and 300 jobs (300: several chunks of 4 in the pick kernel, more
# than 256 jobs on more than one component); kmax 1, 3, 8.  The cluster's components have 1, 63, 64,
# 65 and 600 nodes: below, at and above a wave, and more than one 256-thread pass or slice.
RANDOM = [(1, 1, 1), (8, 64, 3), (64, 65, 8), (1024, 300, 8), (1024, 64, 1), (8, 300, 3), (64, 1, 8)]


@pytest.mark.parametrize("H,j,kmax", RANDOM)
def test_exact_rows_and_nodes_after_reservations(engine, H, j, kmax):
    slot_min = 5
    nodes, tline, parts = wk.rand_cluster(H, slot_min, 7000 + H)
    jobs = wk.rand_jobs(j, H, slot_min, kmax, 31 * H + 7 * j + kmax)
    load(engine, nodes, tline, parts)
    if H >= 8:  # reservations: run lists grow past what release events alone give, with dips
        _, _, st = engine.place_tl(wk.rand_jobs(300, H, slot_min, 1, 99 + H, valid_only=True))
        assert st["placed"] > 50
    dense = engine.read_timeline()
    if H == 1024:  # every run-list length the walks distinguish: header only, its edge, the 4-run loads' edges
        rc = wk.run_counts(dense[nodes.part_mask != 0])
        assert {1, 4, 5, 8, 9} <= set(rc.tolist()) and rc.max() >= 13, sorted(set(rc.tolist()))
    got = when_k_both(engine, jobs, kmax)
    want = wk.ref_when_k(dense, nodes.part_mask, parts, jobs, slot_min, kmax)
    assert_same(got, want)
    if j == 300 and H == 1024:
        assert set(np.unique(got[0]["code"]).tolist()) == set(range(8)), np.unique(got[0]["code"])
        multi = got[0]["need"] > 1
        assert (got[0]["code"][multi] == FIT_ETA_LATER).any() and (got[0]["code"][multi] == FIT_ETA_NOW).any()


# ---- 3. need == 1 is fit_when -------------------------------------------------------------------------
def test_need_one_equals_when():
    nodes, tline, jobs, parts = synth.make_c5(500, 1500)
    _, _, probe, _ = synth.make_c5(500, 300, shard=9)
    with Engine(device=0) as e:
        load(e, nodes, tline, parts)
        e.place_tl(jobs)
        eta = e.when(probe)
        ones, ones_nodes = when_k_both(e, probe, 1)
        null, null_nodes = when_k_both(e, probe, 1, null_k=True)
    assert np.array_equal(ones, null) and np.array_equal(ones_nodes, null_nodes)
    for f in ("code", "dur", "start", "wait_min", "members", "hosts", "now"):
        assert np.array_equal(ones[f], eta[f]), f
    assert np.array_equal(ones_nodes[:, 0], eta["node"])
    assert (eta["code"] == FIT_ETA_LATER).any() and (eta["code"] == FIT_ETA_NOW).any()


# ---- 4. on a flat timeline the nodes are fit_place's ----------------------------------------------------
def test_flat_timeline_agrees_with_place():
    """No releases, avail_min = INT32_MAX, every wall <= H * L: a NOW row lists the nodes, in order,
    that fit_place of that job alone with its nodes_k returns on the same table; a job fit_place
    leaves unplaced is HORIZON; a rejected one has a limit code."""
    nodes, jobs, parts = synth.make_config("c4", 600, 48)
    nodes.avail_min[:] = synth.INT32_MAX
    H, L = 1024, 5
    assert jobs.wall.max() <= H * L and jobs.nodes_k.max() == 8
    flat = synth.Timeline(H, L, np.zeros(nodes.n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    with Engine(device=0) as e:
        load(e, nodes, flat, parts)
        rows, got = when_k_both(e, jobs, 8)
    placed = np.empty((jobs.j, 8), np.int32)
    with Engine(device=0) as e:
        for q in range(jobs.j):
            e.load_nodes(nodes)  # alone: the table as loaded
            e.load_partitions(parts)
            placed[q] = e.place(wk.one_job(jobs, q), kmax=8)[0][0]
    assert not (rows["code"] == FIT_ETA_LATER).any()
    for q in range(jobs.j):
        if placed[q, 0] == fitgpu.FIT_REJECTED:
            assert rows["code"][q] in REJECT_CODES, (q, rows[q])
        elif placed[q, 0] == fitgpu.FIT_UNPLACED:
            assert rows["code"][q] == FIT_ETA_HORIZON, (q, rows[q])
        else:
            assert rows["code"][q] == FIT_ETA_NOW and np.array_equal(got[q], placed[q]), (q, rows[q], got[q], placed[q])
    assert (rows["code"] == FIT_ETA_NOW).sum() >= 8 and (rows["need"][rows["code"] == FIT_ETA_NOW] > 1).any()


# ---- 5. edges ----------------------------------------------------------------------------------------------
def test_edges(engine):
    nodes, tline, jobs, parts = wk.edge_case()
    load(engine, nodes, tline, parts)
    got = when_k_both(engine, jobs, 8)
    assert_same(got, (wk.EDGE_ROWS, wk.EDGE_NODES))
    assert_same(got, wk.ref_when_k(engine.read_timeline(), nodes.part_mask, parts, jobs, tline.slot_min, 8))


# ---- 6. read-only --------------------------------------------------------------------------------------
def test_read_only():
    nodes, tline, jobs, parts = synth.make_c5(300, 600)
    first, second = (synth.Jobs(*(getattr(jobs, f)[s] for f in wk.JOB_FIELDS)) for s in (slice(0, 300), slice(300, 600)))
    probe = wk.rand_jobs(200, tline.slots, tline.slot_min, 8, 5)
    probe.part[:] = probe.part % 16
    outs = []
    for query in (True, False):
        with Engine(device=0) as e:
            load(e, nodes, tline, parts)
            e.place_tl(first)
            before = (e.read_timeline(), e.read_nodes())
            if query:
                rows, _ = when_k_both(e, probe, 8)
                assert np.isin(rows["code"], (FIT_ETA_NOW, FIT_ETA_LATER)).sum() > 20
            after = (e.read_timeline(), e.read_nodes())
            assert before[0].tobytes() == after[0].tobytes(), "when_k changed the timeline"
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1])), "when_k changed the nodes"
            node, start, _ = e.place_tl(second)
            outs.append((node.copy(), start.copy(), e.read_timeline()))
    assert all(np.array_equal(a, b) for a, b in zip(*outs)), "a place_tl after when_k differs"


# ---- 7. state and argument errors --------------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_state_and_argument_errors():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    jobs.nodes_k[:] = np.arange(16) % 4
    L = _lib.lib()
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    none = (None,) * 6
    with Engine(device=0) as e:
        assert _code(lambda: e.when_k(jobs)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.when_k(jobs)) == STATE  # no timeline loaded
        ms = C.c_double()
        assert L.fit_when_k_ms(e._h, C.byref(ms)) == STATE  # before any device call
        e.load_timeline(tline)
        want = e.when_k(jobs, 3)
        assert len(want[0]) == 16 and want[1].shape == (16, 3)
        assert L.fit_when_k_ms(e._h, C.byref(ms)) == STATE  # the host entry point does not count
        for fn in (L.fit_when_k, L.fit_when_k_device):
            assert fn(e._h, 0, *none, 1, None, None) == 0  # j == 0 whatever the pointers are
            assert fn(e._h, 1, *none, 1, None, None) == INVAL
            assert fn(e._h, -1, *none, 1, None, None) == INVAL
        for kmax in (0, -1, 9):
            assert _code(lambda: e.when_k(jobs, kmax)) == INVAL, kmax
        assert _code(lambda: e.when_k(jobs, 2)) == INVAL  # a job of 3 nodes, kmax 2
        for f in ("cpu", "mem", "gpu", "wall"):
            bad = synth.Jobs(*(getattr(jobs, g).copy() for g in wk.JOB_FIELDS))
            getattr(bad, f)[5] = -1
            assert _code(lambda: e.when_k(bad, 3)) == INVAL, f
            got = e.when_k(jobs, 3)  # the context is usable afterwards
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        cols = [np.ascontiguousarray(getattr(jobs, f)) for f in wk.JOB_FIELDS]
        rows, nd = np.zeros(16, ETA_K_DTYPE), np.zeros((16, 3), np.int32)
        assert L.fit_when_k(e._h, 16, *[p(c) for c in cols], 3, None, p(nd)) == INVAL  # NULL rows
        assert L.fit_when_k(e._h, 16, *[p(c) for c in cols], 3, p(rows), None) == INVAL  # NULL nodes
        when_k_both(e, jobs, 3)
        assert L.fit_when_k_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        assert len(e.when(jobs)) == 16  # fit_when is unchanged next to it
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.when_k(jobs, 3)) == STATE

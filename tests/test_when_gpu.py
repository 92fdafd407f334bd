"""fit_when on the GPU against a numpy restatement of DESIGN.md §2d (_when_cases.ref_when, over the dense
[n, H, 3] timeline): exact rows on shapes that cross every wave, tile, slice and run-batch edge of
k_when_walk, after reservations, "alone" = fit_place_tl alone, state and argument errors.  Every
case runs through the host and the device entry point and the rows must be identical."""
import ctypes as C

import numpy as np
import pytest

import _tl_cases
import fitgpu
from _devarray import DevArray
from _when_cases import ref_when
from fitgpu import (ETA_DTYPE, FIT_ETA_HORIZON, FIT_ETA_LATER, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM,
                    FIT_ETA_LIMIT_TIME, FIT_ETA_NOW, FIT_ETA_PARTITION, Engine, FitError, _lib, synth)
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INF = synth.INT32_MAX
JOB_FIELDS = ("cpu", "mem", "gpu", "wall", "part", "nodes_k")
REJECT_CODES = (FIT_ETA_PARTITION, FIT_ETA_LIMIT_TIME, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM)


def when_both(e, jobs):
    """Engine.when through host pointers and through device pointers: the same rows."""
    host = e.when(jobs)
    cols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")]
    out = DevArray(np.full(jobs.j, -7, np.int32).repeat(8).view(ETA_DTYPE))
    ms = e.when_device(*cols, out)
    assert ms > 0
    assert np.array_equal(host, out.numpy()), "host and device entry points differ"
    return host


def assert_rows(got, want):
    for f in ETA_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def one_job(jobs, q):
    return synth.Jobs(*(getattr(jobs, f)[q:q + 1] for f in JOB_FIELDS))


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


# ---- 1. the hand case -----------------------------------------------------------------------------
def test_hand_case(engine):
    nodes, tline, jobs, parts = _tl_cases.hand_case()
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    engine.load_timeline(tline)
    got = when_both(engine, jobs)
    # (code, dur, start, node, wait_min, members, hosts, now), worked out from tests/_tl_cases.py:
    # n0 holds (4, 4096) on slots 0-2 and (8, 8192) from 3 on, n1 (2, 2048) on slots 0-4, n2 is
    # partition 1.  No job has been placed, so every job sees the built timeline.
    want = np.array([
        (FIT_ETA_NOW, 3, 0, 1, 0, 2, 2, 2),        # j0: both at 0, n1 the tighter fit
        (FIT_ETA_NOW, 6, 0, 0, 0, 2, 1, 1),        # j1: n1 has 5 usable slots
        (FIT_ETA_NOW, 1, 0, 1, 0, 2, 2, 2),        # j2: alone it starts now (placed third it waits)
        (FIT_ETA_NOW, 2, 0, 2, 0, 1, 1, 1),        # j3: partition 1 is n2
        (FIT_ETA_HORIZON, 1, -1, -1, -1, 2, 0, 0),  # j4: 16 cpus, nothing that large
        (FIT_ETA_HORIZON, 10, -1, -1, -1, 2, 0, 0),  # j5: 10 slots > 8
        (FIT_ETA_PARTITION, 1, -1, -1, -1, 0, 0, 0),  # j6: partition 5 of 2
    ], ETA_DTYPE)
    assert_rows(got, want)
    dense = po.ref_build_timeline(nodes, tline)
    assert_rows(got, ref_when(dense, nodes.part_mask, parts, jobs, tline.slot_min))
    for q in range(jobs.j):  # the oracle's sequential backfill of this one job on the built timeline
        rn, rs, _, _ = po.ref_place_tl(nodes, tline, one_job(jobs, q), parts, tl=dense)
        if rn[0] >= 0:
            assert (got["node"][q], got["start"][q]) == (rn[0], rs[0]), q
        else:
            assert got["node"][q] == -1 and got["start"][q] == -1, q
            assert (rn[0] == fitgpu.FIT_REJECTED) == (got["code"][q] in REJECT_CODES), q
    assert fitgpu.when_message(got[4]) == "no start inside the horizon on any of 2 nodes"
    assert fitgpu.when_message(got[0]) == "can start now on 2/2 nodes"

    # a job that must wait: 6 cpus fit only n0 once its running job has ended at slot 3
    late = synth.Jobs(np.array([6], np.int32), np.array([1024], np.int32), np.zeros(1, np.int32),
                      np.array([30], np.int32), np.zeros(1, np.uint16), np.ones(1, np.uint16))
    got = when_both(engine, late)
    assert tuple(got[0]) == (FIT_ETA_LATER, 3, 3, 0, 30, 2, 1, 0)
    assert fitgpu.when_message(got[0]) == \
        "earliest start in 30 min (slot 3): 1/2 nodes can run it inside the horizon, none now"


# ---- 2. awkward shapes against the restatement -------------------------------------------------------
# 4 partitions are declared: 0 limits the walltime, 1 the cpus and the memory, 2 nothing, 3 has no
# node at all; jobs also name partitions 4 and 5 (>= P).  Nodes sit in partition 0, 1, both (so
# that component holds two partitions and the mask test matters), 2 (a second component) or none.
def hand_parts(H, slot_min):
    return synth.Partitions(np.array([H * slot_min // 2 + 1, -1, -1, -1], np.int32),
                            np.array([-1, 16, -1, -1], np.int32), np.array([-1, 30000, -1, -1], np.int32))


RUN_TARGETS = (1, 4, 5, 8, 9, 33, 40)


def hand_cluster(n, H, slot_min, seed):
    """Nodes and release events whose run counts per node (runs of equal free resources, the list
    the kernel walks) include 1, 4, 5, 8, 9 and >= 33 where the horizon has room for them: header
    only, the first slab batch, the edges of the four-run loads, long walks."""
    r = np.random.default_rng(seed)
    mask = (1 << r.integers(0, 3, n)).astype(np.uint32)
    mask[(r.random(n) < 0.2) & (mask != 4)] = 3  # in partitions 0 and 1: components {0, 1} and {2}
    if n > 4:
        mask[r.random(n) < 0.1] = 0  # drained: in no partition
    cpu = r.integers(0, 33, n).astype(np.int32)
    mem = (cpu.astype(np.int64) * r.choice([500, 2048, 4096], n)).astype(np.int32)
    gpu = r.choice([0, 0, 2, 4], n).astype(np.int32)
    # avail_min cuts the horizon on a third of the nodes (0: never usable; H * slot_min: no cut)
    avail = np.where(r.random(n) < 0.33, r.integers(0, H * slot_min + 1, n), INF).astype(np.int32)
    off, slot, rc, rm, rg = [0], [], [], [], []
    for x in range(n):
        u = min(int(avail[x]) // slot_min, H)  # usable slots
        tail = 1 if u < H else 0               # the unusable tail is a run of its own
        want = RUN_TARGETS[x % len(RUN_TARGETS)] if r.random() < 0.7 else int(r.integers(1, 13))
        k = max(0, min(want - 1 - tail, u - 1))  # k releases at distinct slots in [1, u): k + 1 runs
        for s in sorted(r.choice(np.arange(1, max(u, 2)), k, replace=False).tolist() if k else []):
            slot.append(s)
            rc.append(int(r.integers(1, 5)))
            rm.append(int(r.integers(0, 3)) * 1024)
            rg.append(int(r.integers(0, 2)))
        off.append(len(slot))
    a = lambda v: np.array(v, np.int32)  # noqa: E731
    return (synth.Nodes(cpu, mem, gpu, avail, mask),
            synth.Timeline(slots=H, slot_min=slot_min, off=a(off), slot=a(slot), cpu=a(rc), mem=a(rm), gpu=a(rg)))


def hand_jobs(j, H, slot_min, seed):
    r = np.random.default_rng(seed)
    cpu = r.choice([0, 1, 2, 4, 8, 16, 24, 40], j).astype(np.int32)
    mem = (np.maximum(cpu, 1).astype(np.int64) * r.choice([500, 1024, 4096], j)).astype(np.int32)
    gpu = r.choice([0, 0, 0, 1, 2, 4], j).astype(np.int32)
    # wall 0 (d = 1), d == H, d == H + 1, and anything between
    wall = r.choice([0, 1, slot_min, H * slot_min, H * slot_min + 1, -1], j)
    wall = np.where(wall < 0, r.integers(0, H * slot_min + 1, j), wall).astype(np.int32)
    return synth.Jobs(cpu, mem, gpu, wall, r.integers(0, 6, j).astype(np.uint16), np.ones(j, np.uint16))


def run_counts(dense):
    return 1 + (dense[:, 1:, :] != dense[:, :-1, :]).any(axis=2).sum(axis=1)


SHAPES = [(1, 1, 1), (1, 65, 8), (7, 63, 8), (7, 257, 1), (513, 64, 1024), (513, 257, 8), (513, 257, 1024),
          (3001, 1, 1024), (3001, 65, 1024), (3001, 257, 8), (3001, 64, 1)]


@pytest.mark.parametrize("n,j,H", SHAPES)
def test_exact_rows_awkward_shapes(engine, n, j, H):
    slot_min = 5
    nodes, tline = hand_cluster(n, H, slot_min, 1000 + n + H)
    parts = hand_parts(H, slot_min)
    jobs = hand_jobs(j, H, slot_min, 17 * n + 3 * j + H)
    dense = po.ref_build_timeline(nodes, tline)
    if n >= 513 and H == 1024:  # the generator reaches every run-list length the walk distinguishes
        rc = run_counts(dense[nodes.part_mask != 0])
        assert {1, 4, 5, 8, 9} <= set(rc.tolist()) and rc.max() >= 33, sorted(set(rc.tolist()))
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    engine.load_timeline(tline)
    got = when_both(engine, jobs)
    assert_rows(got, ref_when(dense, nodes.part_mask, parts, jobs, slot_min))
    if n >= 513 and j >= 257:
        assert set(np.unique(got["code"]).tolist()) == set(range(8)), np.unique(got["code"])


@pytest.mark.parametrize("j", [64, 256])
def test_exact_rows_mixed_components_in_caller_order(engine, j):
    """c3: 16 disjoint partitions, 16 components; up to 256 jobs keep the caller's order, so the
    lanes of one wave name many components and the wave walks them one after the other.  H = 64,
    up to five releases per node."""
    H, slot_min = 64, 30
    nodes, jobs, parts = synth.make_config("c3", 1000, j)
    assert len(np.unique(nodes.part_mask)) == 16 and len(np.unique(jobs.part[:64])) >= 8
    r = np.random.default_rng(64 + j)
    k = r.integers(0, 6, nodes.n)
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    slot = np.concatenate([np.sort(r.choice(np.arange(1, H), m, replace=False)) for m in k]).astype(np.int32)
    m = len(slot)
    tline = synth.Timeline(slots=H, slot_min=slot_min, off=off, slot=slot, cpu=r.integers(1, 9, m).astype(np.int32),
                           mem=(r.integers(0, 5, m) * 4096).astype(np.int32), gpu=r.integers(0, 2, m).astype(np.int32))
    dense = po.ref_build_timeline(nodes, tline)
    want = ref_when(dense, nodes.part_mask, parts, jobs, slot_min)
    assert len(np.unique(want["members"][want["members"] > 0])) >= 8  # not vacuous: the components differ in size
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    engine.load_timeline(tline)
    assert_rows(when_both(engine, jobs), want)


def test_largest_slot_min(engine):
    """The widest slot that still leaves 1,024 usable slots below avail_min = INT32_MAX: wait_min
    and dur near the top of int32 (wall + slot_min - 1 does not fit 32 bits).  start * slot_min
    itself cannot pass INT32_MAX — a start lies below avail_min / slot_min — so the saturation of
    wait_min has no reachable case to test."""
    sm = INF // 1024
    nodes = synth.Nodes(np.array([1], np.int32), np.array([1024], np.int32), np.zeros(1, np.int32),
                        np.array([INF], np.int32), np.ones(1, np.uint32))
    tline = synth.Timeline(slots=1024, slot_min=sm, off=np.array([0, 1], np.int32),
                           slot=np.array([1023], np.int32), cpu=np.array([4], np.int32),
                           mem=np.zeros(1, np.int32), gpu=np.zeros(1, np.int32))
    parts = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
    jobs = synth.Jobs(np.array([2, 1], np.int32), np.array([1, 1], np.int32), np.zeros(2, np.int32),
                      np.array([1, INF], np.int32), np.zeros(2, np.uint16), np.ones(2, np.uint16))
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    engine.load_timeline(tline)
    got = when_both(engine, jobs)
    assert tuple(got[0]) == (FIT_ETA_LATER, 1, 1023, 0, 1023 * sm, 1, 1, 0) and 1023 * sm > 2**31 - 2**22
    assert tuple(got[1]) == (FIT_ETA_HORIZON, 1025, -1, -1, -1, 1, 0, 0)
    assert_rows(got, ref_when(po.ref_build_timeline(nodes, tline), nodes.part_mask, parts, jobs, sm))


# ---- 3. after reservations, and 4. alone means place_tl alone --------------------------------------
@pytest.fixture(scope="module")
def reserved():
    """~500 nodes after a place_tl of ~2,000 jobs (run lists grown past the header, some moved):
    the dense state, and `when` of a fresh job sample against it, with read-backs around it."""
    nodes, tline, jobs, parts = synth.make_c5(500, 2000)
    _, _, probe, _ = synth.make_c5(500, 300, shard=9)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        _, _, st = e.place_tl(jobs)
        assert st["placed"] > 1000
        before = (e.read_timeline(), e.read_nodes())
        got = when_both(e, probe)
        after = (e.read_timeline(), e.read_nodes())
    return nodes, tline, parts, probe, got, before, after


def test_after_reservations(reserved):
    nodes, tline, parts, probe, got, before, after = reserved
    assert before[0].tobytes() == after[0].tobytes(), "when changed the timeline"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1])), "when changed the node table"
    dense = before[0]
    built = po.ref_build_timeline(nodes, tline)
    m = nodes.part_mask != 0
    assert (dense[m] != built[m]).any() and run_counts(dense[m]).max() > run_counts(built[m]).max()
    assert_rows(got, ref_when(dense, nodes.part_mask, parts, probe, tline.slot_min))
    assert (got["code"] == FIT_ETA_NOW).any() and (got["code"] == FIT_ETA_LATER).any()
    # the oracle's sequential backfill of each job alone on the same dense state
    for q in range(probe.j):
        rn, rs, _, _ = po.ref_place_tl(nodes, tline, one_job(probe, q), parts, tl=dense)
        if rn[0] >= 0:
            assert (got["node"][q], got["start"][q]) == (rn[0], rs[0]), (q, got[q])
        else:
            assert (rn[0] == fitgpu.FIT_REJECTED) == (got["code"][q] in REJECT_CODES), (q, got[q])
            assert got["code"][q] not in (FIT_ETA_NOW, FIT_ETA_LATER), (q, got[q])


@pytest.mark.auto_engine
def test_alone_means_place_tl_alone(reserved):
    """32 sampled NOW / LATER jobs: a fresh context brought to the same dense state — reservations
    leave dips that no release event can express, so it re-loads the nodes and the timeline and
    replays the same place_tl, and its read_timeline must equal the state `when` saw — then places
    just that job: (node, start) are the row's.  One context at a time."""
    nodes, tline, parts, probe, got, before, _ = reserved
    _, _, jobs, _ = synth.make_c5(500, 2000)
    cand = np.flatnonzero(np.isin(got["code"], (FIT_ETA_NOW, FIT_ETA_LATER)))
    later = cand[got["code"][cand] == FIT_ETA_LATER][:16]
    pick = np.concatenate([later, cand[got["code"][cand] == FIT_ETA_NOW][:32 - len(later)]])
    assert len(pick) == 32 and len(later) >= 4
    for q in pick.tolist():
        with Engine(device=0) as e:
            e.load_nodes(nodes)
            e.load_partitions(parts)
            e.load_timeline(tline)
            e.place_tl(jobs)
            assert e.read_timeline().tobytes() == before[0].tobytes()  # the same dense state
            node, start, st = e.place_tl(one_job(probe, q))
        assert (node[0], start[0]) == (got["node"][q], got["start"][q]), (q, got[q])


# ---- 5. state and argument errors ----------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_state_and_argument_errors():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    L = _lib.lib()
    with Engine(device=0) as e:
        assert _code(lambda: e.when(jobs)) == _lib.FIT_E_STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.when(jobs)) == _lib.FIT_E_STATE  # no timeline loaded
        ms = C.c_double()
        assert L.fit_when_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE  # before any device call
        e.load_timeline(tline)
        assert len(e.when(jobs)) == 16
        assert L.fit_when_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE  # the host entry point does not count
        assert L.fit_when(e._h, 0, None, None, None, None, None, None) == 0
        assert L.fit_when_device(e._h, 0, None, None, None, None, None, None) == 0
        assert L.fit_when(e._h, 1, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert L.fit_when(e._h, -1, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        want = e.when(jobs)
        for f in ("cpu", "mem", "gpu", "wall"):
            bad = synth.Jobs(*(getattr(jobs, g).copy() for g in JOB_FIELDS))
            getattr(bad, f)[5] = -1
            assert _code(lambda: e.when(bad)) == _lib.FIT_E_INVAL, f
            assert np.array_equal(e.when(jobs), want)  # the context is usable afterwards
        assert _code(lambda: e.explain(jobs)) == _lib.FIT_E_STATE  # fit_explain still refuses a timeline
        when_both(e, jobs)
        assert L.fit_when_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.when(jobs)) == _lib.FIT_E_STATE
        assert len(e.explain(jobs)) == 16
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        assert _code(lambda: e.when(jobs)) == _lib.FIT_E_STATE

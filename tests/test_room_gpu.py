"""fit_room on the GPU against a numpy int64 restatement of DESIGN.md §2e (ref_room below): exact rows
on shapes that cross every wave, tile and slice edge of k_room_count, the quotient's edge values,
the 64-bit sum, what fit_place confirms, fit_explain's counts, the admitter's view, state errors."""
import numpy as np
import pytest

import fitgpu
from _devarray import DevArray
from fitgpu import (FIT_ROOM_LIMIT_CPUS, FIT_ROOM_LIMIT_MEM, FIT_ROOM_LIMIT_TIME, FIT_ROOM_NO_NODES, FIT_ROOM_NONE,
                    FIT_ROOM_PARTITION, FIT_ROOM_SOME, FIT_ROOM_UNBOUNDED, ROOM_DTYPE, Admitter, Engine, FitError, _lib,
                    synth)
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INF = synth.INT32_MAX
REJECT_CODES = (FIT_ROOM_PARTITION, FIT_ROOM_LIMIT_TIME, FIT_ROOM_LIMIT_CPUS, FIT_ROOM_LIMIT_MEM)


def ref_room(cpu, mem, gpu, avail, mask, parts, jobs, stats=None):
    """DESIGN.md §2e over the raw columns, every job alone, J x N tables in int64.  stats: a dict
    that collects how many (job, node) pairs tie on the binding resource and how many jobs tie on
    the roomiest node."""
    P, J, N = parts.p, jobs.j, len(cpu)
    part = jobs.part.astype(np.int64)
    known = part < P
    pc = np.minimum(part, P - 1)
    code = np.zeros(J, np.int32)
    for c, lim, dem in ((FIT_ROOM_LIMIT_MEM, parts.max_mem_per_node, jobs.mem),  # last to first: the
                        (FIT_ROOM_LIMIT_CPUS, parts.max_cpus_per_node, jobs.cpu),  # first match wins
                        (FIT_ROOM_LIMIT_TIME, parts.max_time_min, jobs.wall)):
        code[known & (lim[pc] >= 0) & (dem > lim[pc])] = c
    code[~known] = FIT_ROOM_PARTITION
    live = (code == 0)[:, None]
    member = live & (((mask[None, :].astype(np.int64) >> pc[:, None]) & 1) != 0)
    free = [np.asarray(c, np.int64)[None, :] for c in (gpu, cpu, mem)]  # §2's score order
    dem = [np.asarray(d, np.int64)[:, None] for d in (jobs.gpu, jobs.cpu, jobs.mem)]
    feas = member & (np.asarray(avail, np.int64)[None, :] >= jobs.wall.astype(np.int64)[:, None])
    for f, d in zip(free, dem):
        feas &= f >= d
    quot = [np.where(d > 0, f // np.maximum(d, 1), FIT_ROOM_UNBOUNDED) for f, d in zip(free, dem)]
    per = np.where(feas, np.minimum(np.minimum(quot[0], quot[1]), quot[2]), 0)
    attains = [feas & (d > 0) & (q == per) for q, d in zip(quot, dem)]
    by_gpu = attains[0]
    by_cpu = attains[1] & ~by_gpu
    by_mem = attains[2] & ~by_gpu & ~by_cpu
    out = np.zeros(J, ROOM_DTYPE)
    out["members"] = member.sum(1)
    out["nodes"] = feas.sum(1)
    out["copies"] = per.sum(1)
    best = per.max(1) if N else np.zeros(J, np.int64)
    out["best"] = best
    out["best_node"] = np.where(best > 0, (per == best[:, None]).argmax(1), -1)  # argmax: the first, lowest id
    out["by_gpu"], out["by_cpu"], out["by_mem"] = by_gpu.sum(1), by_cpu.sum(1), by_mem.sum(1)
    lv = live[:, 0]
    code[lv & (out["members"] == 0)] = FIT_ROOM_NO_NODES
    code[lv & (out["members"] > 0) & (out["copies"] == 0)] = FIT_ROOM_NONE
    out["code"] = code
    rej = ~lv
    assert not out["members"][rej].any()  # a rejected job has no member, so every count is 0
    out["best_node"][rej] = -1
    if stats is not None:
        stats["bind_ties"] = stats.get("bind_ties", 0) + int(((attains[0].astype(int) + attains[1] + attains[2]) > 1).sum())
        stats["node_ties"] = stats.get("node_ties", 0) + int((((per == best[:, None]).sum(1) > 1) & (best > 0)).sum())
    return out


def room_both(e, jobs):
    """Engine.room through host pointers and through device pointers: the same rows."""
    host = e.room(jobs)
    cols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")]
    out = DevArray(np.full(jobs.j * 5, -7, np.int64).view(ROOM_DTYPE))
    ms = e.room_device(*cols, out)
    assert ms > 0
    assert np.array_equal(host, out.numpy()), "host and device entry points differ"
    return host


def assert_rows(got, want):
    for f in ROOM_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- 1. exact rows on awkward shapes ------------------------------------------------------------
# 5 partitions are declared: 0 limits the walltime, 1 the cpus, 2 the memory, 3 nothing, 4 has no
# node at all; jobs also name partitions 5 and 6 (>= P).  Nodes sit in one partition of 0..3, in
# both of 0 and 1 or both of 2 and 3 (two components, each holding two partitions, so the
# in-component mask test matters and a long batch takes the component-ordered job list), or in none.
HAND_PARTS = synth.Partitions(np.array([500, -1, -1, -1, -1], np.int32), np.array([-1, 16, -1, -1, -1], np.int32),
                              np.array([-1, -1, 30000, -1, -1], np.int32))


def hand_nodes(n, seed):
    r = np.random.default_rng(seed)
    p = r.integers(0, 4, n)
    mask = (1 << p).astype(np.uint32)
    two = r.random(n) < 0.2
    mask[two] |= (1 << (p ^ 1)).astype(np.uint32)[two]
    mask[r.random(n) < 0.1] = 0  # drained: in no partition
    cpu = r.integers(0, 129, n).astype(np.int32)
    mem = (cpu.astype(np.int64) * r.choice([500, 2048, 4096], n)).astype(np.int32)
    gpu = r.choice([0, 0, 4, 8], n).astype(np.int32)
    for col in (cpu, mem, gpu):  # over-committed nodes: negative free values
        col[r.random(n) < 0.08] = -r.integers(1, 50)
    avail = np.where(r.random(n) < 0.3, r.integers(0, 3000, n), INF).astype(np.int32)
    if n == 1:
        mask[0], cpu[0], mem[0], gpu[0], avail[0] = 0b1100, 8, 16384, 2, 700
    return synth.Nodes(cpu, mem, gpu, avail, mask)


def hand_jobs(j, seed):
    r = np.random.default_rng(seed)
    cpu = r.choice([0, 1, 2, 3, 4, 8, 16, 32, 200], j).astype(np.int32)  # 200: more than any node has
    mem = (np.maximum(cpu, 1).astype(np.int64) * r.choice([0, 500, 1024, 4096], j)).astype(np.int32)
    gpu = r.choice([0, 0, 0, 1, 2, 4], j).astype(np.int32)
    wall = r.integers(0, 2881, j).astype(np.int32)
    return synth.Jobs(cpu, mem, gpu, wall, r.integers(0, 7, j).astype(np.uint16), np.ones(j, np.uint16))


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


@pytest.mark.parametrize("n", [1, 7, 63, 65, 2049])
def test_exact_rows_hand_tables(engine, n):
    nodes = hand_nodes(n, 100 + n)
    engine.load_nodes(nodes)
    engine.load_partitions(HAND_PARTS)
    seen, stats, by = set(), {}, np.zeros(3, np.int64)
    for j in (1, 64, 65, 257):
        jobs = hand_jobs(j, 7 * n + j)
        got = room_both(engine, jobs)
        want = ref_room(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask, HAND_PARTS,
                        jobs, stats)
        assert_rows(got, want)
        seen |= set(np.unique(want["code"]).tolist())
        by += [want["by_gpu"].sum(), want["by_cpu"].sum(), want["by_mem"].sum()]
    if n >= 63:  # the inputs reach every code, every binding resource and both kinds of tie
        assert seen == set(range(7)), seen
        assert (by > 0).all(), by
        assert stats["bind_ties"] > 0 and stats["node_ties"] > 0, stats


@pytest.mark.parametrize("j", [64, 256])
def test_exact_rows_mixed_components_in_caller_order(engine, j):
    """c3: 16 disjoint partitions, 16 components; up to 256 jobs keep the caller's order, so the
    lanes of one wave name many components and the wave walks them one after the other."""
    nodes, jobs, parts = synth.make_config("c3", 1000, j)
    assert len(np.unique(nodes.part_mask)) == 16 and len(np.unique(jobs.part[:64])) >= 8
    want = ref_room(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask, parts, jobs)
    assert len(np.unique(want["members"][want["members"] > 0])) >= 8  # not vacuous: the components differ in size
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    assert_rows(room_both(engine, jobs), want)


# ---- 2. quotient edges and the 64-bit sum -------------------------------------------------------
ONE_PART = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
EDGE_D = [1, 2, 3, 7, 2**30, 2**30 + 1, 2**31 - 1]


def test_quotient_edges(engine):
    """Every demand d of EDGE_D against free values d - 1, d, q*d - 1, q*d, q*d + 1 and 2^31 - 1, for
    q = 2, a middle q and the largest q with q*d < 2^31 — in each resource alone, in all three at
    once, and mixed with another demand — plus the all-zero demand."""
    top = 2**31 - 1
    free = {0, top}
    for d in EDGE_D:
        for q in {1, 2, max(top // d // 2, 1), top // d}:
            free |= {v for v in (d - 1, q * d - 1, q * d, q * d + 1) if 0 <= v <= top}
    free = np.array(sorted(free), np.int64)
    n = len(free)
    # node i offers free[i] cpus, free[n-1-i] MiB and free[(7 i) mod n] gpus (7 and n coprime or not:
    # every value still appears in every column often enough with the single-resource jobs below)
    nodes = synth.Nodes(free.astype(np.int32), free[::-1].astype(np.int32), free[(7 * np.arange(n)) % n].astype(np.int32),
                        np.full(n, INF, np.int32), np.ones(n, np.uint32))
    dem = [(0, 0, 0)]
    for d in EDGE_D:
        dem += [(d, 0, 0), (0, d, 0), (0, 0, d), (d, d, d), (d, 1, 0), (3, 0, d)]
    dem = np.array(dem, np.int32)
    j = len(dem)
    jobs = synth.Jobs(dem[:, 0].copy(), dem[:, 1].copy(), dem[:, 2].copy(), np.zeros(j, np.int32), np.zeros(j, np.uint16),
                      np.ones(j, np.uint16))
    engine.load_nodes(nodes)
    engine.load_partitions(ONE_PART)
    got = room_both(engine, jobs)
    want = ref_room(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask, ONE_PART, jobs)
    assert_rows(got, want)
    z = got[0]  # the all-zero demand: every node is feasible and unbounded
    assert (z["code"], z["nodes"], z["best"], z["best_node"]) == (FIT_ROOM_SOME, n, FIT_ROOM_UNBOUNDED, 0)
    assert z["copies"] == n * FIT_ROOM_UNBOUNDED and (z["by_gpu"], z["by_cpu"], z["by_mem"]) == (0, 0, 0)
    assert fitgpu.room_message(z) == f"no resource demand: unlimited room on {n}/{n} nodes"
    assert want["copies"][1] > 2**32  # demand (1, 0, 0): the cpu column's sum


@pytest.mark.parametrize("n", [3, 2049])
def test_copies_is_a_64_bit_sum(engine, n):
    """Three nodes with 2^31 - 1 free cpus against demand (1, 0, 0): copies = 3 (2^31 - 1) > 2^32.
    n = 3: one node per wave; n = 2049: the three lie in different slices of the node range, among
    nodes without a free cpu."""
    top = 2**31 - 1
    cpu = np.zeros(n, np.int32)
    cpu[[0, n // 2, n - 1]] = top
    nodes = synth.Nodes(cpu, np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32),
                        np.ones(n, np.uint32))
    jobs = synth.Jobs(np.ones(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32),
                      np.zeros(1, np.uint16), np.ones(1, np.uint16))
    engine.load_nodes(nodes)
    engine.load_partitions(ONE_PART)
    r = room_both(engine, jobs)[0]
    assert r["copies"] == 3 * top and r["copies"] > 2**32
    assert (r["code"], r["members"], r["nodes"], r["best"], r["best_node"]) == (FIT_ROOM_SOME, n, 3, top, 0)
    assert (r["by_gpu"], r["by_cpu"], r["by_mem"]) == (0, 3, 0)


# ---- 3. the engine confirms copies --------------------------------------------------------------
@pytest.mark.auto_engine
def test_place_of_copies_plus_three_places_copies():
    nodes, jobs, parts = synth.make_config("c3", 600, 4096)
    pick = np.arange(0, 4096, 4096 // 20)[:20]
    with Engine(device=0) as e:  # its own context: the engine choice is read when it is created
        e.load_nodes(nodes)
        e.load_partitions(parts)
        room = e.room(jobs)
        checked = 0
        for q in pick:
            r = room[q]
            if r["code"] in REJECT_CODES:
                continue
            m = int(r["copies"]) + 3
            assert m < 100000, r
            many = synth.Jobs(*(np.repeat(getattr(jobs, f)[q:q + 1], m) for f in ("cpu", "mem", "gpu", "wall", "part")),
                              np.ones(m, np.uint16))
            e.load_nodes(nodes)  # the same table for every job
            out, st = e.place(many)
            assert st["placed"] == r["copies"] and (out[:, 0] >= 0).sum() == r["copies"], (q, r, st)
            checked += 1
        assert checked >= len(pick) // 2, checked


# ---- 4. against fit_explain ---------------------------------------------------------------------
def test_members_and_nodes_are_fit_explains(engine):
    nodes, jobs, parts = synth.make_config("c3o", 777, 1025)
    jobs.nodes_k = np.ones(jobs.j, np.uint16)
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    room, why = room_both(engine, jobs), engine.explain(jobs)
    assert np.array_equal(room["members"], why["members"]) and np.array_equal(room["nodes"], why["fit"])
    early = np.isin(room["code"], (1, 2, 3, 4, 5)) | np.isin(why["code"], (1, 2, 3, 4, 5))
    assert early.any() and np.array_equal(room["code"][early], why["code"][early])  # FIT_ROOM_1..5 are FIT_WHY_1..5
    assert room["members"].max() == 777 and (room["nodes"] > 0).any()
    assert_rows(room, ref_room(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask, parts,
                               jobs))


# ---- 5. admitter --------------------------------------------------------------------------------
@pytest.mark.auto_engine
def test_admitter_room_sees_reservations():
    # node 1 has two GPUs left, nodes 0 and 2 none; one partition, no limits
    nodes = synth.Nodes(np.full(3, 64, np.int32), np.full(3, 65536, np.int32), np.array([0, 2, 0], np.int32),
                        np.full(3, INF, np.int32), np.ones(3, np.uint32))
    req = (0, 4, 1024, 1, 60, 0, 1)
    jobs = synth.Jobs(*(np.array([v], np.int32) for v in req[1:5]), np.zeros(1, np.uint16), np.ones(1, np.uint16))

    def view(r):
        return tuple(int(r[f]) for f in ("code", "members", "nodes", "best", "copies", "best_node", "by_gpu"))

    with Engine(device=0) as e, Engine(device=0) as plain:
        e.load_partitions(ONE_PART)
        plain.load_partitions(ONE_PART)
        with Admitter(e, max_batch=8, max_wait_us=0) as a:
            a.load_nodes(nodes)
            plain.load_nodes(nodes)
            r = a.room([req])[0]
            assert view(r) == (FIT_ROOM_SOME, 3, 1, 2, 2, 1, 1)
            assert np.array_equal(a.room([req]), plain.room(jobs))
            got, _, _, _, ticket = a.admit(*req)
            assert got == [1] and ticket > 0
            r = a.room([(5, *req[1:6], 7)])[0]  # one GPU of node 1 is reserved; priority and k are ignored
            assert view(r) == (FIT_ROOM_SOME, 3, 1, 1, 1, 1, 1)
            held = synth.Nodes(nodes.cpu_free - np.array([0, 4, 0], np.int32),
                               nodes.mem_free - np.array([0, 1024, 0], np.int32),
                               nodes.gpu_free - np.array([0, 1, 0], np.int32), nodes.avail_min, nodes.part_mask)
            plain.load_nodes(held)
            assert np.array_equal(a.room([req]), plain.room(jobs))
            a.release(ticket)
            assert view(a.room([req])[0]) == (FIT_ROOM_SOME, 3, 1, 2, 2, 1, 1)
            assert len(a.room([])) == 0
            with pytest.raises(FitError) as ei:
                a.room([(0, -1, 0, 0, 0, 0, 1)])
            assert ei.value.code == _lib.FIT_E_INVAL


# ---- 6. state and argument errors ---------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_state_and_argument_errors():
    import ctypes as C

    nodes, jobs, parts = synth.make_config("c2", 64, 16)
    L = _lib.lib()
    with Engine(device=0) as e:
        assert _code(lambda: e.room(jobs)) == _lib.FIT_E_STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        ms = C.c_double()
        assert L.fit_room_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE  # no fit_room_device yet
        assert len(e.room(jobs)) == 16
        assert L.fit_room_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE  # the host entry point is none
        assert L.fit_room(e._h, 0, None, None, None, None, None, None) == 0
        assert L.fit_room_device(e._h, 0, None, None, None, None, None, None) == 0
        assert L.fit_room(e._h, 1, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert L.fit_room(e._h, -1, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert L.fit_room(None, 0, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        for f in ("cpu", "mem", "gpu", "wall"):
            bad = synth.Jobs(*(getattr(jobs, g).copy() for g in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
            getattr(bad, f)[5] = -1
            assert _code(lambda: e.room(bad)) == _lib.FIT_E_INVAL  # the whole call fails
            cols = [DevArray(getattr(bad, g)) for g in ("cpu", "mem", "gpu", "wall", "part")]
            out = DevArray(np.zeros(16, ROOM_DTYPE))
            assert _code(lambda: e.room_device(*cols, out)) == _lib.FIT_E_INVAL
        jobs.nodes_k[:] = 9  # no nodes_k clause: the column plays no part
        assert len(room_both(e, jobs)) == 16
        assert L.fit_room_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        assert _code(lambda: e.room(jobs)) == _lib.FIT_E_STATE  # the backfill view is fit_when's
        e.load_nodes(nodes)  # drops the timeline
        assert len(e.room(jobs)) == 16
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.room(jobs)) == _lib.FIT_E_STATE


# ---- 7. read-only -------------------------------------------------------------------------------
def test_room_changes_nothing(engine):
    nodes, jobs, parts = synth.make_config("c2", 512, 2048)
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    before = engine.read_nodes()
    room_both(engine, jobs)
    after = engine.read_nodes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), "room changed the node table"
    assert all(np.array_equal(a, b) for a, b in zip(after, (nodes.cpu_free, nodes.mem_free, nodes.gpu_free)))
    out, _ = engine.place(jobs)
    ref, _, rfin = po.ref_place(nodes, jobs, parts)
    assert np.array_equal(out, ref), "a placement after room differs from the oracle"
    assert all(np.array_equal(a, b) for a, b in zip(engine.read_nodes(), rfin))

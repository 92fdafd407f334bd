"""fit_explain on the GPU against a numpy restatement of DESIGN.md §2c (ref_explain below): exact
counts on shapes that cross every wave, tile and slice edge of k_explain_count, consistency with
what fit_place decided, FITS means placeable, the admitter's view (reservations), state errors."""
import threading

import numpy as np
import pytest

import fitgpu
from _devarray import DevArray
from fitgpu import (FIT_WHY_FITS, FIT_WHY_LIMIT_CPUS, FIT_WHY_LIMIT_MEM, FIT_WHY_LIMIT_TIME, FIT_WHY_NO_NODES,
                    FIT_WHY_PARTITION, FIT_WHY_RESOURCES, WHY_DTYPE, Admitter, Engine, FitError, _lib, synth)

pytestmark = pytest.mark.gpu

INF = synth.INT32_MAX
REJECT_CODES = (FIT_WHY_PARTITION, FIT_WHY_LIMIT_TIME, FIT_WHY_LIMIT_CPUS, FIT_WHY_LIMIT_MEM)


def ref_explain(cpu, mem, gpu, avail, mask, parts, jobs):
    """DESIGN.md §2c over the raw columns (free columns as read_nodes gives them; avail_min and
    part_mask as loaded): every job alone, a J x N table of each term."""
    P, J = parts.p, jobs.j
    part = jobs.part.astype(np.int64)
    known = part < P
    pc = np.minimum(part, P - 1)
    out = np.zeros(J, WHY_DTYPE)
    out["need"] = np.maximum(jobs.nodes_k.astype(np.int32), 1)
    code = np.zeros(J, np.int32)
    for c, lim, dem in ((FIT_WHY_LIMIT_MEM, parts.max_mem_per_node, jobs.mem),  # last to first: the
                        (FIT_WHY_LIMIT_CPUS, parts.max_cpus_per_node, jobs.cpu),  # first match wins
                        (FIT_WHY_LIMIT_TIME, parts.max_time_min, jobs.wall)):
        code[known & (lim[pc] >= 0) & (dem > lim[pc])] = c
    code[~known] = FIT_WHY_PARTITION
    live = (code == 0)[:, None]
    member = live & (((mask[None, :].astype(np.int64) >> pc[:, None]) & 1) != 0)
    short = [member & (col[None, :] < dem[:, None]) for col, dem in
             ((cpu, jobs.cpu), (mem, jobs.mem), (gpu, jobs.gpu), (avail, jobs.wall))]
    out["members"] = member.sum(1)
    out["fit"] = (member & ~(short[0] | short[1] | short[2] | short[3])).sum(1)
    for name, s in zip(("short_cpu", "short_mem", "short_gpu", "short_time"), short):
        out[name] = s.sum(1)
    code[live[:, 0] & (out["members"] == 0)] = FIT_WHY_NO_NODES
    code[live[:, 0] & (out["members"] > 0) & (out["fit"] < out["need"])] = FIT_WHY_RESOURCES
    out["code"] = code
    return out


def explain_both(e, jobs):
    """Engine.explain through host pointers and through device pointers: the same rows."""
    host = e.explain(jobs)
    cols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")]
    out = DevArray(np.full(jobs.j, -7, np.int32).repeat(8).view(WHY_DTYPE))
    ms = e.explain_device(*cols, out)
    assert ms > 0
    assert np.array_equal(host, out.numpy()), "host and device entry points differ"
    return host


def assert_rows(got, want):
    for f in WHY_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- 1. exact counts on awkward shapes ----------------------------------------------------------
# 5 partitions are declared: 0 limits the walltime, 1 the cpus, 2 the memory, 3 nothing, 4 has no
# node at all; jobs also name partitions 5 and 6 (>= P).  Nodes sit in one or two of partitions
# 0..3 (so components hold several partitions and the in-component mask test matters) or in none.
HAND_PARTS = synth.Partitions(np.array([500, -1, -1, -1, -1], np.int32), np.array([-1, 16, -1, -1, -1], np.int32),
                              np.array([-1, -1, 30000, -1, -1], np.int32))


def hand_nodes(n, seed):
    r = np.random.default_rng(seed)
    mask = (1 << r.integers(0, 4, n)).astype(np.uint32)
    two = r.random(n) < 0.2
    mask[two] |= (1 << r.integers(0, 4, n)).astype(np.uint32)[two]
    mask[r.random(n) < 0.1] = 0  # drained: in no partition
    cpu = r.integers(0, 129, n).astype(np.int32)
    mem = (cpu.astype(np.int64) * r.choice([500, 2048, 4096], n)).astype(np.int32)
    gpu = r.choice([0, 0, 4, 8], n).astype(np.int32)
    for col in (cpu, mem, gpu):  # over-committed nodes: negative free values
        col[r.random(n) < 0.08] = -r.integers(1, 50)
    avail = np.where(r.random(n) < 0.3, r.integers(0, 3000, n), INF).astype(np.int32)
    if n == 1:
        mask[0], cpu[0], mem[0], gpu[0], avail[0] = 0b1010, 8, 16384, -1, 700
    return synth.Nodes(cpu, mem, gpu, avail, mask)


def hand_jobs(j, seed):
    r = np.random.default_rng(seed)
    cpu = r.choice([0, 1, 2, 4, 8, 16, 32, 64], j).astype(np.int32)
    mem = (np.maximum(cpu, 1).astype(np.int64) * r.choice([500, 1024, 4096], j)).astype(np.int32)
    gpu = r.choice([0, 0, 0, 1, 4, 8], j).astype(np.int32)
    wall = r.integers(0, 2881, j).astype(np.int32)
    return synth.Jobs(cpu, mem, gpu, wall, r.integers(0, 7, j).astype(np.uint16), r.integers(0, 9, j).astype(np.uint16))


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_exact_counts_hand_tables(engine, n):
    nodes = hand_nodes(n, 100 + n)
    engine.load_nodes(nodes)
    engine.load_partitions(HAND_PARTS)
    seen = set()
    for j in (1, 255, 257, 4097):
        jobs = hand_jobs(j, 7 * n + j)
        got = explain_both(engine, jobs)
        want = ref_explain(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask,
                           HAND_PARTS, jobs)
        assert_rows(got, want)
        seen |= set(np.unique(want["code"]).tolist())
    if n >= 63:  # the inputs reach every code (n = 1: no job can fit its single node's -1 GPUs)
        assert seen == set(range(7)), seen


@pytest.mark.parametrize("j", [64, 255, 256])
def test_exact_counts_mixed_components_in_caller_order(engine, j):
    """c3: 16 disjoint partitions, 16 components; up to 256 jobs keep the caller's order, so the
    lanes of one wave name many components and the wave walks them one after the other."""
    nodes, jobs, parts = synth.make_config("c3", 1000, j)
    jobs.nodes_k = (np.arange(j) % 9).astype(np.uint16)
    assert len(np.unique(nodes.part_mask)) == 16 and len(np.unique(jobs.part[:64])) >= 8
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    want = ref_explain(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask, parts, jobs)
    assert_rows(explain_both(engine, jobs), want)
    assert (want["members"] > 0).any() and len(np.unique(want["members"][want["members"] > 0])) >= 8


def test_exact_counts_overlapping_partitions(engine):
    """c3o: 777 nodes, 17 partitions, every node in two of them — one component, so membership
    rests on the mask test inside it."""
    nodes, jobs, parts = synth.make_config("c3o", 777, 4097)
    jobs.nodes_k = (np.arange(jobs.j) % 9).astype(np.uint16)
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    want = ref_explain(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min, nodes.part_mask, parts, jobs)
    assert_rows(explain_both(engine, jobs), want)
    assert want["members"].max() == 777 and 0 < want["members"][want["members"] > 0].min() < 777


# ---- 2. consistency with the engine -------------------------------------------------------------
@pytest.mark.parametrize("name,n,j,kmax", [("c2", 512, 8192, 1), ("c3", 1000, 4097, 1), ("c3o", 777, 3001, 1),
                                           ("c4", 1024, 4096, 8)])
def test_consistent_with_place(engine, name, n, j, kmax):
    nodes, jobs, parts = synth.make_config(name, n, j)
    engine.load_nodes(nodes)
    engine.load_partitions(parts)
    out, _ = engine.place(jobs, kmax=kmax)
    before = engine.read_nodes()
    why = explain_both(engine, jobs)
    after = engine.read_nodes()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "explain changed the node table"
    rejected, unplaced = out[:, 0] == fitgpu.FIT_REJECTED, out[:, 0] == fitgpu.FIT_UNPLACED
    assert rejected.any() and unplaced.any()
    assert np.array_equal(rejected, np.isin(why["code"], REJECT_CODES))
    # resources only shrink during a batch: a job unplaced at its turn cannot fit at the end
    assert not (why["code"][unplaced] == FIT_WHY_FITS).any()
    assert_rows(why, ref_explain(*after, nodes.avail_min, nodes.part_mask, parts, jobs))


# ---- 3. FITS means placeable --------------------------------------------------------------------
@pytest.mark.auto_engine
def test_fits_jobs_are_placed_alone():
    nodes = hand_nodes(65, 5)
    jobs = hand_jobs(64, 6)
    jobs.nodes_k = np.minimum(jobs.nodes_k, 3).astype(np.uint16)  # the table has few fitting nodes
    with Engine(device=0) as e:  # its own context: the engine choice is read when it is created
        e.load_nodes(nodes)
        e.load_partitions(HAND_PARTS)
        why = e.explain(jobs)
        fits = why["code"] == FIT_WHY_FITS
        assert 8 <= fits.sum() < 64
        for q in range(64):
            e.load_nodes(nodes)  # the same state for every job
            one = synth.Jobs(*(getattr(jobs, f)[q:q + 1] for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
            out, st = e.place(one, kmax=8)
            assert st["engine"] == 2  # k_small
            assert (out[0, 0] >= 0) == bool(fits[q]), (q, out[0], why[q])
            assert (out[0, 0] == fitgpu.FIT_REJECTED) == (why["code"][q] in REJECT_CODES)


# ---- 4. admitter --------------------------------------------------------------------------------
def _gpu_table():
    # node 1 has one GPU left, nodes 0 and 2 none; one partition, no limits
    nodes = synth.Nodes(np.full(3, 64, np.int32), np.full(3, 65536, np.int32), np.array([0, 1, 0], np.int32),
                        np.full(3, INF, np.int32), np.ones(3, np.uint32))
    parts = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
    return nodes, parts


@pytest.mark.auto_engine
def test_admitter_explain_sees_reservations():
    nodes, parts = _gpu_table()
    req = (0, 4, 1024, 1, 60, 0, 1)
    with Engine(device=0) as e:
        e.load_partitions(parts)
        with Admitter(e, max_batch=8, max_wait_us=0) as a:
            a.load_nodes(nodes)
            w = a.explain([req])[0]
            assert (w["code"], w["members"], w["fit"], w["short_gpu"]) == (FIT_WHY_FITS, 3, 1, 2)
            got, _, _, _, ticket = a.admit(*req)
            assert got == [1] and ticket > 0
            w = a.explain([req])[0]  # node 1's last GPU is reserved
            assert (w["code"], w["members"], w["fit"], w["short_gpu"]) == (FIT_WHY_RESOURCES, 3, 0, 3)
            assert fitgpu.why_message(w) == "0/3 nodes fit now: 3 insufficient gpu"
            a.release(ticket)
            w = a.explain([req])[0]
            assert (w["code"], w["fit"], w["short_gpu"]) == (FIT_WHY_FITS, 1, 2)
            assert len(a.explain([])) == 0
            with pytest.raises(FitError) as ei:
                a.explain([(0, -1, 0, 0, 0, 0, 1)])
            assert ei.value.code == _lib.FIT_E_INVAL


@pytest.mark.auto_engine
def test_admit_and_explain_threads_both_finish():
    nodes, _, parts = synth.make_config("c2", 256, 1)
    errs = []
    with Engine(device=0) as e:
        e.load_partitions(parts)
        with Admitter(e, max_batch=16, max_wait_us=100) as a:
            a.load_nodes(nodes)

            def admit():
                try:
                    for i in range(100):
                        a.admit(i, 1, 500, 0, 30, 0, 1)
                except Exception as ex:  # noqa: BLE001
                    errs.append(ex)

            rows = []

            def explain():
                try:
                    for _ in range(100):
                        rows.append(a.explain([(0, 1, 500, 0, 30, 0, 1)])[0])
                except Exception as ex:  # noqa: BLE001
                    errs.append(ex)

            ts = [threading.Thread(target=admit), threading.Thread(target=explain)]
            for t in ts:
                t.start()
            for t in ts:
                t.join(60)
            assert not any(t.is_alive() for t in ts) and not errs, errs
            assert len(rows) == 100 and all(r["members"] == (nodes.part_mask != 0).sum() for r in rows)
            fit = [int(r["fit"]) for r in rows]
            assert fit == sorted(fit, reverse=True)  # reservations only take capacity away


# ---- 5. state and argument errors ---------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_state_and_argument_errors():
    nodes, jobs, parts = synth.make_config("c2", 64, 16)
    with Engine(device=0) as e:
        assert _code(lambda: e.explain(jobs)) == _lib.FIT_E_STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert len(e.explain(jobs)) == 16
        L = _lib.lib()
        assert L.fit_explain(e._h, 0, None, None, None, None, None, None, None) == 0
        assert L.fit_explain_device(e._h, 0, None, None, None, None, None, None, None) == 0
        assert L.fit_explain(e._h, 1, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert L.fit_explain(e._h, -1, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        bad = synth.Jobs(*(getattr(jobs, f).copy() for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
        bad.gpu[5] = -1
        assert _code(lambda: e.explain(bad)) == _lib.FIT_E_INVAL
        bad.gpu[5] = 0
        bad.nodes_k[15] = 9
        assert _code(lambda: e.explain(bad)) == _lib.FIT_E_INVAL
        bad.nodes_k[15] = 8
        assert len(e.explain(bad)) == 16
        fin = e.read_nodes()
        assert all(np.array_equal(a, b) for a, b in zip(fin, (nodes.cpu_free, nodes.mem_free, nodes.gpu_free)))
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        assert _code(lambda: e.explain(jobs)) == _lib.FIT_E_STATE  # the backfill view is place_tl's
        e.load_nodes(nodes)  # drops the timeline
        assert len(e.explain(jobs)) == 16
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.explain(jobs)) == _lib.FIT_E_STATE

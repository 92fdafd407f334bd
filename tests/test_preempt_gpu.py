"""fit_preempt on the GPU against ref_preempt (tests/_preempt_cases.py, a numpy int64 restatement of
DESIGN.md §2l): rows compared field for field through the host and the device entry point, on shapes
that cross every wave, tile and slice edge of k_pre_walk, list lengths around the walk's four-entry
loads, int32 edge values, what fit_explain, the oracle and fit_place confirm, and the state errors."""
import ctypes as C

import numpy as np
import pytest

import _preempt_cases as pc
import fitgpu
from _devarray import DevArray
from fitgpu import EVICT_DTYPE, Engine, FitError, _lib, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INF, I32MIN = synth.INT32_MAX, -2**31
ONE_PART = synth.Partitions(np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32))
VCOLS = ("off", "prio", "cpu", "mem", "gpu")


def preempt_both(e, jobs, prio):
    """Engine.preempt through host pointers and through device pointers: the same rows."""
    host = e.preempt(jobs, prio)
    cols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")] + [DevArray(np.asarray(prio, np.int32))]
    out = DevArray(np.full(jobs.j * 8, -7, np.int32).view(EVICT_DTYPE))
    ms = e.preempt_device(*cols, out)
    assert ms > 0 and e.preempt_ms() == ms
    assert np.array_equal(host, out.numpy()), "host and device entry points differ"
    return host


def assert_rows(got, want):
    for f in EVICT_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, f"{f}: {bad.size} jobs differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def load(e, c, device=False):
    e.load_nodes(c.nodes)
    e.load_partitions(c.parts)
    if device and c.victims is not None:
        e.load_victims_device(*(DevArray(getattr(c.victims, f)) for f in VCOLS))
    else:
        e.load_victims(c.victims)


def jobs_of(rows):
    """synth.Jobs and priorities from (cpu, mem, gpu, wall, part, prio) rows."""
    a = np.array(rows, np.int64).reshape(-1, 6)
    return (synth.Jobs(*(a[:, k].astype(np.int32) for k in range(4)), a[:, 4].astype(np.uint16), np.ones(len(a), np.uint16)),
            a[:, 5].astype(np.int32))


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


# ---- 1. the packed random cases -----------------------------------------------------------------
@pytest.mark.parametrize("n,j,device", [(65, 65, False), (257, 128, True), (1000, 300, False)])
def test_packed_random_cases(engine, n, j, device):
    c = pc.packed_case(n, j)
    want, stats = pc.packed_ref(n, j)
    pc.rich_enough(want, stats)  # on the reference alone: a comparison of nothing interesting fails
    load(engine, c, device)
    assert_rows(preempt_both(engine, c.jobs, c.prio), want)


# ---- 2. shapes at the seams ---------------------------------------------------------------------
# n: the wave sub-slices (8 waves share a slice's rows) and the 256-row node slices of explain_slices;
# J: the 64-job tiles, and above kExplainSortJobs = 256 on several components the component-ordered
# job list.  Both with the two components of the generator and with one.
SEAM_J = (1, 63, 64, 65, 257, 700)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_shapes_at_the_seams(engine, n):
    total, evict, none = {}, 0, 0
    for one_component in (False, True):
        first = True
        for j in SEAM_J:
            if n * j > 5000 * 257:  # the reference's J x N x list tables: keep the case within seconds
                continue
            c = pc.packed_case(n, j, 0, one_component)
            want, stats = pc.packed_ref(n, j, 0, one_component)
            if first:  # the table depends on j through the generator's seed: load each, the first through the device
                load(engine, c, device=True)
                first = False
            else:
                load(engine, c)
            assert_rows(preempt_both(engine, c.jobs, c.prio), want)
            for k, v in stats.items():
                total[k] = total.get(k, 0) + v
            evict += int((want["code"] == pc.EVICT).sum())
            none += int((want["code"] == pc.NONE).sum())
    assert none > 0
    if n >= 63:  # over its J's every table reaches what rich_enough asks of one random case
        assert evict >= 20 and total["tie_top"] > 0 and total["tie_top_v"] > 0 and total["tie_top_v_score"] > 0, total
        assert total["not_fewest"] > 0, total
    elif n == 2:
        assert evict > 0


def test_a_batch_above_one_chunk_of_positions(engine):
    """16,800 jobs: the walk and the final run twice, the second time over 416 positions of the
    component-ordered job list.  Every job is judged alone, so the 700-job case repeated 24 times has
    the reference's rows repeated 24 times."""
    c = pc.packed_case(257, 700)
    want, _ = pc.packed_ref(257, 700)
    reps = 24
    jobs = synth.Jobs(*(np.tile(getattr(c.jobs, f), reps) for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
    assert jobs.j > 16384 and len(np.unique(c.jobs.part)) > 2
    load(engine, c)
    assert_rows(preempt_both(engine, jobs, np.tile(c.prio, reps)), np.tile(want, reps))


def test_hand_written_case_gives_the_literal_rows(engine):
    c = pc.hand_case()
    load(engine, c)
    got = preempt_both(engine, c.jobs, c.prio)
    for q, want in enumerate(pc.HAND_ROWS):
        assert tuple(int(x) for x in got[q]) == want, (q, got[q], want)
    load(engine, c, device=True)
    assert np.array_equal(preempt_both(engine, c.jobs, c.prio), got)


# ---- 3. list lengths ----------------------------------------------------------------------------
LENS = (0, 1, 2, 63, 64, 65, 300)


def test_list_lengths_around_the_four_entry_loads(engine):
    """40 nodes without a free cpu; node x's list has LENS[x % 7] entries of priorities 0, 1, 2, ...,
    all of them holding nothing but the last, which holds 8 cpus: only the whole list frees enough, so
    the walk runs to its end.  A job at the priority of a list's last entry finds that node outranked,
    one priority higher frees it."""
    n = 40
    lens = np.array([LENS[x % 7] for x in range(n)])
    lists = [[(i, 8 if i == ln - 1 else 0, 0, 0) for i in range(ln)] for ln in lens]
    nodes = synth.Nodes(np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, INF, np.int32),
                        np.ones(n, np.uint32))
    prios = sorted({p for ln in LENS if ln for p in (ln - 1, ln)} | {I32MIN, INF})
    jobs, prio = jobs_of([(8, 0, 0, 0, 0, p) for p in prios])
    c = pc.Case(nodes, pc.victims_of(lists), ONE_PART, jobs, prio)
    load(engine, c)
    got = preempt_both(engine, jobs, prio)
    assert_rows(got, pc.ref_preempt(nodes, c.victims, ONE_PART, jobs, prio))
    for r, p in zip(got, prios):
        # a list of ln entries is freed by a job above its last priority ln - 1; the others that have one hold it
        able = int(((lens > 0) & (lens - 1 < p)).sum())
        assert (r["members"], r["fit"], r["able"], r["outranked"]) == (n, 0, able, int((lens > 0).sum()) - able), (p, r)
        if able:  # the shortest list has the lowest last priority: node 1, one victim; zero-amount victims count
            assert (r["code"], r["node"], r["victims"], r["top_prio"]) == (pc.EVICT, 1, 1, 0)
        else:
            assert (r["code"], r["node"], r["victims"], r["top_prio"]) == (pc.NONE, -1, 0, 0)
    # without the one-entry lists the winner walks 2, then 63, ... entries: victims = the list's length
    for drop in range(1, len(LENS) - 1):
        v = pc.victims_of([[] if ln in LENS[1:drop + 1] else lst for ln, lst in zip(lens, lists)])
        engine.load_victims(v)
        r = preempt_both(engine, jobs, prio)
        assert_rows(r, pc.ref_preempt(nodes, v, ONE_PART, jobs, prio))
        nxt = LENS[drop + 1]
        assert (r[-1]["code"], r[-1]["victims"], r[-1]["top_prio"]) == (pc.EVICT, nxt, nxt - 1)  # the INT32_MAX job
        assert r[-1]["node"] == int(np.flatnonzero(lens == nxt)[0])


# ---- 4. edge values -----------------------------------------------------------------------------
def test_priorities_at_the_int32_ends(engine):
    nodes = synth.Nodes(np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), np.full(2, INF, np.int32),
                        np.ones(2, np.uint32))
    v = pc.victims_of([[(I32MIN, 4, 0, 0), (INF, 4, 0, 0)], [(INF, 8, 0, 0)]])
    jobs, prio = jobs_of([(4, 0, 0, 0, 0, I32MIN), (4, 0, 0, 0, 0, I32MIN + 1), (8, 0, 0, 0, 0, INF),
                          (4, 0, 0, 0, 0, INF), (9, 0, 0, 0, 0, INF)])
    load(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    got = preempt_both(engine, jobs, prio)
    assert_rows(got, pc.ref_preempt(nodes, v, ONE_PART, jobs, prio))
    rows = [tuple(int(x) for x in r) for r in got]
    assert rows[0] == (pc.NONE, -1, 0, 0, 2, 0, 0, 2)        # a job at INT32_MIN evicts nothing
    assert rows[1] == (pc.EVICT, 0, 1, I32MIN, 2, 0, 1, 1)   # one above: the INT32_MIN victim goes
    assert rows[2] == (pc.NONE, -1, 0, 0, 2, 0, 0, 2)        # an INT32_MAX job does not evict an INT32_MAX victim
    assert rows[3] == (pc.EVICT, 0, 1, I32MIN, 2, 0, 1, 1)
    assert rows[4] == (pc.NONE, -1, 0, 0, 2, 0, 0, 0)        # no list frees 9 cpus: neither able nor outranked


def test_sums_are_exact_and_the_residual_is_clamped(engine):
    """Node 0: INT32_MAX free cpus and three victims of INT32_MAX cpus and 1 MiB each; node 1 the same
    free cpus, its victims hold no cpu.  A job of INT32_MAX - 5 cpus and 3 MiB needs all three on
    either: the sum on node 0 is 4 (2^31 - 1), its residual min(sum, INT32_MAX) - demand = 5, node 1's
    as well: the lower id wins.  A sum that wrapped would not fit; an unclamped residual would lose."""
    nodes = synth.Nodes(np.full(2, INF, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), np.full(2, INF, np.int32),
                        np.ones(2, np.uint32))
    v = pc.victims_of([[(1, INF, 1, 0)] * 3, [(1, 0, 1, 0)] * 3])
    jobs, prio = jobs_of([(INF - 5, 3, 0, 0, 0, 2), (INF, 2, 0, 0, 0, 2), (INF, 0, 0, 0, 0, 2), (0, 0, 0, 0, 0, 0)])
    load(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    got = preempt_both(engine, jobs, prio)
    assert_rows(got, pc.ref_preempt(nodes, v, ONE_PART, jobs, prio))
    rows = [tuple(int(x) for x in r) for r in got]
    assert rows[0] == (pc.EVICT, 0, 3, 1, 2, 0, 2, 0)
    assert rows[1] == (pc.EVICT, 0, 2, 1, 2, 0, 2, 0)
    assert rows[2] == (pc.FITS, 0, 0, 0, 2, 2, 0, 0)
    assert rows[3] == (pc.FITS, 0, 0, 0, 2, 2, 0, 0)  # the all-zero demand


def test_a_victim_that_holds_nothing_counts(engine):
    nodes = synth.Nodes(np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.full(1, INF, np.int32),
                        np.ones(1, np.uint32))
    v = pc.victims_of([[(1, 0, 0, 0), (2, 4, 0, 0)]])
    jobs, prio = jobs_of([(4, 0, 0, 0, 0, 5), (0, 0, 0, 0, 0, 5)])
    load(engine, pc.Case(nodes, v, ONE_PART, jobs, prio))
    got = preempt_both(engine, jobs, prio)
    assert tuple(int(x) for x in got[0]) == (pc.EVICT, 0, 2, 2, 1, 0, 1, 0)
    assert tuple(int(x) for x in got[1]) == (pc.FITS, 0, 0, 0, 1, 1, 0, 0)


# ---- 5. identities ------------------------------------------------------------------------------
def test_members_and_fit_are_fit_explains(engine):
    c = pc.packed_case(1000, 300)
    load(engine, c)
    got, why = preempt_both(engine, c.jobs, c.prio), engine.explain(c.jobs)
    assert np.array_equal(got["members"], why["members"]) and np.array_equal(got["fit"], why["fit"])
    early = np.isin(got["code"], (1, 2, 3, 4, 5)) | np.isin(why["code"], (1, 2, 3, 4, 5))
    assert early.any() and np.array_equal(got["code"][early], why["code"][early])  # FIT_PRE_1..5 are FIT_WHY_1..5
    assert np.array_equal(got["code"] == pc.FITS, why["code"] == fitgpu.FIT_WHY_FITS)
    assert (got["fit"] > 0).any() and (why["code"] == fitgpu.FIT_WHY_RESOURCES).any()


def one_job(jobs, q):
    return synth.Jobs(*(getattr(jobs, f)[q:q + 1].copy() for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))


def test_a_fits_rows_node_is_the_oracles_placement(engine):
    c = pc.packed_case(1000, 300)
    want, _ = pc.packed_ref(1000, 300)
    load(engine, c)
    got = preempt_both(engine, c.jobs, c.prio)
    fits = np.flatnonzero(got["code"] == pc.FITS)
    assert len(fits) >= 10
    for q in fits[:: max(1, len(fits) // 10)][:10]:
        ref, _, _ = po.ref_place(c.nodes, one_job(c.jobs, q), c.parts)
        assert got["node"][q] == ref[0, 0] >= 0, (q, got[q], ref)
    assert_rows(got, want)


@pytest.mark.auto_engine
def test_evicting_the_prefix_places_the_job_and_one_less_does_not():
    c = pc.packed_case(257, 128)
    want, _ = pc.packed_ref(257, 128)
    v = c.victims
    with Engine(device=0) as e:  # its own context: the engine choice is read when it is created
        load(e, c)
        got = e.preempt(c.jobs, c.prio)
        assert_rows(got, want)
        ev = np.flatnonzero(got["code"] == pc.EVICT)
        picked = list(ev[:: max(1, len(ev) // 8)][:8])
        many = [q for q in ev if got["victims"][q] >= 2]
        picked += many[:2]  # some that take several victims
        assert len(picked) >= 8 and many
        base = e.read_nodes()
        for q in picked:
            x, k = int(got["node"][q]), int(got["victims"][q])
            for take, placed in ((k, x), (k - 1, fitgpu.FIT_UNPLACED)):
                sl = slice(v.off[x], v.off[x] + take)
                cols = [col.copy() for col in base]
                for col, amt in zip(cols, (v.cpu, v.mem, v.gpu)):
                    col[x] = min(int(col[x]) + int(amt[sl].astype(np.int64).sum()), INF)
                e.load_nodes(synth.Nodes(*cols, c.nodes.avail_min, c.nodes.part_mask))
                out, _ = e.place(one_job(c.jobs, q))
                assert out[0, 0] == placed, (q, got[q], take, out)
        load(e, c)  # the original table and its victims again
        assert np.array_equal(e.preempt(c.jobs, c.prio), got)


@pytest.mark.auto_engine
def test_rows_follow_the_current_table_not_the_loaded_one():
    """After a placement the free columns are read_nodes()'s; the victims are untouched by fit_place."""
    nodes, queue, parts = synth.make_config("c3", 600, 900)
    packed, v = synth.pack_victims(11, nodes, empty_pm=500)  # half the nodes keep their free resources
    jobs = synth.Jobs(*(getattr(queue, f)[:200] for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
    prio = synth.gen_job_prio(11, 200)
    with Engine(device=0) as e:
        e.load_nodes(packed)
        e.load_partitions(parts)
        e.load_victims(v)
        before = e.preempt(jobs, prio)
        assert_rows(before, pc.ref_preempt(packed, v, parts, jobs, prio))
        out, st = e.place(queue)
        assert st["placed"] > 100
        free = e.read_nodes()
        assert any(not np.array_equal(a, b) for a, b in zip(free, (packed.cpu_free, packed.mem_free, packed.gpu_free)))
        after = preempt_both(e, jobs, prio)
        assert_rows(after, pc.ref_preempt(packed, v, parts, jobs, prio, free=free))
        assert not np.array_equal(before, after) and (after["code"] == pc.EVICT).any()


# ---- 6. read-only -------------------------------------------------------------------------------
def test_preempt_changes_nothing(engine):
    c = pc.packed_case(1000, 300)
    load(engine, c)
    before = engine.read_nodes()
    first = preempt_both(engine, c.jobs, c.prio)
    after = engine.read_nodes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), "preempt changed the node table"
    assert all(np.array_equal(a, b) for a, b in zip(after, (c.nodes.cpu_free, c.nodes.mem_free, c.nodes.gpu_free)))
    assert preempt_both(engine, c.jobs, c.prio).tobytes() == first.tobytes(), "a second call differs"


# ---- 7. state and argument errors ---------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_state_errors():
    c = pc.hand_case()
    L = _lib.lib()
    ms = C.c_double()
    with Engine(device=0) as e:
        assert _code(lambda: e.preempt(c.jobs, c.prio)) == _lib.FIT_E_STATE     # before load_nodes
        assert L.fit_load_victims(e._h, None, None, None, None, None) == _lib.FIT_E_STATE
        assert L.fit_load_victims_device(e._h, None, 0, None, None, None, None) == _lib.FIT_E_STATE
        e.load_nodes(c.nodes)
        e.load_partitions(c.parts)
        assert _code(lambda: e.preempt(c.jobs, c.prio)) == _lib.FIT_E_STATE     # before load_victims
        assert b"fit_load_victims" in L.fit_last_error()
        assert L.fit_preempt(e._h, 0, None, None, None, None, None, None, None) == _lib.FIT_E_STATE
        e.load_victims(c.victims)
        assert L.fit_preempt_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE          # no fit_preempt_device yet
        got = e.preempt(c.jobs, c.prio)
        assert [tuple(int(x) for x in r) for r in got] == pc.HAND_ROWS
        assert L.fit_preempt_ms(e._h, C.byref(ms)) == _lib.FIT_E_STATE          # the host entry point is none
        assert L.fit_preempt(e._h, 0, None, None, None, None, None, None, None) == 0
        assert L.fit_preempt_device(e._h, 0, None, None, None, None, None, None, None) == 0
        assert L.fit_preempt(e._h, 1, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert L.fit_preempt(e._h, -1, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        out, _ = e.place(c.jobs)                                                # fit_place leaves the victims alone
        assert len(e.preempt(c.jobs, c.prio)) == c.jobs.j
        e.load_nodes(c.nodes)                                                   # drops them: node ids change
        assert _code(lambda: e.preempt(c.jobs, c.prio)) == _lib.FIT_E_STATE
        e.load_victims(c.victims)
        assert np.array_equal(preempt_both(e, c.jobs, c.prio), got)
        assert L.fit_preempt_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_victims(None)                                                    # every list empty
        none = preempt_both(e, c.jobs, c.prio)
        assert not none["able"].any() and not none["outranked"].any() and not (none["code"] == pc.EVICT).any()
        assert_rows(none, pc.ref_preempt(c.nodes, None, c.parts, c.jobs, c.prio))
        e.load_victims_device(None, None, None, None, None)
        assert np.array_equal(e.preempt(c.jobs, c.prio), none)


def test_no_preemption_while_a_timeline_is_loaded():
    nodes, tline, jobs, parts = synth.make_c5(64, 16)
    prio = np.zeros(16, np.int32)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_victims(None)
        assert len(e.preempt(jobs, prio)) == 16
        e.load_timeline(tline)
        assert _code(lambda: e.preempt(jobs, prio)) == _lib.FIT_E_STATE         # no preemption on the timeline
        e.load_victims(None)                                                    # the timeline calls and the victims
        assert _code(lambda: e.preempt(jobs, prio)) == _lib.FIT_E_STATE         # leave each other alone
        e.load_nodes(nodes)                                                     # drops the timeline and the victims
        e.load_victims(None)
        assert len(e.preempt(jobs, prio)) == 16


def test_a_sharded_context_holds_no_victims():
    nodes, jobs, parts = synth.make_config("c2", 64, 16)
    prio = np.zeros(16, np.int32)
    L = _lib.lib()
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.load_victims(None)) == _lib.FIT_E_STATE
        assert L.fit_load_victims_device(e._h, None, 0, None, None, None, None) == _lib.FIT_E_STATE
        assert _code(lambda: e.preempt(jobs, prio)) == _lib.FIT_E_STATE


def test_a_context_whose_nodes_are_in_no_partition(engine):
    c = pc.hand_case()
    nodes = synth.Nodes(c.nodes.cpu_free, c.nodes.mem_free, c.nodes.gpu_free, c.nodes.avail_min, np.zeros(6, np.uint32))
    load(engine, pc.Case(nodes, c.victims, c.parts, c.jobs, c.prio))  # the victims are validated and never used
    got = preempt_both(engine, c.jobs, c.prio)
    assert_rows(got, pc.ref_preempt(nodes, c.victims, c.parts, c.jobs, c.prio))
    assert set(got["code"].tolist()) == {pc.PARTITION, pc.LIMIT_TIME, pc.LIMIT_CPUS, pc.LIMIT_MEM, pc.NO_NODES}
    assert (got["node"] == -1).all() and not got["members"].any()
    bad = pc.victims_of([[(1, 1, 1, 1)], [], [], [], [(5, 1, 1, 1), (4, 1, 1, 1)], []])
    assert _code(lambda: engine.load_victims(bad)) == _lib.FIT_E_INVAL  # validated all the same


def test_every_invalid_victim_list_fails_as_a_whole_and_keeps_the_loaded_ones(engine):
    c = pc.hand_case()
    load(engine, c)
    good = preempt_both(engine, c.jobs, c.prio)
    L = _lib.lib()
    v = c.victims
    n = c.nodes.n

    def variant(**kw):
        cols = {f: getattr(v, f).copy() for f in VCOLS}
        for f, (i, val) in kw.items():
            cols[f][i] = val
        return cols

    def host(cols):
        return L.fit_load_victims(engine._h, *(C.c_void_p(cols[f].ctypes.data) if cols[f] is not None else None
                                               for f in VCOLS))

    def device(cols, n_vic=None):
        dev = {f: DevArray(cols[f]) if cols[f] is not None else None for f in VCOLS}
        n_vic = len(v.prio) if n_vic is None else n_vic
        return L.fit_load_victims_device(engine._h, *(C.c_void_p(dev[VCOLS[0]].data_ptr()) if dev[VCOLS[0]] else None,
                                                      n_vic),
                                         *(C.c_void_p(dev[f].data_ptr()) if dev[f] else None for f in VCOLS[1:]))

    assert host(variant()) == 0 and device(variant()) == 0  # the harness itself loads the good lists
    bad = [variant(off=(0, 1)),                      # vic_off[0] != 0
           variant(off=(3, 1)),                      # a decreasing vic_off
           variant(cpu=(2, -1)), variant(mem=(0, -1)), variant(gpu=(len(v.prio) - 1, -1)),  # a negative amount
           variant(prio=(1, 0)),                     # node 0: priorities 1, 0 decrease
           variant(prio=(5, 2))]                     # node 2: 3, 3, 2 decrease at its last entry
    for f in VCOLS[1:]:                              # a NULL column when there are entries
        cols = variant()
        cols[f] = None
        bad.append(cols)
    for cols in bad:
        for fn in (host, device):
            assert fn(cols) == _lib.FIT_E_INVAL, cols
            assert np.array_equal(engine.preempt(c.jobs, c.prio), good), "a rejected load changed the loaded victims"
    assert device(variant(), n_vic=len(v.prio) - 1) == _lib.FIT_E_INVAL  # vic_off does not end at n_vic
    assert device(variant(), n_vic=-1) == _lib.FIT_E_INVAL
    assert device(variant(off=(n, len(v.prio) + 1))) == _lib.FIT_E_INVAL  # ends past the entries
    assert L.fit_load_victims_device(engine._h, None, 3, None, None, None, None) == _lib.FIT_E_INVAL
    assert np.array_equal(preempt_both(engine, c.jobs, c.prio), good)
    # priorities may repeat, and decrease from one node to the next
    ok = variant(prio=(1, 1))
    assert host(ok) == 0 and device(ok) == 0
    with pytest.raises(ValueError):
        engine.load_victims(synth.Victims(v.off[:-1], v.prio, v.cpu, v.mem, v.gpu))  # off needs n + 1 entries


def test_every_invalid_job_fails_the_whole_call(engine):
    c = pc.hand_case()
    load(engine, c)
    for f in ("cpu", "mem", "gpu", "wall"):
        bad = synth.Jobs(*(getattr(c.jobs, g).copy() for g in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
        getattr(bad, f)[5] = -1
        assert _code(lambda: engine.preempt(bad, c.prio)) == _lib.FIT_E_INVAL
        cols = [DevArray(getattr(bad, g)) for g in ("cpu", "mem", "gpu", "wall", "part")] + [DevArray(c.prio)]
        out = DevArray(np.zeros(c.jobs.j, EVICT_DTYPE))
        assert _code(lambda: engine.preempt_device(*cols, out)) == _lib.FIT_E_INVAL
    with pytest.raises(ValueError):
        engine.preempt(c.jobs, c.prio[:-1])
    assert [tuple(int(x) for x in r) for r in preempt_both(engine, c.jobs, c.prio)] == pc.HAND_ROWS

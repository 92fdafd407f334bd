"""Recycling of exhausted dirty rows in the multi-wave commit: when the round's
dirty set is full, the decider retires a row that fits no job of the component any more (below the
component's minimum demand in one resource) and gives its slot to the fresh node; the retired rows
reach the node table with the round's write-back.  Every case runs the persistent engine under
four window policies and compares placements and `read_nodes()` with the oracle, bit for bit."""
import functools

import numpy as np
import pytest

from fitgpu import Engine, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

I32_MAX = 2**31 - 1
WINDOWS = [dict(), dict(window_min=64, window_max=64), dict(window_min=256, window_max=256),
           dict(window_min=1, window_max=8)]
PARTS = synth.Partitions(np.array([-1, -1], np.int32), np.array([-1, -1], np.int32),
                         np.array([-1, -1], np.int32))


def _nodes(n, cpu, mem, gpu, mask=1):
    f = lambda v: np.full(n, v, np.int32) if np.isscalar(v) else np.asarray(v, np.int32)  # noqa: E731
    return synth.Nodes(cpu_free=f(cpu), mem_free=f(mem), gpu_free=f(gpu),
                       avail_min=np.full(n, I32_MAX, np.int32),
                       part_mask=np.full(n, mask, np.uint32) if np.isscalar(mask) else np.asarray(mask, np.uint32))


def _jobs(j, cpu, mem, gpu=0, part=0):
    f = lambda v, t=np.int32: np.full(j, v, t) if np.isscalar(v) else np.asarray(v, t)  # noqa: E731
    return synth.Jobs(cpu=f(cpu), mem=f(mem), gpu=f(gpu), wall=np.ones(j, np.int32),
                      part=f(part, np.uint16), nodes_k=np.ones(j, np.uint16))


def _cat(a, b):
    return synth.Jobs(*(np.concatenate([x, y]) for x, y in zip(
        (a.cpu, a.mem, a.gpu, a.wall, a.part, a.nodes_k), (b.cpu, b.mem, b.gpu, b.wall, b.part, b.nodes_k))))


def _exact(n, seed=13):
    """n nodes of 1..n free CPUs and n jobs asking for 1..n CPUs, both in seeded orders: every job
    fills one clean node exactly, so every placement is fresh and leaves a dead row behind."""
    rng = np.random.default_rng(seed)
    return _nodes(n, rng.permutation(n) + 1, 262_144, 0), _jobs(n, rng.permutation(n) + 1, 1024)


def _zero_demand():
    """The exact-fit input followed by 200 jobs of no CPU: best fit sends them onto the nodes whose
    CPUs are used up (leftover 0 is the smallest score), which a recycler that took "no CPU left"
    for dead would have retired.  The component's minimum CPU demand is 0: that criterion is void."""
    nodes, jobs = _exact(180)
    return nodes, _cat(jobs, _jobs(200, 0, 512))


def _dead_by_mem():
    rng = np.random.default_rng(17)
    return (_nodes(180, 1000, (rng.permutation(180) + 1) * 1024, 0),
            _jobs(180, 1, (rng.permutation(180) + 1) * 1024))


def _dead_by_gpu():
    rng = np.random.default_rng(19)
    return (_nodes(180, 1000, 1 << 24, rng.permutation(180) + 1),
            _jobs(180, 1, 1024, rng.permutation(180) + 1))


def _two_jobs_per_node(a=None, b=None):
    """Nodes of 64 CPUs and jobs of 32: every node dies at its second job, so once the set is full
    a slot is recycled at every other step while up to 7 records are in flight.  With (a, b): two
    components of a and b nodes (the second one's bitmap starts inside a word)."""
    if a is None:
        return _nodes(600, 64, 262_144, 0), _jobs(1200, 32, 1024)
    n = a + b
    rng = np.random.default_rng(23)
    return (_nodes(n, 64, 262_144, 0, np.where(np.arange(n) < a, 1, 2)),
            _jobs(2 * n, 32, 1024, 0, rng.permutation(np.repeat([0, 1], [2 * a, 2 * b]))))


@functools.lru_cache(maxsize=None)
def _case(name, *args):
    """A case's inputs and the oracle's answer, computed once and shared by the window policies."""
    nodes, jobs = {"exact": _exact, "zero": _zero_demand, "mem": _dead_by_mem, "gpu": _dead_by_gpu,
                   "two": _two_jobs_per_node}[name](*args)
    ref, _, rfin = po.ref_place(nodes, jobs, PARTS)
    ref = np.asarray(ref).copy()
    ref.setflags(write=False)
    return nodes, jobs, ref, rfin


def _check(monkeypatch, case, kw, again=False):
    nodes, jobs, ref, rfin = case
    monkeypatch.setenv("FIT_ENGINE", "persistent")
    with Engine(device=0, **kw) as e:
        e.load_nodes(nodes)
        e.load_partitions(PARTS)
        out, st = e.place(jobs)
        fin = e.read_nodes()
        out2 = e.place(jobs)[0] if again else None
    assert st["engine"] == 1, "not the persistent engine"
    assert np.array_equal(out, ref), "placements differ from the oracle"
    assert all(np.array_equal(a, b) for a, b in zip(fin, rfin)), "node state differs from the oracle"
    return st, out2


@pytest.mark.parametrize("kw", WINDOWS)
def test_exact_fit_within_capacity_and_retired(monkeypatch, kw):
    case = _case("exact", 180)
    assert np.unique(case[2]).size == 180 and case[2].min() >= 0  # 180 fresh nodes, all filled
    st, _ = _check(monkeypatch, case, kw)
    if not kw:  # the whole queue in the first window: without recycling the set fills and stops it
        assert st["rounds"] == 1 and st["stops_dirty"] == 0


@pytest.mark.parametrize("kw", WINDOWS)
def test_zero_demand_jobs_land_on_exhausted_nodes(monkeypatch, kw):
    case = _case("zero")
    nodes, jobs, ref = case[0], case[1], np.asarray(case[2]).reshape(-1)
    assert (ref[180:] >= 0).all()
    # the oracle: every CPU-free job lands on a node whose CPUs the first 180 jobs used up
    assert np.array_equal(nodes.cpu_free[ref[:180]], jobs.cpu[:180])
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
def test_dead_by_memory(monkeypatch, kw):
    case = _case("mem")
    assert np.unique(case[2]).size == 180 and (case[3][0] == 999).all() and (case[3][1] == 0).all()
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
def test_dead_by_gpu(monkeypatch, kw):
    case = _case("gpu")
    assert np.unique(case[2]).size == 180 and (case[3][2] == 0).all() and (case[3][0] == 999).all()
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
@pytest.mark.parametrize("comps", [(), (33, 65)])
def test_slot_reuse_under_the_helpers(monkeypatch, comps, kw):
    case = _case("two", *comps)
    ref = np.asarray(case[2]).reshape(-1)
    assert (ref >= 0).all() and (np.bincount(ref) == 2).all()  # every node takes exactly two jobs
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
def test_retired_list_full(monkeypatch, kw):
    case = _case("exact", 300)
    assert np.unique(case[2]).size == 300
    st, _ = _check(monkeypatch, case, kw)
    # 300 fresh nodes exceed the set and the retired list together wherever one window holds them
    if kw.get("window_max", 8192) >= 256:
        assert st["stops_dirty"] >= 1


@pytest.mark.parametrize("kw", WINDOWS)
def test_retired_rows_pending_at_round_end(monkeypatch, kw):
    """The window ends at its last job with retired rows not yet written back; a second placement of
    the same jobs on the same table finds every node used up — unless a retired row never reached
    the node table, which `read_nodes()` and the second placement would both show."""
    case = _case("exact", 180)
    _, out2 = _check(monkeypatch, case, kw, again=True)
    assert (np.asarray(out2) == -1).all(), "a job fits a node the first placement had filled"

"""Item staleness in the multi-wave commit: the decider drops a record item whose
node was written after the helper's snapshot.  It reads that off the LDS word the helper named in
the item — a clean item's bitmap word, a dirty item's row version — so these cases put each kind
of item, and the edges of the words they point at, on the GPU against the oracle (bit-exact
placements and node state, persistent engine, four window policies; `window_max=8` decides jobs
in record slots no helper has written yet in that window).  Every case also asserts, on the
oracle's own output, the property it exists for."""
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


def _uniform_nodes(n, cpu, mem, gpu):
    return synth.Nodes(cpu_free=np.full(n, cpu, np.int32), mem_free=np.full(n, mem, np.int32),
                       gpu_free=np.full(n, gpu, np.int32), avail_min=np.full(n, I32_MAX, np.int32),
                       part_mask=np.ones(n, np.uint32))


def _uniform_jobs(j, cpu, mem):
    return synth.Jobs(cpu=np.full(j, cpu, np.int32), mem=np.full(j, mem, np.int32),
                      gpu=np.zeros(j, np.int32), wall=np.ones(j, np.int32),
                      part=np.zeros(j, np.uint16), nodes_k=np.ones(j, np.uint16))


def _repeat_dirty():
    """Best fit keeps filling the node it just took: the winning item is the dirty row written by
    the previous job, which is stale in every record snapshotted before that job."""
    return _uniform_nodes(96, 64, 262_144, 0), _uniform_jobs(4096, 1, 1024)


def _whole_nodes():
    """Every job takes a whole clean node: each record's clean items turn dirty one by one under
    the helpers.  With identical nodes every job has the same short candidate list, so each round
    stops for a rescan after a few placements and its dirty set never fills (that is
    `_exact_fit`'s part)."""
    return _uniform_nodes(700, 64, 262_144, 0), _uniform_jobs(3000, 64, 1024)


def _exact_fit():
    """300 nodes of 1..300 free CPUs in a seeded order and 300 jobs asking for 1..300 CPUs in
    another: best fit sends every job to the one node it fills exactly, which no other job wants
    first, so every job's best candidate stays clean until its turn and a window of more than UCAP
    (128) jobs takes its 129th fresh node with candidates left — the dirty-full stop, in the same
    step as a clean item's win."""
    rng = np.random.default_rng(13)
    nodes = _uniform_nodes(300, 0, 262_144, 0)
    nodes.cpu_free[:] = rng.permutation(300) + 1
    jobs = _uniform_jobs(300, 0, 1024)
    jobs.cpu[:] = rng.permutation(300) + 1
    return nodes, jobs


def _two_parts(a, b):
    """Two disjoint partitions of a and b nodes: the second component's first bitmap word starts
    at a node position that is no multiple of 32, and a / b straddle the word edges."""
    rng = np.random.default_rng(11)
    n, j = a + b, 6000
    nodes = synth.Nodes(cpu_free=rng.integers(128, 385, n).astype(np.int32),
                        mem_free=rng.integers(200_000, 1_000_001, n).astype(np.int32),
                        gpu_free=rng.integers(0, 9, n).astype(np.int32),
                        avail_min=np.full(n, I32_MAX, np.int32),
                        part_mask=np.where(np.arange(n) < a, 1, 2).astype(np.uint32))
    jobs = synth.Jobs(cpu=rng.integers(1, 9, j).astype(np.int32),
                      mem=rng.integers(100, 4000, j).astype(np.int32),
                      gpu=np.where(rng.random(j) < 0.2, 1, 0).astype(np.int32),
                      wall=rng.integers(1, 500, j).astype(np.int32),
                      part=rng.integers(0, 2, j).astype(np.uint16),
                      nodes_k=np.ones(j, np.uint16))
    return nodes, jobs


def _dying_jobs():
    """tests/test_live_jobs_gpu.py's "jobs dying inside the round" shape: 64 nodes, 6,000 jobs, 90 %
    live at the start, most of which no node fits any more when their turn comes — ring lanes of
    unplaced live jobs between those of placed ones."""
    rng = np.random.default_rng(8)
    n, j = 64, 6000
    nodes = synth.Nodes(cpu_free=rng.integers(4, 33, n).astype(np.int32),
                        mem_free=rng.integers(4096, 65537, n).astype(np.int32),
                        gpu_free=rng.integers(0, 5, n).astype(np.int32),
                        avail_min=np.full(n, I32_MAX, np.int32),
                        part_mask=np.where(np.arange(n) % 5 == 0, 3, 1).astype(np.uint32))
    rng = np.random.default_rng(7)
    live = rng.random(j) < 0.9
    part = np.where(rng.random(j) < 0.3, 1, 0).astype(np.uint16)
    rng = np.random.default_rng(9)
    jobs = synth.Jobs(cpu=np.where(live, rng.integers(1, 9, j), 10_000).astype(np.int32),
                      mem=rng.integers(100, 4000, j).astype(np.int32),
                      gpu=np.where(rng.random(j) < 0.2, 1, 0).astype(np.int32),
                      wall=rng.integers(1, 500, j).astype(np.int32), part=part,
                      nodes_k=np.ones(j, np.uint16))
    return nodes, jobs, live


@functools.lru_cache(maxsize=None)
def _case(name, *args):
    """A case's inputs and its oracle answer, computed once and shared by the window policies."""
    made = {"repeat": _repeat_dirty, "whole": _whole_nodes, "exact": _exact_fit, "parts": _two_parts,
            "dying": _dying_jobs}[name](*args)
    nodes, jobs = made[0], made[1]
    ref, _, rfin = po.ref_place(nodes, jobs, PARTS)
    ref = np.asarray(ref).copy()
    ref.setflags(write=False)
    return nodes, jobs, ref, rfin, made[2:]


def _check(monkeypatch, case, kw):
    nodes, jobs, ref, rfin, _ = case
    monkeypatch.setenv("FIT_ENGINE", "persistent")
    with Engine(device=0, **kw) as e:
        e.load_nodes(nodes)
        e.load_partitions(PARTS)
        out, st = e.place(jobs)
        fin = e.read_nodes()
    assert st["engine"] == 1, "not the persistent engine"
    assert np.array_equal(out, ref), "placements differ from the oracle"
    assert all(np.array_equal(a, b) for a, b in zip(fin, rfin)), "node state differs from the oracle"
    return st


def _picks(ref, jobs, part=None):
    """Nodes of the placed jobs (of one partition) in job order, the fraction of them equal to the
    pick before, and how many are a node's first pick."""
    p = np.asarray(ref).reshape(jobs.j, -1)[:, 0]
    p = p[(p >= 0) if part is None else (p >= 0) & (jobs.part == part)]
    same = float((p[1:] == p[:-1]).mean()) if p.size > 1 else 0.0
    return p, same, np.unique(p).size


@pytest.mark.parametrize("kw", WINDOWS)
def test_dirty_item_stale_on_almost_every_job(monkeypatch, kw):
    case = _case("repeat")
    p, same, _ = _picks(case[2], case[1])
    assert p.size == 4096 and same >= 0.9  # the oracle: 98.5 % take the previous job's node
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
def test_clean_items_turn_dirty_under_the_helpers(monkeypatch, kw):
    case = _case("whole")
    p, _, first = _picks(case[2], case[1])
    assert p.size == 700 and first == 700  # every placement is a node's first
    st = _check(monkeypatch, case, kw)
    assert st["stops_dirty"] + st["stops_rescan"] >= 1  # rounds cut short inside their window


@pytest.mark.parametrize("kw", WINDOWS)
def test_dirty_set_fills(monkeypatch, kw):
    case = _case("exact")
    nodes, jobs, ref = case[0], case[1], case[2]
    p, _, first = _picks(ref, jobs)
    assert p.size == 300 and first == 300  # every placement is a node's first ...
    assert np.array_equal(nodes.cpu_free[p], jobs.cpu)  # ... and fills it exactly
    st = _check(monkeypatch, case, kw)
    # a round takes at most its window's jobs: only a window over UCAP = 128 jobs can fill the set
    if kw.get("window_max", 8192) > 128:
        assert st["stops_dirty"] >= 1


@pytest.mark.parametrize("kw", WINDOWS)
@pytest.mark.parametrize("a,b", [(31, 32), (33, 65), (64, 97), (1, 160)])
def test_bitmap_word_edges_with_a_second_component(monkeypatch, a, b, kw):
    case = _case("parts", a, b)
    ref, jobs = case[2], case[1]
    assert _picks(ref, jobs)[0].size >= jobs.j // 2
    for part, size in ((0, a), (1, b)):
        p, _, first = _picks(ref, jobs, part)
        assert (p[1:] == p[:-1]).any(), "no repeat pick"
        assert first >= min(2, size), "no fresh pick after the first"
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
def test_unplaced_live_jobs_between_placed_ones(monkeypatch, kw):
    case = _case("dying")
    live = case[4][0]
    p = np.asarray(case[2]).reshape(-1)
    assert ((p < 0) & live).sum() > 0 and (p >= 0).sum() > 0
    st = _check(monkeypatch, case, kw)
    assert st["unplaced"] > (~live).sum()  # jobs that died during their round too

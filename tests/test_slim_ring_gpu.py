"""The decider's slim ring (DESIGN.md §3.7 "The chain diet"): in a component that is exactly one
partition the ring carries no partition mask and no node id — the winner's position is parked as
the placement and translated to the node id where 64 placements are stored, one group late.
Components of several partitions keep the full ring.  Every case forces the persistent engine and
compares placements, the final node columns and the counts with the oracle, bit for bit."""
import functools

import numpy as np
import pytest

from fitgpu import Engine, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

I32_MAX = 2**31 - 1
WINDOWS = [dict(), dict(window_min=64, window_max=64), dict(window_min=256, window_max=256),
           dict(window_min=1, window_max=8)]


def _parts(p):
    return synth.Partitions(np.full(p, -1, np.int32), np.full(p, -1, np.int32), np.full(p, -1, np.int32))


def _nodes(cpu, mem, gpu, mask):
    n = np.asarray(mask).size
    f = lambda v: np.full(n, v, np.int32) if np.isscalar(v) else np.asarray(v, np.int32)  # noqa: E731
    return synth.Nodes(cpu_free=f(cpu), mem_free=f(mem), gpu_free=f(gpu),
                       avail_min=np.full(n, I32_MAX, np.int32), part_mask=np.asarray(mask, np.uint32))


def _jobs(cpu, mem, gpu, part, k=1):
    j = np.asarray(part).size
    f = lambda v, t=np.int32: np.full(j, v, t) if np.isscalar(v) else np.asarray(v, t)  # noqa: E731
    return synth.Jobs(cpu=f(cpu), mem=f(mem), gpu=f(gpu), wall=np.ones(j, np.int32),
                      part=f(part, np.uint16), nodes_k=f(k, np.uint16))


def _random(n, j, mask, part, seed, k=1):
    rng = np.random.default_rng(seed)
    return (_nodes(rng.integers(4, 33, n), rng.integers(4096, 65537, n), rng.integers(0, 5, n), mask),
            _jobs(rng.integers(1, 9, j), rng.integers(100, 4000, j), (rng.random(j) < 0.2).astype(np.int32),
                  part, k))


def _single():
    return _random(200, 1500, np.ones(200, np.uint32), np.zeros(1500, np.uint16), 31) + (1,)


def _joined(extra):
    """Partitions 0 and 1 of 150 nodes each, every fifth node of either in both (one component of
    two partitions: the full ring); with `extra`, partition 2 of 100 nodes as well (one partition:
    the slim ring) in the same placement."""
    rng = np.random.default_rng(37)
    mask = np.where(np.arange(300) < 150, 1, 2)
    mask[::5] = 3
    p = 2
    if extra:
        mask = np.concatenate([mask, np.full(100, 4)])
        p = 3
    mask = mask[rng.permutation(mask.size)]
    return _random(mask.size, 1500, mask, rng.integers(0, p, 1500), 41) + (p,)


def _interleaved(n0, n1):
    """Two one-partition components whose node ids interleave (even ids: partition 0), so no node's
    id is its position; n0 / n1 live jobs of 1 CPU on nodes of 70 to 100 (best fit fills at most
    three nodes of a component, all within every job's first candidate list: no rescan), all in
    each component's first round: the decider ends with t = n0 / n1 parked placements."""
    rng = np.random.default_rng(43)
    part = rng.permutation(np.repeat([0, 1], [n0, n1]))
    return (_nodes(rng.integers(70, 101, 400), 65536, 0, 1 + np.arange(400) % 2),
            _jobs(1, 16, 0, part), 2)


def _stop_mid_group():
    """20 jobs of one GPU on the only node that has GPUs, then 300 exact-fit jobs on fresh nodes: a
    256-job window fills the set (64 rows, the GPU node's among them, and 128 retired) about 211
    jobs in, in the middle of a 64-group of parked placements."""
    rng = np.random.default_rng(47)
    cpu = np.concatenate([[1000], rng.permutation(300) + 1])
    gpu = np.concatenate([[20], np.zeros(300, np.int32)])
    return (_nodes(cpu, 262_144, gpu, np.ones(301, np.uint32)),
            _jobs(np.concatenate([np.ones(20, np.int32), rng.permutation(300) + 1]), 1024,
                  np.concatenate([np.ones(20, np.int32), np.zeros(300, np.int32)]), np.zeros(320, np.uint16)), 1)


def _unplaced_tail():
    """10 nodes of 8 CPUs, 10 jobs that fill them, then 200 more of the same: each of those fits a
    node when its round starts (live) and none when its turn comes."""
    return (_nodes(8, 65536, 0, np.ones(10, np.uint32)), _jobs(8, 16, 0, np.zeros(210, np.uint16)), 1)


def _mixed_k():
    """k = 1 and k = 2 jobs in one queue: runs of 150 one-node jobs, then 50 among which every
    third takes two nodes, so some windows go through the decider and some through the single-wave
    commit."""
    i = np.arange(600)
    k = np.where((i % 200 >= 150) & (i % 3 == 0), 2, 1)
    return _random(100, 600, np.ones(100, np.uint32), np.zeros(600, np.uint16), 53, k) + (1,)


def _exact(n):
    """tests/test_recycle_gpu.py's recycling shape: every job fills one fresh node exactly."""
    rng = np.random.default_rng(13)
    return (_nodes(rng.permutation(n) + 1, 262_144, 0, np.ones(n, np.uint32)),
            _jobs(rng.permutation(n) + 1, 1024, 0, np.zeros(n, np.uint16)), 1)


@functools.lru_cache(maxsize=None)
def _case(name, *args, kmax=1):
    """A case's inputs and the oracle's answer, computed once and shared by the window policies."""
    nodes, jobs, p = {"single": _single, "joined": _joined, "inter": _interleaved, "stop": _stop_mid_group,
                      "tail": _unplaced_tail, "mixed": _mixed_k, "exact": _exact}[name](*args)
    ref, rst, rfin = po.ref_place(nodes, jobs, _parts(p), kmax=kmax)
    ref = np.asarray(ref).copy()
    ref.setflags(write=False)
    return nodes, jobs, _parts(p), ref, rst, rfin


def _check(monkeypatch, case, kw, kmax=1, again=False):
    nodes, jobs, parts, ref, rst, rfin = case
    monkeypatch.setenv("FIT_ENGINE", "persistent")
    with Engine(device=0, **kw) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        out, st = e.place(jobs, kmax=kmax)
        fin = e.read_nodes()
        second = (e.place(jobs, kmax=kmax)[0], e.read_nodes()) if again else None
    assert st["engine"] == 1, "not the persistent engine"
    assert np.array_equal(np.asarray(out).reshape(ref.shape), ref), "placements differ from the oracle"
    assert all(np.array_equal(a, b) for a, b in zip(fin, rfin)), "node state differs from the oracle"
    assert (st["placed"], st["unplaced"], st["rejected"]) == (rst["placed"], rst["unplaced"], rst["rejected"])
    return st, second


@pytest.mark.parametrize("kw", WINDOWS)
def test_single_partition_component(monkeypatch, kw):
    _check(monkeypatch, _case("single"), kw)


@pytest.mark.parametrize("kw", WINDOWS)
@pytest.mark.parametrize("extra", [False, True])
def test_joined_partitions_keep_the_full_ring(monkeypatch, extra, kw):
    case = _case("joined", extra)
    nodes, jobs, ref = case[0], case[1], case[3].reshape(-1)
    ok = ref >= 0
    assert ok.sum() > 500
    # the oracle: no job lands on a node outside its partition
    assert ((nodes.part_mask[ref[ok]] >> jobs.part[ok]) & 1).all()
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("counts", [(128, 129), (191, 127), (1, 63)])
def test_node_ids_are_not_positions(monkeypatch, counts):
    case = _case("inter", *counts)
    nodes, jobs, ref = case[0], case[1], case[3].reshape(-1)
    assert (ref >= 0).all() and (ref % 2 == jobs.part).all()  # every job placed, in its partition
    st, _ = _check(monkeypatch, case, {})
    assert st["rounds"] == 1, "the live-job counts no longer end the decider where the case says"


@pytest.mark.parametrize("kw", [dict(), dict(window_min=256, window_max=256)])
def test_stop_inside_a_group_of_64(monkeypatch, kw):
    case = _case("stop")
    assert (case[3] >= 0).all() and np.unique(case[3][20:]).size == 300
    st, _ = _check(monkeypatch, case, kw)
    assert st["stops_dirty"] >= 1 and st["rounds"] >= 2


@pytest.mark.parametrize("kw", WINDOWS)
def test_tail_of_unplaced_live_jobs(monkeypatch, kw):
    case = _case("tail")
    assert (case[3][:10] >= 0).all() and (case[3][10:] == -1).all()
    _check(monkeypatch, case, kw)


@pytest.mark.parametrize("kw", WINDOWS)
def test_one_and_two_node_windows_mixed(monkeypatch, kw):
    case = _case("mixed", kmax=2)
    jobs, ref = case[1], case[3]
    two = jobs.nodes_k == 2
    assert two.sum() > 30 and (ref[two][:, 0] >= 0).sum() > 10
    # the oracle: every id is a node id, once per job slot; one-node jobs leave the second slot empty
    assert ref.min() >= -2 and ref.max() < 100
    assert (ref[two][:, 0] != ref[two][:, 1])[ref[two][:, 0] >= 0].all()
    _check(monkeypatch, case, kw, kmax=2)


@pytest.mark.parametrize("kw", WINDOWS[:3])
def test_round_ends_with_retired_and_dirty_rows(monkeypatch, kw):
    """Every round of the exact-fit queue ends with dirty rows, and with retired rows as well where
    the window holds more than 64 jobs; the second placement on the same context starts from what
    the write-back left in the node table."""
    case = _case("exact", 180)
    nodes, jobs, parts, rfin = case[0], case[1], case[2], case[5]
    _, (out2, fin2) = _check(monkeypatch, case, kw, again=True)
    after = synth.Nodes(cpu_free=rfin[0], mem_free=rfin[1], gpu_free=rfin[2], avail_min=nodes.avail_min,
                        part_mask=nodes.part_mask)
    ref2, _, rfin2 = po.ref_place(after, jobs, parts)
    assert np.array_equal(np.asarray(out2).reshape(ref2.shape), ref2), "second placement differs"
    assert all(np.array_equal(a, b) for a, b in zip(fin2, rfin2)), "node state after the second placement"

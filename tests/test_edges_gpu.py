"""The HIP placement engines at the score caps and the int32 edges: tests/_edge_cases.py's inputs
(capped score fields, scores of exactly 0 and 0xFFFFFFFF, ties decided by position, node fields and
demands at the ends of int32, timelines clamped at INT32_MAX) placed by every engine and compared
bit-exactly with the oracle — placements, start slots, counters, final node state / timelines.
tests/test_edges.py shows on the CPU that these inputs reach those corners and that a wrong
constant in a copy of the key would change the placements.

Sizes are the smallest at which the paths exist: at most 700 nodes (one or two block-slices of
64-row sub-slices), at most 1500 jobs (a few windows), one workgroup per component."""
import functools

import numpy as np
import pytest

from _edge_cases import edge_case
from fitgpu import Engine, _lib, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
SEEDS = list(range(24))     # 6 per family (seed % 4); family 0: 2 per level
TL_SEEDS = list(range(12))  # 3 per family


@functools.lru_cache(maxsize=None)
def case(seed, disjoint=False):
    nodes, jobs, parts, kmax = edge_case(seed, disjoint=disjoint)
    ref, rst, rfin = po.ref_place(nodes, jobs, parts, kmax=kmax)
    for a in (ref, *rfin):
        a.setflags(write=False)
    return nodes, jobs, parts, kmax, ref, rst, rfin


@functools.lru_cache(maxsize=None)
def tl_case(seed):
    nodes, tl, jobs, parts = edge_case(seed, timeline=True)
    rn, rs, rst, rfin = po.ref_place_tl(nodes, tl, jobs, parts)
    for a in (rn, rs, rfin):
        a.setflags(write=False)
    return nodes, tl, jobs, parts, rn, rs, rst, rfin


def check_place(seed, disjoint=False, engine_id=None):
    nodes, jobs, parts, kmax, ref, rst, rfin = case(seed, disjoint)
    r = np.random.default_rng(1000 + seed)
    kw = {} if seed % 3 else {"window_min": int(r.integers(1, 64)), "window_max": int(r.integers(64, 2048))}
    with Engine(**kw) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        out, st = e.place(jobs, kmax=kmax)
        fin = e.read_nodes()
    if engine_id is not None:
        assert st["engine"] == engine_id, st
    bad = np.flatnonzero((out != ref).any(axis=1))
    assert bad.size == 0, f"seed {seed}: first mismatch at job {bad[0]}: {out[bad[0]]} vs {ref[bad[0]]}"
    assert (st["placed"], st["unplaced"], st["rejected"]) == (rst["placed"], rst["unplaced"], rst["rejected"])
    # fit_read_nodes returns a field that was loaded negative as it was loaded (the engine's row
    # holds max(field, -1); k_scatter_nodes writes back only fields >= 0 over the loaded columns), and
    # the oracle keeps the raw value too: the final state is compared as it is, not floored at -1
    for name, a, b in zip(("cpu", "mem", "gpu"), fin, rfin):
        d = np.flatnonzero(a != b)
        assert d.size == 0, f"seed {seed}: final {name} of node {d[0]}: {a[d[0]]} vs {b[d[0]]}"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("engine", ["persistent", "rounds", "direct"])
def test_edge_place(engine, seed, monkeypatch):
    monkeypatch.setenv("FIT_ENGINE", engine)
    check_place(seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_edge_place_class(seed, monkeypatch):
    """Disjoint partitions and at most 48 distinct demands per partition in every family (the
    generator draws the demands of families 0-2 from that many shapes, family 3 has 27): the class
    engine takes every case."""
    monkeypatch.setenv("FIT_ENGINE", "class")
    check_place(seed, disjoint=True, engine_id=3)


def test_zero256_short_lists(monkeypatch):
    """The 256-identical-node case (every 64-row sub-slice holds more than KS rows of score 0) with
    the smallest key count and sub-slice target the plan accepts."""
    monkeypatch.setenv("FIT_ENGINE", "persistent")
    monkeypatch.setenv("FIT_KS_MIN", "2")
    monkeypatch.setenv("FIT_SUB_TARGET", "64")
    check_place(1)


@pytest.mark.parametrize("seed", TL_SEEDS)
@pytest.mark.parametrize("engine", ["persistent", "rounds"])
def test_edge_backfill(engine, seed, monkeypatch):
    monkeypatch.setenv("FIT_ENGINE", engine)
    nodes, tl, jobs, parts, rn, rs, rst, rfin = tl_case(seed)
    with Engine() as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tl)
        node, start, st = e.place_tl(jobs)
        fin = e.read_timeline()
    bad = np.flatnonzero((node != rn) | (start != rs))
    assert bad.size == 0, f"seed {seed}: first mismatch at job {bad[0]}: ({node[bad[0]]}, {start[bad[0]]}) " \
                          f"vs ({rn[bad[0]]}, {rs[bad[0]]})"
    live = nodes.part_mask != 0
    assert np.array_equal(fin[live], rfin[live])
    assert (st["placed"], st["unplaced"], st["rejected"]) == (rst["placed"], rst["unplaced"], rst["rejected"])


def test_timeline_node_count_limit():
    """The backfill key is start << 54 | score << 22 | position: with 2^22 rows, start 1023, an
    all-capped score and the last position would be KEY_INF, "no start".  A table of 2^22 rows in
    partitions (four components of 2^20, the component limit) is refused before anything is built."""
    n = 1 << 22
    col = np.ones(n, np.int32)
    mask = (np.uint32(1) << (np.arange(n, dtype=np.uint32) >> np.uint32(20))).astype(np.uint32)
    with Engine() as e:
        e.load_nodes(synth.Nodes(col, col, col, col, mask))
        assert _lib.lib().fit_load_timeline(e._h, 1024, 1, None, None, None, None, None) == _lib.FIT_E_INVAL

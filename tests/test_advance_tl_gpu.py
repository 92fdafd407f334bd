"""fit_advance_tl on the GPU against a numpy restatement of DESIGN.md §2i (_advance_tl_cases.
ref_advance_tl, over the dense [n, H, 3] timeline): the dense result for every kind of tail, the
headers through every consumer, long run lists at the 64-run step seam, the -1 rules, composition,
the commutation with fit_unplace_tl through the row rewrite, errors that leave the timeline alone and
the device entry point."""
import ctypes as C

import numpy as np
import pytest

import fitgpu
import _advance_tl_cases as ac
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from _devarray import DevArray
from fitgpu import Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


def to_base(e, H, kmax):
    """rand_cluster(H) loaded, the warm-up queue and uc.queue(H, kmax) placed: ac.base(H, kmax)."""
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    e.place_tl_k(uc.reference(H, kmax)[0], kmax)


def same_table(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def tails_of(H, kmax):
    tl = ac.base(H, kmax)
    return {"level": ac.level_tail(H), "null": None, "random": ac.random_tail(tl, 3 * H + kmax)}


# ---- 1. the dense result ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["level", "null", "random"])
@pytest.mark.parametrize("H,kmax", ac.BASES)
def test_dense_result(engine, H, kmax, kind):
    e = engine
    tl0 = ac.base(H, kmax)
    tail = tails_of(H, kmax)[kind]
    for a in (1, 7, H // 2, H - 1, H, H + 5):
        to_base(e, H, kmax)
        if a == 1:
            assert np.array_equal(e.read_timeline(), tl0)  # the engine's base is the reference's
            table = e.read_nodes()
            e.advance_tl(0, tail)
            assert e.read_timeline().tobytes() == tl0.tobytes()  # a == 0: nothing moves
        e.advance_tl(a, tail)
        got = e.read_timeline()
        want = ac.ref_advance_tl(tl0, a, tail)
        assert got.tobytes() == want.tobytes(), (a, np.argwhere((got != want).any(axis=(1, 2)))[:5])
        assert e.advance_tl_ms() > 0
        if a == 1:
            assert same_table(table, e.read_nodes()), "the node table changed"
            assert e.slots == H


# ---- 2. the headers, through every consumer ----------------------------------------------------------------
def test_ceilings_follow_the_tail():
    """An advance by 8 whose tail holds more cpus than any slot of any node ever did: a job that needs
    them, 8 slots long, starts at H - 8 — for every consumer that rejects a node by its header ceiling."""
    H, kmax, a = 64, 8, 8
    nodes, tline, parts = pk.cluster(H)
    tl0 = ac.base(H, kmax)
    tail = ac.level_tail(H).copy()
    big = int(tl0[:, :, 0].max()) + 7
    tail[:, 0] = big
    want = ac.ref_advance_tl(tl0, a, tail)
    job = wk.jobs_of([(big, 0, 0, a * pk.SLOT_MIN, 4, 1)])  # partition 4: the 600 nodes, no limits
    rrows, rnodes = wk.ref_when_k(want, nodes.part_mask, parts, job, pk.SLOT_MIN, 1)
    assert rrows["start"][0] == H - a and rnodes[0, 0] >= 0 and rrows["hosts"][0] >= 100
    with Engine(device=0) as e:
        def setup():
            to_base(e, H, kmax)
            e.advance_tl(a, tail)

        setup()
        row = e.when(job)
        assert row["start"][0] == H - a and row["node"][0] == rnodes[0, 0]
        rows, nk = e.when_k(job, 1)
        assert rows["start"][0] == H - a and nk[0, 0] == rnodes[0, 0] and rows["hosts"][0] == rrows["hosts"][0]
        gn, gs, _ = e.place_tl_k(job, 1)
        assert gs[0] == H - a and gn[0, 0] == rnodes[0, 0]
        setup()
        gn, gs, _ = e.place_tl(job)
        assert gs[0] == H - a and gn[0] == rnodes[0, 0]


@pytest.mark.parametrize("H,kmax,a,kind", [(64, 8, 9, "level"), (64, 8, 32, "random"), (256, 8, 63, "level"),
                                           (64, 1, 8, "random")])
def test_a_queue_placed_after_the_advance(engine, H, kmax, a, kind):
    """cnt and head[]: what the multi-node backfill (and at kmax 1 the persistent engine) places on the
    advanced timeline is what the restatement places on the restated one."""
    e = engine
    nodes, tline, parts = pk.cluster(H)
    tail = tails_of(H, kmax)[kind]
    want = ac.ref_advance_tl(ac.base(H, kmax), a, tail)
    queue = pk.busy_case(H, 100, kmax)
    rn, rs, rfin = pk.ref_place_tl_k(want, nodes.part_mask, parts, queue, pk.SLOT_MIN, kmax)
    assert (rs >= 0).sum() >= 20 and (rs > 0).sum() >= (5 if kind == "level" else 1)
    to_base(e, H, kmax)
    e.advance_tl(a, tail)
    gn, gs, _ = e.place_tl_k(queue, kmax)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs)
    assert np.array_equal(e.read_timeline(), rfin)
    if kmax == 1:
        to_base(e, H, kmax)
        e.advance_tl(a, tail)
        n1, s1, _ = e.place_tl(queue)
        assert np.array_equal(s1, rs) and np.array_equal(n1[s1 >= 0], rn[s1 >= 0, 0])
        assert np.array_equal(e.read_timeline(), rfin)


# ---- 3. long lists ---------------------------------------------------------------------------------------
def test_long_lists(engine):
    """ac.staircase(): a list of H = 256 runs (the full slab row of that horizon) and one of 128.
    Advances across the 64-run step seam, with a tail equal to the last run (merge) and another
    (append: H - a survivors and the tail, H runs at a = 1)."""
    e = engine
    H = 256
    nodes, tline, parts = ac.staircase(H)
    tl0 = ac.staircase_dense(H)
    last = tl0[:, H - 1].copy()
    other = last + 3 * (last != -1)
    for a in (1, 63, 64, 65, 200):
        for tail, extra in ((last, 0), (other, 1), (None, 0)):
            load(e, nodes, tline, parts)
            if a == 1 and extra:
                assert np.array_equal(e.read_timeline(), tl0)
            e.advance_tl(a, tail)
            got = e.read_timeline()
            want = ac.ref_advance_tl(tl0, a, tail)
            assert got.tobytes() == want.tobytes(), (a, extra)
            assert wk.run_counts(got)[ac.STAIR_FULL] == H - a + extra
    # the last state (a = 200, continued): hand windows back on the long nodes, then place a queue
    tl = want
    jobs = wk.jobs_of([(2, 5, 0, 3, 0, 1), (1, 0, 1, 40, 0, 2), (7, 7, 0, 1, 0, 1)])
    node = np.array([[ac.STAIR_FULL, -1], [ac.STAIR_HALF, ac.STAIR_FULL], [ac.STAIR_FULL, -1]], np.int32)
    start = np.array([0, 30, 55], np.int32)
    tl, applied = uc.ref_unplace_tl(tl, jobs, node, start, 1, 2)
    assert e.unplace_tl(jobs, node, start, 2) == applied == 4
    assert np.array_equal(e.read_timeline(), tl)
    queue = pk.stair_jobs(40, 23)
    rn, rs, rfin = pk.ref_place_tl_k(tl, nodes.part_mask, parts, queue, 1, 4)
    gn, gs, st = e.place_tl_k(queue, 4)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and st["placed"] >= 10
    assert np.array_equal(e.read_timeline(), rfin)
    # the full row once more, appended: the queue on a list of H runs
    load(e, nodes, tline, parts)
    e.advance_tl(1, other)
    tl = ac.ref_advance_tl(tl0, 1, other)
    rn, rs, rfin = pk.ref_place_tl_k(tl, nodes.part_mask, parts, queue, 1, 4)
    gn, gs, st = e.place_tl_k(queue, 4)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and st["placed"] >= 10
    assert np.array_equal(e.read_timeline(), rfin)


# ---- 4. the -1 rules -------------------------------------------------------------------------------------
def test_minus_one_rules(engine):
    e = engine
    H, L, a = 16, 5, 4
    nodes = synth.Nodes(cpu_free=np.array([4, 4, 4, 4, -3, 4], np.int32), mem_free=np.full(6, 1000, np.int32),
                        gpu_free=np.full(6, 1, np.int32),
                        avail_min=np.array([9 * L, 3 * L, wk.INF, wk.INF, wk.INF, wk.INF], np.int32),
                        part_mask=np.array([1, 1, 0, 1, 1, 1], np.uint32))
    load(e, nodes, uc.no_events(6, H, L), wk.open_parts(1))
    tl0 = e.read_timeline()
    assert (tl0[0, 9:] == -1).all() and (tl0[0, :9] != -1).all() and (tl0[2] == -1).all()
    tail = np.array([[9, 9, 9], [9, 9, 9], [9, 9, 9], [-1, 2000, 0], [9, 9, 9], [9, 1000, 2]], np.int32)
    e.advance_tl(a, tail)
    got = e.read_timeline()
    assert np.array_equal(got, ac.ref_advance_tl(tl0, a, tail))
    assert (got[0, :5] == [4, 1000, 1]).all() and (got[0, 5:] == -1).all()  # past avail_min: -1 whatever the tail
    assert (got[1] == -1).all()                                              # U <= a: nothing usable is left
    assert (got[2] == -1).all()                                              # in no partition
    assert got[3, 11].tolist() == [4, 1000, 1] and (got[3, 12:] == [-1, 2000, 0]).all()  # -1 per column
    assert (got[4, :, 0] == -1).all() and (got[4, 12:, 1:] == 9).all()       # a column loaded negative
    assert (got[5, :12] == [4, 1000, 1]).all() and (got[5, 12:] == [9, 1000, 2]).all()
    assert wk.run_counts(got).tolist() == [2, 1, 1, 2, 2, 2]


# ---- 5. composition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(1, 1), (7, 57), (63, 64)])
def test_composition(engine, a, b):
    e = engine
    H, kmax = 256, 8
    for tail in (ac.level_tail(H), ac.random_tail(ac.base(H, kmax), a)):
        to_base(e, H, kmax)
        e.advance_tl(a, tail)
        e.advance_tl(b, tail)
        two = e.read_timeline()
        to_base(e, H, kmax)
        e.advance_tl(a + b, tail)
        assert two.tobytes() == e.read_timeline().tobytes()
        assert two.tobytes() == ac.ref_advance_tl(ac.base(H, kmax), a + b, tail).tobytes()


# ---- 6. the commutation with fit_unplace_tl ------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax,a", [(64, 8, 7), (64, 8, 40), (256, 8, 100), (64, 1, 1)])
def test_commutes_with_unplace(engine, H, kmax, a):
    e = engine
    jobs, out, start, fin = uc.reference(H, kmax)
    rows = uc.half(H, kmax)
    sub, snode, sstart = uc.take(jobs, rows), out[rows], start[rows]
    tail = ac.level_tail(H)
    sub2, start2 = ac.rewrite_rows(sub, sstart, a, H, pk.SLOT_MIN)
    assert (start2 < 0).any() or a == 1
    # place, advance, unplace the rewritten rows
    to_base(e, H, kmax)
    e.advance_tl(a, tail)
    e.unplace_tl(sub2, snode, start2, kmax)
    one = e.read_timeline()
    # place, unplace, advance
    to_base(e, H, kmax)
    e.unplace_tl(sub, snode, sstart, kmax)
    e.advance_tl(a, tail)
    two = e.read_timeline()
    want = ac.ref_advance_tl(uc.ref_unplace_tl(fin, sub, snode, sstart, pk.SLOT_MIN, kmax)[0], a, tail)
    assert one.tobytes() == want.tobytes() and two.tobytes() == want.tobytes()
    # every row handed back, by both routes: the advanced start timeline
    all2, allstart2 = ac.rewrite_rows(jobs, start, a, H, pk.SLOT_MIN)
    want = ac.ref_advance_tl(pk.start_timeline(H), a, tail)
    to_base(e, H, kmax)
    e.advance_tl(a, tail)
    e.unplace_tl(all2, out, allstart2, kmax)
    assert e.read_timeline().tobytes() == want.tobytes()
    to_base(e, H, kmax)
    e.unplace_tl(jobs, out, start, kmax)
    e.advance_tl(a, tail)
    assert e.read_timeline().tobytes() == want.tobytes()


# ---- 7. errors leave the timeline unchanged ----------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_errors_and_state():
    n, H, L = 70, 16, 5
    nodes, parts = uc.flat_cluster(n), wk.open_parts(1)
    r = np.random.default_rng(4)
    running = [([int(x)], int(r.integers(0, H * L)), 1, 10, 0) for x in r.integers(0, n, 40)]
    tline = fitgpu.release_events(n, running, H, L)
    tail = np.full((n, 3), 5, np.int32)
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    L_ = _lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ms = C.c_double()
    with Engine(device=0) as e:
        assert _code(lambda: e.advance_tl(1, None)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.advance_tl(1, tail)) == STATE  # no timeline loaded
        assert L_.fit_advance_tl_ms(e._h, C.byref(ms)) == STATE
        e.load_timeline(tline)
        before = e.read_timeline()
        assert wk.run_counts(before).max() >= 3
        assert _code(lambda: e.advance_tl(-1, tail)) == INVAL
        assert _code(lambda: e.advance_tl(-1, None)) == INVAL
        bad = tail.copy()
        bad[n - 1, 2] = -2  # the last node's entry
        assert _code(lambda: e.advance_tl(1, bad)) == INVAL
        assert e.read_timeline().tobytes() == before.tobytes()
        dev = [DevArray(np.ascontiguousarray(bad[:, i])) for i in range(3)]
        assert _code(lambda: e.advance_tl_device(3, *dev)) == INVAL
        assert e.read_timeline().tobytes() == before.tobytes()
        col = np.ascontiguousarray(tail[:, 0])
        for fn, ptr in ((L_.fit_advance_tl, p(col)), (L_.fit_advance_tl_device, C.c_void_p(dev[0].data_ptr()))):
            for args in ((ptr, None, None), (None, ptr, None), (None, None, ptr), (ptr, ptr, None), (None, ptr, ptr)):
                assert fn(e._h, 2, *args) == INVAL, args
                assert fn(e._h, 0, *args) == 0  # a == 0: whatever the pointers are
        assert e.read_timeline().tobytes() == before.tobytes()
        assert L_.fit_advance_tl_ms(e._h, C.byref(ms)) == STATE  # no successful call yet
        e.advance_tl(2, tail)
        assert np.array_equal(e.read_timeline(), ac.ref_advance_tl(before, 2, tail))
        assert L_.fit_advance_tl_ms(e._h, C.byref(ms)) == 0 and ms.value > 0
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.advance_tl(1, tail)) == STATE


def test_sharded_context_is_refused():
    n, H, L = 6, 16, 5
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        load(e, uc.flat_cluster(n), uc.no_events(n, H, L), wk.open_parts(1))
        assert _code(lambda: e.advance_tl(1, np.full((n, 3), 5, np.int32))) == _lib.FIT_E_STATE
        assert _code(lambda: e.advance_tl(1, None)) == _lib.FIT_E_STATE


# ---- 8. the device entry point -------------------------------------------------------------------------------
def test_device_entry(engine):
    e = engine
    H, kmax, a = 64, 8, 7
    tail = ac.random_tail(ac.base(H, kmax), 8)
    to_base(e, H, kmax)
    e.advance_tl(a, tail)
    host = e.read_timeline()
    to_base(e, H, kmax)
    dev = [DevArray(np.ascontiguousarray(tail[:, i])) for i in range(3)]
    e.advance_tl_device(a, *dev)
    assert e.read_timeline().tobytes() == host.tobytes()
    assert host.tobytes() == ac.ref_advance_tl(ac.base(H, kmax), a, tail).tobytes()
    assert e.advance_tl_ms() > 0
    to_base(e, H, kmax)
    e.advance_tl_device(a, None, None, None)  # all NULL: continue
    assert e.read_timeline().tobytes() == ac.ref_advance_tl(ac.base(H, kmax), a, None).tobytes()


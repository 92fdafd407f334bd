"""fit_free_tl on the GPU against a numpy restatement of DESIGN.md §2k (_free_tl_cases.ref_free_tl,
over the dense [n, H, 3] timelines of the other suites' references): profiles as loaded and after
placements, masks and closed columns by hand, long run lists, 64-bit sums, the seams between the
walk's workgroups, the §2k identities, that the call changes nothing, errors and the device entry
point.  All values are integers and every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import fitgpu
import _advance_tl_cases as ac
import _free_tl_cases as fc
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from _devarray import DevArray
from fitgpu import Engine, FitError, _lib, synth

pytestmark = pytest.mark.gpu
EMPTY_ROW = np.array((0, 0, 0, 0, -1, -1, -1), fitgpu.FREE_DTYPE)


def load(e, nodes, tline, parts):
    e.load_nodes(nodes)
    e.load_partitions(parts)
    e.load_timeline(tline)


@pytest.fixture(scope="module")
def engine():
    with Engine(device=0) as e:
        yield e


def check_rows(got, want, what=None):
    assert got.shape == want.shape and got.dtype == fitgpu.FREE_DTYPE
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)[:5]
        raise AssertionError((what, bad.tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:2]]))


def check_conditions(ref, H, what, empties=True):
    """The reference exercises what the case claims, at H >= 64: rows without an open node (empties
    False: a profile of the five populated partitions alone, whose smallest keeps its node open), a
    partition whose open nodes change along the horizon, sums that change from one slot to the next."""
    empty, varying, steps = fc.conditions(ref)
    if H >= 64:
        assert (empty >= 1 or not empties) and varying >= 1 and steps >= 1, (what, empty, varying, steps)


# ---- 1. as loaded and after placements -------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 8, 64, 1024])
def test_as_loaded(engine, H):
    e = engine
    nodes, tline, parts = pk.cluster(H)
    tl, ref = fc.loaded_reference(H, 7)  # partitions 5 and 6 have no node
    check_conditions(ref, H, "loaded")
    assert H == 1 or (ref["nodes"][:5].max(axis=1) > 0).all()
    load(e, nodes, tline, parts)
    if H == 8:
        assert np.array_equal(e.read_timeline(), tl)  # the engine's load is the oracle's
    check_rows(e.free_tl(7), ref, H)
    for p_ in (1, 32):
        check_rows(e.free_tl(p_), fc.ref_free_tl(tl, nodes.part_mask, p_), (H, p_))


def test_horizon_of_100_slots(engine):
    """H = 100 is a multiple of neither 64 nor 256: the threads past the horizon own no slot."""
    e = engine
    nodes, tline, parts = wk.rand_cluster(100, 5, 4100)
    tl = fc.as_loaded(nodes, tline)
    ref = fc.ref_free_tl(tl, nodes.part_mask, 6)
    check_conditions(ref, 100, "H = 100")
    assert wk.run_counts(tl).max() > 4  # lists past the header's four runs
    load(e, nodes, tline, parts)
    check_rows(e.free_tl(6), ref)


@pytest.mark.parametrize("H,kmax", ac.BASES)
def test_after_placements(engine, H, kmax):
    e = engine
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    e.place_tl_k(uc.reference(H, kmax)[0], kmax)
    before = fc.loaded_reference(H, 5)[1]
    for p_ in (5, 32):
        ref = fc.base_reference(H, kmax, p_)
        check_conditions(ref, H, ("base", p_), empties=p_ == 32)
        check_rows(e.free_tl(p_), ref, (H, kmax, p_))
    # the placements took something, and only sums: the open nodes are those of the load
    ref = fc.base_reference(H, kmax, 5)
    assert (ref["cpu"] < before["cpu"]).any() and np.array_equal(ref["nodes"], before["nodes"])
    for f in fc.MAXS:
        assert (ref[f] <= before[f]).all()


# ---- 2. masks and closed columns by hand ---------------------------------------------------------------
def test_masks_and_closed_columns(engine):
    e = engine
    nodes, tline, parts = fc.masks_case()
    tl = fc.as_loaded(nodes, tline)
    H = fc.MASKS_H
    # the case is what it claims: closed everywhere / never usable / cut mid-horizon / in no partition
    assert (tl[4, :, 2] < 0).all() and (tl[4, :, 0] == 9).all()
    assert (tl[5] == -1).all() and (tl[6, :7] >= 0).all() and (tl[6, 7:] == -1).all()
    assert wk.run_counts(tl)[[0, 2]].tolist() == [3, 2]
    load(e, nodes, tline, parts)
    dense = e.read_timeline()
    member = nodes.part_mask != 0  # the node in no partition reads -1; the restatement goes by its mask
    assert np.array_equal(dense[member], tl[member]) and (dense[~member] == -1).all()
    got = {p_: e.free_tl(p_) for p_ in (1, 2, 32)}
    for p_, g in got.items():
        check_rows(g, fc.ref_free_tl(tl, nodes.part_mask, p_), p_)
    # partition 0 by hand: nodes 0, 2, 6 (until its cut), 8; node 4 (gpu -5) and node 5 (avail 0) never
    assert got[1]["nodes"][0].tolist() == [4] * 7 + [3] * 9
    assert got[1]["cpu"][0, 0] == 4 + 8 + 5 + 3 and got[1]["cpu"][0, 15] == (4 + 2 + 1) + (8 + 4) + 3
    assert got[1]["max_gpu"][0].tolist() == [4] * H
    # with parts = 2 the bit-31 members appear nowhere; with 32 they are partition 31
    assert got[2].tobytes() == got[32][:2].tobytes()
    assert got[32]["nodes"][31].tolist() == [3] * 7 + [2] * 9  # nodes 3, 6, 8
    assert (got[32][2:31] == EMPTY_ROW).all()
    # the mask-3 node counts in both partitions
    assert got[2]["nodes"][1, 0] == 3 and got[2]["cpu"][1, 0] == 6 + 8 + 11  # nodes 1, 2, 9
    assert got[2]["cpu"][0, 0] + got[2]["cpu"][1, 0] == tl[[0, 2, 6, 8, 1, 2, 9], 0, 0].sum()


# ---- 3. long lists ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [256, 1024])
def test_long_lists(engine, H):
    """ac.staircase(H): a list of H runs (at 1,024 the full slab row) and one of H / 2, beside flat
    nodes and one cut at slot 100."""
    e = engine
    nodes, tline, parts = ac.staircase(H)
    tl = ac.staircase_dense(H)
    assert wk.run_counts(tl).tolist() == [1, 1, 2, H, H // 2, 1]
    ref = fc.ref_free_tl(tl, nodes.part_mask, 2)
    assert ref["nodes"][0].tolist() == [6] * 100 + [5] * (H - 100)
    assert ref["max_cpu"][0, H - 1] == 4 + H - 1 and (np.diff(ref["cpu"][0, :100]) > 0).all()
    load(e, nodes, tline, parts)
    check_rows(e.free_tl(2), ref)


def test_lists_on_both_sides_of_the_header(engine):
    """Lists of 1 .. 33 runs: at and past the header's four runs, and on each side of the sizes at
    which the search of a long list takes one more step."""
    e = engine
    counts = (1, 2, 3, 4, 5, 6, 8, 9, 16, 17, 33)
    nodes, tline, parts = fc.runs_cluster(64, counts)
    tl = fc.as_loaded(nodes, tline)
    assert tuple(wk.run_counts(tl)) == counts
    ref = fc.ref_free_tl(tl, nodes.part_mask, 1)
    assert ref["cpu"][0, 0] == len(counts) and ref["max_cpu"][0, 63] == 33
    load(e, nodes, tline, parts)
    check_rows(e.free_tl(1), ref)
    # advanced by 12 and 29 slots: longer lists shrink to the header's four runs and to five
    for a, left in ((12, {4, 5, 21}), (29, {4})):
        load(e, nodes, tline, parts)
        e.advance_tl(a, None)
        want = ac.ref_advance_tl(tl, a, None)
        assert left <= set(wk.run_counts(want).tolist())
        check_rows(e.free_tl(1), fc.ref_free_tl(want, nodes.part_mask, 1), a)


def test_a_stair_of_64_and_65_runs(engine):
    e = engine
    nodes, tline, parts = fc.runs_cluster(128, (4, 5, 64, 65))
    tl = fc.as_loaded(nodes, tline)
    assert wk.run_counts(tl).tolist() == [4, 5, 64, 65]
    load(e, nodes, tline, parts)
    check_rows(e.free_tl(1), fc.ref_free_tl(tl, nodes.part_mask, 1))


# ---- 4. 64-bit sums --------------------------------------------------------------------------------------
def test_sums_take_64_bits(engine):
    e = engine
    big = synth.INT32_MAX
    nodes = uc.flat_cluster(5, cpu=big, mem=big, gpu=1)
    load(e, nodes, uc.no_events(5, 8, 5), wk.open_parts(1))
    got = e.free_tl(1)
    assert got["cpu"][0].tolist() == [5 * (2**31 - 1)] * 8 and got["mem"][0].tolist() == [5 * (2**31 - 1)] * 8
    assert got["max_cpu"][0].tolist() == [big] * 8 and got["max_mem"][0].tolist() == [big] * 8
    assert got["gpu"][0].tolist() == [5] * 8 and got["nodes"][0].tolist() == [5] * 8
    check_rows(got, fc.ref_free_tl(fc.as_loaded(nodes, uc.no_events(5, 8, 5)), nodes.part_mask, 1))


# ---- 5. chunk seams --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fc.SEAM_N)
def test_chunk_seams(engine, n):
    """cpu_free[x] = x + 1: the sum is n (n + 1) / 2 and the maximum n, so a node dropped or counted
    twice at the seam between two workgroups shows."""
    e = engine
    H = 64
    nodes = fc.seam_cluster(n)
    load(e, nodes, uc.no_events(n, H, 5), wk.open_parts(1))
    got = e.free_tl(1)
    want = np.empty((1, H), fitgpu.FREE_DTYPE)
    want[:] = np.array((n * (n + 1) // 2, 8192 * n, 2 * n, n, n, 8192, 2), fitgpu.FREE_DTYPE)
    check_rows(got, want, n)
    if n == 5000:  # partials of many workgroups meet in one row
        nodes = fc.seam_cluster(n, spread=True)
        load(e, nodes, uc.no_events(n, H, 5), wk.open_parts(8))
        x = np.arange(n)
        want = np.empty((8, H), fitgpu.FREE_DTYPE)
        for p_ in range(8):
            mem = x[x % 7 == p_] if p_ < 7 else x[x % 11 == 0]
            want[p_] = np.array(((mem + 1).sum(), 8192 * len(mem), 2 * len(mem), len(mem), mem.max() + 1, 8192, 2),
                                fitgpu.FREE_DTYPE)
        assert want["nodes"][7, 0] == 455 and want["nodes"][:7].sum(axis=0)[0] == n
        check_rows(e.free_tl(8), want, "spread")


# ---- 6. the identities of §2k ----------------------------------------------------------------------------
def test_identities(engine):
    e = engine
    H, kmax, P = 64, 8, 5
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    tl0 = pk.start_timeline(H)
    row0 = e.free_tl(P)
    check_rows(row0, fc.ref_free_tl(tl0, nodes.part_mask, P))
    # fit_when_k: `now` of the zero-demand one-slot job is the open members at slot 0.  Its wall of
    # slot_min minutes passes partition 0's walltime limit; partition 1 limits cpus and memory only
    zero = wk.jobs_of([(0, 0, 0, pk.SLOT_MIN, p_, 1) for p_ in range(P)])
    rows, _ = e.when_k(zero, 1)
    assert (rows["members"] > 0).all() and (rows["code"] == fitgpu.FIT_ETA_NOW).all()
    assert rows["now"].tolist() == row0["nodes"][:, 0].tolist() and rows["now"].min() >= 1
    # placement: the sums fall by the demands of the placed windows, in every partition of their nodes
    queue = pk.busy_case(H, 100, kmax)
    gn, gs, st = e.place_tl_k(queue, kmax)
    assert st["placed"] >= 20 and (gs > 0).any()
    row1 = e.free_tl(P)
    d = fc.deltas(nodes, queue, gn, gs, pk.SLOT_MIN, P, H)
    assert (d.sum(axis=(1, 2)) > 0).sum() >= 3
    for c, f in enumerate(fc.SUMS):
        assert np.array_equal(row0[f] - row1[f], d[:, :, c]), f
    assert np.array_equal(row0["nodes"], row1["nodes"])
    for f in fc.MAXS:
        assert (row1[f] <= row0[f]).all()
    want1 = pk.ref_place_tl_k(tl0, nodes.part_mask, parts, queue, pk.SLOT_MIN, kmax)[2]
    check_rows(row1, fc.ref_free_tl(want1, nodes.part_mask, P))
    # unplace of exactly the placed rows restores every row bit for bit
    e.unplace_tl(queue, gn, gs, kmax)
    check_rows(e.free_tl(P), row0, "unplace")
    # advance: row'[p][t] == row[p][t + a]
    gn, gs, _ = e.place_tl_k(queue, kmax)
    a = 9
    e.advance_tl(a, ac.level_tail(H))
    row2 = e.free_tl(P)
    assert row2[:, :H - a].tobytes() == np.ascontiguousarray(row1[:, a:]).tobytes()
    check_rows(row2, fc.ref_free_tl(ac.ref_advance_tl(want1, a, ac.level_tail(H)), nodes.part_mask, P))


def test_partition_free_agrees_without_reservations(engine):
    """No reservation, every member usable at slot 0, no negative column: row[p][0] is fit_partition_free."""
    e = engine
    n, H = 300, 16
    nodes = fc.seam_cluster(n, spread=True)
    load(e, nodes, uc.no_events(n, H, 5), wk.open_parts(8))
    got = e.free_tl(8)
    for p_ in range(8):
        f = e.partition_free(p_)
        assert (got["cpu"][p_, 0], got["mem"][p_, 0], got["gpu"][p_, 0]) == (f["cpu"], f["mem_mib"], f["gpu"])
    # ... and once a reservation is on the timeline it no longer does: fit_partition_free does not see it
    job = wk.jobs_of([(1, 1, 1, 5, 0, 1)])
    _, gs, _ = e.place_tl_k(job, 1)
    assert gs[0] == 0
    assert e.free_tl(8)["cpu"][0, 0] == e.partition_free(0)["cpu"] - 1


# ---- 7. read-only ----------------------------------------------------------------------------------------
def test_the_call_changes_nothing(engine):
    e = engine
    H, kmax = 64, 8
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    e.place_tl(pk.pre_jobs(H))
    tl, table = e.read_timeline(), e.read_nodes()
    assert tl.tobytes() == pk.start_timeline(H).tobytes()
    one = e.free_tl(32)
    assert e.read_timeline().tobytes() == tl.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(table, e.read_nodes()))
    assert e.free_tl(32).tobytes() == one.tobytes()
    # the headers were not disturbed: a queue placed after the call lands where the reference puts it
    jobs, rn, rs, rfin = pk.reference("busy", H, 300, kmax)
    gn, gs, _ = e.place_tl_k(jobs, kmax)
    assert np.array_equal(gn, rn) and np.array_equal(gs, rs) and (rs >= 0).sum() >= 20
    assert np.array_equal(e.read_timeline(), rfin)


# ---- 8. errors and entry points ----------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(FitError) as ei:
        fn()
    return ei.value.code


def test_errors_and_state():
    n, H, L = 70, 16, 5
    nodes, parts = uc.flat_cluster(n), wk.open_parts(1)
    INVAL, STATE = _lib.FIT_E_INVAL, _lib.FIT_E_STATE
    L_ = _lib.lib()
    ms = C.c_double()
    with Engine(device=0) as e:
        assert _code(lambda: e.free_tl(1)) == STATE  # before load_nodes
        e.load_nodes(nodes)
        e.load_partitions(parts)
        assert _code(lambda: e.free_tl(1)) == STATE  # no timeline loaded
        assert L_.fit_free_tl_ms(e._h, C.byref(ms)) == STATE
        e.load_timeline(uc.no_events(n, H, L))
        before = e.read_timeline()
        assert _code(lambda: e.free_tl(0)) == INVAL
        assert _code(lambda: e.free_tl(33)) == INVAL
        assert _code(lambda: e.free_tl(-1)) == INVAL
        assert L_.fit_free_tl(e._h, 1, None) == INVAL and L_.fit_free_tl_device(e._h, 1, None) == INVAL
        assert _code(e.free_tl_ms) == STATE  # no successful call yet
        got = e.free_tl(2)
        assert e.free_tl_ms() > 0
        assert got["nodes"].tolist() == [[n] * H, [0] * H] and (got[1] == EMPTY_ROW).all()
        assert e.read_timeline().tobytes() == before.tobytes()
        e.load_nodes(nodes)  # drops the timeline
        assert _code(lambda: e.free_tl(1)) == STATE


def test_no_node_in_any_partition():
    n, H = 5, 8
    with Engine(device=0) as e:
        load(e, uc.flat_cluster(n, mask=np.zeros(n, np.uint32)), uc.no_events(n, H, 5), wk.open_parts(1))
        got = e.free_tl(3)
        assert got.shape == (3, H) and (got == EMPTY_ROW).all()


def test_sharded_context_is_refused():
    n, H, L = 6, 16, 5
    with Engine(device=0, flags=fitgpu.FIT_FLAG_COLLECTIVES) as e:
        load(e, uc.flat_cluster(n), uc.no_events(n, H, L), wk.open_parts(1))
        assert _code(lambda: e.free_tl(1)) == _lib.FIT_E_STATE
        dev = DevArray(np.zeros((1, H), fitgpu.FREE_DTYPE))
        assert _code(lambda: e.free_tl_device(1, dev)) == _lib.FIT_E_STATE


def test_device_entry(engine):
    e = engine
    H, P = 64, 7
    nodes, tline, parts = pk.cluster(H)
    load(e, nodes, tline, parts)
    host = e.free_tl(P)
    dev = DevArray(np.full((P, H), np.array((9, 9, 9, 9, 9, 9, 9), fitgpu.FREE_DTYPE)))
    ms = e.free_tl_device(P, dev)
    assert ms > 0 and ms == e.free_tl_ms()
    assert dev.numpy().tobytes() == host.tobytes() == fc.loaded_reference(H, P)[1].tobytes()
    # a device pointer that is not 8-byte aligned is refused before anything is written
    assert _lib.lib().fit_free_tl_device(e._h, P, C.c_void_p(dev.data_ptr() + 4)) == _lib.FIT_E_INVAL
    assert dev.numpy().tobytes() == host.tobytes()

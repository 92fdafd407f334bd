"""fit_hold_tl and fit_unplace_tl share one set of row and grouping buffers in the context (the
counter words, the node id -> position table, the per-position counts and cursors, the touched list,
the windows, the staged node lists and starts).  Calls of the two alternate here on ONE context, with
sizes that shrink and grow, so that a call reading sizes or contents left behind by the other shows:
after every call the timeline, the states and the counts are the numpy restatements' of DESIGN.md
§2h / §2j (_unplace_tl_cases.ref_unplace_tl, _hold_tl_cases.ref_hold_tl), bit for bit."""
import functools

import numpy as np
import pytest

import _hold_tl_cases as hc
import _unplace_tl_cases as uc
import _when_k_cases as wk
from fitgpu import Engine, synth

N, H, SLOT_MIN, LONE = 36, 64, 2, 5  # node LONE is in no partition: it has no run list, every slot reads -1


def rows_of(r, j, kmax, cpu_hi, pool):
    """j rows of 1..kmax distinct nodes of pool: (jobs, node[j, kmax], start[j])."""
    k = r.integers(1, kmax + 1, j).astype(np.uint16)
    node = np.full((j, kmax), -1, np.int32)
    for q in range(j):
        node[q, :k[q]] = r.choice(pool, k[q], replace=False)
    jobs = synth.Jobs(r.integers(0, cpu_hi, j).astype(np.int32), r.integers(0, 2048, j).astype(np.int32),
                      r.integers(0, 2, j).astype(np.int32), r.integers(0, H * SLOT_MIN, j).astype(np.int32),
                      np.zeros(j, np.uint16), k)
    return jobs, node, r.integers(0, H, j).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case():
    """The four calls and what the restatements say after each, from the dense timeline of the idle
    cluster: [(call, jobs, node, start, kmax, timeline after, state, applied, refused)]."""
    r = np.random.default_rng(2718)
    pool = np.delete(np.arange(N), LONE)
    tl = np.empty((N, H, 3), np.int32)
    tl[:] = (16, 8192, 8)
    tl[LONE] = -1
    steps = []
    # 1. about 50 rows at kmax 8: most held, the greedy ones refused, two skipped
    j1, n1, s1 = rows_of(r, 50, 8, 5, pool)
    s1[[11, 37]] = -1
    tl, st1, ap, rf = hc.ref_hold_tl(tl, j1, n1, s1, SLOT_MIN, 8)
    assert (st1 == hc.HELD).sum() >= 20 and rf >= 1 and (st1 == hc.SKIPPED).sum() == 2
    steps.append(("hold", j1, n1, s1, 8, tl, st1, ap, rf))
    # 2. 3 rows at kmax 1, one of them on the node in no partition (its slots stay -1)
    j2, n2, s2 = rows_of(r, 3, 1, 5, pool)
    n2[1, 0] = LONE
    tl, ap = uc.ref_unplace_tl(tl, j2, n2, s2, SLOT_MIN, 1)
    assert ap == 3 and (tl[LONE] == -1).all()
    steps.append(("unplace", j2, n2, s2, 1, tl, None, ap, None))
    # 3. 5 rows at kmax 2: row 0 asks for more than any slot has, row 1 names the node in no
    # partition among its two, row 2 is skipped, rows 3 and 4 are held
    j3 = wk.jobs_of([(1000, 1, 0, 9, 0, 1), (1, 1, 0, 9, 0, 2), (1, 1, 0, 9, 0, 1), (1, 16, 1, 30, 0, 2),
                     (0, 1, 0, 1, 0, 1)])
    n3 = np.array([[3, -1], [4, LONE], [6, -1], [7, 8], [9, -1]], np.int32)
    s3 = np.array([2, 5, -1, 60, H - 1], np.int32)
    before = tl
    tl, st3, ap, rf = hc.ref_hold_tl(tl, j3, n3, s3, SLOT_MIN, 2)
    assert st3.tolist() == [hc.REFUSED, hc.REFUSED, hc.SKIPPED, hc.HELD, hc.HELD] and (ap, rf) == (3, 2)
    assert (tl[4] == before[4]).all()  # the refused row's good node is left alone
    steps.append(("hold", j3, n3, s3, 2, tl, st3, ap, rf))
    # 4. the first call's held rows handed back at kmax 8, in launch sequences of 7 rows
    held = np.flatnonzero(st1 == hc.HELD)
    j4, n4, s4 = uc.take(j1, held), np.ascontiguousarray(n1[held]), np.ascontiguousarray(s1[held])
    tl, ap = uc.ref_unplace_tl(tl, j4, n4, s4, SLOT_MIN, 8)
    assert len(held) > 3 * 7 and ap == steps[0][7]
    steps.append(("unplace", j4, n4, s4, 8, tl, None, ap, None))
    for step in steps:
        step[5].setflags(write=False)
    return steps


def test_case_is_not_vacuous():
    """The restatements alone (no GPU): case() asserts held, refused and skipped rows in both holds."""
    assert [s[0] for s in case()] == ["hold", "unplace", "hold", "unplace"]


@pytest.mark.gpu
def test_hold_and_unplace_alternate_on_one_context(monkeypatch):
    mask = np.ones(N, np.uint32)
    mask[LONE] = 0
    with Engine(device=0) as e:
        e.load_nodes(uc.flat_cluster(N, cpu=16, gpu=8, mask=mask))
        e.load_partitions(wk.open_parts(1))
        e.load_timeline(uc.no_events(N, H, SLOT_MIN))
        for i, (call, jobs, node, start, kmax, want, wstate, wapplied, wrefused) in enumerate(case()):
            if call == "hold":
                state, applied, refused = e.hold_tl(jobs, node, start, kmax)
                assert np.array_equal(state, wstate), (i, np.flatnonzero(state != wstate)[:8])
                assert (applied, refused) == (wapplied, wrefused), i
            else:
                if i == 3:
                    monkeypatch.setenv("FIT_UTL_CHUNK", "7")  # test-only, read at call time
                assert e.unplace_tl(jobs, node, start, kmax) == wapplied, i
            got = e.read_timeline()
            assert got.tobytes() == want.tobytes(), (i, np.argwhere((got != want).any(axis=(1, 2)))[:5])

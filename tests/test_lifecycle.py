"""The lifecycle sequences of tests/_lifecycle_cases.py on the model alone (no GPU): what the seeded
sequences must reach so that tests/test_lifecycle_gpu.py does not compare nothing — conditions on the
restatements, fixed here and met by the seeds recorded in the cases module — and the identities the
harness itself rests on."""
import collections
import functools

import numpy as np
import pytest

import _evicted_tl_cases as ec
import _lifecycle_cases as lc
import _preempt_tl_cases as tc
from fitgpu import synth


@functools.lru_cache(maxsize=None)
def tally(H):
    t = collections.Counter()
    for seed in lc.SEEDS[H]:
        lc.watch(H, seed, t)
    return t


@pytest.mark.parametrize("H", [16, 64, 256])
def test_the_sequences_are_not_vacuous(H):
    t = tally(H)
    assert len(lc.SEEDS[H]) == 6 and 40 <= lc.STEPS[H] <= 60
    # 1. every step kind, and an advance past the whole horizon
    assert all(t[k] >= 3 for k in lc.KINDS), {k: t[k] for k in lc.KINDS}
    assert t["advance_whole"] >= 1
    # 2. starts in the future   3. holds refused and held
    assert t["placed_later"] >= 20
    assert t["refused"] >= 10 and t["held"] >= 20
    # 4. evictions asked for, on more than one node at once too
    assert t["evict_rows"] >= 10 and t["evict_rows_multi"] >= 1
    # 5. entries evicted: some that have ended (e' = 0), some over a closed slot
    assert t["evicted"] >= 30 and t["evicted_e0"] >= 3 and t["evicted_shut"] >= 3
    assert t["evict_shifted"] >= 2  # calls under a shift that is neither 0 nor the whole horizon
    # 6. fit_set_tl rows that are ignored and rows that change nothing
    assert t["set_ignored"] >= 1 and t["set_nothing"] >= 1
    # 7. lists beyond one wave's lanes, and lists that cross the header's TL_HEAD runs both ways
    assert t["longest"] >= 65 or H < 256
    assert t["down"] >= 5 and t["up"] >= 5
    # 8. a column maximum that fell, then rose above all it had been, on a node a later call names
    assert t["ceiling"] >= 3
    # 9. reloads with reservations to hold
    assert t["resync_live"] >= 2


def test_the_long_horizon():
    """One sequence of 25 steps at H = 1024: too short for the counts above; every step kind occurs, a
    list passes one wave's lanes, and holds, evictions and header crossings are there."""
    t = tally(1024)
    assert lc.STEPS[1024] == 25 and len(lc.SEEDS[1024]) == 1
    assert all(t[k] >= 1 for k in lc.KINDS), {k: t[k] for k in lc.KINDS}
    assert t["longest"] >= 65 and t["down"] >= 5 and t["up"] >= 5
    assert t["placed_later"] >= 20 and t["held"] >= 1 and t["evicted"] >= 1 and t["ceiling"] >= 1


def test_the_cluster():
    for H in lc.SEEDS:
        nodes, tline, parts, lists, loaded = lc.cluster(H)
        sizes = [int(((nodes.part_mask >> p) & 1).sum()) for p in range(lc.PARTS)]
        assert sizes[:3] == [1, 63, 65] and sizes[5] == 0 and parts.p == lc.PARTS
        both = int(((nodes.part_mask & 24) == 24).sum())
        assert both >= 3 and sizes[3] > both and sizes[4] > both and (nodes.part_mask == 0).sum() >= 2
        assert 0.1 < (nodes.avail_min < synth.INT32_MAX).mean() < 0.3
        per = np.diff(tline.off)
        assert per.min() == 0 and per.max() >= 10
        rc = lc.wk.run_counts(loaded[nodes.part_mask != 0])
        assert (rc <= lc.TL_HEAD).sum() >= 20 and (rc > lc.TL_HEAD).sum() >= 20
        ends = np.array([e for lst in lists for _, e, _, _, _ in lst])
        assert (ends == 0).any() and (ends == H).any() and len(ends) >= 150
        assert all(lst == sorted(lst, key=lambda e: e[0]) for lst in lists)


def test_unplace_of_rows_just_placed_restores_the_bytes():
    for H in (16, 256):
        m = lc.Model(H)
        r = np.random.default_rng(H)
        m.place_1(lc.gen_jobs(r, 40, H, 1))  # the timeline carries dips already
        before, rows = m.tl.tobytes(), len(m.start)
        want = m.place_k(lc.gen_jobs(r, 150, H, 8), 8)
        new = np.arange(rows, len(m.start))
        assert len(new) == want["placed"] >= 20 and m.tl.tobytes() != before
        assert m.unplace(r.permutation(new))["applied"] == int(np.maximum(m.jobs.nodes_k[new], 1).sum())
        assert m.tl.tobytes() == before


def drop(victims, rows):
    """The lists without the entries `rows` name, every end as it is: the bookkeeping of a device
    that keeps its raw ends."""
    off = np.asarray(victims.off, np.int64)
    keep = np.ones(len(victims.prio), bool)
    keep[off[rows[:, 0]] + rows[:, 1]] = False
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    noff = np.zeros(len(off), np.int32)
    noff[1:] = np.cumsum(np.bincount(owner[keep], minlength=len(off) - 1))
    return synth.VictimsTL(noff, *(np.asarray(getattr(victims, f))[keep] for f in ec.VCOLS[1:]))


@pytest.mark.parametrize("H", [16, 64])
def test_evicted_ends_read_the_same_across_an_advance(H):
    """fit_evicted_tl keeps the raw ends and the shift; the model goes on with e' = max(end - shift, 0)
    and shift 0.  Both read the same at once and after any further advance."""
    r = np.random.default_rng(5 + H)
    m = lc.Model(H)
    m.load_victims(lc.victims_of(m, r))
    m.advance(3, None)
    raw, shift = m.victims, m.shift
    rows = lc.evict_rows(m, r).astype(np.int64)
    m.evict(rows)
    left = drop(raw, rows)
    assert shift == 3 and m.shift == 0 and len(rows) >= 3 and not ec.same_victims(left, m.victims)
    jobs = lc.gen_jobs(r, 60, H, 1)
    prio = r.integers(0, 12, jobs.j).astype(np.int32)
    none = np.zeros((0, 2), np.int64)
    seen = set()
    for a in (0, 1, 2, H // 2, H + 5):
        T = lc.ac.ref_advance_tl(m.tl, a, None)
        sm, sd = min(m.shift + a, H), min(shift + a, H)
        assert ec.same_victims(ec.ref_evicted_tl(T, m.victims, sm, none, m.mask)[1],
                               ec.ref_evicted_tl(T, left, sd, none, m.mask)[1]), a
        want = tc.ref_preempt_tl(m.mask, T, m.victims, m.parts, jobs, prio, m.L, sm)
        assert want.tobytes() == tc.ref_preempt_tl(m.mask, T, left, m.parts, jobs, prio, m.L, sd).tobytes(), a
        seen.add(want.tobytes())
    assert len(seen) >= 2  # the shift matters to the answers


def test_replay_returns_the_prefix():
    H, seed = 64, lc.SEEDS[64][1]
    at = {}
    for i, st, m in lc.steps(H, seed):
        at[i] = (st.kind, st.what, m.tl.tobytes(), m.shift, m.live.sum())
    for upto in (1, 17, lc.STEPS[H]):
        m, done = lc.replay(H, seed, upto)
        assert len(done) == upto and [s.kind for s in done] == [at[i][0] for i in range(upto)]
        assert (done[-1].what, m.tl.tobytes(), m.shift, m.live.sum()) == at[upto - 1][1:]
    m, done = lc.replay(H, seed, 0)
    assert done == [] and m.tl.tobytes() == lc.cluster(H)[4].tobytes()

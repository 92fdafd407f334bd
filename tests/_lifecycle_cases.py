"""The model and the generators of the timeline's lifecycle tests, shared by
tests/test_lifecycle.py and tests/test_lifecycle_gpu.py (not a test module).

Model holds everything a caller can observe of one context with a loaded timeline: the dense
[n, H, 3] timeline, the victims' lists with their shift, the node table as loaded and the ledger of
recorded reservations.  Each of its methods applies one existing restatement (pk.ref_place_tl_k,
uc.ref_unplace_tl, hc.ref_hold_tl, ac.ref_advance_tl, sc.ref_set_tl, ec.ref_evicted_tl, the query
references) and keeps the books; it has no arithmetic of its own about run lists.  steps(H, seed) draws
a seeded sequence of every writer and query from the model's state and yields each step after the
model took it, so that a GPU test runs the same calls on one Engine in lockstep."""
import collections
import functools
from dataclasses import dataclass, field

import numpy as np

import _advance_tl_cases as ac
import _evicted_tl_cases as ec
import _free_tl_cases as fc
import _hold_tl_cases as hc
import _place_tl_k_cases as pk
import _preempt_tl_cases as tc
import _preempt_tl_k_cases as tk
import _set_tl_cases as sc
import _unplace_tl_cases as uc
import _when_cases as wc
import _when_k_cases as wk
from fitgpu import FIT_REJECTED, synth

INT32_MAX = synth.INT32_MAX
TL_HEAD = 4                                      # runs in a node's header (TlHdr.head)
KMAX = 8                                         # the ledger's node columns; fit_unplace_tl / fit_hold_tl's kmax
SLOT_MIN = {16: 1, 64: 5, 256: 30, 1024: 5}      # horizon -> minutes per slot
STEPS = {16: 50, 64: 50, 256: 50, 1024: 25}
# the seeds per horizon for which the reference alone holds the conditions of tests/test_lifecycle.py
SEEDS = {16: (0, 1, 2, 3, 4, 5), 64: (0, 1, 2, 3, 4, 5), 256: (0, 1, 2, 3, 4, 5), 1024: (46,)}
COMPS = (1, 63, 65)                              # partitions 0..2, one component each
GROUP = 30                                       # nodes under the overlapping partition bits 3 and 4, or under none
PARTS = 6                                        # partition 5 is declared without a node, 6 is not declared
ADVANCES = ("1", "2", "3", "7", "H/2", "H-1", "H", "H+5")
KINDS = ("place_k", "place_1", "unplace", "hold", "advance", "set", "victims", "evict", "resync", "bad", "query")
WEIGHTS = (5, 3, 4, 4, 4, 4, 2, 4, 1.5, 1.5, 4)


# ---- the cluster -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cluster(H):
    """(nodes, tline, parts, lists, loaded): about 160 packed nodes.  Every node runs 0 to 12 jobs that
    end inside the horizon, one release event each; up to four of them are preemptible and make the
    node's list of (prio, end, cpu, mem, gpu) in eviction order, and some of those have ended already
    (end 0, nothing held) or outlive the horizon (end H, no event).  What the jobs hold is not in the
    free columns, as synth.gen_victim_ends leaves it at load.  loaded: the dense timeline of the load,
    by the C oracle, -1 on nodes in no partition."""
    from oracle import pyoracle as po
    L = SLOT_MIN[H]
    r = np.random.default_rng(4100 + H)
    group = r.choice([8, 16, 24, 0], GROUP, p=[.3, .3, .25, .15])
    mask = r.permutation(np.concatenate([np.repeat(1 << np.arange(len(COMPS)), COMPS), group])).astype(np.uint32)
    n = len(mask)
    nodes = synth.Nodes(cpu_free=r.integers(0, 4, n).astype(np.int32),
                        mem_free=(1024 + 2048 * r.integers(0, 3, n)).astype(np.int32),
                        gpu_free=r.integers(0, 2, n).astype(np.int32),
                        avail_min=np.where(r.random(n) < 0.2, r.integers(0, H * L + 1, n), INT32_MAX).astype(np.int32),
                        part_mask=mask)
    off, ev, lists = [0], [], []
    for x in range(n):
        k = int(r.integers(0, 13))
        slots = sorted(r.choice(np.arange(1, H), k, replace=False).tolist())
        amounts = [(int(r.integers(1, 9)), int(r.integers(0, 3)) * 4096, int(r.integers(0, 2))) for _ in slots]
        vic = sorted(r.choice(k, min(k, int(r.integers(0, 5))), replace=False).tolist()) if k else []
        lst = []
        for i in vic:
            end = slots[i]
            if r.random() < 0.15:     # it has ended, or it outlives the horizon: no event either way
                end = int(r.choice([0, H]))
                slots[i] = -1
            lst.append((int(r.integers(0, 9)), end, *amounts[i]))
        lists.append(sorted(lst, key=lambda e: e[0]))
        ev += [(s, *a) for s, a in zip(slots, amounts) if s > 0]
        off.append(len(ev))
    a = np.array(ev, np.int64).reshape(-1, 4).astype(np.int32)
    tline = synth.Timeline(slots=H, slot_min=L, off=np.array(off, np.int32), slot=a[:, 0].copy(), cpu=a[:, 1].copy(),
                           mem=a[:, 2].copy(), gpu=a[:, 3].copy())
    parts = synth.Partitions(np.array([H * L // 2 + 1, -1, -1, -1, -1, -1], np.int32),
                             np.array([-1, 48, -1, -1, -1, -1], np.int32),
                             np.array([-1, 100000, -1, -1, -1, -1], np.int32))  # wk.rand_cluster's limits
    loaded = po.ref_build_timeline(nodes, tline)
    loaded[mask == 0] = -1
    loaded.setflags(write=False)
    return nodes, tline, parts, lists, loaded


def gen_jobs(r, j, H, kmax):
    """Demands around the cluster's node sizes, walls from 0 to beyond the horizon, partitions with one
    node, many, none and an undeclared one, nodes_k in 0..kmax with 1 the commonest."""
    L = SLOT_MIN[H]
    cpu = r.choice([0, 1, 2, 4, 8, 16, 40], j, p=[.05, .2, .25, .2, .15, .1, .05]).astype(np.int32)
    mem = (np.maximum(cpu, 1) * r.choice([256, 512, 1024], j)).astype(np.int32)
    gpu = r.choice([0, 0, 0, 1, 2], j).astype(np.int32)
    wall = r.integers(0, max(H * L // 4, 1) + 1, j)
    wall = np.where(r.random(j) < 0.05, r.choice([H * L, H * L + 1], j), wall).astype(np.int32)
    part = r.choice(7, j, p=[.05, .3, .3, .12, .13, .05, .05]).astype(np.uint16)
    k = np.where(r.random(j) < 0.5, 1, r.integers(0, kmax + 1, j)).astype(np.uint16)
    return synth.Jobs(cpu, mem, gpu, wall, part, k)


def empty_jobs():
    z = np.zeros(0, np.int32)
    return synth.Jobs(z, z, z, z, np.zeros(0, np.uint16), np.zeros(0, np.uint16))


def empty_victims(n):
    return tc.victims_tl_of([[] for _ in range(n)])


def list_nodes(a):
    a = np.asarray(a).ravel()
    return np.unique(a[a >= 0])


# ---- the model --------------------------------------------------------------------------------------
class Model:
    def __init__(self, H):
        self.H, self.L = H, SLOT_MIN[H]
        self.nodes, self.tline, self.parts, self.lists, self.loaded = cluster(H)
        self.n, self.mask = self.nodes.n, self.nodes.part_mask
        self.tl = self.loaded.copy()
        self.victims, self.shift = None, 0       # None: no lists loaded (fit_load_timeline drops them)
        self.elapsed = 0                         # slots since the load: the lists' ends are absolute slots
        self.jobs = empty_jobs()                 # the ledger: the rows as fit_unplace_tl / fit_hold_tl take them,
        self.node = np.zeros((0, KMAX), np.int32)    # start -1 once a row has left the horizon,
        self.start = np.zeros(0, np.int32)
        self.live = np.zeros(0, bool)                # live: on the timeline now; else handed back or refused
        self.stats = collections.Counter()
        self.landed = np.zeros(0, np.int64)      # the nodes the last step's placements and answers name

    # -- the ledger
    def record(self, jobs, out, start):
        got = np.flatnonzero(start >= 0)
        node = np.full((len(got), KMAX), -1, np.int32)
        node[:, :out.shape[1]] = out[got]
        self.jobs = uc.concat(self.jobs, uc.take(jobs, got))
        self.node = np.concatenate([self.node, node])
        self.start = np.concatenate([self.start, start[got]]).astype(np.int32)
        self.live = np.concatenate([self.live, np.ones(len(got), bool)])

    def rows(self, idx):
        return uc.take(self.jobs, idx), np.ascontiguousarray(self.node[idx]), np.ascontiguousarray(self.start[idx])

    def handed_back(self):
        return np.flatnonzero(~self.live & (self.start >= 0))

    # -- the writers
    def place_k(self, jobs, kmax):
        out, start, fin = pk.ref_place_tl_k(self.tl, self.mask, self.parts, jobs, self.L, kmax)
        self.tl = fin
        self.record(jobs, out, start)
        self.landed = list_nodes(out[start >= 0])
        placed, rejected = int((start >= 0).sum()), int((out[:, 0] == FIT_REJECTED).sum())
        self.stats["placed"] += placed
        self.stats["placed_later"] += int((start > 0).sum())
        return dict(node=out, start=start, placed=placed, rejected=rejected, unplaced=jobs.j - placed - rejected)

    def place_1(self, jobs):
        """fit_place_tl is fit_place_tl_k with every nodes_k = 1 (§2g); where the C oracle takes the
        starting timeline it must say the same."""
        from oracle import pyoracle as po
        before = self.tl
        want = self.place_k(pk.ones(jobs), 1)
        rn, rs, rst, rfin = po.ref_place_tl(self.nodes, self.tline, jobs, self.parts, tl=before)
        live = self.mask != 0
        assert np.array_equal(rn, want["node"][:, 0]) and np.array_equal(rs, want["start"]), "§2g: the oracle differs"
        assert np.array_equal(rfin[live], self.tl[live]), "§2g: the oracle's timeline differs"
        assert (rst["placed"], rst["unplaced"], rst["rejected"]) == (want["placed"], want["unplaced"], want["rejected"])
        return dict(want, node=want["node"][:, 0].copy())

    def unplace(self, idx):
        jobs, node, start = self.rows(idx)
        self.tl, applied = uc.ref_unplace_tl(self.tl, jobs, node, start, self.L, KMAX)
        self.live[idx] = False
        self.landed = np.zeros(0, np.int64)
        return dict(applied=applied)

    def hold(self, idx):
        jobs, node, start = self.rows(idx)
        self.tl, state, applied, refused = hc.ref_hold_tl(self.tl, jobs, node, start, self.L, KMAX)
        self.live[idx] = state == hc.HELD
        self.stats["held"] += int((state == hc.HELD).sum())
        self.stats["refused"] += refused
        self.landed = np.zeros(0, np.int64)
        return dict(state=state, applied=applied, refused=refused)

    def advance(self, a, tail):
        assert tail is None or (tail >= -1).all()
        self.tl = ac.ref_advance_tl(self.tl, a, tail)
        self.jobs, self.start = ac.rewrite_rows(self.jobs, self.start, a, self.H, self.L)
        self.live &= self.start >= 0
        self.shift = min(self.shift + a, self.H)
        self.elapsed += a
        self.stats["advance_whole"] += int(a >= self.H)
        self.landed = np.zeros(0, np.int64)
        return {}

    def set(self, cols):
        self.tl, applied, ignored = sc.ref_set_tl(self.tl, *cols, self.mask)
        self.stats["set_ignored"] += ignored
        self.landed = np.zeros(0, np.int64)
        return dict(applied=applied, ignored=ignored)

    def load_victims(self, victims):
        """victims None: every list empty.  Kept as fit_read_victims_tl returns them: the list of a
        node in no partition is empty."""
        v = empty_victims(self.n) if victims is None else victims
        self.victims = ec.ref_evicted_tl(self.tl, v, 0, np.zeros((0, 2), np.int64), self.mask)[1]
        self.shift = 0
        self.landed = np.zeros(0, np.int64)
        return {}

    def read_victims(self):
        """What fit_read_victims_tl returns: every end as max(end - shift, 0)."""
        return ec.ref_evicted_tl(self.tl, self.victims, self.shift, np.zeros((0, 2), np.int64), self.mask)[1]

    def evict(self, rows):
        """The restatement returns the ends as e'; the model goes on with them and shift 0, which reads
        the same as the device's raw ends under its unchanged shift (tests/test_lifecycle.py)."""
        rows = np.asarray(rows, np.int64).reshape(-1, 2)
        k = np.asarray(self.victims.off, np.int64)[rows[:, 0]] + rows[:, 1]
        e1 = np.maximum(np.asarray(self.victims.end, np.int64)[k] - self.shift, 0)
        self.stats["evicted"] += len(rows)
        self.stats["evict_shifted"] += int(0 < self.shift < self.H)
        self.stats["evicted_e0"] += int((e1 == 0).sum())
        self.stats["evicted_shut"] += sum(bool((self.tl[x, :e] == -1).any()) for x, e in zip(rows[:, 0], e1))
        self.tl, self.victims = ec.ref_evicted_tl(self.tl, self.victims, self.shift, rows, self.mask)
        self.shift = 0
        self.landed = np.zeros(0, np.int64)
        return {}

    def resync(self):
        """The README's "reload, hold, place the refused rows": fit_load_timeline drops the lists."""
        self.tl = self.loaded.copy()
        self.victims, self.shift, self.elapsed = None, 0, 0
        idx = np.flatnonzero(self.live)
        self.stats["resync_live"] += int(len(idx) > 0)
        held = self.hold(idx)
        refused = idx[held["state"] == hc.REFUSED]
        again = uc.take(self.jobs, refused)
        return dict(rows=self.rows(idx), hold=held, again=again, place=self.place_k(again, KMAX))

    # -- the queries
    def query(self, jobs, prio, kmax):
        args = (self.parts, jobs, prio, self.L)
        when = wc.ref_when(self.tl, self.mask, self.parts, jobs, self.L)
        when_k, when_k_nodes = wk.ref_when_k(self.tl, self.mask, self.parts, jobs, self.L, kmax)
        free = fc.ref_free_tl(self.tl, self.mask, PARTS)
        pre = tc.ref_preempt_tl(self.mask, self.tl, self.victims, *args, self.shift)
        pre_k, pre_k_nodes, pre_k_victims = tk.ref_preempt_tl_k(self.mask, self.tl, self.victims, *args, kmax, self.shift)
        self.stats["evict_rows"] += int((pre["code"] == tc.EVICT).sum())
        self.stats["evict_rows_multi"] += int((pre_k["evict_nodes"] > 1).sum())
        self.landed = list_nodes(np.concatenate([when["node"], when_k_nodes.ravel(), pre["node"], pre_k_nodes.ravel()]))
        return dict(when=when, when_k=when_k, when_k_nodes=when_k_nodes, free=free, pre=pre, pre_k=pre_k,
                    pre_k_nodes=pre_k_nodes, pre_k_victims=pre_k_victims)


# ---- the steps --------------------------------------------------------------------------------------
@dataclass
class Step:
    kind: str
    args: dict
    want: dict = field(default_factory=dict)
    chunk: str = None          # FIT_UTL_CHUNK, FIT_PTLK_CHUNK and FIT_FREE_CHUNK of this step, or None
    device: bool = False       # the *_device entry points where the call has one
    what: str = ""             # the parameters, for the assertion messages


def batch(r):
    return int(r.choice([1, 2, 7, 40, 150, 300]))


def set_rows(m, r):
    """Random windows, drains, resumes written as the loaded run lengths, rows on nodes in no partition,
    a skipped row, a row that changes nothing and, a quarter of the time, sc.random_rows' staircase of
    one-slot rows with alternating levels on one node: shuffled.  (columns, the row that changes nothing)"""
    H = m.H
    inpart, nopart = np.flatnonzero(m.mask != 0), np.flatnonzero(m.mask == 0)
    quiet = int(r.choice(inpart))
    free = inpart[inpart != quiet]

    def level():
        v = [int(r.integers(0, 65)), int(r.integers(0, 9)) * 4096, int(r.integers(0, 5))]
        return [-1 if r.random() < 0.08 else c for c in v]

    rows = []
    for x in r.choice(free, int(r.integers(1, 30)), replace=False).tolist():
        for _ in range(int(r.integers(1, 4))):
            a = int(r.integers(0, H))
            rows.append((x, a, a + int(r.integers(1, H + 1)), *level()))
    if r.random() < 0.25:
        hot = int(r.choice(free))
        rows += [(hot, i % H, i % H + 1, 10 + i % 2 + 2 * (i // H), 4096, i % 2) for i in range(130)]
    rows += [(int(x), 0, INT32_MAX, -1, -1, -1) for x in r.choice(free, int(r.integers(0, 3)), replace=False)]
    rows += sc.runs_as_rows(m.loaded, r.choice(free, int(r.integers(0, 4)), replace=False).tolist())
    rows += [(int(x), int(r.integers(0, H)), INT32_MAX, 4, 4, 4) for x in r.choice(nopart, 2)]
    rows.append((-7, -1, 0, -9, -9, -9))
    end0 = int(np.flatnonzero(np.append((m.tl[quiet, 1:] != m.tl[quiet, :-1]).any(axis=1), True))[0]) + 1
    nothing = (quiet, 0, end0, *m.tl[quiet, 0].tolist())
    rows.append(nothing)
    return sc.cols([rows[i] for i in r.permutation(len(rows))]), sc.cols([nothing])


def victims_of(m, r):
    """About four fifths of the cluster's lists, the ends moved with the clock; one time in ten None."""
    if r.random() < 0.1:
        return None
    return tc.victims_tl_of([[(p, min(max(e - m.elapsed, 0), m.H), c, g, u) for p, e, c, g, u in lst if r.random() < 0.8]
                             for lst in m.lists])


def evict_rows(m, r):
    ln = ec.list_lengths(m.victims, m.n)
    pairs = np.stack([np.repeat(np.arange(m.n), ln), np.concatenate([np.arange(k) for k in ln] + [np.zeros(0, np.int64)])],
                     axis=1).astype(np.int32)
    take = r.permutation(len(pairs))[:max(1, int(len(pairs) * r.choice([0.02, 0.1, 0.4])))]
    return np.ascontiguousarray(pairs[take])


def bad_calls(m, r):
    """One call per writer that the library refuses, the bad row last in its batch."""
    H, n = m.H, m.n
    jobs = gen_jobs(r, 5, H, 4)
    jobs.cpu[-1] = -1
    some = np.flatnonzero(m.start >= 0)[:4]
    rj, rn, rs = m.rows(some)
    one = wk.jobs_of([(1, 1, 0, 1, 0, 1)])
    row = np.full((1, KMAX), -1, np.int32)

    def with_row(x, s):
        row[0, 0] = x
        return uc.concat(rj, one), np.concatenate([rn, row]), np.append(rs, np.int32(s))

    good, _ = set_rows(m, r)
    tail = np.zeros((n, 3), np.int32)
    tail[-1, 2] = -2
    calls = {"place_k": (jobs, 4), "place_1": (jobs,), "unplace": with_row(n, 0), "hold": with_row(0, H),
             "advance": (-1, None) if r.random() < 0.5 else (1, tail),
             "set": tuple(np.concatenate([a, b]) for a, b in zip(good, sc.cols([(0, 5 % H, 5 % H, 0, 0, 0)])))}
    if m.victims is not None:
        ln = ec.list_lengths(m.victims, n)
        x = int(np.argmax(ln))
        rows = evict_rows(m, r)[:3] if ln.sum() else np.zeros((0, 2), np.int32)
        calls["evict"] = np.concatenate([rows[~((rows[:, 0] == x) & (rows[:, 1] == ln[x]))], [[x, ln[x]]]]).astype(np.int32)
    lists = [list(lst) for lst in m.lists]
    x = max(range(n), key=lambda i: len(lists[i]))
    p, _, c, g, u = lists[x][-1]
    lists[x][-1] = (p, H + 1, c, g, u)
    calls["victims"] = tc.victims_tl_of([[(p, min(e, H + 1), c, g, u) for p, e, c, g, u in lst] for lst in lists])
    return calls


def steps(H, seed, count=None):
    """Yields (index, Step, model) for every step of the sequence, after the model took it.  The model
    is the one object all along: read it before asking for the next step."""
    m = Model(H)
    r = np.random.default_rng([H, seed])
    count = STEPS[H] if count is None else count
    p = np.array(WEIGHTS) / sum(WEIGHTS)
    for i in range(count):
        kind = {0: "place_k", 1: "victims", count - 2: "query", count - 1: "place_k"}.get(i) or str(r.choice(KINDS, p=p))
        if kind == "unplace" and not m.live.any():
            kind = "place_k"
        if kind == "hold" and not len(m.handed_back()):
            kind = "unplace" if m.live.any() else "place_k"
        if kind == "evict" and (m.victims is None or not len(m.victims.prio)):
            kind = "victims"
        st = Step(kind, {}, chunk=str(r.choice(["1", "4", "7"])) if r.random() < 1 / 3 else None, device=bool(r.random() < 0.5))
        if kind == "place_k":
            kmax = int(r.choice([4, 8]))
            jobs = gen_jobs(r, batch(r), H, kmax)
            st.args, st.what = dict(jobs=jobs, kmax=kmax), f"{jobs.j} jobs, kmax {kmax}"
            st.want = m.place_k(jobs, kmax)
        elif kind == "place_1":
            jobs = gen_jobs(r, batch(r), H, 1)
            st.args, st.what = dict(jobs=jobs), f"{jobs.j} jobs"
            st.want = m.place_1(jobs)
        elif kind == "unplace":
            live = np.flatnonzero(m.live)
            idx = r.permutation(live)[:max(1, int(len(live) * r.choice([0.05, 0.3, 1.0])))]
            gone = np.flatnonzero(m.start < 0)[:3]  # rows that left the horizon go in as they are: skipped
            idx = r.permutation(np.concatenate([idx, gone]))
            st.args, st.what = dict(rows=m.rows(idx)), f"{len(idx)} rows {idx[:6].tolist()}"
            st.want = m.unplace(idx)
        elif kind == "hold":
            back = m.handed_back()
            idx = r.permutation(back)[:max(1, int(len(back) * r.choice([0.1, 0.5, 1.0])))]
            st.args, st.what = dict(rows=m.rows(idx)), f"{len(idx)} rows {idx[:6].tolist()}"
            st.want = m.hold(idx)
        elif kind == "advance":
            name = str(r.choice(ADVANCES, p=[.2, .2, .15, .15, .1, .07, .07, .06]))
            a = {"H/2": H // 2, "H-1": H - 1, "H": H, "H+5": H + 5}.get(name) or int(name)
            tail = ac.random_tail(m.tl, int(r.integers(1 << 30))) if r.random() < 0.5 else None
            st.args, st.what = dict(a=a, tail=tail), f"a = {a}, tail {'given' if tail is not None else 'none'}"
            st.want = m.advance(a, tail)
        elif kind == "set":
            cols, nothing = set_rows(m, r)
            m.stats["set_nothing"] += int(sc.ref_set_tl(m.tl, *nothing, m.mask)[0].tobytes() == m.tl.tobytes())
            st.args, st.what = dict(cols=cols), f"{len(cols[0])} rows"
            st.want = m.set(cols)
        elif kind == "victims":
            v = victims_of(m, r)
            st.args, st.what = dict(victims=v), "none" if v is None else f"{len(v.prio)} entries"
            st.want = m.load_victims(v)
        elif kind == "evict":
            rows = evict_rows(m, r)
            st.args, st.what = dict(rows=rows), f"{len(rows)} rows {rows[:4].tolist()}"
            st.want = m.evict(rows)
        elif kind == "resync":
            st.want = m.resync()
            st.what = f"{len(st.want['rows'][2])} live rows, {st.want['again'].j} placed again"
        elif kind == "bad":
            st.args = dict(calls=bad_calls(m, r))
        else:
            kmax = int(r.choice([4, 8]))
            jobs = gen_jobs(r, int(r.choice([1, 5, 40, 120])), H, kmax)
            prio = r.integers(0, 12, jobs.j).astype(np.int32)
            st.args, st.what = dict(jobs=jobs, prio=prio, kmax=kmax, load=m.victims is None), f"{jobs.j} jobs, kmax {kmax}"
            if m.victims is None:  # fit_preempt_tl wants lists loaded: a caller without any loads none
                m.load_victims(None)
            st.want = m.query(jobs, prio, kmax)
        m.stats[kind] += 1
        yield i, st, m


def replay(H, seed, upto):
    """(model, steps) after the first `upto` steps of the sequence: a step does not depend on the steps
    that follow it, so a failing step reruns alone from the model of the steps before it."""
    out = []
    m = Model(H)
    if upto > 0:
        for i, st, m in steps(H, seed):
            out.append(st)
            if i + 1 >= upto:
                break
    return m, out


# ---- what the sequences must reach, on the model alone ------------------------------------------------
def watch(H, seed, tally):
    """Run one sequence on the model and add to `tally` what is measured between steps: run counts
    across TL_HEAD, the longest list, and the ceiling events — a node's column maximum fell, later rose
    above every value it had held, and a later placement or answer names the node."""
    m = Model(H)
    rc = wk.run_counts(m.tl)
    cm = m.tl.max(axis=1)
    top = cm.copy()                       # the highest column maximum so far
    fell = np.zeros(cm.shape, bool)
    rose = np.zeros(m.n, bool)
    for i, st, m in steps(H, seed):
        if st.kind in ("place_k", "place_1", "query", "resync"):
            hit = m.landed[rose[m.landed]]
            tally["ceiling"] += len(hit)
            rose[hit] = False
            fell[hit] = False
        now = wk.run_counts(m.tl)
        tally["down"] += int(((rc > TL_HEAD) & (now <= TL_HEAD)).sum())
        tally["up"] += int(((rc <= TL_HEAD) & (now > TL_HEAD)).sum())
        tally["longest"] = max(tally["longest"], int(now.max()))
        rc = now
        new = m.tl.max(axis=1)
        fell |= new < cm
        rose |= (fell & (new > top)).any(axis=1)
        top = np.maximum(top, new)
        cm = new
    tally.update(m.stats)
    return m

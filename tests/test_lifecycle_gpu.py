"""One timeline kept for a whole sequence: seeded random sequences of every call that writes or reads
the loaded timeline (tests/_lifecycle_cases.py) on ONE Engine, in lockstep with the dense model built
from the restatements of DESIGN.md §2d to §2q.  After every step the call's return values, the
timeline, the victims' lists and the node table are the model's, bit for bit; a refused call leaves
all of them alone.  The launch-seam knobs, the host or the device entry points and the batch sizes
change from step to step, so a call that reads sizes, headers or buffers another call left behind
shows.  A failure names the horizon, the seed, the step and its parameters; lc.replay(H, seed, upto)
gives the model and the steps of a prefix."""
import numpy as np
import pytest

import _evicted_tl_cases as ec
import _lifecycle_cases as lc
from _devarray import DevArray
from fitgpu import ETA_DTYPE, ETA_K_DTYPE, EVICT_DTYPE, EVICT_K_DTYPE, FREE_DTYPE, Engine, FitError, _lib

pytestmark = pytest.mark.gpu
CASES = [(H, seed) for H in (16, 64, 256, 1024) for seed in lc.SEEDS[H]]
KNOBS = ("FIT_UTL_CHUNK", "FIT_PTLK_CHUNK", "FIT_FREE_CHUNK")
JC = ("cpu", "mem", "gpu", "wall")


def dev(a):
    return DevArray(np.ascontiguousarray(a))


def filled(shape, dtype=np.int32):
    """A device array of -7 words: whatever the call leaves unwritten shows."""
    words = int(np.prod(shape)) * np.dtype(dtype).itemsize // 4
    return DevArray(np.full(words, -7, np.int32).view(dtype).reshape(shape))


def jcols(jobs, *more):
    return [dev(getattr(jobs, f)) for f in JC + more]


# ---- one call of each kind, through the host or the device entry point --------------------------------
def place_k(e, device, jobs, kmax):
    if device and jobs.j:
        dn, ds = filled((jobs.j, kmax)), filled(jobs.j)
        st = e.place_tl_k_device(*jcols(jobs, "part", "nodes_k"), dn, ds, kmax)
        node, start = dn.numpy(), ds.numpy()
    else:
        node, start, st = e.place_tl_k(jobs, kmax)
    return dict(node=node, start=start, placed=st["placed"], unplaced=st["unplaced"], rejected=st["rejected"])


def place_1(e, device, jobs):
    if device:
        dn, ds = filled(jobs.j), filled(jobs.j)
        st = e.place_tl_device(*jcols(jobs, "part"), dn, ds)
        node, start = dn.numpy(), ds.numpy()
    else:
        node, start, st = e.place_tl(jobs)
    return dict(node=node, start=start, placed=st["placed"], unplaced=st["unplaced"], rejected=st["rejected"])


def unplace(e, device, jobs, node, start):
    if device:
        return dict(applied=e.unplace_tl_device(*jcols(jobs, "nodes_k"), dev(node), dev(start), lc.KMAX))
    return dict(applied=e.unplace_tl(jobs, node, start, lc.KMAX))


def hold(e, device, jobs, node, start):
    if device and len(start):
        out = filled(len(start))
        applied, refused = e.hold_tl_device(*jcols(jobs, "nodes_k"), dev(node), dev(start), out, lc.KMAX)
        return dict(state=out.numpy(), applied=applied, refused=refused)
    state, applied, refused = e.hold_tl(jobs, node, start, lc.KMAX)
    return dict(state=state, applied=applied, refused=refused)


def advance(e, device, a, tail):
    if device:
        e.advance_tl_device(a, *((None,) * 3 if tail is None else [dev(tail[:, c]) for c in range(3)]))
    else:
        e.advance_tl(a, tail)
    return {}


def set_rows(e, device, node, frm, to, levels):
    if device:
        applied, ignored = e.set_tl_device(dev(node), dev(frm), dev(to), *[dev(levels[:, c]) for c in range(3)])
    else:
        applied, ignored = e.set_tl(node, frm, to, levels)
    return dict(applied=applied, ignored=ignored)


def load_victims(e, device, victims):
    if device and victims is not None:
        e.load_victims_tl_device(*(dev(getattr(victims, f)) for f in ec.VCOLS))
    elif device:
        e.load_victims_tl_device(None, None, None, None, None, None)
    else:
        e.load_victims_tl(victims)
    return {}


def evict(e, device, rows):
    if device:
        e.evicted_tl_device(dev(rows[:, 0]), dev(rows[:, 1]))
    else:
        e.evicted_tl(rows[:, 0], rows[:, 1])
    return {}


def query(e, device, jobs, prio, kmax, load, H):
    if load:
        e.load_victims_tl(None)
    j = jobs.j
    if not device:
        when = e.when(jobs)
        when_k, when_k_nodes = e.when_k(jobs, kmax)
        free = e.free_tl(lc.PARTS)
        pre = e.preempt_tl(jobs, prio)
        pre_k, pre_k_nodes, pre_k_victims = e.preempt_tl_k(jobs, prio, kmax)
    else:
        c5, nk, dp = jcols(jobs, "part"), dev(jobs.nodes_k), dev(prio)
        out = [filled(j, ETA_DTYPE), filled(j, ETA_K_DTYPE), filled((j, kmax)), filled((lc.PARTS, H), FREE_DTYPE),
               filled(j, EVICT_DTYPE), filled(j, EVICT_K_DTYPE), filled((j, kmax)), filled((j, kmax))]
        e.when_device(*c5, out[0])
        e.when_k_device(*c5, nk, out[1], out[2], kmax)
        e.free_tl_device(lc.PARTS, out[3])
        e.preempt_tl_device(*c5, dp, out[4])
        e.preempt_tl_k_device(*c5, nk, dp, out[5], out[6], out[7], kmax=kmax)
        when, when_k, when_k_nodes, free, pre, pre_k, pre_k_nodes, pre_k_victims = (o.numpy() for o in out)
    return dict(when=when, when_k=when_k, when_k_nodes=when_k_nodes, free=free, pre=pre, pre_k=pre_k,
                pre_k_nodes=pre_k_nodes, pre_k_victims=pre_k_victims)


BAD = dict(place_k=place_k, place_1=place_1, unplace=unplace, hold=hold, advance=advance, set=set_rows,
           evict=evict, victims=load_victims)


# ---- the comparison ---------------------------------------------------------------------------------
def same(got, want, where):
    """Every value the model says the call returns: arrays byte for byte."""
    for key, w in want.items():
        g = got[key]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            assert g.shape == w.shape and g.dtype == w.dtype, f"{where}: {key} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
            if g.tobytes() != w.tobytes():
                rows = np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))
                q = int(rows[0])
                raise AssertionError(f"{where}: {key} differs in {len(rows)} rows, first {q}: got {g[q]}, want {w[q]}")
        else:
            assert g == w, f"{where}: {key} is {g}, want {w}"


def same_state(e, m, table, where):
    """The timeline, the lists and the node table of the context against the model."""
    got = e.read_timeline()
    if got.tobytes() != m.tl.tobytes():
        bad = np.flatnonzero((got != m.tl).any(axis=(1, 2)))
        x = int(bad[0])
        t = np.flatnonzero((got[x] != m.tl[x]).any(axis=1))
        raise AssertionError(f"{where}: the timeline differs on {len(bad)} nodes {bad[:8].tolist()}; node {x} (mask "
                             f"{int(m.mask[x])}) slots {t[:8].tolist()}: got {got[x, t[:4]].tolist()}, want {m.tl[x, t[:4]].tolist()}")
    if m.victims is not None:
        lists, want = e.read_victims_tl(), m.read_victims()
        if not ec.same_victims(lists, want):
            ln, wn = np.diff(lists.off), np.diff(want.off)
            bad = np.flatnonzero(ln != wn)
            if not len(bad):
                k = np.flatnonzero(np.any([np.asarray(getattr(lists, f)) != np.asarray(getattr(want, f)) for f in ec.VCOLS[1:]], axis=0))
                bad = np.unique(np.repeat(np.arange(m.n), wn)[k])
            x = int(bad[0])
            raise AssertionError(f"{where}: the victims' lists differ on nodes {bad[:8].tolist()}; node {x}: got "
                                 f"{[getattr(lists, f)[lists.off[x]:lists.off[x + 1]].tolist() for f in ec.VCOLS[1:]]}, want "
                                 f"{[getattr(want, f)[want.off[x]:want.off[x + 1]].tolist() for f in ec.VCOLS[1:]]}")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(e.read_nodes(), table)), f"{where}: the node table changed"


class Run:
    """One Engine and one sequence; step() takes the next step on both and compares."""

    def __init__(self, H, seed, monkeypatch):
        self.H, self.seed, self.mp = H, seed, monkeypatch
        if seed % 3 == 1:  # the host-driven rounds behind fit_place_tl; the engine is chosen at fit_create
            monkeypatch.setenv("FIT_ENGINE", "rounds")
        self.e = Engine(device=0)
        monkeypatch.setenv("FIT_ENGINE", "persistent")
        nodes, tline, parts, _, loaded = lc.cluster(H)
        self.e.load_nodes(nodes)
        self.e.load_partitions(parts)
        self.e.load_timeline(tline)
        self.tline = tline
        self.table = self.e.read_nodes()
        assert self.e.read_timeline().tobytes() == loaded.tobytes(), f"H {H}: the loaded timeline differs"
        self.gen = lc.steps(H, seed)
        self.taken = 0

    def close(self):
        self.e.close()

    def step(self):
        nxt = next(self.gen, None)
        if nxt is None:
            return False
        i, st, m = nxt
        e, d = self.e, st.device
        where = f"H {self.H} seed {self.seed} step {i} {st.kind} ({st.what}; chunk {st.chunk}, device {d})"
        for knob in KNOBS:  # read at call time
            if st.chunk:
                self.mp.setenv(knob, st.chunk)
            else:
                self.mp.delenv(knob, raising=False)
        a = st.args
        if st.kind == "place_k":
            same(place_k(e, d, a["jobs"], a["kmax"]), st.want, where)
        elif st.kind == "place_1":
            same(place_1(e, d, a["jobs"]), st.want, where)
        elif st.kind == "unplace":
            same(unplace(e, d, *a["rows"]), st.want, where)
        elif st.kind == "hold":
            same(hold(e, d, *a["rows"]), st.want, where)
        elif st.kind == "advance":
            advance(e, d, a["a"], a["tail"])
        elif st.kind == "set":
            same(set_rows(e, d, *a["cols"]), st.want, where)
        elif st.kind == "victims":
            load_victims(e, d, a["victims"])
        elif st.kind == "evict":
            evict(e, d, a["rows"])
        elif st.kind == "resync":
            e.load_timeline(self.tline)
            same(hold(e, d, *st.want["rows"]), st.want["hold"], where + " hold")
            same(place_k(e, d, st.want["again"], lc.KMAX), st.want["place"], where + " place")
        elif st.kind == "bad":
            for name, args in a["calls"].items():
                with pytest.raises(FitError) as err:
                    BAD[name](e, d, *(args if isinstance(args, tuple) else (args,)))
                assert err.value.code == _lib.FIT_E_INVAL, f"{where}: {name}"
                same_state(e, m, self.table, f"{where}: after the refused {name}")
        else:
            same(query(e, d, a["jobs"], a["prio"], a["kmax"], a["load"], self.H), st.want, where)
        same_state(e, m, self.table, where)
        self.taken += 1
        return True


@pytest.mark.parametrize("H,seed", CASES)
def test_sequence(H, seed, monkeypatch):
    run = Run(H, seed, monkeypatch)
    try:
        while run.step():
            pass
        assert run.taken == lc.STEPS[H]
    finally:
        run.close()


def test_two_contexts_interleaved(monkeypatch):
    """Two sequences of different horizons and seeds, step by step in turn on two contexts of one GPU,
    each against its own model: anything a call keeps outside its context shows."""
    runs = [Run(64, 7, monkeypatch), Run(16, 8, monkeypatch)]
    try:
        more = [True, True]
        while any(more):
            more = [run.step() for run in runs]
        assert [run.taken for run in runs] == [lc.STEPS[64], lc.STEPS[16]]
    finally:
        for run in runs:
            run.close()

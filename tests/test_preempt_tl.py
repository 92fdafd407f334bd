"""fit_preempt_tl's host half (no device): the exports and the unchanged ABI version, argument checks
that must answer before any device call, the reference (tests/_preempt_tl_cases.py ref_preempt_tl) on
a hand-written case with literal rows and a reservation dip, the generators with the recorded seeds,
and text checks of the Go binding (no Go toolchain in the image, as tests/test_go_binding.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _preempt_cases as pc
import _preempt_tl_cases as tc
import fitgpu
from fitgpu import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
SYMS = ("fit_load_victims_tl", "fit_load_victims_tl_device", "fit_preempt_tl", "fit_preempt_tl_device", "fit_preempt_tl_ms")


# ---- exports -------------------------------------------------------------------------------------
def test_exports_and_the_abi_version_is_still_8():
    hdr = open(HDR).read()
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    assert _lib.lib().fit_abi_version() == 8
    for sym in SYMS:
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"^int " + sym + r"\(", hdr, re.M), sym
    for meth in ("load_victims_tl", "load_victims_tl_device", "preempt_tl", "preempt_tl_device", "preempt_tl_ms"):
        assert callable(getattr(fitgpu.Engine, meth))
    # no new struct and no new text: the rows are fit_evict, the message fit_preempt_message
    assert not re.search(r"fit_evict_tl|fit_preempt_tl_message", hdr)


def test_null_and_negative_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.EVICT_DTYPE)
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_preempt_tl, L.fit_preempt_tl_device):
        assert fn(None, 0, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, -1, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(one), p(one), p(out)) == _lib.FIT_E_INVAL
    assert b"null ctx" in L.fit_last_error()
    off = np.zeros(1, np.int32)
    assert L.fit_load_victims_tl(None, p(off), None, None, None, None, None) == _lib.FIT_E_INVAL
    assert L.fit_load_victims_tl(None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
    assert L.fit_load_victims_tl_device(None, None, 0, None, None, None, None, None) == _lib.FIT_E_INVAL
    ms = C.c_double()
    assert L.fit_preempt_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


# ---- the reference on the hand-written case ------------------------------------------------------
def test_reference_gives_the_hand_written_rows():
    c = tc.hand_case()
    T = tc.hand_timeline()
    assert T[:, :, 0].tolist() == tc.HAND_CPUS  # the dips are where the docstring draws them
    got = tc.ref_preempt_tl(c.nodes.part_mask, T, c.victims, c.parts, c.jobs, c.prio, tc.HAND_SLOT_MIN)
    assert c.jobs.j == len(tc.HAND_ROWS)
    for q, want in enumerate(tc.HAND_ROWS):
        assert tuple(int(x) for x in got[q]) == want, (q, got[q], want)
    assert set(got["code"].tolist()) == set(range(8))  # every code
    assert (c.victims.end == 0).any()
    for r in got:  # every row has fit_preempt_message's text
        assert fitgpu.preempt_message(r)
    assert fitgpu.preempt_message(got[0]) == \
        "fits node 0 after evicting 2 lower-priority jobs (highest priority 2): 2/5 nodes can be freed"


def test_the_dip_is_what_separates_the_hand_case_from_the_slot_0_rule():
    """Job 0 on the timeline WITHOUT the two reservations: A's release at slot 3 fills what A's eviction
    stops freeing, slot 0 binds, and node 0 needs one victim, as fit_preempt's rule says.  With the
    dip it needs two; node 1, whose dip outlasts C's end, goes from able to nothing."""
    from oracle import pyoracle as po
    c = tc.hand_case()
    flat = po.ref_build_timeline(c.nodes, c.tline)
    one = synth.Jobs(*(getattr(c.jobs, f)[:1] for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
    r = tc.ref_preempt_tl(c.nodes.part_mask, flat, c.victims, c.parts, one, c.prio[:1], tc.HAND_SLOT_MIN)[0]
    assert tuple(int(x) for x in r) == (tc.EVICT, 0, 1, 1, 5, 0, 3, 1)
    assert tc.HAND_ROWS[0][:4] == (tc.EVICT, 0, 2, 2)
    # the node table alone knows no ends: fit_preempt's reference would evict D on node 2, which frees nothing
    v = synth.Victims(c.victims.off, c.victims.prio, c.victims.cpu, c.victims.mem, c.victims.gpu)
    nodes = synth.Nodes(c.nodes.cpu_free, c.nodes.mem_free, c.nodes.gpu_free, np.full(6, tc.INF, np.int32), c.nodes.part_mask)
    r0 = pc.ref_preempt(nodes, v, c.parts, one, c.prio[:1])[0]
    assert (r0["code"], r0["node"], r0["victims"], r0["top_prio"]) == (tc.EVICT, 2, 1, 0)


def test_ends_shift_with_the_clock():
    """The reference with shift a reads every end as max(end - a, 0): on a timeline of zeros, A and B
    of node 0 (ends 3 and 8) free 2 slots for a 2-slot job after a shift of 1 and nothing after 8."""
    c = tc.hand_case()
    T = np.zeros((6, tc.HAND_H, 3), np.int32)
    jobs, prio = tc.jobs_of([(4, 0, 0, 20, 0, 5)])
    rows = [tc.ref_preempt_tl(c.nodes.part_mask, T, c.victims, c.parts, jobs, prio, tc.HAND_SLOT_MIN, shift=a)[0]
            for a in (0, 1, 2, 8)]
    assert [(int(r["code"]), int(r["node"]), int(r["victims"])) for r in rows] == \
        [(tc.EVICT, 0, 1), (tc.EVICT, 0, 1), (tc.EVICT, 0, 2), (tc.NONE, -1, 0)]


# ---- the generators ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,j", sorted(tc.SEEDS))
def test_recorded_seeds_are_rich_on_the_reference_alone(n, j):
    want, stats, T = tc.packed_tl_ref(n, j)
    tc.rich_enough(want, stats)
    c = tc.packed_tl_case(n, j)
    flat = tc.oracle_timeline(tc.CaseTL(c.nodes, c.victims, c.tline, synth.Jobs(*(getattr(c.queue, f)[:0] for f in (
        "cpu", "mem", "gpu", "wall", "part", "nodes_k"))), c.parts, c.jobs, c.prio))
    assert (T < flat).any(), "the queue reserved nothing"
    dips = (np.diff(T[:, :, 0].astype(np.int64), axis=1) < 0) & (T[:, 1:, 0] >= 0)
    assert dips.any(), "no reservation dip: the timeline never decreases in t"


def test_victim_ends_match_their_release_events():
    c = pc.packed_case(257, 128)
    vt, tline = synth.gen_victim_ends(5, c.victims, 64, 30, tc.ENDS)
    v = c.victims
    assert all(np.array_equal(getattr(vt, f), getattr(v, f)) for f in ("off", "prio", "cpu", "mem", "gpu"))
    assert set(np.unique(vt.end).tolist()) == set(tc.ENDS)
    n = c.nodes.n
    assert tline.slots == 64 and tline.slot_min == 30 and len(tline.off) == n + 1 and tline.off[-1] == len(tline.slot)
    node_v = np.repeat(np.arange(n), np.diff(vt.off))
    node_e = np.repeat(np.arange(n), np.diff(tline.off))
    inside = np.ones(len(tline.slot), bool)
    inside[tline.off[:-1][np.diff(tline.off) > 0]] = False
    assert (np.diff(tline.slot)[inside[1:]] >= 0).all(), "slots do not decrease inside a node"
    live = vt.end < 64  # a victim that ends at the horizon has no event
    assert live.sum() == len(tline.slot) and (tline.slot < 64).all()
    for a, b in ((vt.cpu, tline.cpu), (vt.mem, tline.mem), (vt.gpu, tline.gpu)):  # per (node, slot) the same amounts
        want = np.zeros((n, 65), np.int64)
        got = np.zeros((n, 65), np.int64)
        np.add.at(want, (node_v[live], vt.end[live]), a[live])
        np.add.at(got, (node_e, tline.slot), b)
        assert np.array_equal(want, got)
    default, _ = synth.gen_victim_ends(5, v, 64, 30)
    assert default.end.min() >= 1 and default.end.max() <= 64 and len(np.unique(default.end)) > 32
    again, _ = synth.gen_victim_ends(5, v, 64, 30, tc.ENDS)
    assert np.array_equal(again.end, vt.end)  # a pure function


# ---- Go binding: text checks ---------------------------------------------------------------------
def test_go_binds_load_victims_tl_and_preempt_tl():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    eng = open(GO).read()
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", eng))
    assert called <= declared, sorted(called - declared)
    assert {"fit_load_victims_tl", "fit_preempt_tl"} <= called
    assert re.search(r"type VictimsTL struct \{\n\tOff, Prio, End, CPU, MemMiB, GPU \[\]int32\n\}", eng)
    assert re.search(r"func \(e \*Engine\) LoadVictimsTL\(v VictimsTL\) error", eng)
    assert re.search(r"func \(e \*Engine\) PreemptTL\(j Jobs, prio \[\]int32\) \(\[\]Evict, error\)", eng)
    load = eng[eng.index("func (e *Engine) LoadVictimsTL("):eng.index("func (e *Engine) PreemptTL(")]
    assert "C.fit_load_victims_tl(e.ctx, nil, nil, nil, nil, nil, nil)" in load  # no victims at all
    assert "len(v.End)" in load and "errLen" in load and "&v.End[0]" in load
    pre = eng[eng.index("func (e *Engine) PreemptTL("):]
    pre = pre[:pre.index("\n}\n")]
    assert "len(prio)" in pre and "&prio[0]" in pre and "C.fit_evict" in pre and "goEvict(&rows[i])" in pre

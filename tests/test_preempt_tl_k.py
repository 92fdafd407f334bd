"""fit_preempt_tl_k's host half (no device): the exports and the unchanged ABI version, argument checks
that must answer before any device call, the reference (tests/_preempt_tl_k_cases.py ref_preempt_tl_k)
on hand-written cases with literal rows, against ref_preempt_tl at need 1 and against ref_preempt_k on
a flat timeline, the shift, the packed cases' conditions at the recorded seeds, and text checks of the
Go binding (no Go toolchain in the image, as tests/test_go_binding.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _preempt_cases as pc
import _preempt_k_cases as pk
import _preempt_tl_cases as tc
import _preempt_tl_k_cases as tk
import fitgpu
from fitgpu import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
SYMS = ("fit_preempt_tl_k", "fit_preempt_tl_k_device", "fit_preempt_tl_k_ms")
F, E, N = tk.FITS, tk.EVICT, tk.NONE


# ---- exports -------------------------------------------------------------------------------------
def test_exports_and_the_abi_version_is_still_8():
    hdr = open(HDR).read()
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    assert _lib.lib().fit_abi_version() == 8
    for sym in SYMS:
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"^int " + sym + r"\(", hdr, re.M), sym
    for meth in ("preempt_tl_k", "preempt_tl_k_device", "preempt_tl_k_ms"):
        assert callable(getattr(fitgpu.Engine, meth))


def test_the_header_gained_no_struct_and_no_message_function():
    hdr = open(HDR).read()
    assert not re.search(r"fit_evict_tl|fit_preempt_tl_message|fit_preempt_tl_k_message|fit_evict_k_tl", hdr)
    assert len(re.findall(r"\}\s*fit_evict_k;", hdr)) == 1 and len(re.findall(r"\}\s*fit_evict;", hdr)) == 1
    assert sorted(set(re.findall(r"\bfit_preempt_tl_k\w*", hdr))) == sorted(SYMS)
    decl = hdr[hdr.index("int fit_preempt_tl_k("):]
    decl = decl[:decl.index(";")]
    assert "fit_evict_k* out" in decl and "nodes_k" in decl and "kmax" in decl and "out_victims" in decl


def test_null_negative_and_kmax_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.EVICT_K_DTYPE)
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_preempt_tl_k, L.fit_preempt_tl_k_device):
        for kmax in (0, 1, 8, 9):
            assert fn(None, 0, None, None, None, None, None, None, None, kmax, None, None, None) == _lib.FIT_E_INVAL
            assert fn(None, -1, None, None, None, None, None, None, None, kmax, None, None, None) == _lib.FIT_E_INVAL
            assert fn(None, 1, p(one), p(one), p(one), p(one), p(one), None, p(one), kmax, p(out), p(one), p(one)) == \
                _lib.FIT_E_INVAL
    assert b"null ctx" in L.fit_last_error()
    ms = C.c_double()
    assert L.fit_preempt_tl_k_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


def test_the_two_copies_of_the_fold_say_the_same():
    """k_prek_walk keeps its spelled-out fold and k_ptlk_walk calls fit_pre_top.h's
    prek_fold: the statements, from the counters' stores to the list's, are the same text."""
    csrc = os.path.join(ROOT, "slurm-bridge-operator_amd", "csrc")
    first, last = "int32_t* red = reinterpret_cast<int32_t*>(sm);", "if (i < kmax) dst[i] = top.k[i];"

    def fold(name):
        text = open(os.path.join(csrc, name)).read()
        assert text.count(first) == 1 and text.count(last) == 1, name
        body = text[text.index(first):text.index(last) + len(last)]
        return [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith("//")]

    a, b = fold("fit_pre_top.h"), fold("fit_preempt_k.hip")
    assert len(a) > 30 and a == b
    walk = open(os.path.join(csrc, "fit_preempt_tl_k.hip")).read()
    assert "prek_fold<K>(sm, qs, wave, lane, on, q, n, top, tb, t0, nt, kmax, out, part);" in walk


# ---- the reference on the hand-written cases -----------------------------------------------------
def same(got, want):
    (rows, node, vic), (wrows, wnode, wvic) = got, want
    assert len(rows) == len(wrows)
    for q in range(len(rows)):
        assert tuple(int(x) for x in rows[q]) == tuple(int(x) for x in wrows[q]), (q, rows[q], wrows[q])
        assert node[q].tolist() == wnode[q].tolist() and vic[q].tolist() == wvic[q].tolist(), (q, node[q], vic[q])


def test_reference_gives_the_hand_written_rows():
    c = tk.hand_case_k()
    T = tc.hand_timeline()
    assert T[:, :, 0].tolist() == tc.HAND_CPUS  # the dips are where the docstring draws them
    got = tk.ref_preempt_tl_k(c.nodes.part_mask, T, c.victims, c.parts, c.jobs, c.prio, tc.HAND_SLOT_MIN, tk.KMAX)
    assert c.jobs.j == len(tk.HAND_ROWS_K)
    same(got, tk.hand_arrays())
    rows, node, vic = got
    code, need, fit, able = rows["code"], rows["need"], rows["fit"], rows["able"]
    assert set(code.tolist()) == set(range(8))                                   # every code
    assert set(range(1, 6)) <= set(code[need > 1].tolist())                      # codes 1-5 with need > 1
    assert ((code == F) & (need == 2)).any()
    assert ((code == N) & (fit + able == need - 1)).any() and ((code == N) & (rows["members"] < need)).any()
    nk0 = np.asarray(c.jobs.nodes_k) == 0
    assert nk0.any() and need[nk0].tolist() == [1]
    # row 2: node 0 takes v = 2 where the slot-0 rule says 1 (A has ended at the dip), and its picks differ in top
    assert node[2, :2].tolist() == [0, 2] and vic[2, :2].tolist() == [2, 2] and rows[2]["top_prio"] == 3
    one = synth.Jobs(*(getattr(c.jobs, f)[2:3] for f in ("cpu", "mem", "gpu", "wall", "part")), np.ones(1, np.uint16))
    from oracle import pyoracle as po
    flat = po.ref_build_timeline(c.nodes, c.tline)  # without the reservations slot 0 binds: one victim on node 0
    r0 = tc.ref_preempt_tl(c.nodes.part_mask, flat, c.victims, c.parts, one, c.prio[2:3], tc.HAND_SLOT_MIN)[0]
    assert (r0["code"], r0["node"], r0["victims"]) == (E, 0, 1)
    assert fitgpu.preempt_k_message(rows[2]) == ("fits 2 nodes after evicting 4 lower-priority jobs on 2 of them "
                                                 "(highest priority 3): 0 fit now, 2 can be freed, of 5 nodes")
    for r in rows:  # every row has fit_preempt_k_message's text
        assert fitgpu.preempt_k_message(r)


def test_reference_mixes_a_fitting_and_an_evicting_pick():
    """§2n's hand case has no node of partition 0 with a free cpu, so no job there can fit on one node
    and evict on another: three nodes on an open timeline show it, and the v = 2 against slot 0's 1."""
    c = tk.flat_hand_case_k()
    T = np.zeros((3, 8, 3), np.int32)
    T[0, :, 0] = 4
    got = tk.ref_preempt_tl_k(c.nodes.part_mask, T, c.victims, c.parts, c.jobs, c.prio, c.tline.slot_min, tk.KMAX)
    same(got, tk.hand_arrays(tk.FLAT_ROWS_K))
    rows = got[0]
    assert ((rows["code"] == E) & (rows["fit"] > 0) & (rows["fit"] < rows["need"])).all()


@pytest.mark.parametrize("nodes_k", [1, 0, None])
def test_reference_at_need_one_is_ref_preempt_tl(nodes_k):
    cases = [(tc.hand_case(), tc.hand_timeline(), tc.HAND_SLOT_MIN)]
    for n, j in ((257, 128), (65, 65)):
        want, _, T = tc.packed_tl_ref(n, j)
        cases.append((tc.packed_tl_case(n, j), T, tc.SLOT_MIN))
    for c, T, sm in cases:
        jobs = tk.with_k(c.jobs, None if nodes_k is None else np.full(c.jobs.j, nodes_k))
        want = tc.ref_preempt_tl(c.nodes.part_mask, T, c.victims, c.parts, c.jobs, c.prio, sm)
        for kmax in (1, 8):
            rows, node, vic = tk.ref_preempt_tl_k(c.nodes.part_mask, T, c.victims, c.parts, jobs, c.prio, sm, kmax)
            assert (rows["need"] == 1).all() and not rows["reserved"].any()
            for f in ("code", "victims", "top_prio", "members", "fit", "able", "outranked"):
                assert np.array_equal(rows[f], want[f]), f
            assert np.array_equal(node[:, 0], want["node"]) and np.array_equal(vic[:, 0], want["victims"])
            assert np.array_equal(rows["evict_nodes"], (want["victims"] > 0).astype(np.int32))
            assert (node[:, 1:] == -1).all() and not vic[:, 1:].any()


def flat_case(n=257, j=128, seed=0):
    """Relation 3's inputs: the packed cluster, no release events, slot_min 1, walls in [1, H], every
    end H, avail_min random around H.  Returns (node-table case with nodes_k, its dense timeline, the
    victims with ends)."""
    base = pk.packed_case_k(n, j, seed)
    Hh = tc.H
    r = np.random.default_rng(5)
    jobs = synth.Jobs(base.jobs.cpu, base.jobs.mem, base.jobs.gpu, r.integers(1, Hh + 1, j).astype(np.int32), base.jobs.part,
                      base.jobs.nodes_k)
    nd = base.nodes
    nodes = synth.Nodes(nd.cpu_free, nd.mem_free, nd.gpu_free, r.integers(0, 2 * Hh, n).astype(np.int32), nd.part_mask)
    v = base.victims
    vt = synth.VictimsTL(v.off, v.prio, np.full(len(v.prio), Hh, np.int32), v.cpu, v.mem, v.gpu)
    return pc.Case(nodes, v, base.parts, jobs, base.prio), vt


def test_reference_on_a_flat_timeline_with_ends_h_is_ref_preempt_k():
    from oracle import pyoracle as po
    c, vt = flat_case()
    empty = synth.Timeline(tc.H, 1, np.zeros(c.nodes.n + 1, np.int32), *(np.zeros(0, np.int32) for _ in range(4)))
    T = po.ref_build_timeline(c.nodes, empty)
    T[c.nodes.part_mask == 0] = -1
    got = tk.ref_preempt_tl_k(c.nodes.part_mask, T, vt, c.parts, c.jobs, c.prio, 1, tk.KMAX)
    want = pk.ref_preempt_k(c.nodes, c.victims, c.parts, c.jobs, c.prio, tk.KMAX)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    rows = want[0]
    assert ((rows["code"] == E) & (rows["need"] >= 2)).sum() >= 10 and (rows["code"] == N).any()


def test_ends_shift_with_the_clock():
    """The reference with shift a reads every end as max(end - a, 0): on a timeline of zeros, nodes 0
    (A ends at 3, B at 8) and 2 (D at 0, E at 8) free 2 slots for a 2-slot job of two nodes; after a
    shift of 2 node 0 needs B as well, after 8 nothing can be freed."""
    c = tc.hand_case()
    T = np.zeros((6, tc.HAND_H, 3), np.int32)
    jobs, prio = tk.jobs_of_k([(4, 0, 0, 20, 0, 5, 2)])
    got = [tk.ref_preempt_tl_k(c.nodes.part_mask, T, c.victims, c.parts, jobs, prio, tc.HAND_SLOT_MIN, 2, shift=a)
           for a in (0, 1, 2, 8)]
    # node 1's C ends at 2: it covers [0, 2) until the shift reaches 1
    assert [(int(r[0]["code"]), n[0].tolist(), v[0].tolist()) for r, n, v in got] == \
        [(E, [0, 1], [1, 1]), (E, [0, 2], [1, 2]), (E, [0, 2], [2, 2]), (N, [-1, -1], [0, 0])]


# ---- the packed cases ----------------------------------------------------------------------------
PACKED = [(variant, n, j, seed) for (variant, n, j), (seeds, _) in sorted(tk.SEEDS.items()) for seed in seeds]


@pytest.mark.parametrize("variant,n,j,seed", PACKED)
def test_recorded_seeds_hold_the_conditions_on_the_reference_alone(variant, n, j, seed):
    c = tk.packed_tl_case_k(variant, n, j, seed)
    (rows, node, vic), stats, T = tk.packed_tl_ref_k(variant, n, j, seed)
    tk.SEEDS[(variant, n, j)][1](rows, stats)
    assert np.array_equal(np.asarray(c.jobs.nodes_k), np.random.default_rng(7 * n + j).choice(tk.K_DRAW, j))
    assert c.queue.j == (2 * n if variant == "full" else n // 8)
    if variant == "full" and n >= 257:  # so full that no row mixes fitting and evicting picks, and no wide job fits
        assert not ((rows["code"] == E) & (rows["fit"] > 0)).any()
        assert not ((rows["code"] == F) & (rows["need"] >= 2)).any()
    # the outputs are consistent with themselves: need picks on FITS / EVICT rows, none elsewhere
    picked = np.isin(rows["code"], (F, E))
    assert ((node >= 0).sum(1) == np.where(picked, rows["need"], 0)).all()
    assert (vic.sum(1) == rows["victims"]).all() and ((vic > 0).sum(1) == rows["evict_nodes"]).all()
    for q in np.flatnonzero(picked):
        assert len(set(node[q, :rows["need"][q]].tolist())) == rows["need"][q]  # distinct nodes
    dips = (np.diff(T[:, :, 0].astype(np.int64), axis=1) < 0) & (T[:, 1:, 0] >= 0)
    assert dips.any() or variant == "short", "no reservation dip: the timeline never decreases in t"


# ---- Go binding: text checks ---------------------------------------------------------------------
def test_go_binds_preempt_tl_k():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    eng = open(GO).read()
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", eng))
    assert called <= declared, sorted(called - declared)
    assert "fit_preempt_tl_k" in called
    assert re.search(r"func \(e \*Engine\) PreemptTLK\(j Jobs, prio \[\]int32, kmax int\) "
                     r"\(\[\]EvictK, \[\]int32, \[\]int32, error\)", eng)
    pre = eng[eng.index("func (e *Engine) PreemptTLK("):]
    pre = pre[:pre.index("\n}\n")]
    assert "len(prio)" in pre and "&prio[0]" in pre and "C.fit_evict_k" in pre and "j.NodesK" in pre
    assert "goEvictK(&rows[i])" in pre and "C.fit_preempt_tl_k(e.ctx" in pre
    assert "kmax > MaxK" in pre and pre.index("kmax > MaxK") < pre.index("cnt*kmax")  # checked before it sizes the slices
    assert "PreemptKMessage" in eng[eng.index("// PreemptTLK is"):eng.index("func (e *Engine) PreemptTLK(")]
    assert len(re.findall(r"^type EvictK struct", eng, re.M)) == 1  # no second row type

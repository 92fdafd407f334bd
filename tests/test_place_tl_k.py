"""fit_place_tl_k without a device: the numpy restatement of DESIGN.md §2g (the GPU tests' checker)
against the C oracle at k = 1 and on the hand case, the conditions that keep the GPU comparison from
being vacuous — asserted on the reference alone, so a wrong generator fails here — and the host half
of the entry points (header, ABI version, NULL ctx)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _place_tl_k_cases as pk
import _when_k_cases as wk
from fitgpu import FIT_REJECTED, _lib
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")


# ---- 1. the restatement against the C oracle at k = 1 ------------------------------------------------
@pytest.mark.parametrize("kind,H,j,kmax", [("busy",) + c for c in pk.BUSY] + [("rand", 64, 65, 8)])
def test_restatement_equals_the_c_oracle_at_k1(kind, H, j, kmax):
    nodes, tline, parts = pk.cluster(H)
    jobs = pk.ones((pk.busy_case if kind == "busy" else pk.rand_case)(H, j, kmax))
    tl0 = po.ref_build_timeline(nodes, tline)
    out, start, fin = pk.ref_place_tl_k(tl0, nodes.part_mask, parts, jobs, pk.SLOT_MIN, 1)
    rn, rs, st, rfin = po.ref_place_tl(nodes, tline, jobs, parts)
    assert np.array_equal(out[:, 0], rn), np.flatnonzero(out[:, 0] != rn)[:5]
    assert np.array_equal(start, rs)
    assert np.array_equal(fin, rfin)
    assert st["placed"] == (start >= 0).sum() and st["placed"] > 0


# ---- 2. the hand case through the restatement --------------------------------------------------------
def test_hand_case():
    nodes, tline, jobs, parts = pk.hand_case()
    tl0 = po.ref_build_timeline(nodes, tline)
    out, start, fin = pk.ref_place_tl_k(tl0, nodes.part_mask, parts, jobs, tline.slot_min, pk.HAND_KMAX)
    assert out.tolist() == pk.HAND_NODES.tolist()
    assert start.tolist() == pk.HAND_START.tolist()
    assert fin[:, :, 0].tolist() == pk.HAND_CPU.tolist()
    # q2 alone on the loaded timeline starts at 5: it is the jobs before it that leave it unplaced
    assert pk.alone_starts(tl0, nodes.part_mask, parts, jobs, tline.slot_min, pk.HAND_KMAX)[2] == 5
    assert ((start >= 0).sum(), (out[:, 0] == FIT_REJECTED).sum()) == (pk.HAND_STATS["placed"], 1) == (6, 1)


# ---- 3. the inputs are contended ---------------------------------------------------------------------
@pytest.mark.parametrize("H,j,kmax", pk.BUSY)
def test_busy_cases_are_contended(H, j, kmax):
    """A sequential-blind implementation (every job judged against the starting timeline) fails
    each of these inputs: jobs start later than judged alone, some are placed and some are not.
    The reference gives, on the starting timeline of the GPU cases (at H >= 64 after the warm-up
    queue), placed / unplaced / multi-node jobs moved against judged-alone / longest run list after:
    (8, 200, 3) 192 / 8 / 19 / 8; (64, 300, 8) 287 / 13 / 158 / 28; (1024, 300, 8) 289 / 11 / 152 /
    33 (128 lists above 13 runs); (1024, 300, 1) 294 / 6 / 63 moved, all one-node / 32."""
    nodes, tline, parts = pk.cluster(H)
    jobs, out, start, fin = pk.reference("busy", H, j, kmax)
    alone = pk.alone_starts(pk.start_timeline(H), nodes.part_mask, parts, jobs, pk.SLOT_MIN, kmax)
    placed = start >= 0
    rejected = out[:, 0] == FIT_REJECTED
    multi = jobs.nodes_k > 1
    moved = placed & (start != alone)
    runs = wk.run_counts(fin)
    print(f"H {H} j {j} kmax {kmax}: placed {placed.sum()} unplaced {(~placed & ~rejected).sum()} rejected "
          f"{rejected.sum()} moved {moved.sum()} (multi-node {(moved & multi).sum()}) longest list {runs.max()} "
          f"lists above 13 runs {(runs > 13).sum()}")
    assert placed.any() and (~placed & ~rejected).any()
    if kmax > 1:
        assert (moved & multi).sum() >= 10
    else:
        assert moved.sum() >= 10
    if H == 1024:  # more than two 4-Seg loads past the header's runs
        assert runs.max() >= 17


def test_busy_case_drives_every_run_list_length_and_both_node_paths():
    """("busy", 64, 300, 8), which the GPU test runs as well: (a) its starting run lists have every
    length the visit of a list distinguishes — header only, the header's edge, the four-run loads'
    edges — and (b), (c) its placed jobs take both ways to the node list: some start later than a
    node that is free at slot 0 (the window [start, start + d) is evaluated again), some start at 0
    (the count walk's keys are the answer).  The reference gives run counts 1 .. 11 and 13 .. 17, and
    of 287 placed jobs 60 of kind (b) and 92 of kind (c)."""
    H, j, kmax = 64, 300, 8
    nodes, tline, parts = pk.cluster(H)
    jobs, out, start, fin = pk.reference("busy", H, j, kmax)
    rc = wk.run_counts(pk.start_timeline(H)[nodes.part_mask != 0])
    assert {1, 4, 5, 8, 9} <= set(rc.tolist()) and rc.max() >= 13, sorted(set(rc.tolist()))
    # the replay: `now` of every job on the timeline as the jobs before it left it
    tl = np.array(pk.start_timeline(H), np.int32, copy=True)
    now = np.zeros(j, np.int32)
    for q in range(j):
        one = wk.one_job(jobs, q)
        rows, sel = wk.ref_when_k(tl, nodes.part_mask, parts, one, pk.SLOT_MIN, kmax)
        now[q] = rows["now"][0]
        assert rows["start"][0] == start[q] or start[q] < 0
        if start[q] >= 0:
            need, d = int(rows["need"][0]), int(rows["dur"][0])
            assert np.array_equal(sel[0, :need], out[q, :need])
            tl[sel[0, :need], start[q]:start[q] + d] -= np.array([one.cpu[0], one.mem[0], one.gpu[0]], np.int32)
    assert np.array_equal(tl, fin)
    later_with_early, at_zero = (start > 0) & (now > 0), start == 0
    print(f"run counts {sorted(set(rc.tolist()))} placed {(start >= 0).sum()} start > 0 and now > 0 "
          f"{later_with_early.sum()} start == 0 {at_zero.sum()}")
    assert later_with_early.any() and at_zero.any()


def test_stairs_are_long_and_contended():
    nodes, tline, parts = pk.stairs()
    jobs, tl0, out, start, fin = pk.stairs_reference()
    assert (wk.run_counts(tl0) == 128).all()
    runs = wk.run_counts(fin)
    alone = pk.alone_starts(tl0, nodes.part_mask, parts, jobs, tline.slot_min, 4)
    placed = start >= 0
    moved = placed & (start != alone)
    print(f"stairs: runs {runs.min()}..{runs.max()} placed {placed.sum()} unplaced {(~placed).sum()} placeable alone "
          f"{(~placed & (alone >= 0)).sum()} moved {moved.sum()} starts beyond 128 {(start > 128).sum()}")
    assert (runs > 128).all()  # reservations split runs beyond index 64 of every list
    assert (~placed & (alone >= 0)).sum() >= 20
    assert moved.sum() >= 20


# ---- 4. the host half ----------------------------------------------------------------------------------
def test_header_declares_both_entry_points():
    hdr = open(HDR).read()
    for name in ("fit_place_tl_k", "fit_place_tl_k_device"):
        assert re.search(r"\bint " + name + r"\(fit_ctx\* ctx, int32_t j,", hdr), name
        assert name in _lib.EXPORTS
    assert re.search(r"#define FITGPU_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert re.search(r"/\* 4: multi-node backfill", hdr)        # fit_stats.engine = 4 is documented


def test_null_ctx_answers_without_a_device():
    L = _lib.lib()
    one = np.ones(1, np.int32)
    k = np.ones(1, np.uint16)
    st = _lib.FitStats()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_place_tl_k, L.fit_place_tl_k_device):
        assert fn(None, 0, None, None, None, None, None, None, 1, None, None, None) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(k), p(k), 1, p(one), p(one), C.byref(st)) == \
            _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()

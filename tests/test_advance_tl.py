"""fit_advance_tl without a device: the host half of the entry points (header, exports, ABI version,
NULL ctx), the Go binding's text, the numpy restatement of DESIGN.md §2i itself (the GPU tests'
checker) — composition, the commutation with fit_unplace_tl through the row rewrite, and why a NULL
tail does not commute — and the conditions that keep the GPU tests from being vacuous, asserted on
the references alone so a wrong generator fails here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _advance_tl_cases as ac
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
import _when_k_cases as wk
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
NAMES = ("fit_advance_tl", "fit_advance_tl_device", "fit_advance_tl_ms")


# ---- 1. the host half ------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    hdr = open(HDR).read()
    for name in NAMES[:2]:
        assert re.search(r"\bint " + name + r"\(fit_ctx\* ctx, int32_t a, const int32_t\* tail_cpu, "
                         r"const int32_t\* tail_mem,\s+const int32_t\* tail_gpu", hdr), name
    assert re.search(r"\bint fit_advance_tl_ms\(fit_ctx\* ctx, double\* ms\);", hdr)
    for name in NAMES:
        assert name in _lib.EXPORTS
    assert re.search(r"#define FITGPU_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert _lib.lib().fit_abi_version() == 8


def test_null_ctx_answers_without_a_device():
    L = _lib.lib()
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_advance_tl, L.fit_advance_tl_device):
        for a in (0, 1, -1):
            assert fn(None, a, None, None, None) == _lib.FIT_E_INVAL
            assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, p(one), p(one), p(one)) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
    ms = C.c_double()
    assert L.fit_advance_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


def test_go_binding_text():
    src = open(GO).read()
    m = re.search(r"func \(e \*Engine\) AdvanceTL\(a int, tailCPU, tailMemMiB, tailGPU \[\]int32\) error \{(.*?)\n\}\n",
                  src, re.S)
    assert m, "AdvanceTL is missing or has another signature"
    assert "C.fit_advance_tl(e.ctx," in m.group(1)
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\(", src))
    assert "fit_advance_tl" in called and called <= declared, called - declared


# ---- 2. the restatement itself -----------------------------------------------------------------------------
def test_hand_example():
    """One node, H = 6, columns (cpu, mem, gpu): the gpu column is -1 at the last slot and stays so."""
    tl = np.array([[[4, 9, 1], [3, 9, 1], [3, 9, 1], [5, 9, -1], [5, 9, -1], [6, 9, -1]]], np.int32)
    got = ac.ref_advance_tl(tl, 2, np.array([[8, -1, 7]]))
    assert got[0].tolist() == [[3, 9, 1], [5, 9, -1], [5, 9, -1], [6, 9, -1], [8, -1, -1], [8, -1, -1]]
    assert ac.ref_advance_tl(tl, 2, None)[0, 4:].tolist() == [[6, 9, -1]] * 2
    assert ac.ref_advance_tl(tl, 0, np.array([[8, -1, 7]])).tobytes() == tl.tobytes()
    for a in (6, 7, 600):
        assert ac.ref_advance_tl(tl, a, np.array([[8, 2, 7]]))[0].tolist() == [[8, 2, -1]] * 6


@pytest.mark.parametrize("H,kmax", ac.BASES)
def test_composition(H, kmax):
    tl = ac.base(H, kmax)
    for tail in (ac.level_tail(H), ac.random_tail(tl, 5)):
        for a, b in ((1, 1), (7, 57), (63, 64), (H - 1, 1), (H, 3), (5, H + 5)):
            two = ac.ref_advance_tl(ac.ref_advance_tl(tl, a, tail), b, tail)
            assert np.array_equal(two, ac.ref_advance_tl(tl, a + b, tail)), (a, b)
    assert not np.array_equal(ac.ref_advance_tl(tl, 1, ac.level_tail(H)), tl)


@pytest.mark.parametrize("H,kmax", ac.BASES)
def test_commutes_with_unplace_through_the_row_rewrite(H, kmax):
    jobs, out, start, fin = uc.reference(H, kmax)
    rows = uc.half(H, kmax)
    sub, snode, sstart = uc.take(jobs, rows), out[rows], start[rows]
    tail = ac.level_tail(H)
    dropped = clipped = 0
    for a in (1, 7, H // 2, H - 1, H, H + 5):
        before, _ = uc.ref_unplace_tl(fin, sub, snode, sstart, pk.SLOT_MIN, kmax)
        want = ac.ref_advance_tl(before, a, tail)
        sub2, start2 = ac.rewrite_rows(sub, sstart, a, H, pk.SLOT_MIN)
        got, _ = uc.ref_unplace_tl(ac.ref_advance_tl(fin, a, tail), sub2, snode, start2, pk.SLOT_MIN, kmax)
        assert np.array_equal(got, want), a
        dropped += int((start2 < 0).sum())
        clipped += int(((sstart < a) & (start2 == 0)).sum())
    assert dropped >= 10 and clipped >= 10  # both branches of the rewrite are taken
    # every row handed back: the advanced start timeline
    back, _ = uc.ref_unplace_tl(fin, jobs, out, start, pk.SLOT_MIN, kmax)
    assert np.array_equal(ac.ref_advance_tl(back, 7, tail), ac.ref_advance_tl(pk.start_timeline(H), 7, tail))


def test_a_null_tail_does_not_commute():
    """A window that touches slot H - 1 changes what continues: handing it back before the advance
    continues the freed level, handing the rewritten row back afterwards leaves the new slots at the
    reserved level."""
    tl = np.full((1, 8, 3), 4, np.int32)
    tl[0, 6:, 0] = 1  # 3 cpus reserved on [6, 8)
    job = wk.jobs_of([(3, 0, 0, 2, 0, 1)])
    node, start = np.zeros((1, 1), np.int32), np.array([6], np.int32)
    before, _ = uc.ref_unplace_tl(tl, job, node, start, 1, 1)
    j2, s2 = ac.rewrite_rows(job, start, 2, 8, 1)
    assert s2.tolist() == [4] and j2.wall.tolist() == [2]
    for tail, same in ((np.array([[4, 4, 4]]), True), (None, False)):
        a = ac.ref_advance_tl(before, 2, tail)
        b, _ = uc.ref_unplace_tl(ac.ref_advance_tl(tl, 2, tail), j2, node, s2, 1, 1)
        assert np.array_equal(a, b) == same
        if not same:
            assert a[0, :, 0].tolist() == [4] * 8 and b[0, :, 0].tolist() == [4] * 6 + [1, 1]


# ---- 3. the GPU tests are not vacuous ------------------------------------------------------------------------
def test_base_timelines_are_not_vacuous():
    """reference(64, 8) gives, for a = 1 / 7 / 32 / 63: cuts on a run boundary 223 / 114 / 127 / 46,
    inside a run 570 / 679 / 666 / 747, nodes that lose a run 223 / 503 / 721 / 737; 194 nodes -1 at
    slot H - 1 but usable at slot 0, 3 nodes all -1, 16 nodes whose last slot carries a reservation,
    the longest list 23 runs."""
    H, kmax = 64, 8
    tl = ac.base(H, kmax)
    for a in ac.CUTS:
        on, inside, lose = ac.cut_counts(tl, a)
        print(a, on, inside, lose)
        assert on >= 40 and inside >= 500 and lose >= 150, a
    dead_end = (tl[:, H - 1] == -1).all(axis=1)
    usable0 = (tl[:, 0] != -1).any(axis=1)
    reserved_edge = (tl[:, H - 1] != pk.start_timeline(H)[:, H - 1]).any(axis=1)
    longest = int(wk.run_counts(tl).max())
    print(int((dead_end & usable0).sum()), int((tl == -1).all(axis=(1, 2)).sum()), int(reserved_edge.sum()), longest)
    assert (dead_end & usable0).sum() >= 150
    assert (tl == -1).all(axis=(1, 2)).sum() >= 3
    assert reserved_edge.sum() >= 8  # so the level tail is not the continuation
    assert not np.array_equal(ac.ref_advance_tl(tl, 1, None), ac.ref_advance_tl(tl, 1, ac.level_tail(H)))
    assert longest >= 16
    for Hb, kb in ac.BASES:  # lists inside and beyond the TL_HEAD runs of the header copy, every base
        runs = wk.run_counts(ac.base(Hb, kb))
        assert (runs <= 4).sum() >= 50 and (runs > 4).sum() >= 50
    rt = ac.random_tail(tl, 64)
    top = tl.max(axis=1)
    assert (rt == -1).sum() >= 100 and (rt > top).sum() >= 100 and (rt.min() >= -1)


def test_staircase_has_the_long_lists():
    H = 256
    tl = ac.staircase_dense(H)
    runs = wk.run_counts(tl)
    assert runs[ac.STAIR_FULL] == H and runs[ac.STAIR_HALF] == H // 2 and runs[2] == 2
    assert (runs[[0, 1, 5]] == 1).all()
    # an advance by 1 with another tail keeps H runs (H - 1 survivors and the tail); the same tail merges
    last = tl[:, H - 1].copy()
    assert wk.run_counts(ac.ref_advance_tl(tl, 1, last + (last != -1)))[ac.STAIR_FULL] == H
    assert wk.run_counts(ac.ref_advance_tl(tl, 1, last))[ac.STAIR_FULL] == H - 1
    assert wk.run_counts(ac.ref_advance_tl(tl, 1, None))[ac.STAIR_FULL] == H - 1

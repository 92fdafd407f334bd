"""fit_unplace_tl without a device: the host half of the entry points (header, exports, ABI version,
NULL ctx), the Go binding's text, the numpy restatement of DESIGN.md §2h itself (the GPU tests'
checker) — the round trip and the freedom of order — and the conditions that keep the GPU round trips
from being vacuous, asserted on the references alone so a wrong generator fails here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
NAMES = ("fit_unplace_tl", "fit_unplace_tl_device", "fit_unplace_tl_ms")


# ---- 1. the host half ------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    hdr = open(HDR).read()
    for name in NAMES[:2]:
        assert re.search(r"\bint " + name + r"\(fit_ctx\* ctx, int32_t j, const int32_t\* cpu,", hdr), name
    assert re.search(r"\bint fit_unplace_tl_ms\(fit_ctx\* ctx, double\* ms\);", hdr)
    for name in NAMES:
        assert name in _lib.EXPORTS
    assert re.search(r"#define FITGPU_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert _lib.lib().fit_abi_version() == 8


def test_null_ctx_answers_without_a_device():
    L = _lib.lib()
    one = np.ones(1, np.int32)
    k = np.ones(1, np.uint16)
    applied = C.c_int64(-5)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_unplace_tl, L.fit_unplace_tl_device):
        assert fn(None, 0, None, None, None, None, None, 1, None, None, None) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(k), 1, p(one), p(one), C.byref(applied)) == \
            _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error() and applied.value == -5
    ms = C.c_double()
    assert L.fit_unplace_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


def test_go_binding_text():
    src = open(GO).read()
    m = re.search(r"func \(e \*Engine\) UnplaceTL\(j Jobs, kmax int, node, start \[\]int32\) \(int64, error\) \{(.*?)\n\}\n",
                  src, re.S)
    assert m, "UnplaceTL is missing or has another signature"
    assert "C.fit_unplace_tl(e.ctx," in m.group(1)
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\(", src))
    assert "fit_unplace_tl" in called and called <= declared, called - declared


# ---- 2. the restatement itself -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_unplacing_every_row_restores_the_start(H, kmax):
    jobs, out, start, fin = uc.reference(H, kmax)
    tl0 = pk.start_timeline(H)
    assert not np.array_equal(fin, tl0)
    back, applied = uc.ref_unplace_tl(fin, jobs, out, start, pk.SLOT_MIN, kmax)
    assert np.array_equal(back, tl0)
    assert applied == np.maximum(jobs.nodes_k[start >= 0], 1).sum()


@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP[1:3])
def test_order_and_split_do_not_matter(H, kmax):
    jobs, out, start, fin = uc.reference(H, kmax)
    rows = uc.half(H, kmax)
    a, na = uc.ref_unplace_tl(fin, jobs, out, start, pk.SLOT_MIN, kmax, rows)
    b, nb = uc.ref_unplace_tl(fin, jobs, out, start, pk.SLOT_MIN, kmax, rows[::-1])
    c1, n1 = uc.ref_unplace_tl(fin, jobs, out, start, pk.SLOT_MIN, kmax, rows[:len(rows) // 3])
    c2, n2 = uc.ref_unplace_tl(c1, jobs, out, start, pk.SLOT_MIN, kmax, rows[len(rows) // 3:])
    assert np.array_equal(a, b) and np.array_equal(a, c2) and na == nb == n1 + n2
    assert not np.array_equal(a, fin) and not np.array_equal(a, pk.start_timeline(H))


def test_order_does_not_matter_at_the_clamp_and_at_minus_one():
    """§2h's two rules against each other: windows that saturate and windows over -1 slots, in two
    orders and in two calls."""
    tl = np.zeros((2, 8, 3), np.int32)
    tl[0, :, 0] = uc.INT32_MAX - 6
    tl[0, 5:, :] = -1
    tl[1, :, 1] = -1
    jobs = uc.wk.jobs_of([(5, 1, 0, 4, 0, 2), (4, 2, 1, 8, 0, 1), (uc.INT32_MAX, 0, 7, 3, 0, 2)])
    node = np.array([[0, 1], [0, -1], [1, 0]], np.int32)
    start = np.array([0, 2, 4], np.int32)
    a, _ = uc.ref_unplace_tl(tl, jobs, node, start, 1, 2, [0, 1, 2])
    b, _ = uc.ref_unplace_tl(tl, jobs, node, start, 1, 2, [2, 1, 0])
    c, _ = uc.ref_unplace_tl(uc.ref_unplace_tl(tl, jobs, node, start, 1, 2, [1])[0], jobs, node, start, 1, 2, [2, 0])
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert a[0, 2, 0] == uc.INT32_MAX and a[0, 4, 0] == uc.INT32_MAX and (a[0, 5:] == -1).all()
    assert (a[1, :, 1] == -1).all() and a[1, 0, 0] == 5 and a[1, 4, 0] == uc.INT32_MAX


# ---- 3. the round trips are not vacuous ------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_round_trip_cases_are_not_vacuous(H, kmax):
    """At least 20 placed rows, 5 of them multi-node (at kmax 1 no row can be), an unplaced and a
    rejected row passed through, and a node touched by at least 3 windows.  The references give
    placed / multi-node / unplaced / rejected / windows on the busiest node: (64, 1) 152 / 0 / 24 /
    4 / 6; (64, 8) 152 / 117 / 21 / 7 / 9; (256, 1) 155 / 0 / 18 / 7 / 6; (256, 8) 144 / 108 / 28 /
    8 / 7."""
    c = uc.conditions(H, kmax)
    print(H, kmax, c)
    assert c["placed"] >= 20 and c["unplaced"] >= 1 and c["rejected"] >= 1 and c["busiest"] >= 3
    assert c["multi"] >= (5 if kmax > 1 else 0)
    rows = uc.half(H, kmax)
    assert len(rows) >= 10 and len(set(rows.tolist())) == len(rows)


def test_crowd_is_a_crowd():
    jobs, node, start = uc.crowd()
    cnt = uc.windows_per_node(jobs, node, start, 40)
    assert cnt[7] == 312 and (cnt == 1).sum() >= 30 and ((cnt > 1) & (cnt < 20)).sum() >= 6
    d = np.maximum(1, jobs.wall)
    assert (start + d > 64).any() and (jobs.nodes_k == 3).sum() == 12

"""fit_hold_tl without a device: the host half of the entry points (header, exports, ABI version,
NULL ctx), the Go binding's text, the numpy restatement of DESIGN.md §2j itself (the GPU tests'
checker) — replay, inverse, freedom of order and split, and a hand-built case that pins every sentence
of the judging rule — and the conditions that keep the GPU cases from being vacuous, asserted on the
restatement alone so a wrong generator fails here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fitgpu
import _hold_tl_cases as hc
import _place_tl_k_cases as pk
import _unplace_tl_cases as uc
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
NAMES = ("fit_hold_tl", "fit_hold_tl_device", "fit_hold_tl_ms")


# ---- 1. the host half ------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    hdr = open(HDR).read()
    for name in NAMES[:2]:
        assert re.search(r"\bint " + name + r"\(fit_ctx\* ctx, int32_t j, const int32_t\* cpu,", hdr), name
    assert re.search(r"\bint fit_hold_tl_ms\(fit_ctx\* ctx, double\* ms\);", hdr)
    assert re.search(r"int32_t\* out_state /\* j \*/, int64_t\* applied /\* may be NULL \*/, "
                     r"int64_t\* refused /\* may be NULL \*/\);", hdr)
    for name, value in (("HELD", "1"), ("REFUSED", "0"), ("SKIPPED", r"\(-1\)")):
        assert re.search(r"#define FIT_HOLD_" + name + r"\s+" + value + r"\s", hdr), name
    assert re.search(r"#define FITGPU_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert (fitgpu.FIT_HOLD_HELD, fitgpu.FIT_HOLD_REFUSED, fitgpu.FIT_HOLD_SKIPPED) == (1, 0, -1) == \
        (hc.HELD, hc.REFUSED, hc.SKIPPED)


def test_exports_and_abi_version():
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().fit_abi_version() == 8


def test_null_ctx_answers_without_a_device():
    L = _lib.lib()
    one = np.ones(1, np.int32)
    k = np.ones(1, np.uint16)
    state = np.full(1, 77, np.int32)
    applied, refused = C.c_int64(-5), C.c_int64(-6)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_hold_tl, L.fit_hold_tl_device):
        assert fn(None, 0, None, None, None, None, None, 1, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(k), 1, p(one), p(one), p(state), C.byref(applied),
                  C.byref(refused)) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
        assert applied.value == -5 and refused.value == -6 and state[0] == 77
    ms = C.c_double()
    assert L.fit_hold_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


def test_go_binding_text():
    src = open(GO).read()
    m = re.search(r"func \(e \*Engine\) HoldTL\(j Jobs, kmax int, node, start \[\]int32\) "
                  r"\(\[\]int32, int64, int64, error\) \{(.*?)\n\}\n", src, re.S)
    assert m, "HoldTL is missing or has another signature"
    assert "C.fit_hold_tl(e.ctx," in m.group(1)
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\(", src))
    assert "fit_hold_tl" in called and called <= declared, called - declared
    for name in ("FIT_HOLD_HELD", "FIT_HOLD_REFUSED", "FIT_HOLD_SKIPPED"):
        assert "C." + name in src, name


# ---- 2. the restatement itself -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_replay_gives_the_placement_s_timeline(H, kmax):
    jobs, out, start, fin = uc.reference(H, kmax)
    got, state, applied, refused = hc.ref_hold_tl(pk.start_timeline(H), jobs, out, start, pk.SLOT_MIN, kmax)
    assert np.array_equal(got, fin) and refused == 0
    assert np.array_equal(state, np.where(start >= 0, hc.HELD, hc.SKIPPED))
    assert applied == np.maximum(jobs.nodes_k[start >= 0], 1).sum()


@pytest.mark.parametrize("H,kmax", hc.REFRESH)
def test_unplace_after_hold_is_the_identity_on_the_held_rows(H, kmax):
    jobs, out, start, _ = uc.reference(H, kmax)
    tl0, fin, state, applied, refused = hc.refresh_reference(H, kmax)
    assert not np.array_equal(fin, tl0)
    held = np.flatnonzero(state == hc.HELD)
    back, n = uc.ref_unplace_tl(fin, jobs, out, start, pk.SLOT_MIN, kmax, held)
    assert np.array_equal(back, tl0) and n == applied
    # and the other way round: hold of rows just unplaced, where the unplace did not saturate
    again, st2, n2, r2 = hc.ref_hold_tl(back, jobs, out, start, pk.SLOT_MIN, kmax, held)
    assert np.array_equal(again, fin) and n2 == applied and r2 == 0 and (st2[held] == hc.HELD).all()


@pytest.mark.parametrize("H,kmax", hc.REFRESH)
def test_order_and_split_do_not_matter(H, kmax):
    jobs, out, start, _ = uc.reference(H, kmax)
    tl0, fin, state, applied, refused = hc.refresh_reference(H, kmax)
    perm, pj, pn, ps = hc.shuffled(jobs, out, start, 5 * H + kmax)
    got, pstate, a2, r2 = hc.ref_hold_tl(tl0, pj, pn, ps, pk.SLOT_MIN, kmax)
    assert np.array_equal(got, fin) and np.array_equal(pstate, state[perm]) and (a2, r2) == (applied, refused)
    # two calls give what one gives when neither route refuses a row: the held rows, in two halves
    held = np.random.default_rng(H).permutation(np.flatnonzero(state == hc.HELD))
    one, s1, n1, r1 = hc.ref_hold_tl(tl0, jobs, out, start, pk.SLOT_MIN, kmax, held[:len(held) // 3])
    two, s2, n2, r2 = hc.ref_hold_tl(one, jobs, out, start, pk.SLOT_MIN, kmax, held[len(held) // 3:])
    assert r1 == r2 == 0 and n1 + n2 == applied and np.array_equal(two, fin)
    assert not np.array_equal(one, tl0) and not np.array_equal(one, fin)


def test_the_rule_case_pins_every_sentence():
    jobs, node, start = hc.rule_rows()
    tl0 = hc.rule_dense()
    got, state, applied, refused = hc.ref_hold_tl(tl0, jobs, node, start, hc.RULE_SLOT_MIN, hc.RULE_KMAX)
    assert state.tolist() == hc.RULE_STATE.tolist()
    assert refused == (hc.RULE_STATE == hc.REFUSED).sum() == 10
    assert applied == 7  # rows 2, 3, 8, 12, 13 of one node and row 16 of two
    assert (got[0, :20] == tl0[0, :20]).all() and got[0, 20:25].tolist() == [[3, 8092, 1]] * 5  # rows 0-2
    assert (got[1, :8] == 0).all() and got[1, 8].tolist() == [4, 8192, 2]                        # S == T
    assert np.array_equal(got[2], tl0[2]) and np.array_equal(got[3], tl0[3])                     # rows 4-6
    assert np.array_equal(got[4], tl0[4])                                                         # rows 7, 8
    assert (got[5, 10] == tl0[5, 10]).all() and got[5, 20:22, 0].tolist() == [0, 0] and got[5, 22, 0] == hc.INT32_MAX
    assert got[6, 60:62].tolist() == [[3, 8191, 1]] * 2 and got[6, 62:].tolist() == [[2, 8191, 1]] * 2  # clipped at H
    assert got[1, 62:, 0].tolist() == [3, 3] and (got[7] == -1).all()
    # each refused row of the B-node sentence fits alone
    alone = hc.ref_hold_tl(tl0, jobs, node, start, hc.RULE_SLOT_MIN, hc.RULE_KMAX, [6])
    assert alone[1][6] == hc.HELD and alone[3] == 0
    for q in (0, 1, 4, 5, 9):
        assert hc.ref_hold_tl(tl0, jobs, node, start, hc.RULE_SLOT_MIN, hc.RULE_KMAX, [q])[1][q] == hc.HELD, q
    # the outcome does not depend on the order of the rows
    perm, pj, pn, ps = hc.shuffled(jobs, node, start, 3)
    g2, s2, a2, r2 = hc.ref_hold_tl(tl0, pj, pn, ps, hc.RULE_SLOT_MIN, hc.RULE_KMAX)
    assert np.array_equal(g2, got) and np.array_equal(s2, state[perm]) and (a2, r2) == (applied, refused)


def test_the_seam_rows_conflict_only_in_pairs():
    jobs, node, start, pairs = hc.seam_rows()
    tl0 = np.empty((64, 64, 3), np.int32)
    tl0[:, :] = (hc.SEAM_CPU, 8192, 2)
    assert len(start) == 16390 and pairs[1] - pairs[0] > 16384 and pairs[2] // 16384 == pairs[3] // 16384
    _, state, applied, refused = hc.ref_hold_tl(tl0, jobs, node, start, 1, 1)
    assert refused == 4 and (state[pairs] == hc.REFUSED).all() and applied == 16386
    for q in pairs:
        assert hc.ref_hold_tl(tl0, jobs, node, start, 1, 1, [q])[1][q] == hc.HELD


# ---- 3. the cases are not vacuous ------------------------------------------------------------------------
@pytest.mark.parametrize("H,kmax", uc.ROUND_TRIP)
def test_replay_cases_are_not_vacuous(H, kmax):
    """At least 20 held rows, 5 of them multi-node at kmax 8, and a skipped row of each kind (an
    unplaced and a rejected one)."""
    c = hc.replay_conditions(H, kmax)
    print(H, kmax, c)
    assert c["held"] >= 20 and c["skipped_unplaced"] >= 1 and c["skipped_rejected"] >= 1 and c["refused"] == 0
    assert c["multi"] >= (5 if kmax == 8 else 0)


@pytest.mark.parametrize("H,kmax", hc.REFRESH)
def test_refresh_case_is_not_vacuous(H, kmax):
    """At least 20 held and 5 refused rows, a refused multi-node row where there are multi-node rows,
    rows refused by the running jobs and rows refused by the shortened avail_min."""
    jobs, out, start, _ = uc.reference(H, kmax)
    tl0, fin, state, applied, refused = hc.refresh_reference(H, kmax)
    nodes, _, _ = hc.refresh_cluster(H, kmax)
    old = pk.cluster(H)[0]
    print(H, kmax, dict(held=int((state == hc.HELD).sum()), refused=refused, applied=applied))
    assert (state == hc.HELD).sum() >= 20 and refused >= 5 and refused == (state == hc.REFUSED).sum()
    if kmax > 1:
        assert ((state == hc.REFUSED) & (jobs.nodes_k > 1)).any()
        assert ((state == hc.HELD) & (jobs.nodes_k > 1)).sum() >= 5
    assert len(np.unique(old.part_mask)) == 5 and (nodes.cpu_free != old.cpu_free).sum() == 5
    cut = np.flatnonzero(nodes.avail_min != old.avail_min)
    assert len(cut) >= 3
    ref = np.flatnonzero(state == hc.REFUSED)
    touched = [set(out[q, :max(int(jobs.nodes_k[q]), 1)].tolist()) for q in ref]
    assert any(t & set(cut.tolist()) for t in touched)
    assert any(t & set(np.flatnonzero(nodes.cpu_free != old.cpu_free).tolist()) for t in touched)

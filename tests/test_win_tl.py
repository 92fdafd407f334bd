"""fit_when_k_win / fit_place_tl_k_win without a device: the numpy restatement of DESIGN.md §2r (the
GPU tests' checker) against the unwindowed restatements with open windows and against the hand
table, the conditions that keep the GPU comparison from being vacuous — asserted on the restatement
alone, so a wrong draw fails here — and the host half of the entry points (header, ABI version,
message texts, NULL ctx)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _place_tl_k_cases as pk
import _when_k_cases as wk
import _win_tl_cases as wc
import fitgpu
from fitgpu import FIT_ETA_WINDOW, FIT_REJECTED, _lib
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
ENTRY = ("fit_when_k_win", "fit_when_k_win_device", "fit_place_tl_k_win", "fit_place_tl_k_win_device")
WINDOW_TEXT = "no start inside its window for 2 nodes at once: 3/7 nodes can run it there"


# ---- 1. the host half -----------------------------------------------------------------------------
def test_exports_and_abi():
    hdr = open(HDR).read()
    for name in ENTRY:
        assert re.search(r"\bint " + name + r"\(fit_ctx\* ctx, int32_t j,", hdr), name
        assert name in _lib.EXPORTS
    for name in ("fit_when_k_win_ms", "fit_when_k_win_message"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _lib.EXPORTS
    assert re.search(r"#define FITGPU_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert re.search(r"#define FIT_ETA_WINDOW 8\b", hdr) and FIT_ETA_WINDOW == _lib.FIT_ETA_WINDOW == 8
    for name in ("when_k_win", "when_k_win_device", "place_tl_k_win", "place_tl_k_win_device"):
        assert callable(getattr(fitgpu.Engine, name)), name
    assert "when_k_win_message" in fitgpu.__all__ and "FIT_ETA_WINDOW" in fitgpu.__all__


def _row(code, **kw):
    f = dict(code=code, dur=2, need=2, start=-1, wait_min=-1, members=7, hosts=3, now=1, ready=0, reserved=0)
    f.update(kw)
    return f


def test_message_texts_are_pinned():
    hdr = re.sub(r"\s*\n \*\s+", " ", open(HDR).read())  # the comment's wrapped lines joined
    assert '"no start inside its window for <need> nodes at once: <hosts>/<members> nodes can run it there"' in hdr
    assert fitgpu.when_k_win_message(_row(FIT_ETA_WINDOW)) == WINDOW_TEXT
    # every other code: fit_when_k_message's text, verbatim
    rows = [_row(c) for c in (1, 2, 3, 4, 5, 7)]
    rows += [_row(0, start=0, wait_min=0, ready=4), _row(6, start=3, wait_min=15, ready=2)]
    for r in rows:
        assert fitgpu.when_k_win_message(r) == fitgpu.when_k_message(r), r
    assert fitgpu.when_k_win_message(_row(0, start=0, wait_min=0, ready=4)) == "can start now on 2 of 4/7 nodes"
    # the unwindowed texts keep refusing the new code, the new text an unknown one and a short buffer
    L = _lib.lib()
    e = _lib.FitEtaK(code=FIT_ETA_WINDOW, need=2, members=7, hosts=3)
    buf = C.create_string_buffer(256)
    assert L.fit_when_k_message(C.byref(e), buf, 256) == _lib.FIT_E_INVAL
    e4 = _lib.FitEta(code=FIT_ETA_WINDOW)
    assert L.fit_when_message(C.byref(e4), buf, 256) == _lib.FIT_E_INVAL
    assert L.fit_when_k_win_message(C.byref(e), buf, 256) == len(WINDOW_TEXT) and buf.value.decode() == WINDOW_TEXT
    assert L.fit_when_k_win_message(C.byref(e), buf, len(WINDOW_TEXT)) == _lib.FIT_E_INVAL
    assert L.fit_when_k_win_message(C.byref(e), buf, len(WINDOW_TEXT) + 1) == len(WINDOW_TEXT)
    assert L.fit_when_k_win_message(None, buf, 256) == _lib.FIT_E_INVAL
    assert L.fit_when_k_win_message(C.byref(e), None, 256) == _lib.FIT_E_INVAL
    e.code = 9
    assert L.fit_when_k_win_message(C.byref(e), buf, 256) == _lib.FIT_E_INVAL


def test_null_ctx_answers_without_a_device():
    L = _lib.lib()
    one = np.ones(1, np.int32)
    k = np.ones(1, np.uint16)
    row = np.zeros(1, fitgpu.ETA_K_DTYPE)
    st = _lib.FitStats()
    ms = C.c_double()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    cols = (p(one), p(one), p(one), p(one), p(k), p(k))
    for fn in (L.fit_when_k_win, L.fit_when_k_win_device):
        assert fn(None, 0, *(None,) * 6, 1, None, None, None, None) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, *cols, 1, p(one), p(one), p(row), p(one)) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
    for fn in (L.fit_place_tl_k_win, L.fit_place_tl_k_win_device):
        assert fn(None, 0, *(None,) * 6, 1, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, *cols, 1, p(one), p(one), p(one), p(one), C.byref(st)) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
    assert L.fit_when_k_win_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


# ---- 2. open windows: the restatement is the unwindowed one ---------------------------------------
def _open_columns(j, H):
    """Columns that clamp to (0, H): NULL, 0 / INT32_MAX, negative not_before, deadline = H and above."""
    r = np.random.default_rng(j)
    return [(None, None), (np.zeros(j, np.int32), np.full(j, wc.NONE, np.int32)),
            (r.integers(-9, 1, j).astype(np.int32), r.choice([H, H + 1, wc.NONE], j).astype(np.int32))]


@pytest.mark.parametrize("case,rows,nodes", [(wk.hand_case, wk.HAND_ROWS, wk.HAND_NODES),
                                             (wk.edge_case, wk.EDGE_ROWS, wk.EDGE_NODES)])
def test_open_windows_equal_when_k(case, rows, nodes):
    nd, tline, jobs, parts = case()
    tl0 = po.ref_build_timeline(nd, tline)
    kmax = nodes.shape[1]
    want = wk.ref_when_k(tl0, nd.part_mask, parts, jobs, tline.slot_min, kmax)
    assert np.array_equal(want[0], rows) and np.array_equal(want[1], nodes)
    for nb, dl in _open_columns(jobs.j, tline.slots):
        got = wc.ref_when_k_win(tl0, nd.part_mask, parts, jobs, tline.slot_min, kmax, nb, dl)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_open_windows_equal_place_tl_k():
    nd, tline, jobs, parts = pk.hand_case()
    tl0 = po.ref_build_timeline(nd, tline)
    for nb, dl in _open_columns(jobs.j, tline.slots):
        out, start, fin = wc.ref_place_tl_k_win(tl0, nd.part_mask, parts, jobs, tline.slot_min, pk.HAND_KMAX, nb, dl)
        assert out.tolist() == pk.HAND_NODES.tolist() and start.tolist() == pk.HAND_START.tolist()
        assert fin[:, :, 0].tolist() == pk.HAND_CPU.tolist()
    H, j, kmax = 64, 300, 8
    nd, tline, parts = pk.cluster(H)
    jobs, wout, wstart, wfin = pk.reference("busy", H, j, kmax)
    for nb, dl in _open_columns(j, H):
        out, start, fin = wc.ref_place_tl_k_win(pk.start_timeline(H), nd.part_mask, parts, jobs, pk.SLOT_MIN, kmax,
                                                nb, dl)
        assert np.array_equal(out, wout) and np.array_equal(start, wstart) and np.array_equal(fin, wfin)


# ---- 3. the hand table ------------------------------------------------------------------------------
def test_hand_table():
    nodes, tline, jobs, parts, nb, dl = wc.hand_case()
    tl0 = po.ref_build_timeline(nodes, tline)
    rows, nd = wc.ref_when_k_win(tl0, nodes.part_mask, parts, jobs, tline.slot_min, wc.HAND_KMAX, nb, dl)
    assert rows.tolist() == wc.HAND_ROWS.tolist()
    assert nd.tolist() == wc.HAND_NODES.tolist()
    out, start, fin = wc.ref_place_tl_k_win(tl0, nodes.part_mask, parts, jobs, tline.slot_min, wc.HAND_KMAX, nb, dl)
    assert start.tolist() == wc.HAND_Q_START.tolist()
    assert out.tolist() == wc.HAND_Q_NODES.tolist() and out[10, 0] == FIT_REJECTED
    assert fin[:, :, 0].tolist() == wc.HAND_Q_CPU.tolist()
    assert rows["start"][7] == 1 and start[7] == -1  # placed alone, unplaced behind row 3
    job, tnb, tdl = wc.TRAP
    rows, nd = wc.ref_when_k_win(tl0, nodes.part_mask, parts, wk.jobs_of([job]), tline.slot_min, 1, [tnb], [tdl])
    assert (rows["start"][0], nd[0, 0]) == (5, wc.TRAP_NODE)


# ---- 4. the random inputs really exercise the window ---------------------------------------------------
@pytest.mark.parametrize("H,j,kmax", wc.WIN_CASES[1:])
def test_the_draw_exercises_the_window(H, j, kmax):
    """Asserted on the restatement alone.  This draw (seed 900 + H) gives placed / placed with
    start > from / placed later than judged alone / unplaced though placed unwindowed:
    H 64: 167 / 21 / 19 / 120;  H 1024: 158 / 15 / 15 / 131."""
    jobs, nb, dl = wc.win_case(H, j, kmax)
    out, start, fin = wc.reference(H, j, kmax)
    rows, _ = wc.alone(H, j, kmax)
    _, _, ustart, _ = pk.reference("busy", H, j, kmax)
    frm = np.clip(nb, 0, H)
    until = np.clip(dl, 0, H)
    d = wc.durs(jobs, wc.SLOT_MIN)
    placed = start >= 0
    later_than_from = placed & (start > frm)
    later_than_alone = placed & (start > rows["start"])
    lost = ~placed & (ustart >= 0)
    print(f"H {H}: placed {placed.sum()} start > from {later_than_from.sum()} later than alone "
          f"{later_than_alone.sum()} unplaced by the window {lost.sum()}")
    assert placed.sum() >= 100
    assert later_than_from.sum() >= 10
    assert later_than_alone.sum() >= 10
    assert lost.sum() >= 50
    # consequence 3 on the restatement itself
    assert (frm[placed] <= start[placed]).all() and (start[placed] + d[placed] <= until[placed]).all()

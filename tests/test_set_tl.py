"""fit_set_tl's host half (no device): the exports and the unchanged ABI version, argument checks that
must answer before any device call, the Python wrapper's shape errors, the laws of the restatement
(tests/_set_tl_cases.py ref_set_tl) on random rows, the conditions that keep the GPU cases from being
vacuous, asserted on the restatement alone, and text checks of the Go binding (no Go toolchain in the
image, as tests/test_go_binding.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _set_tl_cases as sc
import _when_k_cases as wk
import fitgpu
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
SYMS = ("fit_set_tl", "fit_set_tl_device", "fit_set_tl_ms")
INT32_MAX = sc.INT32_MAX


# ---- exports -------------------------------------------------------------------------------------
def test_exports_and_the_abi_version_is_still_8():
    hdr = open(HDR).read()
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    assert _lib.lib().fit_abi_version() == 8
    for sym in SYMS:
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"^int " + sym + r"\(", hdr, re.M), sym
    assert sorted(set(re.findall(r"\bfit_set_tl\w*", hdr))) == sorted(SYMS)
    for meth in ("set_tl", "set_tl_device", "set_tl_ms"):
        assert callable(getattr(fitgpu.Engine, meth))
    for name in SYMS[:2]:
        decl = hdr[hdr.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        assert all(f"const int32_t* {f}" in decl for f in ("node", "from", "to", "cpu", "mem", "gpu")), name
        assert "int64_t* applied" in decl and "int64_t* ignored" in decl, name


def test_null_ctx_answers_without_a_device_and_leaves_the_counts():
    L = _lib.lib()
    one = np.zeros(1, np.int32)
    p = C.c_void_p(one.ctypes.data)
    applied, ignored = C.c_int64(-5), C.c_int64(-6)
    for fn in (L.fit_set_tl, L.fit_set_tl_device):
        for m, ptr in ((0, None), (-1, None), (1, None), (1, p)):
            assert fn(None, m, *(ptr,) * 6, C.byref(applied), C.byref(ignored)) == _lib.FIT_E_INVAL
            assert b"null ctx" in L.fit_last_error()
        assert fn(None, 1, *(p,) * 6, None, None) == _lib.FIT_E_INVAL
    assert (applied.value, ignored.value) == (-5, -6)
    ms = C.c_double()
    assert L.fit_set_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


def test_the_wrapper_refuses_columns_that_disagree():
    e = object.__new__(fitgpu.Engine)  # no context: the shapes are judged before the library is called
    z = np.zeros(3, np.int32)
    lv = np.zeros((3, 3), np.int32)
    for bad in ((z[:2], z, z, lv), (z, z[:2], z, lv), (z, z, z[:1], lv), (z, z, z, lv[:2]), (z, z, z, lv[:, :2]),
                (z, z, z, z), (lv, z, z, lv), (z, z, z, np.zeros((3, 3, 1), np.int32))):
        with pytest.raises(ValueError):
            e.set_tl(*bad)


# ---- the laws of the restatement -----------------------------------------------------------------
def _random_batch(seed, n=6, H=20, m=60):
    r = np.random.default_rng(seed)
    tl = r.integers(-1, 9, (n, H, 3)).astype(np.int32)
    mask = np.array([1, 1, 0, 1, 2, 1], np.uint32)
    frm = r.integers(-2, H, m).astype(np.int32)
    to = (np.maximum(frm, 0) + r.integers(1, H, m)).astype(np.int32)
    to[r.random(m) < 0.1] = INT32_MAX
    return tl, mask, (r.integers(0, n, m).astype(np.int32), frm, to, r.integers(-1, 9, (m, 3)).astype(np.int32))


@pytest.mark.parametrize("seed", range(6))
def test_restatement_split_repeat_and_commutation(seed):
    tl, mask, c = _random_batch(seed)
    before = tl.tobytes()
    want, applied, ignored = sc.ref_set_tl(tl, *c, mask)
    assert tl.tobytes() == before, "the restatement wrote to its input"
    live = c[1] >= 0
    assert applied + ignored == live.sum() and ignored == (live & (mask[c[0]] == 0)).sum() > 0
    assert (want[mask == 0] == tl[mask == 0]).all() and want.dtype == np.int32
    # one call equals any split of its rows into consecutive calls
    r = np.random.default_rng(100 + seed)
    cuts = [0] + sorted(r.choice(np.arange(1, len(c[0])), 3, replace=False).tolist()) + [len(c[0])]
    step, tot = tl, [0, 0]
    for a, b in zip(cuts[:-1], cuts[1:]):
        step, x, y = sc.ref_set_tl(step, *sc.take(c, slice(a, b)), mask)
        tot = [tot[0] + x, tot[1] + y]
    assert step.tobytes() == want.tobytes() and tot == [applied, ignored]
    # a call repeated gives what one gives
    assert sc.ref_set_tl(want, *c, mask)[0].tobytes() == want.tobytes()
    # rows on different nodes or on disjoint windows commute: a stable sort by node keeps each node's order
    order = np.argsort(c[0], kind="stable")
    assert sc.ref_set_tl(tl, *sc.take(c, order), mask)[0].tobytes() == want.tobytes()
    a, b = (3, 0, 5, 1, 1, 1), (3, 5, INT32_MAX, 2, -1, 2)
    assert sc.ref_set_tl(tl, *sc.cols([a, b]))[0].tobytes() == sc.ref_set_tl(tl, *sc.cols([b, a]))[0].tobytes()
    # and rows that overlap with different levels do not: the rule is not vacuous
    a, b = (3, 0, 6, 1, 1, 1), (3, 5, 9, 2, -1, 2)
    assert sc.ref_set_tl(tl, *sc.cols([a, b]))[0].tobytes() != sc.ref_set_tl(tl, *sc.cols([b, a]))[0].tobytes()


@pytest.mark.parametrize("row", [(6, 0, 1, 0, 0, 0), (-1, 0, 1, 0, 0, 0), (0, 20, 21, 0, 0, 0), (0, 5, 5, 0, 0, 0),
                                 (0, 5, 4, 0, 0, 0), (0, 0, 1, -2, 0, 0), (0, 0, 1, 0, -2, 0), (0, 0, 1, 0, 0, -2)])
def test_restatement_refuses_what_the_library_refuses(row):
    tl, mask, _ = _random_batch(0)
    with pytest.raises(ValueError):
        sc.ref_set_tl(tl, *sc.cols([(0, 0, 3, 1, 1, 1), row]), mask)
    skipped = (row[0], -1) + row[2:]  # the same values in a skipped row are no error
    assert sc.ref_set_tl(tl, *sc.cols([skipped]), mask)[1:] == (0, 0)


def test_runs_as_rows_rebuild_a_timeline():
    tl, mask, c = _random_batch(3)
    want = sc.ref_set_tl(tl, *c)[0]
    rows = sc.runs_as_rows(want, range(tl.shape[0]))
    assert len(rows) == wk.run_counts(want).sum()
    assert sc.ref_set_tl(np.full_like(tl, 7), *sc.cols(rows))[0].tobytes() == want.tobytes()


# ---- the GPU cases are not vacuous -----------------------------------------------------------------
@pytest.mark.parametrize("H", sc.RANDOM_H)
def test_the_random_case_holds_its_conditions_on_the_restatement_alone(H):
    k = sc.random_conditions(H)
    assert 370 <= k["rows"] <= 440 and k["ignored"] == 3 and k["applied"] + k["ignored"] == k["live"]
    assert 4 * k["overlap"] >= k["live"], k          # >= 25 % overlap an earlier row with another level
    assert k["busiest"] > 64, k                      # more than 64 windows on one node: two window loads
    assert k["from0"] >= 3 and k["from_last"] >= 2 and k["to_h"] >= 3 and k["to_beyond"] >= 2 and k["to_max"] >= 4, k
    assert k["nothing"] and k["quiet_rows"] == 1 and k["one_closed"] >= 3 and k["skipped"] == 4, k
    # more than 64 runs need more than 64 slots: below that, a list that changes at most of its slots
    assert k["longest"] > (64 if H >= 100 else H // 2), k
    assert k["fell"] >= 1 and k["changed"] >= 45, k


def test_the_other_generators_hold_what_their_tests_rely_on():
    on7, others = sc.crowd()
    assert len(on7) == 300 and len(others) == 30 and len({r[0] for r in others}) == 30 and all(r[0] != 7 for r in others)
    node, frm, to, levels = sc.cols(on7)
    assert 4 * len(sc.overlapping(node, frm, to, levels, 64)) >= 3 * 300
    orders = [sc.interleaved(on7, others, s) for s in (1, 2, 3)]
    assert len({o[0].tobytes() for o in orders}) == 3  # three different orders of the same rows
    for o in orders:
        assert [tuple(r) for r in np.column_stack(o)[o[0] == 7].tolist()] == [tuple(r) for r in on7]
    c, pairs = sc.seam_rows()
    assert len(c[0]) == 16390 and pairs[0] // 16384 != pairs[1] // 16384 and pairs[2] // 16384 == pairs[3] // 16384
    hit = sc.overlapping(*c, 64)
    assert pairs[1] in hit and pairs[3] in hit
    (x, tx), (y, ty), differ = sc.two_clusters()
    from oracle import pyoracle as po
    dx, dy = po.ref_build_timeline(x, tx), po.ref_build_timeline(y, ty)
    assert np.flatnonzero((dx != dy).any(axis=(1, 2))).tolist() == differ
    assert (dy[1] == -1).all() and (dx[2] == -1).all() and wk.run_counts(dy)[2] >= 6
    assert (dy[3] == -1).sum() > (dx[3] == -1).sum() and (dy[4] == -1).sum() < (dx[4] == -1).sum()
    assert (dy[5].max(axis=0) > dx.max(axis=(0, 1))).all(), "node 5 is not above every ceiling of X"
    assert (dy[6].max(axis=0) < dx[6].max(axis=0)).all()


# ---- Go binding: text checks ---------------------------------------------------------------------
def test_go_binds_set_tl():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    eng = open(GO).read()
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", eng))
    assert called <= declared, sorted(called - declared)
    assert "fit_set_tl" in called
    assert re.search(r"func \(e \*Engine\) SetTL\(rows \[\]TLSet\) \(applied, ignored int64, err error\)", eng)
    assert len(re.findall(r"^type TLSet struct", eng, re.M)) == 1
    fn = eng[eng.index("func (e *Engine) SetTL("):]
    fn = fn[:fn.index("\n}\n")]
    assert fn.count("C.fit_set_tl(e.ctx") == 2 and "runtime.KeepAlive(e)" in fn and "check(rc)" in fn
    assert eng.index("func (e *Engine) ReadVictimsTL(") < eng.index("func (e *Engine) SetTL(")

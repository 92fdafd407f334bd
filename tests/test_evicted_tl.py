"""fit_evicted_tl's host half (no device): the exports and the unchanged ABI version, argument checks
that must answer before any device call, the reference (tests/_evicted_tl_cases.py ref_evicted_tl) on
the hand-written case with literal timelines and lists, what the reference refuses, the packed cases'
conditions at the recorded seeds, and text checks of the Go binding (no Go toolchain in the image, as
tests/test_go_binding.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _evicted_tl_cases as ec
import _preempt_tl_cases as tc
import fitgpu
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
SYMS = ("fit_evicted_tl", "fit_evicted_tl_device", "fit_evicted_tl_ms", "fit_read_victims_tl")


# ---- exports -------------------------------------------------------------------------------------
def test_exports_and_the_abi_version_is_still_8():
    hdr = open(HDR).read()
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    assert _lib.lib().fit_abi_version() == 8
    for sym in SYMS:
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"^int " + sym + r"\(", hdr, re.M), sym
    for meth in ("evicted_tl", "evicted_tl_device", "evicted_tl_ms", "read_victims_tl"):
        assert callable(getattr(fitgpu.Engine, meth))


def test_the_header_gained_no_struct_and_keeps_the_names_apart():
    hdr = open(HDR).read()
    assert not re.search(r"fit_evict_tl|fit_evict_k_tl", hdr)
    assert len(re.findall(r"\}\s*fit_evict_k;", hdr)) == 1 and len(re.findall(r"\}\s*fit_evict;", hdr)) == 1
    assert sorted(set(re.findall(r"\bfit_evicted_tl\w*", hdr))) == sorted(SYMS[:3])
    assert sorted(set(re.findall(r"\bfit_read_victims\w*", hdr))) == ["fit_read_victims_tl"]
    decl = hdr[hdr.index("int fit_read_victims_tl("):]
    decl = decl[:decl.index(";")]
    assert "int64_t cap" in decl and all(f"int32_t* {f}" in decl for f in ("off", "prio", "end", "cpu", "mem", "gpu"))


def test_null_and_negative_arguments_answer_without_a_device():
    L = _lib.lib()
    one = np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_evicted_tl, L.fit_evicted_tl_device):
        assert fn(None, 0, None, None) == _lib.FIT_E_INVAL
        assert fn(None, -1, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one)) == _lib.FIT_E_INVAL
    assert b"null ctx" in L.fit_last_error()
    ms = C.c_double()
    assert L.fit_evicted_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL
    assert L.fit_read_victims_tl(None, p(one), 0, None, None, None, None, None) == _lib.FIT_E_INVAL


# ---- the reference on the hand-written case ------------------------------------------------------
def lists_of(v):
    return [list(zip(*(np.asarray(getattr(v, f))[v.off[x]:v.off[x + 1]].tolist() for f in ec.VCOLS[1:])))
            for x in range(len(v.off) - 1)]


def test_reference_gives_the_hand_written_timelines_and_lists():
    T0, v0 = ec.hand_timeline(), tc.victims_tl_of(ec.HAND_LISTS)
    before = ec.bytes_of(T0, v0)
    T1, v1 = ec.ref_evicted_tl(T0, v0, ec.HAND_SHIFT, ec.HAND_ROWS_1, ec.HAND_MASK)
    assert ec.bytes_of(T0, v0) == before, "the reference wrote to its inputs"
    assert T1.dtype == np.int32 and T1.tolist() == ec.hand_expected(T0, ec.HAND_T1).tolist()
    assert lists_of(v1) == ec.HAND_LISTS_1
    # what the literal rows cover: an entry with e' = 0 that frees nothing, a middle entry, a last
    # entry, a whole list, several nodes, a closed slot inside a window, a -1 in one column, saturation
    assert T1[0, 4].tolist() == [-1, -1, -1] and T1[3, 1].tolist() == [5, 16, -1]
    assert T1[5, 0].tolist() == [ec.INF, ec.INF, 0] and T0[5, 0, 0] + 10 > ec.INF
    assert (T1[2] == T0[2]).all() and (T1[4] == -1).all()
    rows = np.array(ec.HAND_ROWS_1)
    assert len(set(rows[:, 0].tolist())) == 4
    # sorted rows give the same bytes
    T1s, v1s = ec.ref_evicted_tl(T0, v0, ec.HAND_SHIFT, sorted(ec.HAND_ROWS_1), ec.HAND_MASK)
    assert ec.bytes_of(T1s, v1s) == ec.bytes_of(T1, v1)
    # the prefix of node 0, on the state call 1 left: its ends are e' already
    T2, v2 = ec.ref_evicted_tl(T1, v1, 0, ec.HAND_ROWS_2)
    assert T2.tolist() == ec.hand_expected(T1, ec.HAND_T2).tolist() and lists_of(v2) == ec.HAND_LISTS_2
    # no rows: the timeline as it was, the ends as the queries read them, node 4's list gone
    T3, v3 = ec.ref_evicted_tl(T0, v0, ec.HAND_SHIFT, np.zeros((0, 2), np.int32), ec.HAND_MASK)
    assert T3.tolist() == T0.tolist() and lists_of(v3)[4] == [] and lists_of(v3)[0][0] == (1, 0, 1, 10, 0)
    assert [len(v) for v in lists_of(v3)] == [5, 2, 0, 3, 0, 1]


@pytest.mark.parametrize("rows", [
    [(0, 1), (0, 1)],            # the same pair twice
    [(0, 0), (1, 0), (0, 0)],
    [(0, 5)], [(2, 0)], [(1, 2)],  # a position equal to the length
    [(0, -1)], [(6, 0)], [(-1, 0)],
    [(4, 0)],                    # node 4 is in no partition: its list reads as empty
])
def test_reference_refuses_what_the_library_refuses(rows):
    T0, v0 = ec.hand_timeline(), tc.victims_tl_of(ec.HAND_LISTS)
    with pytest.raises(ValueError):
        ec.ref_evicted_tl(T0, v0, ec.HAND_SHIFT, rows, ec.HAND_MASK)
    if rows == [(4, 0)]:  # without the mask the entry is there
        ec.ref_evicted_tl(T0, v0, ec.HAND_SHIFT, rows)


def test_the_unplace_rows_of_the_defining_relation():
    v0 = tc.victims_tl_of(ec.HAND_LISTS)
    jobs, node, start = ec.unplace_rows(v0, ec.HAND_SHIFT, ec.HAND_ROWS_1, 10)
    # (0, 0) has e' = 0 and hands nothing back
    assert node.tolist() == [3, 0, 1, 5, 1] and not start.any() and jobs.wall.tolist() == [40, 50, 50, 50, 10]
    assert jobs.cpu.tolist() == [5, 4, 2, 10, 1] and (np.asarray(jobs.nodes_k) == 1).all()


# ---- the packed cases ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,one_component", sorted(ec.SEEDS))
def test_recorded_seeds_hold_the_conditions_on_the_reference_alone(n, one_component):
    c, rows = ec.packed_rows(n, one_component)
    T = ec.advanced(tc.oracle_timeline(c), ec.PACKED_SHIFT)
    ec.rich_enough(T, c.victims, ec.PACKED_SHIFT, rows, c.nodes.part_mask)
    assert (c.nodes.part_mask == 0).any() or n < 65


def test_the_recorded_case_has_a_job_the_double_count_changes():
    """INTEGRATION.md item 11 as it was: fit_unplace_tl of the evicted windows alone leaves the entries
    in the lists, and the next fit_preempt_tl counts their amounts on top of a timeline that holds them."""
    c, rows, T1, v1, wrong, true = ec.double_count_case()
    differ = [q for q in range(c.jobs.j) if tuple(wrong[q].tolist()) != tuple(true[q].tolist())]
    assert differ, "no job's answer differs: take another seed (DOUBLE_COUNT)"
    assert any(wrong[q]["code"] == tc.EVICT for q in differ)


# ---- Go binding: text checks ---------------------------------------------------------------------
def test_go_binds_evicted_tl_and_read_victims_tl():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    eng = open(GO).read()
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", eng))
    assert called <= declared, sorted(called - declared)
    assert {"fit_evicted_tl", "fit_read_victims_tl"} <= called
    assert re.search(r"func \(e \*Engine\) EvictedTL\(node, pos \[\]int32\) error", eng)
    assert re.search(r"func \(e \*Engine\) ReadVictimsTL\(\) \(VictimsTL, error\)", eng)
    assert eng.index("func (e *Engine) PreemptTLK(") < eng.index("func (e *Engine) EvictedTL(") < \
        eng.index("func (e *Engine) ReadVictimsTL(")
    ev = eng[eng.index("func (e *Engine) EvictedTL("):]
    ev = ev[:ev.index("\n}\n")]
    assert "len(node) != len(pos)" in ev and "&node[0]" in ev and "&pos[0]" in ev and "C.fit_evicted_tl(e.ctx" in ev
    rd = eng[eng.index("func (e *Engine) ReadVictimsTL("):]
    rd = rd[:rd.index("\n}\n")]
    assert rd.count("C.fit_read_victims_tl(e.ctx") == 2 and "e.nodes+1" in rd and "&v.End[0]" in rd
    assert len(re.findall(r"^type VictimsTL struct", eng, re.M)) == 1  # no second list type

"""fit_preempt's host half (no device): the codes, the row's layout against the header's struct, the
exact texts of fit_preempt_message as include/fitgpu.h fixes them, argument checks that must answer
before any device call, the reference (tests/_preempt_cases.py ref_preempt) on a hand-written case
with literal rows, the victim generator, and text checks of the Go binding (no Go toolchain in the
image, as tests/test_go_binding.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _preempt_cases as pc
import fitgpu
from fitgpu import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg")
FIELDS = ("code", "node", "victims", "top_prio", "members", "fit", "able", "outranked")
I32MAX, I32MIN = 2**31 - 1, -2**31


def row(code, node=-1, victims=0, top_prio=0, members=0, fit=0, able=0, outranked=0):
    return _lib.FitEvict(code, node, victims, top_prio, members, fit, able, outranked)


def msg(r, buflen=256):
    buf = C.create_string_buffer(buflen)
    n = _lib.lib().fit_preempt_message(C.byref(r), buf, buflen)
    return n, buf.value.decode()


# ---- codes, exports and layout -------------------------------------------------------------------
def test_codes_are_the_headers_and_one_to_five_are_fit_whys():
    hdr = open(HDR).read()
    names = ("FITS", "PARTITION", "LIMIT_TIME", "LIMIT_CPUS", "LIMIT_MEM", "NO_NODES", "EVICT", "NONE")
    for want, name in enumerate(names):
        m = re.search(r"#define FIT_PRE_" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == getattr(fitgpu, "FIT_PRE_" + name) == want, name
    for name in names[1:6]:
        assert getattr(fitgpu, "FIT_PRE_" + name) == getattr(fitgpu, "FIT_WHY_" + name)
    assert (pc.FITS, pc.PARTITION, pc.LIMIT_TIME, pc.LIMIT_CPUS, pc.LIMIT_MEM, pc.NO_NODES, pc.EVICT, pc.NONE) == \
        tuple(getattr(fitgpu, "FIT_PRE_" + n) for n in names)


def test_exports_and_the_abi_version_is_still_8():
    hdr = open(HDR).read()
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    assert _lib.lib().fit_abi_version() == 8
    for sym in ("fit_load_victims", "fit_load_victims_device", "fit_preempt", "fit_preempt_device", "fit_preempt_ms",
                "fit_preempt_message"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"^int " + sym + r"\(", hdr, re.M), sym
    for name in ("preempt_message", "EVICT_DTYPE", "FitEvict", "FIT_PRE_EVICT", "FIT_PRE_NONE"):
        assert name in fitgpu.__all__
    for meth in ("load_victims", "load_victims_device", "preempt", "preempt_device", "preempt_ms"):
        assert callable(getattr(fitgpu.Engine, meth))


def test_row_layout_is_the_headers_struct(tmp_path):
    """A C translation unit that includes the header prints sizeof and every offset of fit_evict:
    EVICT_DTYPE and the ctypes structure say the same, 32 bytes of int32."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fitgpu.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(fit_evict));\n' +
                   "".join(f'    printf(" %zu", offsetof(fit_evict, {f}));\n' for f in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    dt = fitgpu.EVICT_DTYPE
    assert dt.names == FIELDS == tuple(n for n, _ in _lib.FitEvict._fields_)
    assert got == [32] + [4 * i for i in range(8)]
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in FIELDS]
    assert got == [C.sizeof(_lib.FitEvict)] + [getattr(_lib.FitEvict, f).offset for f in FIELDS]
    assert all(dt.fields[f][0] == np.dtype(np.int32) for f in FIELDS)


# ---- texts ---------------------------------------------------------------------------------------
FIXED = [
    (fitgpu.FIT_PRE_PARTITION, "unknown partition"),
    (fitgpu.FIT_PRE_LIMIT_TIME, "walltime exceeds the partition's MaxTime"),
    (fitgpu.FIT_PRE_LIMIT_CPUS, "cpus per node exceed the partition's MaxCPUsPerNode"),
    (fitgpu.FIT_PRE_LIMIT_MEM, "memory per node exceeds the partition's MaxMemPerNode"),
    (fitgpu.FIT_PRE_NO_NODES, "no schedulable node in the partition"),
]


@pytest.mark.parametrize("code,text", FIXED)
def test_codes_one_to_five_take_fit_why_messages_sentences(code, text):
    for r in (row(code), row(code, 3, 2, 9, 7, 1, 1, 1)):  # the other fields play no part in these
        assert msg(r) == (len(text), text)
    w = _lib.FitWhy(code, 1, 0, 0, 0, 0, 0, 0)
    buf = C.create_string_buffer(256)
    assert _lib.lib().fit_why_message(C.byref(w), buf, 256) == len(text) and buf.value.decode() == text
    assert fitgpu.preempt_message(dict(zip(FIELDS, (code, -1, 0, 0, 0, 0, 0, 0)))) == text


def test_fits_evict_and_none_texts_byte_for_byte():
    F, E, N = fitgpu.FIT_PRE_FITS, fitgpu.FIT_PRE_EVICT, fitgpu.FIT_PRE_NONE
    assert msg(row(F, 7, members=40, fit=3, able=5)) == (len("3/40 nodes fit now"), "3/40 nodes fit now")
    want = "fits node 812 after evicting 2 lower-priority jobs (highest priority 10): 37/512 nodes can be freed"
    assert msg(row(E, 812, 2, 10, 512, 0, 37, 4)) == (len(want), want)
    # a negative top_prio, and one victim: the sentence does not inflect
    assert msg(row(E, 0, 1, -5, 1, 0, 1, 0))[1] == \
        "fits node 0 after evicting 1 lower-priority jobs (highest priority -5): 1/1 nodes can be freed"
    want = "no node can be freed on any of 512 nodes: 9 held by jobs of equal or higher priority"
    assert msg(row(N, members=512, outranked=9)) == (len(want), want)
    # outranked == 0: the colon and everything after it are left out
    want = "no node can be freed on any of 512 nodes"
    assert msg(row(N, members=512)) == (len(want), want)
    assert msg(row(N, members=0))[1] == "no node can be freed on any of 0 nodes"


def test_int32_extremes_fit_256_bytes():
    E = fitgpu.FIT_PRE_EVICT
    n, text = msg(row(E, I32MAX, I32MAX, I32MIN, I32MAX, 0, I32MAX, I32MAX))
    assert text == (f"fits node {I32MAX} after evicting {I32MAX} lower-priority jobs (highest priority {I32MIN}): "
                    f"{I32MAX}/{I32MAX} nodes can be freed")
    assert n == len(text) < 256
    n, text = msg(row(E, I32MIN, I32MIN, I32MAX, I32MIN, 0, I32MIN, 0))  # the longest there is: every field signed
    assert n == len(text) < 256 and text.count(str(I32MIN)) == 4 and f"priority {I32MAX})" in text
    n, text = msg(row(fitgpu.FIT_PRE_NONE, members=I32MIN, outranked=I32MIN))
    assert text == f"no node can be freed on any of {I32MIN} nodes: {I32MIN} held by jobs of equal or higher priority"
    assert msg(row(fitgpu.FIT_PRE_FITS, members=I32MAX, fit=I32MAX))[1] == f"{I32MAX}/{I32MAX} nodes fit now"


def test_buffer_too_small_null_arguments_and_unknown_codes():
    r = row(fitgpu.FIT_PRE_NONE, members=12)
    text = "no node can be freed on any of 12 nodes"
    assert msg(r, len(text) + 1) == (len(text), text)  # the text and its NUL fit exactly
    assert msg(r, len(text))[0] == _lib.FIT_E_INVAL      # one byte too small
    assert msg(r, 1)[0] == _lib.FIT_E_INVAL
    e = row(fitgpu.FIT_PRE_EVICT, 1, 1, 1, 1, 0, 1, 0)
    assert msg(e, len(msg(e)[1]))[0] == _lib.FIT_E_INVAL and msg(e, len(msg(e)[1]) + 1)[0] == len(msg(e)[1])
    assert msg(row(fitgpu.FIT_PRE_NO_NODES), 8)[0] == _lib.FIT_E_INVAL  # through fit_why_message too
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    assert L.fit_preempt_message(None, buf, 64) == _lib.FIT_E_INVAL
    assert L.fit_preempt_message(C.byref(r), None, 64) == _lib.FIT_E_INVAL
    assert L.fit_preempt_message(C.byref(r), buf, 0) == _lib.FIT_E_INVAL
    assert msg(row(8))[0] == _lib.FIT_E_INVAL and msg(row(-1))[0] == _lib.FIT_E_INVAL  # no such code
    with pytest.raises(fitgpu.FitError):
        fitgpu.preempt_message(row(99))


def test_preempt_message_takes_a_structured_row():
    a = np.zeros(2, fitgpu.EVICT_DTYPE)
    a[1] = (fitgpu.FIT_PRE_EVICT, 4, 3, 100, 9, 0, 2, 1)
    assert fitgpu.preempt_message(a[1]) == \
        "fits node 4 after evicting 3 lower-priority jobs (highest priority 100): 2/9 nodes can be freed"
    assert fitgpu.preempt_message(a[0]) == "0/0 nodes fit now"


def test_null_and_negative_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.EVICT_DTYPE)
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_preempt, L.fit_preempt_device):
        assert fn(None, 0, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, -1, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(one), p(one), p(out)) == _lib.FIT_E_INVAL
    assert b"null ctx" in L.fit_last_error()
    off = np.zeros(1, np.int32)
    assert L.fit_load_victims(None, p(off), None, None, None, None) == _lib.FIT_E_INVAL
    assert L.fit_load_victims(None, None, None, None, None, None) == _lib.FIT_E_INVAL
    assert L.fit_load_victims_device(None, None, 0, None, None, None, None) == _lib.FIT_E_INVAL
    ms = C.c_double()
    assert L.fit_preempt_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


# ---- the reference on the hand-written case ------------------------------------------------------
def test_reference_gives_the_hand_written_rows():
    c = pc.hand_case()
    got = pc.ref_preempt(c.nodes, c.victims, c.parts, c.jobs, c.prio)
    assert c.nodes.n == 6 and c.jobs.j == len(pc.HAND_ROWS)
    for q, want in enumerate(pc.HAND_ROWS):
        assert tuple(int(x) for x in got[q]) == want, (q, got[q], want)
    assert set(got["code"].tolist()) == set(range(8))  # every code
    for r in got:  # every row has a text
        assert fitgpu.preempt_message(r)
    assert fitgpu.preempt_message(got[4]) == \
        "fits node 0 after evicting 2 lower-priority jobs (highest priority 5): 2/5 nodes can be freed"
    assert fitgpu.preempt_message(got[1]) == \
        "no node can be freed on any of 5 nodes: 3 held by jobs of equal or higher priority"


def test_reference_follows_the_current_free_columns_and_an_empty_load():
    c = pc.hand_case()
    none = pc.ref_preempt(c.nodes, None, c.parts, c.jobs, c.prio)
    assert not none["able"].any() and not none["outranked"].any() and not (none["code"] == pc.EVICT).any()
    base = pc.ref_preempt(c.nodes, c.victims, c.parts, c.jobs, c.prio)
    assert np.array_equal(none["fit"], base["fit"]) and np.array_equal(none["members"], base["members"])
    free = (c.nodes.cpu_free + 6, c.nodes.mem_free, c.nodes.gpu_free)  # 6 more cpus everywhere: node 4 opens
    got = pc.ref_preempt(c.nodes, c.victims, c.parts, c.jobs, c.prio, free=free)
    # job 1, (6 cpus, 2048 MiB) at priority 5: nodes 0 (8, 8192) and 1 (6, 4096) fit, 1 the tighter; node 2 has
    # the cpus but no memory and node 4 only 5 cpus: one victim frees each
    assert tuple(int(x) for x in got[1]) == (pc.FITS, 1, 0, 0, 5, 2, 2, 0)


# ---- the generators ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,j", [(65, 65), (257, 128), (1000, 300)])
def test_packed_generator_meets_the_counts_on_the_reference_alone(n, j):
    c = pc.packed_case(n, j)
    want, stats = pc.packed_ref(n, j)
    pc.rich_enough(want, stats)
    assert (want["code"] == pc.FITS).any() or n == 65
    v = c.victims
    assert v.off[0] == 0 and len(v.off) == n + 1 and v.off[-1] == len(v.prio) and (np.diff(v.off) >= 0).all()
    inside = np.ones(len(v.prio), bool)
    inside[v.off[:-1][np.diff(v.off) > 0]] = False  # not a node's first entry
    assert (np.diff(v.prio)[inside[1:]] >= 0).all(), "eviction order: priorities do not decrease inside a node"
    assert min(v.cpu.min(), v.mem.min(), v.gpu.min()) >= 0
    assert 0 < (np.diff(v.off) == 0).sum() < n // 4  # a few nodes have no victim
    neg = (c.nodes.cpu_free < 0) | (c.nodes.mem_free < 0) | (c.nodes.gpu_free < 0)
    assert neg.any() and (c.nodes.part_mask == 0).any() and (c.nodes.avail_min < pc.INF).any()
    assert ((c.nodes.part_mask & (c.nodes.part_mask - 1)) != 0).any()  # nodes in two partitions


def test_pack_victims_packs_the_cluster_and_accounts_for_every_unit():
    nodes, _, _ = synth.make_config("c3", 3000, 1)
    packed, v = synth.pack_victims(7, nodes)
    n = nodes.n
    held = [np.add.reduceat(np.append(a, 0).astype(np.int64), v.off[:-1])
            * (np.diff(v.off) > 0) for a in (v.cpu, v.mem, v.gpu)]
    for before, after, h in zip((nodes.cpu_free, nodes.mem_free, nodes.gpu_free),
                                (packed.cpu_free, packed.mem_free, packed.gpu_free), held):
        assert np.array_equal(before.astype(np.int64), after.astype(np.int64) + h)  # free + held = what was free
        assert (after >= 0).all()
    has = np.diff(v.off) > 0
    assert (packed.cpu_free[has] == 0).all()  # packed: no free cpu where a victim runs
    assert 0.005 * n < (~has).sum() < 0.05 * n  # about 2 % stay as they were
    assert np.array_equal(packed.cpu_free[~has], nodes.cpu_free[~has])
    assert set(np.unique(v.prio).tolist()) <= set(synth.VIC_PRIO.tolist())
    assert set(np.unique(synth.gen_job_prio(7, 500)).tolist()) == set(synth.JOB_PRIO.tolist())
    again, v2 = synth.pack_victims(7, nodes)
    assert all(np.array_equal(a, b) for a, b in zip((v.off, v.prio, v.cpu, v.mem, v.gpu),
                                                    (v2.off, v2.prio, v2.cpu, v2.mem, v2.gpu)))  # a pure function


# ---- Go binding: text checks ---------------------------------------------------------------------
def _read(*parts):
    with open(os.path.join(GO, *parts)) as fh:
        return fh.read()


GO_FIELD = {"code": "Code", "node": "Node", "victims": "Victims", "top_prio": "TopPrio", "members": "Members",
            "fit": "Fit", "able": "Able", "outranked": "Outranked"}


def test_go_binds_preempt_and_every_field_crosses_both_ways():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    eng = _read("fitgpu", "fitgpu.go")
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", eng))
    assert called <= declared, sorted(called - declared)
    assert {"fit_load_victims", "fit_preempt", "fit_preempt_message"} <= called
    assert re.search(r"type Victims struct \{\n\tOff, Prio, CPU, MemMiB, GPU \[\]int32\n\}", eng)
    assert re.search(r"type Evict struct \{", eng)
    assert re.search(r"func \(e \*Engine\) LoadVictims\(v Victims\) error", eng)
    assert re.search(r"func \(e \*Engine\) Preempt\(j Jobs, prio \[\]int32\) \(\[\]Evict, error\)", eng)
    assert re.search(r"func PreemptMessage\(r Evict\) string", eng)
    load = eng[eng.index("func (e *Engine) LoadVictims("):eng.index("// Preempt codes")]
    assert "C.fit_load_victims(e.ctx, nil, nil, nil, nil, nil)" in load  # no victims at all
    assert "len(v.Prio)" in load and "errLen" in load  # the lengths are checked before the pointers cross
    go_evict = eng[eng.index("func goEvict("):eng.index("func (e *Engine) Preempt(")]
    pre = eng[eng.index("func (e *Engine) Preempt("):eng.index("func PreemptMessage(")]
    assert "len(prio)" in pre and "&prio[0]" in pre and "C.fit_evict" in pre
    message = eng[eng.index("func PreemptMessage("):]
    message = message[:message.index("\n}\n")]
    for c, g in GO_FIELD.items():
        assert re.search(r"\b" + g + r"\s+int32\b", eng), f"Evict has no {g} int32"
        assert re.search(r"\b" + g + r":\s*int32\(r\." + c + r"\)", go_evict), f"goEvict does not copy {c}"
        assert re.search(r"\b" + c + r":\s*C\.int32_t\(r\." + g + r"\)", message), f"PreemptMessage does not set {c}"
    for name in ("Fits", "Partition", "LimitTime", "LimitCPUs", "LimitMem", "NoNodes", "Evict", "None"):
        assert re.search(r"\bPre" + name + r"\s*=\s*int32\(C\.FIT_PRE_", eng), name

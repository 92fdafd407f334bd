"""fit_room's host half (no device): the exact texts of fit_room_message as include/fitgpu.h fixes
them, the row's layout against the header's struct, argument checks that must answer before any
device call, and text checks of the Go binding and call site (no Go toolchain in the image, as
tests/test_go_binding.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fitgpu
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg")
FIELDS = ("code", "members", "nodes", "best", "copies", "best_node", "by_gpu", "by_cpu", "by_mem")


def row(code, members=0, nodes=0, best=0, copies=0, best_node=-1, gpu=0, cpu=0, mem=0):
    return _lib.FitRoom(code, members, nodes, best, copies, best_node, gpu, cpu, mem)


def msg(r, buflen=256):
    buf = C.create_string_buffer(buflen)
    n = _lib.lib().fit_room_message(C.byref(r), buf, buflen)
    return n, buf.value.decode()


# ---- codes and layout ----------------------------------------------------------------------------
def test_codes_are_the_headers_and_one_to_five_are_fit_whys():
    hdr = open(HDR).read()
    names = ("SOME", "PARTITION", "LIMIT_TIME", "LIMIT_CPUS", "LIMIT_MEM", "NO_NODES", "NONE")
    for want, name in enumerate(names):
        m = re.search(r"#define FIT_ROOM_" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == getattr(fitgpu, "FIT_ROOM_" + name) == want, name
    for name in names[1:6]:
        assert getattr(fitgpu, "FIT_ROOM_" + name) == getattr(fitgpu, "FIT_WHY_" + name)
    m = re.search(r"#define FIT_ROOM_UNBOUNDED\s+(\d+)", hdr)
    assert m and int(m.group(1)) == fitgpu.FIT_ROOM_UNBOUNDED == 2**31 - 1
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    for sym in ("fit_room", "fit_room_device", "fit_room_ms", "fit_room_message", "fit_admitter_room"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym


def test_row_layout_is_the_headers_struct(tmp_path):
    """A C translation unit that includes the header prints sizeof and every offset of struct
    fit_room: ROOM_DTYPE and the ctypes structure say the same, with copies at offset 16."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fitgpu.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(struct fit_room));\n' +
                   "".join(f'    printf(" %zu", offsetof(struct fit_room, {f}));\n' for f in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    dt = fitgpu.ROOM_DTYPE
    assert dt.names == FIELDS == tuple(n for n, _ in _lib.FitRoom._fields_)
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in FIELDS]
    assert got == [C.sizeof(_lib.FitRoom)] + [getattr(_lib.FitRoom, f).offset for f in FIELDS]
    assert dt.itemsize == 40 and dt.fields["copies"] == (np.dtype(np.int64), 16)
    assert all(dt.fields[f][0] == np.dtype(np.int32) for f in FIELDS if f != "copies")


# ---- texts ---------------------------------------------------------------------------------------
FIXED = [
    (fitgpu.FIT_ROOM_PARTITION, "unknown partition"),
    (fitgpu.FIT_ROOM_LIMIT_TIME, "walltime exceeds the partition's MaxTime"),
    (fitgpu.FIT_ROOM_LIMIT_CPUS, "cpus per node exceed the partition's MaxCPUsPerNode"),
    (fitgpu.FIT_ROOM_LIMIT_MEM, "memory per node exceeds the partition's MaxMemPerNode"),
    (fitgpu.FIT_ROOM_NO_NODES, "no schedulable node in the partition"),
]


@pytest.mark.parametrize("code,text", FIXED)
def test_codes_one_to_five_take_fit_why_messages_sentences(code, text):
    for r in (row(code), row(code, 9, 3, 2, 5, 1, 1, 1, 1)):  # the counters play no part in these
        assert msg(r) == (len(text), text)
    w = _lib.FitWhy(code, 1, 0, 0, 0, 0, 0, 0)
    buf = C.create_string_buffer(256)
    assert _lib.lib().fit_why_message(C.byref(w), buf, 256) == len(text) and buf.value.decode() == text
    assert fitgpu.room_message(dict(zip(FIELDS, (code, 0, 0, 0, 0, -1, 0, 0, 0)))) == text


def test_some_text_and_zero_term_elision():
    S = fitgpu.FIT_ROOM_SOME
    want = "room for 12 more on 3/40 nodes (at most 5 on one node): limited by gpu on 1, cpu on 1, memory on 1"
    assert msg(row(S, 40, 3, 5, 12, 7, 1, 1, 1)) == (len(want), want)
    assert msg(row(S, 40, 3, 5, 12, 7, gpu=3))[1] == "room for 12 more on 3/40 nodes (at most 5 on one node): limited by gpu on 3"
    assert msg(row(S, 40, 3, 5, 12, 7, cpu=3))[1] == "room for 12 more on 3/40 nodes (at most 5 on one node): limited by cpu on 3"
    assert msg(row(S, 40, 3, 5, 12, 7, mem=3))[1] == \
        "room for 12 more on 3/40 nodes (at most 5 on one node): limited by memory on 3"
    assert msg(row(S, 40, 3, 5, 12, 7, gpu=2, mem=1))[1] == \
        "room for 12 more on 3/40 nodes (at most 5 on one node): limited by gpu on 2, memory on 1"
    assert msg(row(S, 40, 3, 5, 12, 7, cpu=1, mem=2))[1] == \
        "room for 12 more on 3/40 nodes (at most 5 on one node): limited by cpu on 1, memory on 2"
    # no term left: the ": limited by " goes too
    assert msg(row(S, 40, 3, 5, 12, 7))[1] == "room for 12 more on 3/40 nodes (at most 5 on one node)"


def test_unbounded_none_and_a_copies_above_two_to_the_32():
    S, U = fitgpu.FIT_ROOM_SOME, fitgpu.FIT_ROOM_UNBOUNDED
    assert msg(row(S, 9, 7, U, 7 * U, 0))[1] == "no resource demand: unlimited room on 7/9 nodes"
    assert msg(row(S, 9, 7, U - 1, 7, 0, cpu=7))[1].startswith("room for 7 more on 7/9 nodes (at most 2147483646 on one")
    assert msg(row(fitgpu.FIT_ROOM_NONE, 6273))[1] == "no room now on any of 6273 nodes"
    big = 3 * (2**31 - 2)
    assert big > 2**32
    want = f"room for {big} more on 3/3 nodes (at most 2147483646 on one node): limited by cpu on 3"
    assert msg(row(S, 3, 3, 2**31 - 2, big, 0, cpu=3)) == (len(want), want)
    top = 2**63 - 1  # the longest row there is still fits 256 bytes
    n, text = msg(row(S, U, U, U - 1, top, U, U, U, U))
    assert n == len(text) < 256 and str(top) in text


def test_buffer_too_small_null_arguments_and_unknown_codes():
    r = row(fitgpu.FIT_ROOM_NONE, 12)
    text = "no room now on any of 12 nodes"
    assert msg(r, len(text) + 1) == (len(text), text)  # the text and its NUL fit exactly
    assert msg(r, len(text))[0] == _lib.FIT_E_INVAL
    assert msg(r, 1)[0] == _lib.FIT_E_INVAL
    assert msg(row(fitgpu.FIT_ROOM_NO_NODES), 8)[0] == _lib.FIT_E_INVAL  # through fit_why_message too
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    assert L.fit_room_message(None, buf, 64) == _lib.FIT_E_INVAL
    assert L.fit_room_message(C.byref(r), None, 64) == _lib.FIT_E_INVAL
    assert L.fit_room_message(C.byref(r), buf, 0) == _lib.FIT_E_INVAL
    assert msg(row(7))[0] == _lib.FIT_E_INVAL and msg(row(-1))[0] == _lib.FIT_E_INVAL  # no such code
    with pytest.raises(fitgpu.FitError):
        fitgpu.room_message(row(99))


def test_room_message_takes_a_structured_row():
    a = np.zeros(2, fitgpu.ROOM_DTYPE)
    a[1] = (fitgpu.FIT_ROOM_SOME, 5, 2, 4, 2**33 + 1, 3, 0, 2, 0)
    assert fitgpu.room_message(a[1]) == f"room for {2**33 + 1} more on 2/5 nodes (at most 4 on one node): limited by cpu on 2"
    assert fitgpu.room_message(a[0]) == "room for 0 more on 0/0 nodes (at most 0 on one node)"


def test_null_and_zero_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.ROOM_DTYPE)
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_room, L.fit_room_device):
        assert fn(None, 0, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(one), p(out)) == _lib.FIT_E_INVAL
    ms = C.c_double()
    assert L.fit_room_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL
    assert L.fit_admitter_room(None, None, 0, None) == _lib.FIT_E_INVAL
    q = _lib.FitAdmitReq(0, 1, 1, 0, 1, 0, 1)
    assert L.fit_admitter_room(None, C.byref(q), 1, p(out)) == _lib.FIT_E_INVAL
    assert b"bad arguments" in L.fit_last_error()


# ---- Go binding and call site: text checks -------------------------------------------------------
def _read(*parts):
    with open(os.path.join(GO, *parts)) as fh:
        return fh.read()


GO_FIELD = {"code": "Code", "members": "Members", "nodes": "Nodes", "best": "Best", "copies": "Copies",
            "best_node": "BestNode", "by_gpu": "ByGPU", "by_cpu": "ByCPU", "by_mem": "ByMem"}


def test_go_binds_room_and_every_field_crosses_both_ways():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    srcs = {f: _read("fitgpu", f) for f in sorted(os.listdir(os.path.join(GO, "fitgpu"))) if f.endswith(".go")}
    called = set()
    for text in srcs.values():
        called |= set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", text))
    assert called <= declared, sorted(called - declared)
    assert {"fit_room", "fit_admitter_room", "fit_room_message"} <= called
    eng, adm = srcs["fitgpu.go"], srcs["admit.go"]
    assert re.search(r"type Room struct \{", eng)
    assert re.search(r"func \(e \*Engine\) Room\(j Jobs\) \(\[\]Room, error\)", eng)
    assert re.search(r"func \(ad \*Admitter\) Room\(ds \[\]Demand\) \(\[\]Room, error\)", adm)
    assert re.search(r"func RoomMessage\(r Room\) string", eng)
    assert "C.struct_fit_room" in eng and "C.struct_fit_room" in adm  # the row is a struct tag in the header
    go_room = eng[eng.index("func goRoom("):eng.index("func (e *Engine) Room(")]
    message = eng[eng.index("func RoomMessage("):]
    message = message[:message.index("\n}\n")]
    for c, g in GO_FIELD.items():
        ctype = "int64" if c == "copies" else "int32"
        assert re.search(r"\b" + g + r"\s+" + ctype + r"\b", eng), f"Room has no {g} {ctype}"
        assert re.search(r"\b" + g + r":\s*" + ctype + r"\(r\." + c + r"\)", go_room), f"goRoom does not copy {c}"
        assert re.search(r"\b" + c + r":\s*C\." + ctype + r"_t\(r\." + g + r"\)", message), f"RoomMessage does not set {c}"
    for name in ("Some", "Partition", "LimitTime", "LimitCPUs", "LimitMem", "NoNodes", "None", "Unbounded"):
        assert re.search(r"\bRoom" + name + r"\s*=\s*int32\(C\.FIT_ROOM_", eng), name


def test_call_site_reports_the_room_for_an_array_job():
    src = _read("slurm-virtual-kubelet", "fit_admission.go")
    assert "exceeds the partition's limits" in src
    assert "no Slurm node of the partition fits it now" in src
    assert "f.adm.Room(" in src
    assert '": room for %d of its %d array tasks now"' in src
    admit = src[src.index("func (f *FitAdmission) admit("):src.index("func (f *FitAdmission) release(")]
    assert admit.count("f.why(pod, ds)") == 2
    why = admit[admit.index("func (f *FitAdmission) why("):]
    fits = why[why.index("fitgpu.WhyFits"):]
    fits = fits[:fits.index("fitgpu.WhyMessage(")]
    # inside the WhyFits branch: only an array job of one-node tasks asks, of its first request
    assert re.search(r"len\(ds\) > 1 && ds\[0\]\.NodesK <= 1", fits)
    assert "f.adm.Room(ds[:1])" in fits and re.search(r"Copies < int64\(len\(ds\)\)", fits)
    assert "klog." in fits and fits.count('return ""') >= 2  # a Room error only logs; otherwise the old text

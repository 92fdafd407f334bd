"""fit_when's host half (no device): the exact texts of fit_when_message as include/fitgpu.h fixes
them, the row layout, the codes shared with fit_why, argument checks that must answer before any
device call, and text checks of the Go binding (no Go toolchain in the image, as
tests/test_go_binding.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fitgpu
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu")
FIELDS = ["code", "dur", "start", "node", "wait_min", "members", "hosts", "now"]


def row(code, dur=1, start=-1, node=-1, wait_min=-1, members=0, hosts=0, now=0):
    return _lib.FitEta(code, dur, start, node, wait_min, members, hosts, now)


def msg(e, buflen=256):
    buf = C.create_string_buffer(buflen)
    n = _lib.lib().fit_when_message(C.byref(e), buf, buflen)
    return n, buf.value.decode()


def test_row_layout_matches_the_header():
    assert C.sizeof(_lib.FitEta) == 32 and fitgpu.ETA_DTYPE.itemsize == 32
    assert list(fitgpu.ETA_DTYPE.names) == FIELDS == [n for n, _ in _lib.FitEta._fields_]
    assert all(fitgpu.ETA_DTYPE.fields[n][0] == np.int32 for n in FIELDS)
    assert [fitgpu.ETA_DTYPE.fields[n][1] for n in FIELDS] == list(range(0, 32, 4))
    hdr = open(HDR).read()
    body = re.search(r"typedef struct \{([^}]*)\} fit_eta;", hdr).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == FIELDS


def test_codes_match_the_header_and_fit_why():
    hdr = open(HDR).read()
    want = {"NOW": 0, "PARTITION": 1, "LIMIT_TIME": 2, "LIMIT_CPUS": 3, "LIMIT_MEM": 4, "NO_NODES": 5, "LATER": 6,
            "HORIZON": 7}
    for name, v in want.items():
        m = re.search(r"#define FIT_ETA_" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == v == getattr(fitgpu, "FIT_ETA_" + name), name
    for name in ("PARTITION", "LIMIT_TIME", "LIMIT_CPUS", "LIMIT_MEM", "NO_NODES"):  # FIT_ETA_1..5 = FIT_WHY_1..5
        assert getattr(fitgpu, "FIT_ETA_" + name) == getattr(fitgpu, "FIT_WHY_" + name), name


TEXTS = [
    (row(fitgpu.FIT_ETA_NOW, 3, 0, 17, 0, members=40, hosts=33, now=12), "can start now on 12/40 nodes"),
    (row(fitgpu.FIT_ETA_LATER, 6, 7, 412, 35, members=40, hosts=12, now=0),
     "earliest start in 35 min (slot 7): 12/40 nodes can run it inside the horizon, none now"),
    (row(fitgpu.FIT_ETA_LATER, 1, 1023, 0, 2**31 - 1, members=1, hosts=1),
     "earliest start in 2147483647 min (slot 1023): 1/1 nodes can run it inside the horizon, none now"),
    (row(fitgpu.FIT_ETA_HORIZON, 2000, members=6273), "no start inside the horizon on any of 6273 nodes"),
    (row(fitgpu.FIT_ETA_PARTITION), "unknown partition"),
    (row(fitgpu.FIT_ETA_LIMIT_TIME), "walltime exceeds the partition's MaxTime"),
    (row(fitgpu.FIT_ETA_LIMIT_CPUS), "cpus per node exceed the partition's MaxCPUsPerNode"),
    (row(fitgpu.FIT_ETA_LIMIT_MEM), "memory per node exceeds the partition's MaxMemPerNode"),
    (row(fitgpu.FIT_ETA_NO_NODES), "no schedulable node in the partition"),
]


@pytest.mark.parametrize("e,text", TEXTS, ids=[str(e.code) + "-" + str(i) for i, (e, _) in enumerate(TEXTS)])
def test_exact_texts(e, text):
    assert msg(e) == (len(text), text)
    assert fitgpu.when_message(e) == text
    assert fitgpu.when_message({n: getattr(e, n) for n in FIELDS}) == text
    assert msg(e, len(text) + 1) == (len(text), text)  # the text and its NUL fit exactly
    assert msg(e, len(text))[0] == _lib.FIT_E_INVAL


def test_codes_one_to_five_reuse_fit_why_message():
    for code in range(1, 6):
        w = _lib.FitWhy(code, 1, 0, 0, 0, 0, 0, 0)
        buf = C.create_string_buffer(256)
        n = _lib.lib().fit_why_message(C.byref(w), buf, 256)
        assert msg(row(code, dur=9, members=5, hosts=4, now=3)) == (n, buf.value.decode())


def test_bad_arguments():
    L = _lib.lib()
    e = row(fitgpu.FIT_ETA_NOW)
    buf = C.create_string_buffer(64)
    assert L.fit_when_message(None, buf, 64) == _lib.FIT_E_INVAL
    assert L.fit_when_message(C.byref(e), None, 64) == _lib.FIT_E_INVAL
    assert L.fit_when_message(C.byref(e), buf, 0) == _lib.FIT_E_INVAL
    assert msg(e, 1)[0] == _lib.FIT_E_INVAL
    assert msg(row(8))[0] == _lib.FIT_E_INVAL and msg(row(-1))[0] == _lib.FIT_E_INVAL  # no such code
    with pytest.raises(fitgpu.FitError):
        fitgpu.when_message(row(99))


def test_when_message_takes_a_structured_row():
    a = np.zeros(2, fitgpu.ETA_DTYPE)
    a[1] = (fitgpu.FIT_ETA_LATER, 2, 4, 9, 20, 7, 5, 0)
    assert fitgpu.when_message(a[1]) == \
        "earliest start in 20 min (slot 4): 5/7 nodes can run it inside the horizon, none now"
    assert fitgpu.when_message(a[0]) == "can start now on 0/0 nodes"


def test_null_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.ETA_DTYPE)
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_when, L.fit_when_device):
        assert fn(None, 0, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(one), p(out)) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
    ms = C.c_double()
    assert L.fit_when_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL


# ---- Go binding: text checks -------------------------------------------------------------------
def test_go_binds_when_with_declared_functions_and_every_field():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    srcs = {f: open(os.path.join(GO, f)).read() for f in sorted(os.listdir(GO)) if f.endswith(".go")}
    called = set()
    for text in srcs.values():
        called |= set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", text))
    when_calls = {c for c in called if c.startswith("fit_when")}
    assert when_calls == {"fit_when", "fit_when_message"} and when_calls <= declared
    assert called <= declared, sorted(called - declared)
    go = srcs["fitgpu.go"]
    assert re.search(r"func \(e \*Engine\) When\(j Jobs\) \(\[\]Eta, error\)", go)
    assert re.search(r"func WhenMessage\(\w+ Eta\) string", go)
    eta = re.search(r"type Eta struct \{(.*?)\n\}", go, re.S).group(1)
    assert re.findall(r"^\s*(\w+)\s+int32\b", eta, re.M) == ["Code", "Dur", "Start", "Node", "WaitMin", "Members",
                                                             "Hosts", "Now"]
    # every field of fit_eta crosses into the Go row and back into the C row WhenMessage builds
    for f in FIELDS:
        assert re.search(r"\br\." + f + r"\b", go), f"goEta does not copy {f}"
        assert re.search(r"\b" + f + r":\s*C\.int32_t\(", go), f"WhenMessage does not set {f}"
    for name in ("NOW", "PARTITION", "LIMIT_TIME", "LIMIT_CPUS", "LIMIT_MEM", "NO_NODES", "LATER", "HORIZON"):
        assert "C.FIT_ETA_" + name in go, name

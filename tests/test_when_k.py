"""fit_when_k's host half (no device): the exact texts of fit_when_k_message as include/fitgpu.h
fixes them, the 40-byte row layout, and argument checks that must answer before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fitgpu
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
FIELDS = ["code", "dur", "need", "start", "wait_min", "members", "hosts", "now", "ready", "reserved"]


def row(code, dur=1, need=1, start=-1, wait_min=-1, members=0, hosts=0, now=0, ready=0):
    return _lib.FitEtaK(code, dur, need, start, wait_min, members, hosts, now, ready, 0)


def msg(e, buflen=256):
    buf = C.create_string_buffer(buflen)
    n = _lib.lib().fit_when_k_message(C.byref(e), buf, buflen)
    return n, buf.value.decode()


def test_row_layout_matches_the_header():
    assert C.sizeof(_lib.FitEtaK) == 40 and fitgpu.ETA_K_DTYPE.itemsize == 40  # sizeof(fit_eta_k)
    assert list(fitgpu.ETA_K_DTYPE.names) == FIELDS == [n for n, _ in _lib.FitEtaK._fields_]
    assert all(fitgpu.ETA_K_DTYPE.fields[n][0] == np.int32 for n in FIELDS)
    assert [fitgpu.ETA_K_DTYPE.fields[n][1] for n in FIELDS] == list(range(0, 40, 4))
    hdr = open(HDR).read()
    body = re.search(r"typedef struct \{([^}]*)\} fit_eta_k;", hdr).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == FIELDS
    assert re.search(r"#define FITGPU_ABI_VERSION\s+8\b", hdr)  # additive: the version stays


M = 2**31 - 1
TEXTS = [
    (row(fitgpu.FIT_ETA_NOW, 3, 2, 0, 0, members=40, hosts=33, now=12, ready=12), "can start now on 2 of 12/40 nodes"),
    (row(fitgpu.FIT_ETA_NOW, 1, 1, 0, 0, members=1, hosts=1, now=1, ready=1), "can start now on 1 of 1/1 nodes"),
    (row(fitgpu.FIT_ETA_LATER, 6, 4, 7, 35, members=40, hosts=12, now=1, ready=5),
     "earliest start in 35 min (slot 7) on 4 of 5/40 nodes, 1 free now"),
    (row(fitgpu.FIT_ETA_LATER, 1, 8, 1023, M, members=M, hosts=M, now=M, ready=M),
     f"earliest start in {M} min (slot 1023) on 8 of {M}/{M} nodes, {M} free now"),
    (row(fitgpu.FIT_ETA_HORIZON, 2000, 8, members=6273, hosts=5),
     "no start inside the horizon for 8 nodes at once: 5/6273 nodes can run it"),
    (row(fitgpu.FIT_ETA_PARTITION), "unknown partition"),
    (row(fitgpu.FIT_ETA_LIMIT_TIME), "walltime exceeds the partition's MaxTime"),
    (row(fitgpu.FIT_ETA_LIMIT_CPUS), "cpus per node exceed the partition's MaxCPUsPerNode"),
    (row(fitgpu.FIT_ETA_LIMIT_MEM), "memory per node exceeds the partition's MaxMemPerNode"),
    (row(fitgpu.FIT_ETA_NO_NODES), "no schedulable node in the partition"),
]


@pytest.mark.parametrize("e,text", TEXTS, ids=[str(e.code) + "-" + str(i) for i, (e, _) in enumerate(TEXTS)])
def test_exact_texts(e, text):
    assert msg(e) == (len(text), text) and len(text) < 256
    assert fitgpu.when_k_message(e) == text
    assert fitgpu.when_k_message({n: getattr(e, n) for n in FIELDS}) == text
    assert msg(e, len(text) + 1) == (len(text), text)  # the text and its NUL fit exactly
    assert msg(e, len(text))[0] == _lib.FIT_E_INVAL    # a buffer too small


def test_codes_one_to_five_reuse_fit_why_message():
    for code in range(1, 6):
        w = _lib.FitWhy(code, 1, 0, 0, 0, 0, 0, 0)
        buf = C.create_string_buffer(256)
        n = _lib.lib().fit_why_message(C.byref(w), buf, 256)
        assert msg(row(code, dur=9, need=4, members=5, hosts=4, now=3)) == (n, buf.value.decode())


def test_bad_arguments():
    L = _lib.lib()
    e = row(fitgpu.FIT_ETA_NOW)
    buf = C.create_string_buffer(64)
    assert L.fit_when_k_message(None, buf, 64) == _lib.FIT_E_INVAL
    assert L.fit_when_k_message(C.byref(e), None, 64) == _lib.FIT_E_INVAL
    assert L.fit_when_k_message(C.byref(e), buf, 0) == _lib.FIT_E_INVAL
    assert msg(e, 1)[0] == _lib.FIT_E_INVAL
    assert msg(row(8))[0] == _lib.FIT_E_INVAL and msg(row(-1))[0] == _lib.FIT_E_INVAL  # no such code
    with pytest.raises(fitgpu.FitError):
        fitgpu.when_k_message(row(99))


def test_when_k_message_takes_a_structured_row():
    a = np.zeros(2, fitgpu.ETA_K_DTYPE)
    a[1] = (fitgpu.FIT_ETA_LATER, 2, 3, 4, 20, 7, 5, 0, 3, 0)
    assert fitgpu.when_k_message(a[1]) == "earliest start in 20 min (slot 4) on 3 of 3/7 nodes, 0 free now"
    assert fitgpu.when_k_message(a[0]) == "can start now on 0 of 0/0 nodes"


def test_null_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.ETA_K_DTYPE)
    one = np.ones(1, np.int32)
    k = np.ones(1, np.uint16)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_when_k, L.fit_when_k_device):
        assert fn(None, 0, None, None, None, None, None, None, 1, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(k), p(k), 1, p(out), p(one)) == _lib.FIT_E_INVAL
        assert b"null ctx" in L.fit_last_error()
    ms = C.c_double()
    assert L.fit_when_k_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL

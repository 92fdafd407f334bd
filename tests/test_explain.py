"""fit_explain's host half (no device): the exact texts of fit_why_message as include/fitgpu.h fixes
them, argument checks that must answer before any device call, and text checks of the Go binding
and call site (no Go toolchain in the image, as tests/test_go_binding.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fitgpu
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg")


def row(code, need=1, members=0, fit=0, cpu=0, mem=0, gpu=0, time=0):
    return _lib.FitWhy(code, need, members, fit, cpu, mem, gpu, time)


def msg(w, buflen=256):
    buf = C.create_string_buffer(buflen)
    n = _lib.lib().fit_why_message(C.byref(w), buf, buflen)
    return n, buf.value.decode()


FIXED = [
    (fitgpu.FIT_WHY_PARTITION, "unknown partition"),
    (fitgpu.FIT_WHY_LIMIT_TIME, "walltime exceeds the partition's MaxTime"),
    (fitgpu.FIT_WHY_LIMIT_CPUS, "cpus per node exceed the partition's MaxCPUsPerNode"),
    (fitgpu.FIT_WHY_LIMIT_MEM, "memory per node exceeds the partition's MaxMemPerNode"),
    (fitgpu.FIT_WHY_NO_NODES, "no schedulable node in the partition"),
]


def test_codes_are_distinct_and_fits_is_zero():
    codes = [fitgpu.FIT_WHY_FITS, fitgpu.FIT_WHY_PARTITION, fitgpu.FIT_WHY_LIMIT_TIME, fitgpu.FIT_WHY_LIMIT_CPUS,
             fitgpu.FIT_WHY_LIMIT_MEM, fitgpu.FIT_WHY_NO_NODES, fitgpu.FIT_WHY_RESOURCES]
    assert fitgpu.FIT_WHY_FITS == 0 and len(set(codes)) == 7
    hdr = open(HDR).read()
    for name in ("FITS", "PARTITION", "LIMIT_TIME", "LIMIT_CPUS", "LIMIT_MEM", "NO_NODES", "RESOURCES"):
        m = re.search(r"#define FIT_WHY_" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == getattr(fitgpu, "FIT_WHY_" + name), name
    assert C.sizeof(_lib.FitWhy) == 32 and fitgpu.WHY_DTYPE.itemsize == 32
    assert [n for n, _ in _lib.FitWhy._fields_] == list(fitgpu.WHY_DTYPE.names)


@pytest.mark.parametrize("code,text", FIXED)
def test_fixed_texts(code, text):
    # the counters and need play no part in these
    for w in (row(code), row(code, need=4, members=9, fit=3, cpu=1, mem=2, gpu=3, time=4)):
        assert msg(w) == (len(text), text)
    assert fitgpu.why_message({"code": code, "need": 1, "members": 0, "fit": 0, "short_cpu": 0, "short_mem": 0,
                               "short_gpu": 0, "short_time": 0}) == text


def test_resources_text_is_the_header_example():
    w = row(fitgpu.FIT_WHY_RESOURCES, need=2, members=6273, fit=0, cpu=5120, mem=73, gpu=1200, time=40)
    want = ("0/6273 nodes fit now (need 2): 5120 insufficient cpu, 73 insufficient memory, 1200 insufficient gpu, "
            "40 not available for the walltime")
    assert msg(w) == (len(want), want)


def test_zero_terms_are_left_out_and_need_shows_only_above_one():
    R = fitgpu.FIT_WHY_RESOURCES
    assert msg(row(R, 1, 10, 0, cpu=10))[1] == "0/10 nodes fit now: 10 insufficient cpu"
    assert msg(row(R, 0, 10, 0, mem=7))[1] == "0/10 nodes fit now: 7 insufficient memory"
    assert msg(row(R, 1, 10, 0, gpu=3, time=9))[1] == \
        "0/10 nodes fit now: 3 insufficient gpu, 9 not available for the walltime"
    assert msg(row(R, 1, 10, 0, cpu=4, time=6))[1] == \
        "0/10 nodes fit now: 4 insufficient cpu, 6 not available for the walltime"
    # every member fits, there are too few of them: no term, so no colon either
    assert msg(row(R, 8, 3, 3))[1] == "3/3 nodes fit now (need 8)"
    assert msg(row(R, 2, 5, 1, cpu=4))[1] == "1/5 nodes fit now (need 2): 4 insufficient cpu"
    F = fitgpu.FIT_WHY_FITS
    assert msg(row(F, 1, 10, 4, cpu=6))[1] == "4/10 nodes fit now"  # a fitting job lists no shortage
    assert msg(row(F, 2, 10, 4, cpu=6))[1] == "4/10 nodes fit now (need 2)"


def test_buffer_too_small_and_bad_arguments():
    w = row(fitgpu.FIT_WHY_NO_NODES)
    text = "no schedulable node in the partition"
    assert msg(w, len(text) + 1) == (len(text), text)  # the text and its NUL fit exactly
    assert msg(w, len(text))[0] == _lib.FIT_E_INVAL
    assert msg(w, 1)[0] == _lib.FIT_E_INVAL
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    assert L.fit_why_message(None, buf, 64) == _lib.FIT_E_INVAL
    assert L.fit_why_message(C.byref(w), None, 64) == _lib.FIT_E_INVAL
    assert L.fit_why_message(C.byref(w), buf, 0) == _lib.FIT_E_INVAL
    assert msg(row(7))[0] == _lib.FIT_E_INVAL and msg(row(-1))[0] == _lib.FIT_E_INVAL  # no such code
    with pytest.raises(fitgpu.FitError):
        fitgpu.why_message(row(99))


def test_why_message_takes_a_structured_row():
    a = np.zeros(2, fitgpu.WHY_DTYPE)
    a[1] = (fitgpu.FIT_WHY_RESOURCES, 1, 5, 0, 5, 0, 2, 0)
    assert fitgpu.why_message(a[1]) == "0/5 nodes fit now: 5 insufficient cpu, 2 insufficient gpu"
    assert fitgpu.why_message(a[0]) == "0/0 nodes fit now"
    assert fitgpu.why_message(row(fitgpu.FIT_WHY_NO_NODES)) == "no schedulable node in the partition"


def test_null_and_zero_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.WHY_DTYPE)
    one = np.ones(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (L.fit_explain, L.fit_explain_device):
        assert fn(None, 0, None, None, None, None, None, None, None) == _lib.FIT_E_INVAL
        assert fn(None, 1, p(one), p(one), p(one), p(one), p(one), None, p(out)) == _lib.FIT_E_INVAL
    assert L.fit_admitter_explain(None, None, 0, None) == _lib.FIT_E_INVAL
    q = _lib.FitAdmitReq(0, 1, 1, 0, 1, 0, 1)
    assert L.fit_admitter_explain(None, C.byref(q), 1, p(out)) == _lib.FIT_E_INVAL
    assert b"null ctx" in L.fit_last_error() or b"bad arguments" in L.fit_last_error()


# ---- Go binding and call site: text checks ---------------------------------------------------
def _read(*parts):
    with open(os.path.join(GO, *parts)) as fh:
        return fh.read()


def test_go_calls_only_declared_functions_and_binds_the_new_ones():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    srcs = {f: _read("fitgpu", f) for f in sorted(os.listdir(os.path.join(GO, "fitgpu"))) if f.endswith(".go")}
    called = set()
    for text in srcs.values():
        called |= set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", text))
    assert called <= declared, sorted(called - declared)
    assert {"fit_explain", "fit_admitter_explain", "fit_why_message"} <= called
    assert re.search(r"func \(e \*Engine\) Explain\(", srcs["fitgpu.go"])
    assert re.search(r"func \(ad \*Admitter\) Explain\(", srcs["admit.go"])
    assert re.search(r"func WhyMessage\(", srcs["admit.go"])
    # every field of fit_why crosses into the Go row and back into the C row WhyMessage builds
    for f in fitgpu.WHY_DTYPE.names:
        assert re.search(r"\bw\." + f + r"\b", "\n".join(srcs.values())), f"goWhy does not copy {f}"
        assert re.search(r"\b" + f + r":\s*C\.int32_t\(", srcs["admit.go"]), f"WhyMessage does not set {f}"


def test_call_site_keeps_both_texts_and_appends_the_diagnosis():
    src = _read("slurm-virtual-kubelet", "fit_admission.go")
    assert "exceeds the partition's limits" in src
    assert "no Slurm node of the partition fits it now" in src
    assert re.search(r"f\.adm\.Explain\(", src), "the call site does not call Explain"
    assert "fitgpu.WhyMessage(" in src and '": " + ' in src
    # both decisions carry the diagnosis, and a failed diagnosis only logs
    admit = src[src.index("func (f *FitAdmission) admit("):src.index("func (f *FitAdmission) release(")]
    assert admit.count("f.why(pod, ds)") == 2
    why = admit[admit.index("func (f *FitAdmission) why("):]
    assert "klog." in why and 'return ""' in why

"""fit_free_tl's host half (no device): the row's layout against the header's struct, argument checks
that answer before any device call, the exact texts of fit_free_message as include/fitgpu.h fixes
them, the numpy restatement of DESIGN.md §2k on a hand-written case with literal rows, and text
checks of the Go binding (no Go toolchain in the image, as tests/test_go_binding.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fitgpu
import _free_tl_cases as fc
from fitgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fitgpu.h")
GO = os.path.join(ROOT, "slurm-bridge-operator_amd", "pkg", "fitgpu", "fitgpu.go")
FIELDS = ("cpu", "mem", "gpu", "nodes", "max_cpu", "max_mem", "max_gpu")
OFFSETS = (0, 8, 16, 24, 28, 32, 36)


def msg(r, buflen=256):
    buf = C.create_string_buffer(buflen)
    n = _lib.lib().fit_free_message(C.byref(r), buf, buflen)
    return n, buf.value.decode()


# ---- layout --------------------------------------------------------------------------------------
def test_row_is_40_bytes_with_the_sums_first():
    assert C.sizeof(_lib.FitFree) == 40
    assert tuple(n for n, _ in _lib.FitFree._fields_) == FIELDS == fitgpu.FREE_DTYPE.names
    assert tuple(getattr(_lib.FitFree, f).offset for f in FIELDS) == OFFSETS
    assert fitgpu.FREE_DTYPE.itemsize == 40
    assert tuple(fitgpu.FREE_DTYPE.fields[f][1] for f in FIELDS) == OFFSETS
    for sym in ("fit_free_tl", "fit_free_tl_device", "fit_free_tl_ms", "fit_free_message"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
    assert int(re.search(r"#define FITGPU_ABI_VERSION\s+(\d+)", open(HDR).read()).group(1)) == 8


def test_row_layout_is_the_headers_struct(tmp_path):
    """A C translation unit that includes the header prints sizeof and every offset of fit_free."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fitgpu.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(fit_free));\n' +
                   "".join(f'    printf(" %zu", offsetof(fit_free, {f}));\n' for f in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [40, *OFFSETS]


# ---- argument checks that need no device ---------------------------------------------------------
def test_null_arguments_answer_without_a_device():
    L = _lib.lib()
    out = np.zeros(1, fitgpu.FREE_DTYPE)
    assert L.fit_free_tl(None, 1, None) == _lib.FIT_E_INVAL
    assert L.fit_free_tl(None, 1, C.c_void_p(out.ctypes.data)) == _lib.FIT_E_INVAL
    assert L.fit_free_tl_device(None, 1, None) == _lib.FIT_E_INVAL
    ms = C.c_double()
    assert L.fit_free_tl_ms(None, C.byref(ms)) == _lib.FIT_E_INVAL
    assert out.tobytes() == bytes(40)


# ---- the texts -----------------------------------------------------------------------------------
def test_message_texts_byte_for_byte():
    r = _lib.FitFree(2**40 + 3, 5 * (2**31 - 1), 0, 17, 64, 2**31 - 1, 0)
    text = (f"17 nodes open: {2**40 + 3} cpus, {5 * (2**31 - 1)} MiB, 0 gpus free "
            f"(at most 64 cpus, {2**31 - 1} MiB, 0 gpus on one node)")
    assert msg(r) == (len(text), text)
    one = _lib.FitFree(4, 100, 1, 1, 4, 100, 1)
    text1 = "1 nodes open: 4 cpus, 100 MiB, 1 gpus free (at most 4 cpus, 100 MiB, 1 gpus on one node)"
    assert msg(one) == (len(text1), text1)
    none = _lib.FitFree(0, 0, 0, 0, -1, -1, -1)
    assert msg(none) == (12, "no open node")
    # a too-small buffer: the text and its NUL must fit
    assert msg(r, len(text) + 1) == (len(text), text)
    assert msg(r, len(text))[0] == _lib.FIT_E_INVAL
    assert msg(none, 13) == (12, "no open node")
    assert msg(none, 12)[0] == _lib.FIT_E_INVAL
    assert msg(none, 1)[0] == _lib.FIT_E_INVAL
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    assert L.fit_free_message(None, buf, 64) == _lib.FIT_E_INVAL
    assert L.fit_free_message(C.byref(r), None, 64) == _lib.FIT_E_INVAL
    assert L.fit_free_message(C.byref(r), buf, 0) == _lib.FIT_E_INVAL
    # the largest row there can be fits 256 bytes
    big = _lib.FitFree(*([2**63 - 1] * 3), *([2**31 - 1] * 4))
    n, s = msg(big)
    assert 0 < n < 256 and s.startswith(f"{2**31 - 1} nodes open: {2**63 - 1} cpus")


def test_free_message_takes_a_structured_row():
    a = np.zeros(2, fitgpu.FREE_DTYPE)
    a[1] = (12, 3000, 2, 3, 8, 2000, 1)
    assert fitgpu.free_message(a[1]) == ("3 nodes open: 12 cpus, 3000 MiB, 2 gpus free "
                                         "(at most 8 cpus, 2000 MiB, 1 gpus on one node)")
    assert fitgpu.free_message(a[0]) == "no open node"
    assert fitgpu.free_message(dict(zip(FIELDS, (1, 2, 3, 1, 1, 2, 3)))).startswith("1 nodes open: 1 cpus, 2 MiB")


# ---- the restatement on a hand-written case --------------------------------------------------------
def test_restatement_on_the_hand_case():
    tl, mask = fc.hand_case()
    ref = fc.ref_free_tl(tl, mask, 32)
    assert ref.shape == (32, 8) and ref.dtype == fitgpu.FREE_DTYPE
    for p in range(32):
        want = fc.HAND_ROWS.get(p, fc.HAND_ROWS[2])
        assert ref[p].tobytes() == want.tobytes(), (p, ref[p])
    # mask bits >= parts are ignored: the first two partitions are the same rows
    two = fc.ref_free_tl(tl, mask, 2)
    assert two.tobytes() == ref[:2].tobytes()
    # the node in both partitions counts in each; the node in no partition in none
    assert ref["nodes"][0, 0] == 3 and ref["nodes"][1, 0] == 2 and ref["nodes"].sum(axis=0).max() == 6
    assert fc.conditions(ref)[:2] == (29 * 8, 2)
    # no node at all: every row is {0, 0, 0, 0, -1, -1, -1}
    empty = fc.ref_free_tl(np.zeros((0, 8, 3), np.int32), np.zeros(0, np.uint32), 3)
    assert empty.tobytes() == np.broadcast_to(fc.HAND_ROWS[2], (3, 8)).tobytes()


def test_restatement_sums_in_64_bits():
    tl = np.full((5, 2, 3), 2**31 - 1, np.int32)
    tl[:, :, 2] = 0
    ref = fc.ref_free_tl(tl, np.ones(5, np.uint32), 1)
    assert ref["cpu"][0].tolist() == [5 * (2**31 - 1)] * 2 and ref["max_mem"][0].tolist() == [2**31 - 1] * 2


# ---- Go binding: text checks -----------------------------------------------------------------------
GO_FIELD = {"cpu": "CPU", "mem": "Mem", "gpu": "GPU", "nodes": "Nodes", "max_cpu": "MaxCPU", "max_mem": "MaxMem",
            "max_gpu": "MaxGPU"}


def test_go_binds_free_tl_and_every_field_crosses_both_ways():
    declared = set(re.findall(r"\b(fit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    eng = open(GO).read()
    called = set(re.findall(r"\bC\.(fit_[a-z0-9_]+)\s*\(", eng))
    assert called <= declared, sorted(called - declared)
    assert {"fit_free_tl", "fit_free_message"} <= called
    assert re.search(r"type Free struct \{", eng)
    assert re.search(r"func \(e \*Engine\) FreeTL\(parts int\) \(\[\]\[\]Free, error\)", eng)
    assert re.search(r"func FreeMessage\(r Free\) string", eng)
    go_free = eng[eng.index("func goFree("):eng.index("func (e *Engine) FreeTL(")]
    message = eng[eng.index("func FreeMessage("):]
    message = message[:message.index("\n}\n")]
    for c, g in GO_FIELD.items():
        ctype = "int64" if c in ("cpu", "mem", "gpu") else "int32"
        assert re.search(r"\b" + g + r"\s+" + ctype + r"\b", eng), f"Free has no {g} {ctype}"
        assert re.search(r"\b" + g + r":\s*" + ctype + r"\(r\." + c + r"\)", go_free), f"goFree does not copy {c}"
        assert re.search(r"\b" + c + r":\s*C\." + ctype + r"_t\(r\." + g + r"\)", message), f"FreeMessage does not set {c}"


def test_integration_names_the_capacity_call_site():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fit_free_tl" in text and "GetPartitionCapacity" in text
    assert re.search(r"fit_partition_free[^.]*\bignores\b[^.]*reservations", text)

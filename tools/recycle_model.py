"""Driver of tools/recycle_model.c: the CPU round model with the multi-wave commit's recycling of
exhausted dirty rows (diagnostic and test infrastructure).

    python tools/recycle_model.py [c3] [nodes jobs]

prints, for the dirty capacities and retired-list sizes of DESIGN.md §3.7, the rounds of the
longest component, the rescan and dirty-full stops and the rows recycled, each arm checked
bit for bit against the sequential oracle.  The model's parameters are the persistent engine's for
a C3 component (8 waves x 98 nodes per block-slice, 16 keys per slice, 128 candidates per job,
windows 256 .. 8192, next window after a stop = 10 / 8 of the jobs resolved).
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]
from oracle import pyoracle as po  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

KEYS = ["rounds", "scan_evals", "dirty_evals", "stops_rescan", "stops_ucap", "commits", "max_window",
        "placed", "recycled", "rounds_all"]


class Params(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("slice", "ks", "km", "ucap", "wmin", "wmax", "shards", "rcap",
                                         "wgrow8")]


def lib(build_dir=None):
    """tools/librecycle_model.so, compiled on first use (or when the source is newer)."""
    global _LIB
    if _LIB is None:
        src = os.path.join(_HERE, "recycle_model.c")
        path = os.path.join(build_dir or _HERE, "librecycle_model.so")
        if not os.path.exists(path) or os.path.getmtime(src) > os.path.getmtime(path):
            subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-shared", "-fPIC", "-o", path, src])
        _LIB = C.CDLL(path)
    return _LIB


def recycle_place(nodes, jobs, parts, slice=2048, ks=8, km=32, ucap=256, wmin=256, wmax=65536, shards=1,
                  rcap=0, wgrow8=16, build_dir=None):
    """The round model with recycling (k = 1 jobs): (out[J], counters, final (cpu, mem, gpu)).
    rcap = 0 and wgrow8 = 16 are oracle/round_model.c's rules."""
    cf, mf, gf, av, mk, pt, jb, jp, _ = po._prep(nodes, jobs, parts)
    j = jobs.j
    out = np.empty(j, np.int32)
    st = np.zeros(len(KEYS), np.int64)
    prm = Params(slice, ks, km, ucap, wmin, wmax, shards, rcap, wgrow8)
    I32, U32, U16 = C.c_int32, C.c_uint32, C.c_uint16
    p = po._p
    rc = lib(build_dir).recycle_place(
        I32(nodes.n), p(cf, I32), p(mf, I32), p(gf, I32), p(av, I32), p(mk, U32),
        I32(parts.p), p(pt[0], I32), p(pt[1], I32), p(pt[2], I32),
        I32(j), p(jb[0], I32), p(jb[1], I32), p(jb[2], I32), p(jb[3], I32), p(jp, U16),
        C.byref(prm), p(out, I32), p(st, C.c_int64))
    if rc != 0:
        raise ValueError("recycle_place: invalid parameters")
    return out, {k: int(v) for k, v in zip(KEYS, st)}, (cf, mf, gf)


ENGINE = dict(slice=8 * 98, ks=16, km=128, wmin=256, wmax=8192, wgrow8=10)
ARMS = [(128, 0), (64, 0), (128, 64), (128, 1 << 20), (64, 32), (64, 64), (64, 128)]


def main(argv):
    from fitgpu import synth
    name = argv[0] if argv else "c3"
    size = [int(a) for a in argv[1:3]]
    nodes, jobs, parts = synth.make_config(name, *size)
    ref, _, rfin = po.ref_place(nodes, jobs, parts)
    print(f"{name}: {nodes.n} nodes, {jobs.j} jobs")
    print("| dirty capacity | retired rows per round | longest component's rounds | rescans | dirty-full | "
          "rows recycled | exact |")
    print("|---|---|---|---|---|---|---|")
    for ucap, rcap in ARMS:
        t0 = time.time()
        out, st, fin = recycle_place(nodes, jobs, parts, ucap=ucap, rcap=rcap, **ENGINE)
        exact = np.array_equal(out, ref[:, 0]) and all(np.array_equal(a, b) for a, b in zip(fin, rfin))
        r = "–" if rcap == 0 else "unbounded" if rcap >= 1 << 20 else f"≤ {rcap}"
        print(f"| {ucap} | {r} | {st['rounds']} | {st['stops_rescan']} | {st['stops_ucap']} | "
              f"{st['recycled']:,} | {'yes' if exact else 'NO'} |  ({time.time() - t0:.0f} s)", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])

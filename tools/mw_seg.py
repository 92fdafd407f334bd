"""Diagnostic: the decider's per-segment cycles inside the engine (a -DMW_SEGSTAMP variant build,
`make variant V=seg DEFS=-DMW_SEGSTAMP`; dev tool).  Each stamp costs ~40 cycles of its own."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]
from fitgpu import _lib  # noqa: E402
_lib.LIB_PATH = os.path.join(ROOT, "slurm-bridge-operator_amd", "fitgpu",
                             sys.argv[2] if len(sys.argv) > 2 else "libfitgpu_seg.so")
from fitgpu import Engine, synth  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
nodes, jobs, parts = synth.make_array_config(name) if name.endswith("a") else synth.make_config(name)
with Engine() as e:
    e.load_nodes(nodes)
    e.load_partitions(parts)
    out, st = e.place(jobs)
    buf = (C.c_ulonglong * 9)()
    assert _lib.lib().fit_debug_mw_seg(buf) == 0
n = max(buf[8], 1)
print({k: st[k] for k in ("ms_total", "ms_commit", "ms_device", "rounds")})
print(f"{os.path.basename(_lib.LIB_PATH)} {name}: {buf[8]} live jobs, segments (cycles/job, incl. ~40/stamp):",
      [round(buf[i] / n) for i in range(8)], "sum", round(sum(buf[1:8]) / n))

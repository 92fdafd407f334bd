"""fit_explain on the MI355X: the two regimes of DESIGN.md §3.11, one JSON line each, written to
profiles/explain_bench.json (and printed).

  (a) queue tail: fit_explain_device over the jobs config C3 (100k nodes, 1M jobs, 16 partitions)
      leaves unplaced, against the node table its placement left.  Device ms from HIP events on
      the context's stream (fit_explain_ms): one warm-up call, then the median of 5; pairs/s =
      sum over the jobs of their component's rows / time — the evaluations the kernel performs,
      the unit of k_scan's rate.
  (b) admission: fit_admitter_explain of one request on the table one virtual kubelet holds (C3's
      partition 0, 6,273 nodes), on the whole 100k-node table (the request's component is the same
      6,273 rows, so the same launch) and on C3o's table, one component of 100k rows: host clock
      around the call (it ends in a stream synchronisation), p50 / p99 over 2,000 calls after 200 warm-up calls.  The
      call goes through ctypes, which is inside the figure.

    python tools/explain_bench.py [--out profiles/explain_bench.json] [--nodes N --jobs J]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]

SCAN_PAIRS_PER_S = 1.96e11  # k_scan's evaluation rate on C3 (BENCH_r06.json)
ADMIT_FLOOR_US = 31.0       # one admission call's floor


def queue_tail(nodes, jobs, parts):
    import torch

    from fitgpu import FIT_UNPLACED, WHY_DTYPE, Engine
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        out, st = e.place(jobs)
        un = np.flatnonzero(out[:, 0] == FIT_UNPLACED)
        cols = [T(getattr(jobs, f)[un]) for f in ("cpu", "mem", "gpu", "wall")]
        cols += [T(jobs.part[un].view(np.int16)), T(jobs.nodes_k[un].view(np.int16))]
        rows = torch.empty((len(un), 8), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.explain_device(*cols, rows)  # warm-up: code objects, buffers
        ms = sorted(e.explain_device(*cols, rows) for _ in range(5))
        why = rows.cpu().numpy().view(WHY_DTYPE).reshape(-1)
    # rows of each job's component: C3's partitions are disjoint, so the component is the partition
    per_part = np.array([int(((nodes.part_mask >> p) & 1).sum()) for p in range(parts.p)], np.int64)
    pairs = int(per_part[jobs.part[un]].sum())
    med = ms[2]
    return {"what": "fit_explain_device, unplaced jobs of the placement", "nodes": nodes.n, "jobs": jobs.j,
            "unplaced": int(len(un)), "pairs": pairs, "ms_median_of_5": round(med, 4),
            "ms_min": round(ms[0], 4), "ms_max": round(ms[4], 4), "pairs_per_s": round(pairs / (med * 1e-3), 1),
            "yardstick_k_scan_pairs_per_s": SCAN_PAIRS_PER_S,
            "vs_k_scan": round(pairs / (med * 1e-3) / SCAN_PAIRS_PER_S, 3),
            "codes": {str(c): int(n) for c, n in zip(*np.unique(why["code"], return_counts=True))},
            "place_ms": round(st["ms_total"], 3)}


def admission(nodes, parts, label, part=0, calls=2000, warm=200):
    from fitgpu import Admitter, Engine, WHY_DTYPE, _lib
    L = _lib.lib()
    with Engine(device=0) as e:
        e.load_partitions(parts)
        with Admitter(e, max_batch=1024, max_wait_us=0) as a:
            a.load_nodes(nodes)
            # a large request inside every partition limit (5 minutes), so its partition's rows are counted
            q = _lib.FitAdmitReq(0, 64, 64 * 4096, 8, 5, part, 1)
            out = np.zeros(1, WHY_DTYPE)
            po, pq = C.c_void_p(out.ctypes.data), C.byref(q)
            lat = np.empty(calls)
            for i in range(warm + calls):
                t = time.perf_counter_ns()
                rc = L.fit_admitter_explain(a._h, pq, 1, po)
                dt = time.perf_counter_ns() - t
                if rc:
                    raise RuntimeError(f"fit_admitter_explain: {rc}")
                if i >= warm:
                    lat[i - warm] = dt / 1e3
    p50, p99 = (float(np.percentile(lat, p)) for p in (50, 99))
    return {"what": "fit_admitter_explain, one request", "table": label, "nodes": nodes.n,
            "code": int(out["code"][0]), "members": int(out["members"][0]), "calls": calls,
            "p50_us": round(p50, 2), "p99_us": round(p99, 2),
            "yardstick_admit_floor_us": ADMIT_FLOOR_US, "p50_over_floor_us": round(p50 - ADMIT_FLOOR_US, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C3 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import synth
    nodes, jobs, parts = synth.make_config("c3", a.nodes, a.jobs)
    sel = (nodes.part_mask & 1) != 0  # one virtual kubelet: partition 0's nodes, one partition
    n1 = synth.Nodes(*(np.ascontiguousarray(x[sel]) for x in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free,
                                                               nodes.avail_min)),
                     np.ones(int(sel.sum()), np.uint32))
    p1 = synth.Partitions(*(np.ascontiguousarray(x[:1]) for x in (parts.max_time_min, parts.max_cpus_per_node,
                                                                   parts.max_mem_per_node)))
    # c3o: every node also in partition 16, so the table is ONE component of all its rows and a
    # request for partition 16 has its node range split over the whole chip
    no, _, po = synth.make_config("c3o", a.nodes, 1)
    lines = [queue_tail(nodes, jobs, parts), admission(n1, p1, "one partition"),
             admission(nodes, parts, "all 16 partitions"),
             admission(no, po, "overlapping partitions, one component", part=16)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

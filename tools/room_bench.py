"""fit_room on the MI355X next to fit_explain, its yardstick, one JSON line each,
written to profiles/room_bench.json (and printed).

  (a) queue tail: fit_room_device and fit_explain_device, in the same run, over the jobs config C3
      (100k nodes, 1M jobs, 16 partitions) leaves unplaced, against the node table its placement
      left.  Device ms from HIP events on the context's stream (fit_room_ms / fit_explain_ms): one
      warm-up call each, then the median of 5; pairs/s = sum over the jobs of their component's
      rows / time, and the ratio of the two rates.
  (b) admission: fit_admitter_room next to fit_admitter_explain, one request, on the three tables
      of tools/explain_bench.py: host clock around the call (it ends in a stream synchronisation),
      p50 / p99 over 2,000 calls after 200 warm-up calls each.  ctypes is inside the figure.
  (c) the record of the division A/B that chose the kernel's quotient (DIV_AB below; the plain
      `n / d` form is no longer in the source, so the line is a record, not a measurement).

    python tools/room_bench.py [--out profiles/room_bench.json] [--nodes N --jobs J]
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

# k_room_count on the C3 queue tail with each quotient form (device ms, median of 5, one process
# each, same table and jobs as (a))
DIV_AB = {"what": "k_room_count quotient forms, C3 queue tail (recorded when the form was chosen, not re-measured)",
          "pairs": 565055584, "mulhi_fixup_ms_median_of_5": 1.0654, "mulhi_fixup_over_explain_rate": 0.32,
          "plain_division_ms_median_of_5": 1.2023, "plain_division_over_explain_rate": 0.282, "kept": "mulhi_fixup"}


def queue_tail(nodes, jobs, parts):
    import torch

    from fitgpu import FIT_UNPLACED, ROOM_DTYPE, WHY_DTYPE, Engine
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        out, st = e.place(jobs)
        un = np.flatnonzero(out[:, 0] == FIT_UNPLACED)
        cols = [T(getattr(jobs, f)[un]) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part[un].view(np.int16))]
        ones = T(np.ones(len(un), np.int16))
        rows = torch.empty((len(un), 5), dtype=torch.int64, device=dev)  # 40-byte rows, 8-byte aligned
        wrows = torch.empty((len(un), 8), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.room_device(*cols, rows)  # warm-up: code objects, buffers
        e.explain_device(*cols, ones, wrows)
        ms = sorted(e.room_device(*cols, rows) for _ in range(5))
        xms = sorted(e.explain_device(*cols, ones, wrows) for _ in range(5))
        room = rows.cpu().numpy().view(ROOM_DTYPE).reshape(-1)
        why = wrows.cpu().numpy().view(WHY_DTYPE).reshape(-1)
    if not (np.array_equal(room["members"], why["members"]) and np.array_equal(room["nodes"], why["fit"])):
        raise RuntimeError("fit_room and fit_explain disagree on members / nodes")
    # rows of each job's component: C3's partitions are disjoint, so the component is the partition
    per_part = np.array([int(((nodes.part_mask >> p) & 1).sum()) for p in range(parts.p)], np.int64)
    pairs = int(per_part[jobs.part[un]].sum())
    rate, xrate = pairs / (ms[2] * 1e-3), pairs / (xms[2] * 1e-3)
    return {"what": "fit_room_device next to fit_explain_device, unplaced jobs of the placement", "nodes": nodes.n,
            "jobs": jobs.j, "unplaced": int(len(un)), "pairs": pairs, "room_ms_median_of_5": round(ms[2], 4),
            "room_ms_min": round(ms[0], 4), "room_ms_max": round(ms[4], 4), "room_pairs_per_s": round(rate, 1),
            "explain_ms_median_of_5": round(xms[2], 4), "explain_ms_min": round(xms[0], 4),
            "explain_ms_max": round(xms[4], 4), "explain_pairs_per_s": round(xrate, 1),
            "room_over_explain_rate": round(rate / xrate, 3),
            "codes": {str(c): int(n) for c, n in zip(*np.unique(room["code"], return_counts=True))},
            "copies_sum": int(room["copies"].sum()), "place_ms": round(st["ms_total"], 3)}


def admission(nodes, parts, label, part=0, calls=2000, warm=200):
    from fitgpu import ROOM_DTYPE, WHY_DTYPE, Admitter, Engine, _lib
    L = _lib.lib()
    with Engine(device=0) as e:
        e.load_partitions(parts)
        with Admitter(e, max_batch=1024, max_wait_us=0) as a:
            a.load_nodes(nodes)
            # a small request inside every partition limit (5 minutes): its partition's rows all divide
            q = _lib.FitAdmitReq(0, 2, 2 * 1024, 1, 5, part, 1)
            pq = C.byref(q)
            res = {}
            for name, fn, dt_ in (("room", L.fit_admitter_room, ROOM_DTYPE), ("explain", L.fit_admitter_explain, WHY_DTYPE)):
                out = np.zeros(1, dt_)
                po = C.c_void_p(out.ctypes.data)
                lat = np.empty(calls)
                for i in range(warm + calls):
                    t = time.perf_counter_ns()
                    rc = fn(a._h, pq, 1, po)
                    dt = time.perf_counter_ns() - t
                    if rc:
                        raise RuntimeError(f"fit_admitter_{name}: {rc}")
                    if i >= warm:
                        lat[i - warm] = dt / 1e3
                res[name] = (out, [float(np.percentile(lat, p)) for p in (50, 99)])
    room, (r50, r99) = res["room"]
    _, (x50, x99) = res["explain"]
    return {"what": "fit_admitter_room next to fit_admitter_explain, one request", "table": label, "nodes": nodes.n,
            "code": int(room["code"][0]), "members": int(room["members"][0]), "copies": int(room["copies"][0]),
            "calls": calls, "room_p50_us": round(r50, 2), "room_p99_us": round(r99, 2), "explain_p50_us": round(x50, 2),
            "explain_p99_us": round(x99, 2), "room_minus_explain_p50_us": round(r50 - x50, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "room_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C3 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=None)
    ap.add_argument("--tail-only", action="store_true", help="only (a)")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import synth
    nodes, jobs, parts = synth.make_config("c3", a.nodes, a.jobs)
    lines = [queue_tail(nodes, jobs, parts)]
    if not a.tail_only:
        sel = (nodes.part_mask & 1) != 0  # one virtual kubelet: partition 0's nodes, one partition
        n1 = synth.Nodes(*(np.ascontiguousarray(x[sel]) for x in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free,
                                                                   nodes.avail_min)),
                         np.ones(int(sel.sum()), np.uint32))
        p1 = synth.Partitions(*(np.ascontiguousarray(x[:1]) for x in (parts.max_time_min, parts.max_cpus_per_node,
                                                                       parts.max_mem_per_node)))
        # c3o: every node also in partition 16, so the table is ONE component of all its rows
        no, _, po = synth.make_config("c3o", a.nodes, 1)
        lines += [admission(n1, p1, "one partition"), admission(nodes, parts, "all 16 partitions"),
                  admission(no, po, "overlapping partitions, one component", part=16)]
        if DIV_AB:
            lines.append(DIV_AB)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

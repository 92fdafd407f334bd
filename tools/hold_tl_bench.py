"""fit_hold_tl on the MI355X: one JSON line per batch, written to
profiles/hold_tl_bench.json (and printed).

Config C5 as tools/unplace_tl_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min),
and its state S: fit_place_tl_k of the first 16,384 jobs with nodes_k drawn as config C4 draws it
(kmax 8).  The records are that placement's outputs.  Two routes put records back after a reload, each
timed from the freshly loaded timeline: one warm-up, then the median of 5 with min and max.
  route (a), the one being replaced: fit_load_timeline_device (host clock around the call, which ends in
             a stream synchronisation) plus fit_place_tl_k_device of the surviving rows (stats.ms_device)
  route (b), the new one: fit_load_timeline_device plus fit_hold_tl_device of the same records
             (fit_hold_tl_ms, HIP events on the context's stream)
  (all) every row, the placement's outputs verbatim (unplaced and rejected rows included)
  (1k)  the queue prefix that holds the first 1,024 placed rows        (one) ... the first placed row
A prefix of the queue is placed exactly as it was, so both routes must end in the same read_timeline():
asserted, as is that no record is refused.

    python tools/hold_tl_bench.py [--out profiles/hold_tl_bench.json] [--nodes N] [--only all|1k|one]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]
KMAX = 8
FIELDS = ("cpu", "mem", "gpu", "wall")


def stat3(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hold_tl_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--only", choices=["all", "1k", "one"], default=None, help="one batch (for a kernel trace)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    dev = "cuda:0"
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    from fitgpu import FIT_HOLD_HELD, Engine, synth
    nodes, tline, jobs, parts = synth.make_c5(a.nodes, a.jobs)
    jobs = synth.gen_jobs(synth.SEEDS["c5"], a.jobs, parts.p, multi_node=True)
    J, H, L = jobs.j, int(tline.slots), int(tline.slot_min)
    dtl = [T(x) for x in (tline.off, tline.slot, tline.cpu, tline.mem, tline.gpu)]
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)

        def reload():
            t0 = time.perf_counter()
            e.load_timeline_device(H, L, *dtl)
            return (time.perf_counter() - t0) * 1e3

        def dev_jobs(rows):
            cols = [T(getattr(jobs, f)[rows]) for f in FIELDS]
            return cols, T(jobs.part[rows].view(np.int16)), T(jobs.nodes_k[rows].view(np.int16))

        def place(rows):
            """fit_place_tl_k_device of the rows on the current timeline: (nodes, start, device ms)."""
            cols, part, nk = dev_jobs(rows)
            on = torch.empty((len(rows), KMAX), dtype=torch.int32, device=dev)
            os_ = torch.empty(len(rows), dtype=torch.int32, device=dev)
            st = e.place_tl_k_device(*cols, part, nk, on, os_, KMAX)
            return on, os_, st["ms_device"]

        every = np.arange(J)
        reload()
        d_node, d_start, _ = place(every)
        node, start = d_node.cpu().numpy(), d_start.cpu().numpy()
        placed = np.flatnonzero(start >= 0)

        def bench(what, rows):
            """rows: a prefix of the queue; its records are node[rows], start[rows]."""
            cols, _, nk = dev_jobs(rows)
            rec_node, rec_start = T(node[rows]), T(start[rows])
            state = torch.empty(len(rows), dtype=torch.int32, device=dev)
            ra, pa, rb, hb = [], [], [], []
            applied = refused = 0
            for _ in range(a.reps + 1):  # the first is the warm-up
                ra.append(reload())
                pa.append(place(rows)[2])
            want = e.read_timeline()
            for _ in range(a.reps + 1):
                rb.append(reload())
                applied, refused = e.hold_tl_device(*cols, nk, rec_node, rec_start, state, KMAX)
                hb.append(e.hold_tl_ms())
            assert np.array_equal(want, e.read_timeline()), "the two routes end in different timelines"
            st = state.cpu().numpy()
            assert refused == 0 and np.array_equal(st == FIT_HOLD_HELD, start[rows] >= 0), "a record was refused"
            A, P, B, Hm = stat3(ra[1:]), stat3(pa[1:]), stat3(rb[1:]), stat3(hb[1:])
            line = {"what": what, "rows": int(len(rows)), "held_rows": int((st == FIT_HOLD_HELD).sum()),
                    "windows": int(applied),
                    "hold_tl_ms_median_of_%d" % a.reps: Hm[0], "hold_tl_ms_min": Hm[1], "hold_tl_ms_max": Hm[2],
                    "place_tl_k_ms_median": P[0], "place_tl_k_ms_min": P[1], "place_tl_k_ms_max": P[2],
                    "reload_a_ms_median": A[0], "reload_a_ms_min": A[1], "reload_a_ms_max": A[2],
                    "reload_b_ms_median": B[0], "reload_b_ms_min": B[1], "reload_b_ms_max": B[2],
                    "route_a_ms": round(A[0] + P[0], 4), "route_b_ms": round(B[0] + Hm[0], 4),
                    "hold_over_place": round(Hm[0] / P[0], 5) if P[0] else None,
                    "same_timeline": True, "nodes": nodes.n, "slots": H, "queue": J,
                    "placed_in_S": int(len(placed))}
            lines.append(line)
            print(json.dumps(line), flush=True)

        def prefix(k):
            """The queue prefix that ends with the k-th placed row."""
            return np.arange(int(placed[k - 1]) + 1)

        if a.only in (None, "all"):
            bench("(all) every row, the placement's outputs verbatim", every)
        if a.only in (None, "1k"):
            bench("(1k) the prefix with the first 1,024 placed rows", prefix(min(1024, len(placed))))
        if a.only in (None, "one"):
            bench("(one) the prefix with the first placed row", prefix(1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

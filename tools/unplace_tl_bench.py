"""fit_unplace_tl on the MI355X: one JSON line per batch, written to
profiles/unplace_tl_bench.json (and printed).

Config C5 as tools/place_tl_k_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min),
after fit_place_tl_k of its first 16,384 jobs with nodes_k drawn as config C4 draws it (kmax 8): the
state S.  Every timed call starts from S, rebuilt by a reload and the placement.  Device ms is
fit_unplace_tl_ms (HIP events on the context's stream): one warm-up call, then the median of 5 with
min and max.
  (a) the last placed row of the queue            (b) the last 1,024 placed rows
  (c) all rows, the placement's outputs verbatim (rejected rows included)
  (d) 16,384 one-node rows that all name one node of S, never reserved: the most windows a launch
      sequence can give one wave.  Checked against the numpy restatement of §2h on that node's row.
The yardstick is what a caller had to do before to reach the same state: fit_load_timeline_device of
the same release events (host clock around the call, which ends in a stream synchronisation) plus
fit_place_tl_k_device of the surviving rows (stats.ms_device), timed the same way in the same run.
(a)-(c) hand back a suffix of the queue, so the surviving prefix is placed exactly as before and both
routes must end in the same read_timeline(): asserted.  (d)'s state cannot be reached by a placement;
its yardstick is the rebuild of S.

    python tools/unplace_tl_bench.py [--out profiles/unplace_tl_bench.json] [--nodes N] [--only a|b|c|d]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unplace_tl_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--only", choices=["a", "b", "c", "d"], default=None, help="one batch (for a kernel trace)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    dev = "cuda:0"
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    from fitgpu import Engine, synth
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
        S = e.read_timeline()
        placed = np.flatnonzero(start >= 0)

        def to_S():
            reload()
            place(every)

        def bench(what, rows, un_node, un_start, un_jobs, survivors):
            """un_*: device columns of the call; survivors: the queue prefix the yardstick places (None:
            (d), the yardstick is the rebuild of S)."""
            cols, nk = un_jobs
            ms, applied = [], 0
            for _ in range(a.reps + 1):  # the first is the warm-up
                to_S()
                applied = e.unplace_tl_device(*cols, nk, un_node, un_start, KMAX)
                ms.append(e.unplace_tl_ms())
            after = e.read_timeline()
            rl, pl = [], []
            again = every if survivors is None else survivors
            for _ in range(a.reps + 1):
                rl.append(reload())
                pl.append(place(again)[2] if len(again) else 0.0)
            if survivors is not None:
                assert np.array_equal(after, e.read_timeline()), "the two routes end in different timelines"
            m, r, p = stat3(ms[1:]), stat3(rl[1:]), stat3(pl[1:])
            line = {"what": what, "rows": int(rows), "windows": int(applied),
                    "unplace_tl_ms_median_of_%d" % a.reps: m[0], "unplace_tl_ms_min": m[1], "unplace_tl_ms_max": m[2],
                    "reload_ms_median": r[0], "reload_ms_min": r[1], "reload_ms_max": r[2],
                    "replace_ms_median": p[0], "replace_ms_min": p[1], "replace_ms_max": p[2],
                    "replaced_rows": int(J if survivors is None else len(survivors)),
                    "ratio_to_reload": round(m[0] / r[0], 5), "ratio_to_reload_plus_replace": round(m[0] / (r[0] + p[0]), 5),
                    "same_timeline_as_yardstick": survivors is not None,
                    "nodes": nodes.n, "slots": H, "queue": J, "placed_in_S": int(len(placed))}
            lines.append(line)
            print(json.dumps(line), flush=True)
            return after

        def suffix(k):
            """The last k placed rows: the rows handed back and the surviving queue prefix."""
            cut = int(placed[-k])
            rows = np.arange(cut, J)
            cols, _, nk = dev_jobs(rows)
            return len(rows), T(node[rows]), T(start[rows]), (cols, nk), np.arange(cut)

        if a.only in (None, "a"):
            bench("(a) the last placed row", *suffix(1))
        if a.only in (None, "b"):
            bench("(b) the last 1,024 placed rows", *suffix(min(1024, len(placed))))
        if a.only in (None, "c"):
            cols, _, nk = dev_jobs(every)
            # no row survives: the yardstick is the reload alone
            bench("(c) all rows, the placement's outputs verbatim", J, d_node, d_start, (cols, nk), np.arange(0))
        if a.only in (None, "d"):
            r = np.random.default_rng(4)
            x = int(node[placed[0], 0])
            W = 16384
            dj = synth.Jobs(r.integers(0, 3, W).astype(np.int32), r.integers(0, 64, W).astype(np.int32),
                            np.zeros(W, np.int32), r.integers(0, H * L // 2, W).astype(np.int32),
                            np.zeros(W, np.uint16), np.ones(W, np.uint16))
            dn = np.full((W, KMAX), -1, np.int32)
            dn[:, 0] = x
            ds = r.integers(0, H, W).astype(np.int32)
            after = bench("(d) 16,384 windows on one node", W, T(dn), T(ds),
                          ([T(getattr(dj, f)) for f in FIELDS], T(dj.nodes_k.view(np.int16))), None)
            want = S[x].astype(np.int64)
            for q in range(W):
                d = max(1, -(-int(dj.wall[q]) // L))
                v = want[ds[q]:ds[q] + d]
                want[ds[q]:ds[q] + d] = np.where(v == -1, -1, np.minimum(v + [dj.cpu[q], dj.mem[q], 0], 2**31 - 1))
            assert np.array_equal(after[x], want), "(d) differs from the restatement of §2h"
            assert np.array_equal(after[:x], S[:x]) and np.array_equal(after[x + 1:], S[x + 1:]), "(d) changed another node"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

"""fit_when on the MI355X: one JSON line per batch, written to
profiles/when_bench.json (and printed).

Config C5 (100k nodes, 1M jobs, 16 partitions, 1,024 slots of 5 min) after one full place_tl, so
that the run lists carry the reservations of a placed queue.  Then fit_when_device over
  (a) the jobs the placement left unplaced (the queue tail a virtual kubelet would annotate), and
  (b) a 1,024-job batch: the next 1,024 arrivals of the same stream,
and, for the walk's rate when the launches are not the cost, (c) the whole queue once more.
Device ms from HIP events on the context's stream (fit_when_ms): one warm-up call, then the median
of 5.  pairs = sum over the jobs that reach the walk (codes 1-4 end in the classify launch) of
their component's nodes — the (job, node) evaluations the kernel performs; C5's partitions are
disjoint, so the component is the partition.

The yardstick is the backfill engine's scan, the same walk with candidate lists and cuts, from the
parent commit's profiles/r06z_c5_bench.json: fit_evals_per_s.performed x ms_per_step evaluations
per step over kernels.k_engine_tl.scan_worker_busy_ms.

    python tools/when_bench.py [--out profiles/when_bench.json] [--nodes N --jobs J]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]

# 53,880,311,687 evals/s x 118.598 ms = 6.390e9 evaluations per step, in 86.277 ms of scan-worker time
SCAN_TL_PAIRS_PER_S = 53880311687.0 * 118.598e-3 / 86.277e-3


def measure(e, what, jobs, per_part):
    import torch

    from fitgpu import ETA_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part.view(np.int16))]
    rows = torch.empty((jobs.j, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.when_device(*cols, rows)  # warm-up: code objects, buffers
    ms = sorted(e.when_device(*cols, rows) for _ in range(5))
    eta = rows.cpu().numpy().view(ETA_DTYPE).reshape(-1)
    walked = ~np.isin(eta["code"], (1, 2, 3, 4))
    pairs = int(per_part[jobs.part[walked]].sum())
    med = ms[2]
    rate = pairs / (med * 1e-3)
    return {"what": what, "jobs": jobs.j, "walked": int(walked.sum()), "pairs": pairs,
            "ms_median_of_5": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[4], 4),
            "pairs_per_s": round(rate, 1), "yardstick_scan_tl_pairs_per_s": round(SCAN_TL_PAIRS_PER_S, 1),
            "vs_scan_tl": round(rate / SCAN_TL_PAIRS_PER_S, 3),
            "codes": {str(c): int(n) for c, n in zip(*np.unique(eta["code"], return_counts=True))},
            "hosts_over_members": round(float(eta["hosts"][walked].sum()) / max(int(eta["members"][walked].sum()), 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "when_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import FIT_UNPLACED, Engine, synth
    nodes, tline, jobs, parts = synth.make_c5(a.nodes, a.jobs)
    per_part = np.zeros(65536, np.int64)  # indexed by any uint16 partition a job may name
    per_part[:parts.p] = [int(((nodes.part_mask >> p) & 1).sum()) for p in range(parts.p)]
    nxt = synth.gen_jobs(synth.SEEDS["c5"], 1024, parts.p, start=jobs.j)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        node, _, st = e.place_tl(jobs)
        un = np.flatnonzero(node == FIT_UNPLACED)
        tail = synth.Jobs(*(np.ascontiguousarray(getattr(jobs, f)[un]) for f in ("cpu", "mem", "gpu", "wall", "part",
                                                                                  "nodes_k")))
        lines = [measure(e, "fit_when_device, unplaced jobs of the placement", tail, per_part)] if tail.j else []
        lines.append(measure(e, "fit_when_device, the next 1,024 arrivals", nxt, per_part))
        # beyond the two batches a caller sends: the whole queue, enough work to show the walk's rate
        lines.append(measure(e, "fit_when_device, the whole queue again", jobs, per_part))
    for ln in lines:
        ln.update(nodes=nodes.n, queue=jobs.j, slots=int(tline.slots), placed=int(st["placed"]),
                  place_ms=round(st["ms_total"], 3))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

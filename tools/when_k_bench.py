"""fit_when_k on the MI355X: one JSON line per batch, written to
profiles/when_k_bench.json (and printed).

Config C5 (100k nodes, 1M jobs, 16 partitions, 1,024 slots of 5 min) after one full place_tl, as
tools/when_bench.py, so that the run lists carry the reservations of a placed queue.  Then
fit_when_k_device over
  (a) the next 1,024 arrivals of the same stream with nodes_k = 1,
  (b) the same arrivals with nodes_k drawn as config C4 draws it (1, 2, 4 or 8; kmax 8), and
  (c) one 16,384-job chunk, the next 16,384 arrivals with C4's nodes_k.
Device ms from HIP events on the context's stream (fit_when_k_ms): one warm-up call, then the median
of 5.  The yardstick is fit_when_device on the same jobs in the same run (fit_when_ms): it leaves a
node at its first window and passes over the nodes once; fit_when_k walks every run, passes over
the nodes twice and keeps a difference array per job.  ratio = fit_when_k ms / fit_when ms.

    python tools/when_k_bench.py [--out profiles/when_k_bench.json] [--nodes N --jobs J] [--only a|b|c]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]


def measure(e, what, jobs, kmax, per_part):
    import torch

    from fitgpu import ETA_DTYPE, ETA_K_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part.view(np.int16))]
    nk = T(jobs.nodes_k.view(np.int16))
    rows = torch.empty((jobs.j, 10), dtype=torch.int32, device=dev)
    out_node = torch.empty((jobs.j, kmax), dtype=torch.int32, device=dev)
    eta = torch.empty((jobs.j, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.when_k_device(*cols, nk, rows, out_node, kmax)  # warm-up: code objects, buffers
    ms = sorted(e.when_k_device(*cols, nk, rows, out_node, kmax) for _ in range(5))
    e.when_device(*cols, eta)
    ref = sorted(e.when_device(*cols, eta) for _ in range(5))
    r = rows.cpu().numpy().view(ETA_K_DTYPE).reshape(-1)
    w = eta.cpu().numpy().view(ETA_DTYPE).reshape(-1)
    walked = ~np.isin(r["code"], (1, 2, 3, 4))
    pairs = int(per_part[jobs.part[walked]].sum())
    if int(jobs.nodes_k.max()) <= 1:  # need == 1 is fit_when (§2f)
        assert all(np.array_equal(r[f], w[f]) for f in ("code", "start", "wait_min", "members", "hosts", "now"))
        assert np.array_equal(out_node.cpu().numpy()[:, 0], w["node"])
    return {"what": what, "jobs": jobs.j, "kmax": kmax, "walked": int(walked.sum()), "pairs": pairs,
            "nodes_k": {str(k): int(n) for k, n in zip(*np.unique(jobs.nodes_k, return_counts=True))},
            "when_k_ms_median_of_5": round(ms[2], 4), "when_k_ms_min": round(ms[0], 4), "when_k_ms_max": round(ms[4], 4),
            "when_ms_median_of_5": round(ref[2], 4), "when_ms_min": round(ref[0], 4), "when_ms_max": round(ref[4], 4),
            "ratio": round(ms[2] / ref[2], 3), "ratio_low": round(ms[0] / ref[4], 3), "ratio_high": round(ms[4] / ref[0], 3),
            "pairs_per_s": round(pairs / (ms[2] * 1e-3), 1),
            "codes": {str(c): int(n) for c, n in zip(*np.unique(r["code"], return_counts=True))},
            "later_multi": int(((r["code"] == 6) & (r["need"] > 1)).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "when_k_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=None)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None, help="one batch (for a kernel trace)")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import Engine, synth
    nodes, tline, jobs, parts = synth.make_c5(a.nodes, a.jobs)
    per_part = np.zeros(65536, np.int64)  # indexed by any uint16 partition a job may name
    per_part[:parts.p] = [int(((nodes.part_mask >> p) & 1).sum()) for p in range(parts.p)]
    seed = synth.SEEDS["c5"]
    one = synth.gen_jobs(seed, 1024, parts.p, start=jobs.j)
    wide = synth.gen_jobs(seed, 1024, parts.p, multi_node=True, start=jobs.j)
    chunk = synth.gen_jobs(seed, 16384, parts.p, multi_node=True, start=jobs.j)
    batches = {"a": ("fit_when_k_device, the next 1,024 arrivals, nodes_k = 1", one, 1),
               "b": ("fit_when_k_device, the next 1,024 arrivals, nodes_k as C4", wide, 8),
               "c": ("fit_when_k_device, a 16,384-job chunk, nodes_k as C4", chunk, 8)}
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        _, _, st = e.place_tl(jobs)
        lines = [measure(e, *batches[k], per_part) for k in batches if a.only in (None, k)]
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

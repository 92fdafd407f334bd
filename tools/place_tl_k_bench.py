"""fit_place_tl_k on the MI355X: one JSON line per batch, written to
profiles/place_tl_k_bench.json (and printed).

Config C5 as tools/when_k_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min), a
fresh load_timeline before every timed call.  Device ms is stats.ms_device (HIP events on the
context's stream): one warm-up call, then the median of 5 with min and max.
  (1) the first 16,384 jobs of C5's queue with nodes_k = 1.  The yardstick is fit_place_tl_device
      on the same jobs in the same run; ratio = fit_place_tl_k ms / fit_place_tl ms.  The results
      must be equal (§2g).  us_per_job_longest = ms / the longest component job list: the
      components' workgroups run side by side, so the launch lasts as long as its slowest.
  (2) the same jobs with nodes_k drawn as config C4 draws it (1, 2, 4 or 8; kmax 8); ratio_to_1.
  (3) 1,024 jobs (nodes_k as C4) on a single-component table: C3o's partition layout — every node
      also in an all-nodes partition 16 that 10 % of the jobs name — with C5's timeline.  The known
      weak case: one workgroup walks all 100k nodes per job.  It has no yardstick.

    python tools/place_tl_k_bench.py [--out profiles/place_tl_k_bench.json] [--nodes N] [--only 1|2|3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]


def stat3(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)


def measure(e, what, tline, jobs, kmax, yardstick):
    import torch
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part.view(np.int16))]
    nk = T(jobs.nodes_k.view(np.int16))
    out_node = torch.empty((jobs.j, kmax), dtype=torch.int32, device=dev)
    out_start = torch.empty(jobs.j, dtype=torch.int32, device=dev)
    node1 = torch.empty(jobs.j, dtype=torch.int32, device=dev)
    start1 = torch.empty(jobs.j, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def run_k():
        e.load_timeline(tline)
        return e.place_tl_k_device(*cols, nk, out_node, out_start, kmax)

    def run_1():
        e.load_timeline(tline)
        return e.place_tl_device(*cols, node1, start1)

    run_k()  # warm-up: code objects, buffers
    sts = [run_k() for _ in range(5)]
    st = sts[-1]
    ms = stat3([s["ms_device"] for s in sts])
    nodes_h, start_h = out_node.cpu().numpy(), out_start.cpu().numpy()
    live = nodes_h[:, 0] != -2
    longest = int(np.bincount(jobs.part[live], minlength=1).max()) if st["components"] > 1 else int(live.sum())
    line = {"what": what, "jobs": jobs.j, "kmax": kmax, "components": st["components"],
            "nodes_k": {str(k): int(n) for k, n in zip(*np.unique(jobs.nodes_k, return_counts=True))},
            "placed": st["placed"], "unplaced": st["unplaced"], "rejected": st["rejected"],
            "in_the_future": int((start_h > 0).sum()),
            "place_tl_k_ms_median_of_5": ms[0], "place_tl_k_ms_min": ms[1], "place_tl_k_ms_max": ms[2],
            "host_ms_total_median_of_5": stat3([s["ms_total"] for s in sts])[0],
            "longest_component_jobs": longest, "us_per_job_longest": round(ms[0] * 1e3 / max(longest, 1), 2)}
    if yardstick:
        run_1()
        ref = [run_1() for _ in range(5)]
        rm = stat3([s["ms_device"] for s in ref])
        assert np.array_equal(node1.cpu().numpy(), nodes_h[:, 0]) and np.array_equal(start1.cpu().numpy(), start_h)
        line.update({"place_tl_ms_median_of_5": rm[0], "place_tl_ms_min": rm[1], "place_tl_ms_max": rm[2],
                     "place_tl_engine": ref[-1]["engine"], "ratio": round(ms[0] / rm[0], 3),
                     "ratio_low": round(ms[1] / rm[2], 3), "ratio_high": round(ms[2] / rm[1], 3)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_tl_k_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--only", choices=["1", "2", "3"], default=None, help="one batch (for a kernel trace)")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import Engine, synth
    nodes, tline, jobs, parts = synth.make_c5(a.nodes, 16384)
    seed = synth.SEEDS["c5"]
    wide = synth.gen_jobs(seed, 16384, parts.p, multi_node=True)
    assert all(np.array_equal(getattr(wide, f), getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part"))
    # (3): every node also in partition 16, which 10 % of the first 1,024 jobs name
    one_nodes = synth.Nodes(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min,
                            nodes.part_mask | np.uint32(1 << parts.p))
    one_parts = synth.gen_partitions(seed, parts.p + 1)
    few = synth.Jobs(*(getattr(wide, f)[:1024].copy() for f in ("cpu", "mem", "gpu", "wall", "part", "nodes_k")))
    few.part[np.random.default_rng(16).random(1024) < 0.10] = parts.p
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        if a.only in (None, "1"):
            lines.append(measure(e, "fit_place_tl_k_device, C5's first 16,384 jobs, nodes_k = 1", tline, jobs, 1, True))
        if a.only in (None, "2"):
            lines.append(measure(e, "fit_place_tl_k_device, the same jobs, nodes_k as C4", tline, wide, 8, False))
            if lines[0]["kmax"] == 1:
                lines[-1]["ratio_to_1"] = round(lines[-1]["place_tl_k_ms_median_of_5"] /
                                                lines[0]["place_tl_k_ms_median_of_5"], 3)
        if a.only in (None, "3"):
            e.load_nodes(one_nodes)
            e.load_partitions(one_parts)
            lines.append(measure(e, "fit_place_tl_k_device, 1,024 jobs on a single-component table (no yardstick)",
                                 tline, few, 8, False))
    for ln in lines:
        ln.update(nodes=nodes.n, slots=int(tline.slots))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

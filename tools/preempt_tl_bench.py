"""fit_preempt_tl on the MI355X next to fit_when, its yardstick, one JSON line per
batch size, written to profiles/preempt_tl_bench.json (and printed).

The table is tools/preempt_bench.py's: config C3's 100k nodes packed with victims
(synth.pack_victims).  The victims get ends over a horizon of 1,024 slots of 5 minutes
(synth.gen_victim_ends), the timeline is loaded from their release events, and a queue of C5's jobs
is placed with place_tl, so that the timeline carries reservations.  The batches are the first 1,024
and 16,384 jobs of C3's stream with priorities from synth.gen_job_prio.  fit_when walks the same run
lists for the same batch and stops a lane at its first window; fit_preempt_tl reads only the window
[0, d) but comes back to it with the victims, so the result is a ratio against that kernel, not a gate.

  preempt_tl_ms / when_ms   device ms from HIP events on the context's stream (fit_preempt_tl_ms /
                            fit_when_ms): one warm-up call each, then the median of 5, same batch,
                            same timeline, same process
  per (job, member node) pair, counted in numpy over a sample of jobs x a sample of nodes by
  replaying a lane's three visits on the dense timeline (read_timeline()):
  runs_window               runs that meet [0, d): the first visit
  short                     pairs that are eligible and short: the second visit takes place
  runs_short                runs of the second visit on which the lane is short
  entries_cover             victim entries a lane reads on them until its prefix covers the run (or
                            the list ends)
  entries_score             entries of the third visit: runs_window x v, for a pair that can be freed

    python tools/preempt_tl_bench.py [--out profiles/preempt_tl_bench.json] [--nodes N] [--queue Q]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]

H, SLOT_MIN = 1024, 5


def replay(T, mask, vt, parts, jobs, prio, jsample, nsample):
    """The counts of the docstring over jsample x nsample: a lane's visits, slot runs taken from the
    dense rows T[nsample]."""
    tot = dict(pairs=0, runs_window=0, short=0, runs_short=0, entries_cover=0, entries_score=0, able=0)
    runs = []
    for x in nsample:  # the node's runs: (start, end, values)
        row = T[x]
        cut = np.flatnonzero((np.diff(row, axis=0) != 0).any(axis=1)) + 1
        b = np.concatenate([[0], cut, [len(row)]])
        runs.append([(int(b[i]), int(b[i + 1]), row[b[i]].astype(np.int64)) for i in range(len(b) - 1)])
    for q in jsample:
        p, w = int(jobs.part[q]), int(jobs.wall[q])
        dem = np.array([jobs.cpu[q], jobs.mem[q], jobs.gpu[q]], np.int64)
        if p >= parts.p or (0 <= parts.max_time_min[p] < w or 0 <= parts.max_cpus_per_node[p] < dem[0] or
                            0 <= parts.max_mem_per_node[p] < dem[1]):
            continue
        d = max(1, -(-w // SLOT_MIN))
        for x, rl in zip(nsample, runs):
            if not (int(mask[x]) >> p) & 1:
                continue
            tot["pairs"] += 1
            if d > H:
                continue
            win = [r for r in rl if r[0] < d]
            tot["runs_window"] += len(win)
            if any((r[2] < 0).any() for r in win):
                continue
            shorts = [r for r in win if (r[2] < dem).any()]
            a, b = int(vt.off[x]), int(vt.off[x + 1])
            if not shorts or b <= a:
                continue
            tot["short"] += 1
            tot["runs_short"] += len(shorts)
            amt = np.stack([vt.cpu[a:b], vt.mem[a:b], vt.gpu[a:b]], axis=1).astype(np.int64)
            v, dead = 0, False
            for s, e, val in shorts:
                stop = min(e, d)
                cum = np.cumsum(amt * (vt.end[a:b] >= stop)[:, None], axis=0)
                ok = ((val + cum) >= dem).all(axis=1) & (vt.end[a:b] >= stop)
                vr = int(ok.argmax()) + 1 if ok.any() else 0
                tot["entries_cover"] += vr if vr else b - a
                dead |= vr == 0
                v = max(v, vr)
            if not dead and vt.prio[a + v - 1] < prio[q]:
                tot["able"] += 1
                tot["entries_score"] += len(win) * v
    n = max(tot["pairs"], 1)
    return {k: round(tot[k] / n, 4) for k in tot if k != "pairs"} | {"sample_pairs": tot["pairs"]}


def measure(e, jobs, prio, j, counts):
    import torch

    from fitgpu import ETA_DTYPE, EVICT_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)[:j]) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part[:j].view(np.int16))]
    pr = T(prio[:j])
    rows = torch.empty((j, 8), dtype=torch.int32, device=dev)
    eta = torch.empty((j, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.when_device(*cols, eta)  # warm-up: code objects, buffers
    e.preempt_tl_device(*cols, pr, rows)
    wms = sorted(e.when_device(*cols, eta) for _ in range(5))
    pms = sorted(e.preempt_tl_device(*cols, pr, rows) for _ in range(5))
    got = rows.cpu().numpy().view(EVICT_DTYPE).reshape(-1)
    when = eta.cpu().numpy().view(ETA_DTYPE).reshape(-1)
    if not (np.array_equal(got["members"], when["members"]) and np.array_equal(got["fit"], when["now"])):
        raise RuntimeError("fit_preempt_tl and fit_when disagree on members / the nodes that fit now")
    return {"what": "fit_preempt_tl_device next to fit_when_device", "jobs": j,
            "preempt_tl_ms_median_of_5": round(pms[2], 4), "preempt_tl_ms_min": round(pms[0], 4),
            "preempt_tl_ms_max": round(pms[4], 4), "when_ms_median_of_5": round(wms[2], 4),
            "when_ms_min": round(wms[0], 4), "when_ms_max": round(wms[4], 4),
            "preempt_tl_over_when": round(pms[2] / wms[2], 3), **counts,
            "codes": {str(c): int(k) for c, k in zip(*np.unique(got["code"], return_counts=True))},
            "when_codes": {str(c): int(k) for c, k in zip(*np.unique(when["code"], return_counts=True))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_tl_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C3 (a rehearsal; the record is the full size)")
    ap.add_argument("--queue", type=int, default=32768, help="jobs placed with place_tl before the query")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import Engine, synth
    nodes, jobs, parts = synth.make_config("c3", a.nodes, 16384)
    packed, v = synth.pack_victims(synth.SEEDS["c3"], nodes)
    vt, tline = synth.gen_victim_ends(synth.SEEDS["c3"], v, H, SLOT_MIN)
    prio = synth.gen_job_prio(synth.SEEDS["c3"], jobs.j)
    queue = synth.gen_jobs(synth.SEEDS["c5"], a.queue, parts.p)
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(packed)
        e.load_partitions(parts)
        e.load_timeline(tline)
        _, start, st = e.place_tl(queue)
        e.load_victims_tl(vt)
        nsample = np.arange(0, packed.n, max(1, packed.n // 512))[:512]
        dense = e.read_timeline()[nsample]  # the sample's rows only are kept
        rows = {int(x): dense[i] for i, x in enumerate(nsample)}
        base = {"nodes": packed.n, "victims": int(len(vt.prio)), "slots": H, "slot_min": SLOT_MIN,
                "queue": int(queue.j), "queue_placed": int(st["placed"]), "queue_in_the_future": int((start > 0).sum())}
        for j in (1024, 16384):
            jsample = np.arange(0, j, max(1, j // 32))[:32]
            counts = replay(rows, packed.part_mask, vt, parts, jobs, prio, jsample, nsample)
            lines.append(base | measure(e, jobs, prio, j, counts))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

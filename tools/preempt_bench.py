"""fit_preempt on the MI355X next to fit_room, its yardstick, one JSON line per
batch size, written to profiles/preempt_bench.json (and printed).

The table is config C3's (100k nodes, 16 partitions) packed with victims (synth.pack_victims: every
node but about 2 % runs preemptible jobs until it has no free cpu); the batches are the first 1,024
and 16,384 jobs of C3's stream with priorities from synth.gen_job_prio.  fit_room does the same walk
over the rows without the victims, so the result is a ratio against that kernel, not a gate:

  preempt_ms / room_ms   device ms from HIP events on the context's stream (fit_preempt_ms /
                         fit_room_ms): one warm-up call each, then the median of 5, same batch, same
                         table, same process
  victims_per_node       mean list length
  walked_per_pair        victim entries a lane has to look at per (job, row of its partition): a lane
                         looks when the row is eligible, short, and its whole list would free enough,
                         and stops at its first fit or at the first entry it does not outrank; counted
                         in numpy over a sample of the batch
  wave_loads_per_row     entries the WAVE loads per row of the first 64 jobs' partitions: the longest
                         walk among its 64 lanes, rounded up to the four entries of one wait

    python tools/preempt_bench.py [--out profiles/preempt_bench.json] [--nodes N]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]


def walked(nodes, v, parts, jobs, prio, sample):
    """Entries walked per (job, member row) over the jobs `sample`, and for the wave of jobs
    sample[:64] the entries loaded per row.  Jobs a partition limit rejects walk nothing."""
    n = nodes.n
    ln = np.diff(v.off).astype(np.int64)
    W = int(ln.max())
    col = np.arange(W)[None, :]
    inside = col < ln[:, None]
    src = np.minimum(v.off[:-1, None].astype(np.int64) + col, len(v.prio) - 1)
    vp = np.where(inside, v.prio.astype(np.int64)[src], np.iinfo(np.int64).max)
    S = np.zeros((n, W + 1, 3), np.int64)
    S[:, 1:, :] = np.cumsum(np.stack([np.where(inside, a.astype(np.int64)[src], 0) for a in (v.cpu, v.mem, v.gpu)], axis=2),
                            axis=1)
    free = [c.astype(np.int64) for c in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free)]
    is_open = (free[0] >= 0) & (free[1] >= 0) & (free[2] >= 0)
    ar = np.arange(W + 1)[None, :]
    pairs = entries = 0
    wave = {}  # partition -> per-row longest walk among the first 64 jobs
    for i, q in enumerate(sample):
        p, w = int(jobs.part[q]), int(jobs.wall[q])
        d = (int(jobs.cpu[q]), int(jobs.mem[q]), int(jobs.gpu[q]))
        if 0 <= parts.max_time_min[p] < w or 0 <= parts.max_cpus_per_node[p] < d[0] or 0 <= parts.max_mem_per_node[p] < d[1]:
            continue
        member = ((nodes.part_mask >> p) & 1) != 0
        elig = member & (nodes.avail_min >= w) & is_open
        ok = elig[:, None] & np.all([free[k][:, None] + S[:, :, k] >= d[k] for k in range(3)], axis=0)
        L = (vp < int(prio[q])).sum(1)
        low = ok & (ar <= L[:, None])
        has = low.any(1)
        looks = elig & ~ok[:, 0] & ok[np.arange(n), ln]
        steps = np.where(looks, np.where(has, low.argmax(1), L + 1), 0)
        pairs += int(member.sum())
        entries += int(steps.sum())
        if i < 64:
            wave[p] = np.maximum(wave.get(p, 0), np.where(member, steps, 0))
    rows = sum(int((((nodes.part_mask >> p) & 1) != 0).sum()) for p in wave)
    loads = sum(int((4 * ((w + 3) // 4)).sum()) for w in wave.values())
    return entries / max(pairs, 1), loads / max(rows, 1)


def measure(e, nodes, v, parts, jobs, prio, j):
    import torch

    from fitgpu import EVICT_DTYPE, ROOM_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)[:j]) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part[:j].view(np.int16))]
    pr = T(prio[:j])
    rows = torch.empty((j, 8), dtype=torch.int32, device=dev)
    rrows = torch.empty((j, 5), dtype=torch.int64, device=dev)  # 40-byte rows, 8-byte aligned
    torch.cuda.synchronize()
    e.preempt_device(*cols, pr, rows)  # warm-up: code objects, buffers
    e.room_device(*cols, rrows)
    ms = sorted(e.preempt_device(*cols, pr, rows) for _ in range(5))
    rms = sorted(e.room_device(*cols, rrows) for _ in range(5))
    got = rows.cpu().numpy().view(EVICT_DTYPE).reshape(-1)
    room = rrows.cpu().numpy().view(ROOM_DTYPE).reshape(-1)
    if not (np.array_equal(got["members"], room["members"]) and np.array_equal(got["fit"], room["nodes"])):
        raise RuntimeError("fit_preempt and fit_room disagree on members / fit")
    sub = {f: getattr(jobs, f)[:j] for f in ("cpu", "mem", "gpu", "wall", "part")}
    # the first tile's wave, then a spread over the rest of the batch
    sample = np.concatenate([np.arange(min(64, j)), np.arange(64, j, max(1, (j - 64) // 64))[:64]])
    per_pair, wave_loads = walked(nodes, v, parts, type("J", (), sub), prio[:j], sample)
    per_part = np.array([int(((nodes.part_mask >> p) & 1).sum()) for p in range(parts.p)], np.int64)
    live = ~np.isin(got["code"], (1, 2, 3, 4))
    pairs = int(per_part[jobs.part[:j][live]].sum())
    return {"what": "fit_preempt_device next to fit_room_device, same batch, same packed table", "nodes": nodes.n, "jobs": j,
            "victims": int(len(v.prio)), "victims_per_node": round(len(v.prio) / nodes.n, 3), "pairs": pairs,
            "preempt_ms_median_of_5": round(ms[2], 4), "preempt_ms_min": round(ms[0], 4), "preempt_ms_max": round(ms[4], 4),
            "room_ms_median_of_5": round(rms[2], 4), "room_ms_min": round(rms[0], 4), "room_ms_max": round(rms[4], 4),
            "preempt_over_room": round(ms[2] / rms[2], 3), "walked_per_pair": round(per_pair, 4),
            "wave_loads_per_row": round(wave_loads, 3), "walked_sample_jobs": int(len(sample)),
            "codes": {str(c): int(k) for c, k in zip(*np.unique(got["code"], return_counts=True))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C3 (a rehearsal; the record is the full size)")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import Engine, synth
    nodes, jobs, parts = synth.make_config("c3", a.nodes, 16384)
    packed, v = synth.pack_victims(synth.SEEDS["c3"], nodes)
    prio = synth.gen_job_prio(synth.SEEDS["c3"], jobs.j)
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(packed)
        e.load_partitions(parts)
        e.load_victims(v)
        for j in (1024, 16384):
            lines.append(measure(e, packed, v, parts, jobs, prio, j))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

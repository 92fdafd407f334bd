"""fit_evicted_tl on the MI355X next to the recipe it replaces, one JSON line per row
count, written to profiles/evicted_tl_bench.json (and printed).

The setup is tools/preempt_tl_bench.py's: config C3's 100k nodes packed with victims
(synth.pack_victims), ends over a horizon of 1,024 slots of 5 minutes (synth.gen_victim_ends), the
timeline loaded from their release events, 32,768 of C5's jobs placed with place_tl.  Three reports:
the picks of one 8-node job (the first EVICT row of fit_preempt_tl_k among C3's jobs asked as 8-node
jobs: every pick's first out_victims entries), then 1,024 and 16,384 entries drawn without
replacement from the lists of the nodes in a partition, in random order.  Every timed call starts
from the same state: the timeline, the reservations and the lists are loaded again before it.

  evicted_ms           device ms of evicted_tl_device (HIP events on the context's stream): one warm-up,
                       then the median of 5 with min and max
  evicted_wall_ms      the same calls by the host's clock, every call ends synchronised
  the yardstick, in the same process: what a caller had to do before —
  unplace_ms / _wall   unplace_tl_device of the same windows (start 0, wall end x slot minutes)
  reload_wall_ms       load_victims_tl_device of the whole reduced CSR, resident on the device; it has no
                       device-time diagnostic, so the host's clock around the synchronised call
  old_over_new_wall    (unplace_wall + reload_wall) / evicted_wall, medians
  checked inside: after the warm-up call read_timeline() and read_victims_tl() are what the yardstick
  leaves behind, byte for byte

    python tools/evicted_tl_bench.py [--out profiles/evicted_tl_bench.json] [--nodes N] [--queue Q]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]

H, SLOT_MIN = 1024, 5
VCOLS = ("off", "prio", "end", "cpu", "mem", "gpu")


def reduced(vt, mask, rows):
    """The lists without the rows' entries and without the lists of nodes in no partition."""
    from fitgpu import synth
    n = len(vt.off) - 1
    owner = np.repeat(np.arange(n), np.diff(vt.off))
    keep = mask[owner] != 0
    keep[vt.off[rows[:, 0]] + rows[:, 1]] = False
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(owner[keep], minlength=n))
    return synth.VictimsTL(off.astype(np.int32), *(np.ascontiguousarray(getattr(vt, f)[keep]) for f in VCOLS[1:]))


def stats(name, v):
    v = sorted(v)
    return {f"{name}_median_of_5": round(v[2], 4), f"{name}_min": round(v[0], 4), f"{name}_max": round(v[4], 4)}


def measure(e, reload, vt, mask, rows, what):
    import torch
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    node, pos = T(rows[:, 0]), T(rows[:, 1])
    k = vt.off[rows[:, 0]] + rows[:, 1]
    k, x = k[vt.end[k] > 0], rows[vt.end[k] > 0, 0]  # an entry with end 0 hands nothing back
    ucols = [T(vt.cpu[k]), T(vt.mem[k]), T(vt.gpu[k]), T((vt.end[k].astype(np.int64) * SLOT_MIN).astype(np.int32))]
    unode, ustart = T(x.astype(np.int32)), T(np.zeros(len(k), np.int32))
    left = reduced(vt, mask, rows)
    lcols = [T(getattr(left, f)) for f in VCOLS]
    torch.cuda.synchronize()

    def new():
        reload()
        t0 = time.perf_counter()
        ms = e.evicted_tl_device(node, pos)
        return ms, (time.perf_counter() - t0) * 1e3

    def old():
        reload()
        t0 = time.perf_counter()
        e.unplace_tl_device(*ucols, None, unode, ustart, kmax=1)
        t1 = time.perf_counter()
        e.load_victims_tl_device(*lcols)
        t2 = time.perf_counter()
        return e.unplace_tl_ms(), (t1 - t0) * 1e3, (t2 - t1) * 1e3

    new()  # warm-up: code objects, buffers; and the check
    got = (e.read_timeline().tobytes(), [getattr(e.read_victims_tl(), f).tobytes() for f in VCOLS])
    old()
    want = (e.read_timeline().tobytes(), [getattr(e.read_victims_tl(), f).tobytes() for f in VCOLS])
    if got != want:
        raise RuntimeError("fit_evicted_tl and fit_unplace_tl + fit_load_victims_tl leave different states")
    n5, o5 = [new() for _ in range(5)], [old() for _ in range(5)]
    out = {"what": "fit_evicted_tl_device next to fit_unplace_tl_device + fit_load_victims_tl_device", "rows": what,
           "m": int(len(rows)), "touched_nodes": int(len(np.unique(rows[:, 0]))), "entries_left": int(left.off[-1])}
    out |= stats("evicted_ms", [v[0] for v in n5]) | stats("evicted_wall_ms", [v[1] for v in n5])
    out |= stats("unplace_ms", [v[0] for v in o5]) | stats("unplace_wall_ms", [v[1] for v in o5])
    out |= stats("reload_wall_ms", [v[2] for v in o5])
    old_wall = out["unplace_wall_ms_median_of_5"] + out["reload_wall_ms_median_of_5"]
    out["old_over_new_wall"] = round(old_wall / out["evicted_wall_ms_median_of_5"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evicted_tl_bench.json"))
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
    mask = packed.part_mask
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(packed)
        e.load_partitions(parts)

        def reload():
            e.load_timeline(tline)
            e.place_tl(queue)
            e.load_victims_tl(vt)

        reload()
        base = {"nodes": packed.n, "victims": int(len(vt.prio)), "slots": H, "slot_min": SLOT_MIN,
                "queue": int(queue.j)}
        wide = synth.Jobs(jobs.cpu[:1024], jobs.mem[:1024], jobs.gpu[:1024], jobs.wall[:1024], jobs.part[:1024],
                          np.full(1024, 8, np.uint16))
        rows8, node8, vic8 = e.preempt_tl_k(wide, prio[:1024], 8)
        q = int(np.flatnonzero(rows8["code"] == 6)[0])  # FIT_PRE_EVICT
        picks = np.array([(node8[q, i], p) for i in range(8) for p in range(vic8[q, i])], np.int32).reshape(-1, 2)
        lines.append(base | measure(e, reload, vt, mask, picks, f"the picks of one 8-node job (job {q})"))
        ln = np.where(mask != 0, np.diff(vt.off), 0)
        every = np.stack([np.repeat(np.arange(packed.n), ln), np.concatenate([np.arange(k) for k in ln])], axis=1)
        r = np.random.default_rng(synth.SEEDS["c3"])
        for m in (1024, 16384):
            rows = every[r.permutation(len(every))[:m]].astype(np.int32)
            lines.append(base | measure(e, reload, vt, mask, rows, "drawn from every list, in random order"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for s in map(json.dumps, lines):
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

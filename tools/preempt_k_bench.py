"""fit_preempt_k on the MI355X next to fit_preempt, its yardstick, one JSON line per
batch size and nodes_k column, written to profiles/preempt_k_bench.json (and printed).

The table and the batches are tools/preempt_bench.py's: config C3's 100k nodes packed with victims
(synth.pack_victims), the first 1,024 and 16,384 jobs of C3's stream with priorities from
synth.gen_job_prio.  fit_preempt does the same walk and keeps one minimum where fit_preempt_k keeps
the kmax smallest keys, so the result is a ratio against that kernel, not a gate.  Three runs per
batch: every nodes_k 1 at kmax 1, every nodes_k 1 at kmax 8, nodes_k as config C4 draws it (1, 2, 4, 8)
at kmax 8.  At need 1 the rows must be fit_preempt's, row for row, or the tool fails.

  preempt_k_ms / preempt_ms   device ms from HIP events on the context's stream (fit_preempt_k_ms /
                              fit_preempt_ms): one warm-up call each, then the median of 5, same
                              batch, same table, same process
  offers_per_pair             keys a lane is offered per (job, row of its partition): the rows with
                              some v in [0, L]
  lane_inserts_per_pair       of those, the ones below the lane's worst kept key when they come: a
                              wave's rows in order, its list empty at the start of its share of a
                              slice; counted in numpy over a sample of the batch
  wave_inserts_per_row        rows at which the insertion chain runs at all, a ballot over the 64 lanes
                              of the batch's first wave, per row it visits

    python tools/preempt_k_bench.py [--out profiles/preempt_k_bench.json] [--nodes N]
"""
import argparse
import bisect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]

WAVES, TILE, MIN_ROWS, CUS = 8, 64, 32, 256  # the walk's workgroup and explain_slices' rule (fit_explain.hip)


def rows_per_wave(j, members, maxn):
    """Rows of a component of `members` rows one wave visits in a row, for a batch of j jobs."""
    tiles = (min(j, 16384) + TILE - 1) // TILE
    want = (CUS * 8 + tiles - 1) // tiles
    most = (maxn + WAVES * MIN_ROWS - 1) // (WAVES * MIN_ROWS)
    slices = max(1, min(want, most, 4096))
    per = (members + slices - 1) // slices
    return max(1, (per + WAVES - 1) // WAVES)


def inserts(nodes, v, parts, jobs, prio, sample, kmax, j):
    """(offers, lane inserts, pairs) over the jobs `sample`, and for the wave of sample[:64] the rows
    visited and those at which some lane's key enters its list.  The rows of a partition in node-id
    order, which is their order in the table for C3's disjoint partitions."""
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
    per_part = np.array([int(((nodes.part_mask >> p) & 1).sum()) for p in range(parts.p)], np.int64)
    maxn = int(per_part.max())
    offers = lane = pairs = 0
    wave = {}  # partition -> per member row, whether some lane of the first wave inserts there
    for i, q in enumerate(sample):
        p, w = int(jobs.part[q]), int(jobs.wall[q])
        d = (int(jobs.cpu[q]), int(jobs.mem[q]), int(jobs.gpu[q]))
        if 0 <= parts.max_time_min[p] < w or 0 <= parts.max_cpus_per_node[p] < d[0] or 0 <= parts.max_mem_per_node[p] < d[1]:
            continue
        member = ((nodes.part_mask >> p) & 1) != 0
        ids = np.flatnonzero(member)
        elig = member & (nodes.avail_min >= w) & is_open
        ok = elig[:, None] & np.all([free[k][:, None] + S[:, :, k] >= d[k] for k in range(3)], axis=0)
        L = (vp < int(prio[q])).sum(1)
        low = ok & (ar <= L[:, None])
        has = low.any(1)[ids]
        vv = low.argmax(1)[ids]
        top = np.where(vv > 0, vp[ids, np.maximum(vv - 1, 0)], np.iinfo(np.int64).min)
        res = [np.minimum(free[k][ids] + S[ids, vv, k], 2**31 - 1) - d[k] for k in range(3)]
        sc = (np.minimum(res[2], 255) << 24) | (np.minimum(res[0], 4095) << 12) | np.minimum(res[1] >> 10, 4095)
        keys = list(zip(top.tolist(), vv.tolist(), sc.tolist(), ids.tolist()))
        seg = rows_per_wave(j, len(ids), maxn)
        entered = np.zeros(len(ids), bool)
        kept = []
        for x in np.flatnonzero(has):
            if x % seg == 0 or (kept and kept[0][3] < ids[x - x % seg]):
                kept = [k for k in kept if k[3] >= ids[x - x % seg]]  # a new wave's share: the list starts empty
            if len(kept) < kmax or keys[x] < kept[-1]:
                bisect.insort(kept, keys[x])
                del kept[kmax:]
                entered[x] = True
        pairs += len(ids)
        offers += int(has.sum())
        lane += int(entered.sum())
        if i < 64:
            wave[p] = wave.get(p, np.zeros(len(ids), bool)) | entered
    rows = sum(len(w) for w in wave.values())
    return offers / max(pairs, 1), lane / max(pairs, 1), sum(int(w.sum()) for w in wave.values()) / max(rows, 1)


def measure(e, nodes, v, parts, jobs, prio, j, nk, kmax, what):
    import torch

    from fitgpu import EVICT_DTYPE, EVICT_K_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)[:j]) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part[:j].view(np.int16))]
    pr = T(prio[:j])
    dk = T(nk[:j].view(np.int16))
    rows = torch.empty((j, 8), dtype=torch.int32, device=dev)
    krows = torch.empty((j, 10), dtype=torch.int32, device=dev)
    knode = torch.empty((j, kmax), dtype=torch.int32, device=dev)
    kvic = torch.empty((j, kmax), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.preempt_device(*cols, pr, rows)  # warm-up: code objects, buffers
    e.preempt_k_device(*cols, dk, pr, krows, knode, kvic, kmax=kmax)
    ms = sorted(e.preempt_device(*cols, pr, rows) for _ in range(5))
    kms = sorted(e.preempt_k_device(*cols, dk, pr, krows, knode, kvic, kmax=kmax) for _ in range(5))
    one = rows.cpu().numpy().view(EVICT_DTYPE).reshape(-1)
    got = krows.cpu().numpy().view(EVICT_K_DTYPE).reshape(-1)
    node, vic = knode.cpu().numpy(), kvic.cpu().numpy()
    if not (np.array_equal(got["members"], one["members"]) and np.array_equal(got["fit"], one["fit"]) and
            np.array_equal(got["able"], one["able"]) and np.array_equal(got["outranked"], one["outranked"])):
        raise RuntimeError("fit_preempt_k and fit_preempt disagree on the counters")
    if (nk[:j] <= 1).all() and not (all(np.array_equal(got[f], one[f]) for f in ("code", "victims", "top_prio")) and
                                     np.array_equal(node[:, 0], one["node"]) and np.array_equal(vic[:, 0], one["victims"])):
        raise RuntimeError("fit_preempt_k at need 1 and fit_preempt disagree")
    sub = type("J", (), {f: getattr(jobs, f)[:j] for f in ("cpu", "mem", "gpu", "wall", "part")})
    sample = np.concatenate([np.arange(min(64, j)), np.arange(64, j, max(1, (j - 64) // 64))[:64]])
    offers, lane, wave = inserts(nodes, v, parts, sub, prio[:j], sample, kmax, j)
    return {"what": what, "nodes": nodes.n, "jobs": j, "kmax": kmax,
            "need": {str(c): int(k) for c, k in zip(*np.unique(got["need"], return_counts=True))},
            "preempt_k_ms_median_of_5": round(kms[2], 4), "preempt_k_ms_min": round(kms[0], 4),
            "preempt_k_ms_max": round(kms[4], 4), "preempt_ms_median_of_5": round(ms[2], 4),
            "preempt_ms_min": round(ms[0], 4), "preempt_ms_max": round(ms[4], 4),
            "preempt_k_over_preempt": round(kms[2] / ms[2], 3), "offers_per_pair": round(offers, 4),
            "lane_inserts_per_pair": round(lane, 5), "wave_inserts_per_row": round(wave, 4),
            "insert_sample_jobs": int(len(sample)),
            "codes": {str(c): int(k) for c, k in zip(*np.unique(got["code"], return_counts=True))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_k_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C3 (a rehearsal; the record is the full size)")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    from fitgpu import Engine, synth
    nodes, jobs, parts = synth.make_config("c3", a.nodes, 16384)
    packed, v = synth.pack_victims(synth.SEEDS["c3"], nodes)
    prio = synth.gen_job_prio(synth.SEEDS["c3"], jobs.j)
    ones = np.ones(jobs.j, np.uint16)
    c4 = synth.gen_jobs(synth.SEEDS["c4"], jobs.j, parts.p, multi_node=True).nodes_k
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(packed)
        e.load_partitions(parts)
        e.load_victims(v)
        for j in (1024, 16384):
            for nk, kmax, what in ((ones, 1, "nodes_k 1, kmax 1"), (ones, 8, "nodes_k 1, kmax 8"),
                                   (c4, 8, "nodes_k as C4 (1, 2, 4, 8), kmax 8")):
                lines.append(measure(e, packed, v, parts, jobs, prio, j, nk, kmax,
                                     "fit_preempt_k_device next to fit_preempt_device: " + what))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

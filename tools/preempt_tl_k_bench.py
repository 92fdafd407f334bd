"""fit_preempt_tl_k on the MI355X next to fit_preempt_tl, its yardstick, one JSON line
per batch size and nodes_k column, written to profiles/preempt_tl_k_bench.json (and printed).

The setup is tools/preempt_tl_bench.py's: config C3's 100k nodes packed with victims
(synth.pack_victims), ends over a horizon of 1,024 slots of 5 minutes (synth.gen_victim_ends), the
timeline loaded from their release events, 32,768 of C5's jobs placed with place_tl.  The batches are
the first 1,024 and 16,384 jobs of C3's stream with priorities from synth.gen_job_prio, three times
each: every nodes_k 1 at kmax 1, every nodes_k 1 at kmax 8, nodes_k as config C4 draws it (1, 2, 4, 8)
at kmax 8.  The result is a ratio against fit_preempt_tl_device on the same batch, timeline and
process, not a gate.

  preempt_tl_k_ms / preempt_tl_ms   device ms from HIP events on the context's stream: one warm-up
                                    call each, then the median of 5 with min and max
  checked inside: the need-1 rows and pick 0 are fit_preempt_tl's rows, field for field; members and
  fit are fit_when_k's members and now
  per (job, member node) pair, counted in numpy over one tile of 64 consecutive jobs x one node slice
  of consecutive node ids by working out every pair's key on the dense timeline (read_timeline()) and
  keeping, as the kernel does, one list of kmax keys per (job, wave) that starts empty, a wave's
  positions modelled as PER_WAVE consecutive ids (see there; the ids stand in for positions, and the
  merges of the fold and of the final kernel are not counted):
  offers_per_pair             keys a pair offers: it fits, or it can be freed
  lane_inserts_per_pair       offers that enter the lane's list of kmax keys
  chain_nodes_share           nodes at which the insertion chain runs at all: some lane of the 64 inserts

    python tools/preempt_tl_k_bench.py [--out profiles/preempt_tl_k_bench.json] [--nodes N] [--queue Q]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd")]

H, SLOT_MIN = 1024, 5
I32MAX = 2**31 - 1
# The walk cuts a component's positions into node slices (preempt_slices) and a slice over its 8 waves.
# On C3's components of some 6,000 nodes a wave's share is about 32 positions at 1,024 jobs (the
# smallest the slicing allows) and about 96 at 16,384 jobs (8 slices per component): the counts below
# take runs of that many consecutive node ids for a wave's positions.
PRE_WAVES, PER_WAVE = 8, (32, 96)


def score(dc, dm, dg):
    return (np.minimum(dg, 255) << 24) | (np.minimum(dc, 4095) << 12) | np.minimum(dm >> 10, 4095)


def pair_keys(T, ids, mask, vt, parts, jobs, prio, tile):
    """The key of every (job of `tile`, node of `ids`) pair, T the nodes' dense rows: (member [J, N], has
    [J, N], keys [J, N] of (top, v, score)).  A node's free amounts and what a prefix frees change only
    at the starts of its runs and at its victims' ends, so every window is judged at those slots: a
    few dozen per node instead of up to 1,024."""
    J, N = len(tile), len(ids)
    dem = np.stack([jobs.cpu[tile], jobs.mem[tile], jobs.gpu[tile]], axis=1).astype(np.int64)  # [J, 3]
    part, wall, pr = jobs.part[tile].astype(np.int64), jobs.wall[tile].astype(np.int64), prio[tile].astype(np.int64)
    P = parts.p
    lim = [np.asarray(a, np.int64)[np.minimum(part, P - 1)] for a in (parts.max_time_min, parts.max_cpus_per_node,
                                                                       parts.max_mem_per_node)]
    live_job = (part < P) & ~((0 <= lim[0]) & (lim[0] < wall)) & ~((0 <= lim[1]) & (lim[1] < dem[:, 0])) & \
        ~((0 <= lim[2]) & (lim[2] < dem[:, 1]))
    d = np.maximum(1, -(-wall // SLOT_MIN))
    member = np.zeros((J, N), bool)
    has = np.zeros((J, N), bool)
    keys = np.zeros((J, N, 3), np.int64)
    for k, x in enumerate(ids):
        row = T[k].astype(np.int64)
        a, b = int(vt.off[x]), int(vt.off[x + 1])
        end = vt.end[a:b].astype(np.int64)
        cut = np.flatnonzero((np.diff(row, axis=0) != 0).any(axis=1)) + 1
        bp = np.unique(np.concatenate([[0], cut, end[(end > 0) & (end < H)]]))  # the starts of the constant stretches
        amt = np.stack([vt.cpu[a:b], vt.mem[a:b], vt.gpu[a:b]], axis=1).astype(np.int64)
        cum = np.zeros((b - a + 1, len(bp), 3), np.int64)
        cum[1:] = np.cumsum(amt[:, None, :] * (end[:, None] > bp[None, :])[:, :, None], axis=0)
        tot = row[bp][None] + cum                                            # [W + 1, B, 3]
        mb = live_job & (((int(mask[x]) >> np.minimum(part, 31)) & 1) != 0)
        member[:, k] = mb
        inwin = bp[None, :] < d[:, None]                                      # [J, B]
        elig = mb & (d <= H) & ((row[bp] >= 0).all(axis=1)[None, :] | ~inwin).all(axis=1)
        ok = ((tot[None] >= dem[:, None, None, :]).all(axis=3) | ~inwin[:, None, :]).all(axis=2)  # [J, W + 1]
        L = (vt.prio[a:b].astype(np.int64)[None, :] < pr[:, None]).sum(axis=1)
        low = ok & elig[:, None] & (np.arange(b - a + 1)[None, :] <= L[:, None])
        h = low.any(axis=1)
        v = low.argmax(axis=1)
        res = np.where(inwin[:, :, None], np.minimum(tot[v], I32MAX), I32MAX).min(axis=1) - dem  # [J, 3]
        has[:, k] = h
        keys[:, k, 0] = np.where(v > 0, vt.prio[a:b].astype(np.int64)[np.maximum(v - 1, 0)] if b > a else 0,
                                 np.iinfo(np.int64).min)
        keys[:, k, 1] = v
        keys[:, k, 2] = score(res[:, 0], res[:, 1], res[:, 2])
    return member, has, keys


def inserts(member, has, keys, kmax, per_wave):
    """The counts of the docstring: the nodes in runs of per_wave consecutive ids, one run per wave, every
    (job, wave) with a list of kmax keys of its own that starts empty, as k_ptlk_walk keeps them."""
    J, N = has.shape
    pairs, offers, lane = int(member.sum()), int(has.sum()), 0
    chain = np.zeros(N, bool)
    for q in range(J):
        for w0 in range(0, N, per_wave):
            kept = []
            for x in np.flatnonzero(has[q, w0:w0 + per_wave]) + w0:  # in id order, as a lane meets them
                key = (*keys[q, x].tolist(), int(x))
                if len(kept) < kmax or key < kept[-1]:
                    kept = sorted(kept + [key])[:kmax]
                    lane += 1
                    chain[x] = True
    n = max(pairs, 1)
    return {"offers_per_pair": round(offers / n, 4), "lane_inserts_per_pair": round(lane / n, 4),
            "chain_nodes_share": round(float(chain.sum()) / max(int(member.any(axis=0).sum()), 1), 4),
            "sample_pairs": pairs, "sample_nodes": N, "sample_jobs": J, "ids_per_wave": per_wave}


def measure(e, jobs, prio, nk, kmax, j, what, counts):
    import torch

    from fitgpu import ETA_K_DTYPE, EVICT_DTYPE, EVICT_K_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)[:j]) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part[:j].view(np.int16))]
    pr, dk = T(prio[:j]), T(np.ascontiguousarray(nk[:j], np.uint16).view(np.int16))
    one = torch.empty((j, 8), dtype=torch.int32, device=dev)
    rows = torch.empty((j, 10), dtype=torch.int32, device=dev)
    eta = torch.empty((j, 10), dtype=torch.int32, device=dev)
    on, ov, en = (torch.empty((j, kmax), dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    e.preempt_tl_device(*cols, pr, one)  # warm-up: code objects, buffers
    e.preempt_tl_k_device(*cols, dk, pr, rows, on, ov, kmax=kmax)
    tms = sorted(e.preempt_tl_device(*cols, pr, one) for _ in range(5))
    kms = sorted(e.preempt_tl_k_device(*cols, dk, pr, rows, on, ov, kmax=kmax) for _ in range(5))
    e.when_k_device(*cols, dk, eta, en, kmax=kmax)
    got = rows.cpu().numpy().view(EVICT_K_DTYPE).reshape(-1)
    want = one.cpu().numpy().view(EVICT_DTYPE).reshape(-1)
    when = eta.cpu().numpy().view(ETA_K_DTYPE).reshape(-1)
    node, vic = on.cpu().numpy(), ov.cpu().numpy()
    if not (np.array_equal(got["members"], when["members"]) and np.array_equal(got["fit"], when["now"])):
        raise RuntimeError("fit_preempt_tl_k and fit_when_k disagree on members / the nodes that fit now")
    n1 = got["need"] == 1
    same = all(np.array_equal(got[f][n1], want[f][n1]) for f in ("code", "victims", "top_prio", "members", "fit", "able",
                                                                 "outranked"))
    if not (same and np.array_equal(node[n1, 0], want["node"][n1]) and np.array_equal(vic[n1, 0], want["victims"][n1])):
        raise RuntimeError("a need-1 row of fit_preempt_tl_k is not fit_preempt_tl's")
    return {"what": "fit_preempt_tl_k_device next to fit_preempt_tl_device", "nodes_k": what, "kmax": kmax, "jobs": j,
            "need_1_rows_checked": int(n1.sum()),
            "preempt_tl_k_ms_median_of_5": round(kms[2], 4), "preempt_tl_k_ms_min": round(kms[0], 4),
            "preempt_tl_k_ms_max": round(kms[4], 4), "preempt_tl_ms_median_of_5": round(tms[2], 4),
            "preempt_tl_ms_min": round(tms[0], 4), "preempt_tl_ms_max": round(tms[4], 4),
            "preempt_tl_k_over_preempt_tl": round(kms[2] / tms[2], 3), **counts,
            "codes": {str(c): int(k) for c, k in zip(*np.unique(got["code"], return_counts=True))},
            "picks": int((node >= 0).sum()), "picks_that_evict": int((vic > 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_tl_k_bench.json"))
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
    ones = np.ones(jobs.j, np.uint16)
    c4 = synth.gen_jobs(synth.SEEDS["c4"], jobs.j, parts.p, multi_node=True).nodes_k
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(packed)
        e.load_partitions(parts)
        e.load_timeline(tline)
        _, start, st = e.place_tl(queue)
        e.load_victims_tl(vt)
        base = {"nodes": packed.n, "victims": int(len(vt.prio)), "slots": H, "slot_min": SLOT_MIN,
                "queue": int(queue.j), "queue_placed": int(st["placed"]), "queue_in_the_future": int((start > 0).sum())}
        tile = np.arange(64)  # the keys do not depend on nodes_k: one count per batch size and list capacity
        dense = e.read_timeline()[:PRE_WAVES * max(PER_WAVE)].copy()  # the sample's rows only are kept
        for j, per_wave in ((1024, PER_WAVE[0]), (16384, PER_WAVE[1])):
            ids = np.arange(min(packed.n, PRE_WAVES * per_wave))  # one node slice: a lane meets its nodes in order
            member, has, keys = pair_keys(dense[ids], ids, packed.part_mask, vt, parts, jobs, prio, tile)
            counts = {kmax: inserts(member, has, keys, kmax, per_wave) for kmax in (1, 8)}
            for nk, kmax, what in ((ones, 1, "1"), (ones, 8, "1"), (c4, 8, "as C4 (1, 2, 4, 8)")):
                lines.append(base | measure(e, jobs, prio, nk, kmax, j, what, counts[kmax]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

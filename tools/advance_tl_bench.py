"""fit_advance_tl on the MI355X: one JSON line per advance, written to
profiles/advance_tl_bench.json (and printed).

Config C5 as tools/unplace_tl_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min),
after fit_place_tl_k_device of its first 16,384 jobs with nodes_k drawn as config C4 draws it (kmax 8):
the state S.  Every timed call starts from S, rebuilt by a reload and the placement.  Device ms is
fit_advance_tl_ms (HIP events on the context's stream) of fit_advance_tl_device for a = 1, 12 and 512
with level tails (every node's level at the loaded horizon edge): one warm-up call, then the median of
5 with min and max.
The yardstick is what a caller does without the call, timed in the same run: fit_load_nodes_device
plus fit_load_timeline_device of the shifted release events (host clock around the two calls, which
end in a stream synchronisation; events at or before slot a folded into the node table, avail_min
lowered by a slots) plus fit_place_tl_k_device of the rows whose window ends after a
(stats.ms_device).  The two routes are NOT claimed to end in the same timeline: re-placement may pick
other slots.  What is asserted, once per a, is read_timeline() after the advance against the numpy
restatement of §2i on S.
list_bytes is what the call must move: per node its header read and written (96 B each) and 16 B per
run read and per run written.

    python tools/advance_tl_bench.py [--out profiles/advance_tl_bench.json] [--nodes N] [--only A]
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


def ref_advance_tl(tl, a, tail):
    """§2i on the dense [n, H, 3] timeline (tests/_advance_tl_cases.ref_advance_tl)."""
    n, H, _ = tl.shape
    ap = min(a, H)
    out = np.empty_like(tl)
    out[:, :H - ap] = tl[:, ap:]
    out[:, H - ap:] = np.where(tl[:, H - 1] == -1, -1, tail)[:, None, :]
    return out


def run_counts(dense):
    cnt = np.ones(dense.shape[0], np.int64)
    for lo in range(0, dense.shape[0], 8192):  # in blocks: the comparison's temporaries stay small
        d = dense[lo:lo + 8192]
        cnt[lo:lo + 8192] += (d[:, 1:] != d[:, :-1]).any(axis=2).sum(axis=1)
    return cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "advance_tl_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--only", type=int, default=None, help="one advance, no yardstick and no check (for a "
                    "kernel trace)")
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
    J, H, L, n = jobs.j, int(tline.slots), int(tline.slot_min), nodes.n
    dnodes = [T(x) for x in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min,
                             nodes.part_mask.view(np.int32))]
    dtl = [T(x) for x in (tline.off, tline.slot, tline.cpu, tline.mem, tline.gpu)]
    ev_node = np.repeat(np.arange(n), np.diff(tline.off))
    lines = []
    with Engine(device=0) as e:
        def reload(dn=dnodes, dt=dtl):
            t0 = time.perf_counter()
            e.load_nodes_device(*dn)
            t1 = time.perf_counter()
            e.load_partitions(parts)  # not timed: a caller keeps its partitions
            t2 = time.perf_counter()
            e.load_timeline_device(H, L, *dt)
            return (t1 - t0 + time.perf_counter() - t2) * 1e3

        def place(rows):
            """fit_place_tl_k_device of the rows on the current timeline: (nodes, start, device ms)."""
            cols = [T(getattr(jobs, f)[rows]) for f in FIELDS]
            part, nk = T(jobs.part[rows].view(np.int16)), T(jobs.nodes_k[rows].view(np.int16))
            on = torch.empty((len(rows), KMAX), dtype=torch.int32, device=dev)
            os_ = torch.empty(len(rows), dtype=torch.int32, device=dev)
            st = e.place_tl_k_device(*cols, part, nk, on, os_, KMAX)
            return on, os_, st["ms_device"]

        every = np.arange(J)
        reload()
        level = e.read_timeline()[:, H - 1].copy()  # [n, 3]: the loaded level at the horizon edge
        dtail = [T(level[:, i]) for i in range(3)]
        _, d_start, _ = place(every)
        start = d_start.cpu().numpy()

        def to_S():
            reload()
            place(every)

        def timed(adv):
            ms = []
            for _ in range(a.reps + 1):  # the first is the warm-up
                to_S()
                e.advance_tl_device(adv, *dtail)
                ms.append(e.advance_tl_ms())
            return stat3(ms[1:])

        if a.only is not None:
            print(json.dumps({"a": a.only, "advance_tl_ms": timed(a.only)}), flush=True)
            return
        S = e.read_timeline()
        cnt_S = run_counts(S)
        d = np.maximum(1, -(-jobs.wall.astype(np.int64) // L))
        end = np.minimum(start.astype(np.int64) + d, H)
        for adv in (1, 12, 512):
            ms = timed(adv)
            to_S()
            e.advance_tl_device(adv, *dtail)
            got = e.read_timeline()
            want = ref_advance_tl(S, adv, level)
            assert got.tobytes() == want.tobytes(), "the advance differs from the restatement of §2i"
            cnt_after = run_counts(want)
            del got, want
            # the yardstick: the shifted cluster loaded, then the surviving rows placed again
            early = tline.slot <= adv
            add = lambda col: np.bincount(ev_node[early], weights=col[early], minlength=n).astype(np.int64)  # noqa: E731
            av = np.where(nodes.avail_min == synth.INT32_MAX, synth.INT32_MAX,
                          np.maximum(nodes.avail_min.astype(np.int64) - adv * L, 0))
            dn2 = [T((nodes.cpu_free + add(tline.cpu)).astype(np.int32)), T((nodes.mem_free + add(tline.mem)).astype(np.int32)),
                   T((nodes.gpu_free + add(tline.gpu)).astype(np.int32)), T(av.astype(np.int32)), dnodes[4]]
            keep = ~early
            off2 = np.concatenate([[0], np.cumsum(np.bincount(ev_node[keep], minlength=n))]).astype(np.int32)
            dt2 = [T(off2), T(tline.slot[keep] - adv), T(tline.cpu[keep]), T(tline.mem[keep]), T(tline.gpu[keep])]
            survivors = np.flatnonzero((start >= 0) & (end > adv))
            rl, pl = [], []
            for _ in range(a.reps + 1):
                rl.append(reload(dn2, dt2))
                pl.append(place(survivors)[2] if len(survivors) else 0.0)
            r, p = stat3(rl[1:]), stat3(pl[1:])
            list_bytes = int(2 * 96 * n + 16 * (cnt_S.sum() + cnt_after.sum()))
            line = {"a": adv, "advance_tl_ms_median_of_%d" % a.reps: ms[0], "advance_tl_ms_min": ms[1],
                    "advance_tl_ms_max": ms[2],
                    "reload_ms_median": r[0], "reload_ms_min": r[1], "reload_ms_max": r[2],
                    "replace_ms_median": p[0], "replace_ms_min": p[1], "replace_ms_max": p[2],
                    "replaced_rows": int(len(survivors)), "ratio_to_reload": round(ms[0] / r[0], 5),
                    "ratio_to_reload_plus_replace": round(ms[0] / (r[0] + p[0]), 5),
                    "list_bytes": list_bytes, "gbytes_per_s": round(list_bytes / (ms[0] * 1e-3) / 1e9, 1),
                    "runs_in_S": int(cnt_S.sum()), "runs_after": int(cnt_after.sum()),
                    "lists_over_4_runs": int((cnt_S > 4).sum()), "lists_over_8_runs": int((cnt_S > 8).sum()),
                    "longest_list": int(cnt_S.max()), "checked_against_restatement": True,
                    "nodes": n, "slots": H, "queue": J, "placed_in_S": int((start >= 0).sum())}
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

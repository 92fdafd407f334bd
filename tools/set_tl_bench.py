"""fit_set_tl on the MI355X next to the reload it replaces: one JSON line per batch,
written to profiles/set_tl_bench.json (and printed).

Config C5 as tools/place_tl_k_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min),
after fit_place_tl_k_device of its first 16,384 jobs with nodes_k drawn as config C4 draws it (kmax 8)
and a fit_load_victims_tl_device of 0-3 entries per node: the state S.  The nodes a batch names carry
no record of that placement, so the reload route can put every record back.
  (a) one node closed                       (b) 1,000 random nodes closed
  (c) the same 1,000 reopened, from the state (b) leaves: a base row plus 3 release rows each
  (d) 16,384 rows on one node: the most windows a launch sequence can give one wave
Every timed call starts from its state, rebuilt before it.  set_tl_ms is fit_set_tl_ms (HIP events on
the context's stream), set_tl_wall_ms the same calls by the host's clock: one warm-up, then the median
of 5 with min and max.
The yardstick is the route a caller had before, timed in the same run on the same inputs by the host's
clock around calls that end synchronised: fit_load_nodes of the changed node table, fit_load_timeline_device
of the changed release events, fit_load_victims_tl_device, fit_hold_tl_device of all 16,384 records.
Both routes must end in the same read_timeline(): asserted for (a)-(c).  (d)'s timeline cannot be
written as a node row plus release events; its yardstick is the rebuild of S, and its result is
checked against a numpy restatement of §2q on that node's row.

    python tools/set_tl_bench.py [--out profiles/set_tl_bench.json] [--nodes N] [--only a|b|c|d]
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
INT32_MAX = 2**31 - 1


def stat3(name, v):
    v = sorted(v)
    return {f"{name}_median_of_{len(v)}": round(v[len(v) // 2], 4), f"{name}_min": round(v[0], 4),
            f"{name}_max": round(v[-1], 4)}


def with_events(tline, drop, extra):
    """tline without the events of the nodes in `drop`, plus extra = [(node, slot, cpu, mem, gpu)]."""
    from fitgpu import synth
    n = len(tline.off) - 1
    owner = np.repeat(np.arange(n), np.diff(tline.off))
    keep = ~np.isin(owner, drop)
    ex = np.array(extra, np.int64).reshape(-1, 5)
    own = np.concatenate([owner[keep], ex[:, 0]])
    cols = [np.concatenate([np.asarray(c)[keep], ex[:, k]]) for k, c in
            enumerate((tline.slot, tline.cpu, tline.mem, tline.gpu), start=1)]
    order = np.lexsort((cols[0], own))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(own, minlength=n))
    return synth.Timeline(slots=tline.slots, slot_min=tline.slot_min, off=off.astype(np.int32),
                          **{f: c[order].astype(np.int32) for f, c in zip(("slot", "cpu", "mem", "gpu"), cols)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_tl_bench.json"))
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
    nodes, tline, _, parts = synth.make_c5(a.nodes, a.jobs)
    jobs = synth.gen_jobs(synth.SEEDS["c5"], a.jobs, parts.p, multi_node=True)
    n, J, H, L = nodes.n, jobs.j, int(tline.slots), int(tline.slot_min)
    r = np.random.default_rng(synth.SEEDS["c5"])
    ln = r.integers(0, 4, n)  # the victims: 0-3 entries per node, in priority order
    own = np.repeat(np.arange(n), ln)
    prio = r.integers(0, 100, len(own))
    prio = prio[np.lexsort((prio, own))]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(ln)
    vic = [T(x.astype(np.int32)) for x in (off, prio, r.integers(0, H + 1, len(own)), r.integers(1, 9, len(own)),
                                           r.integers(0, 4096, len(own)), r.integers(0, 2, len(own)))]
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline_device(H, L, *[T(x) for x in (tline.off, tline.slot, tline.cpu, tline.mem, tline.gpu)])
        jcols = [T(getattr(jobs, f)) for f in FIELDS]
        jnk = T(jobs.nodes_k.view(np.int16))
        d_node = torch.empty((J, KMAX), dtype=torch.int32, device=dev)
        d_start = torch.empty(J, dtype=torch.int32, device=dev)
        d_state = torch.empty(J, dtype=torch.int32, device=dev)
        st = e.place_tl_k_device(*jcols, T(jobs.part.view(np.int16)), jnk, d_node, d_start, KMAX)
        node, start = d_node.cpu().numpy(), d_start.cpu().numpy()
        S = e.read_timeline()
        used = np.unique(node[start >= 0])
        # nodes without a record, open over the whole horizon: what a drain closes and a resume reopens
        idle = np.setdiff1d(np.flatnonzero((nodes.part_mask != 0) & (S[:, 0] >= 0).all(axis=1) & (S[:, H - 1] >= 0).all(axis=1)),
                            used)
        pick = r.permutation(idle)[:1001]
        one, many = pick[:1], pick[1:]

        def route(table, events):
            """The reload route: (host ms of the four calls that end synchronised, refused records)."""
            dtl = [T(x) for x in (events.off, events.slot, events.cpu, events.mem, events.gpu)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.load_nodes(table)
            t1 = time.perf_counter()
            e.load_timeline_device(H, L, *dtl)
            t2 = time.perf_counter()
            e.load_victims_tl_device(*vic)
            t3 = time.perf_counter()
            _, refused = e.hold_tl_device(*jcols, jnk, d_node, d_start, d_state, KMAX)
            t4 = time.perf_counter()
            return [(y - x) * 1e3 for x, y in ((t0, t4), (t0, t1), (t1, t2), (t2, t3), (t3, t4))], refused

        def drained(table, which):
            t = synth.Nodes(*(getattr(table, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min",
                                                                   "part_mask")))
            t.avail_min[which] = 0
            return t

        _, refused = route(nodes, tline)
        assert refused == 0 and np.array_equal(e.read_timeline(), S), "hold of every record does not rebuild S"

        def bench(what, rows, before, after, check=None):
            """rows: (node, from, to, cpu, mem, gpu) columns; before / after: the (table, events) of the
            state the call starts from and of the state the reload route ends in."""
            cols = [T(np.ascontiguousarray(c, np.int32)) for c in rows]
            ms, wall, counts = [], [], None
            for _ in range(a.reps + 1):  # the first is the warm-up
                route(*before)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                counts = e.set_tl_device(*cols)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(e.set_tl_ms())
            got = e.read_timeline()
            old = [route(*after)[0] for _ in range(a.reps + 1)]
            if check is None:
                assert np.array_equal(got, e.read_timeline()), "the two routes end in different timelines"
            else:
                check(got)
            line = {"what": what, "rows": int(len(rows[0])), "applied": int(counts[0]), "ignored": int(counts[1]),
                    "touched_nodes": int(len(np.unique(rows[0])))}
            line |= stat3("set_tl_ms", ms[1:]) | stat3("set_tl_wall_ms", wall[1:])
            for k, name in enumerate(("reload_route_wall_ms", "load_nodes_wall_ms", "load_timeline_device_wall_ms",
                                      "load_victims_tl_device_wall_ms", "hold_tl_device_wall_ms")):
                line |= stat3(name, [o[k] for o in old[1:]])
            line["old_over_new_wall"] = round(line[f"reload_route_wall_ms_median_of_{a.reps}"] /
                                              line[f"set_tl_wall_ms_median_of_{a.reps}"], 1)
            line |= {"same_timeline_as_reload_route": check is None, "nodes": n, "slots": H, "records": J,
                     "placed_in_S": int(st["placed"]), "victims": int(len(own))}
            lines.append(line)
            print(json.dumps(line), flush=True)

        def close(which):
            m = len(which)
            return [which, np.zeros(m), np.full(m, INT32_MAX), np.full(m, -1), np.full(m, -1), np.full(m, -1)]

        if a.only in (None, "a"):
            bench("(a) one node closed", close(one), (nodes, tline), (drained(nodes, one), tline))
        if a.only in (None, "b"):
            bench("(b) 1,000 random nodes closed", close(many), (nodes, tline), (drained(nodes, many), tline))
        if a.only in (None, "c"):
            rows, extra = [], []
            for x in many.tolist():
                lv = np.array([nodes.cpu_free[x], nodes.mem_free[x], nodes.gpu_free[x]], np.int64)
                rows.append((x, 0, H, *lv))
                for s in sorted(r.choice(np.arange(1, H), 3, replace=False).tolist()):
                    ev = (int(r.integers(1, 17)), int(r.integers(0, 9)) * 1024, int(r.integers(0, 2)))
                    lv = lv + ev
                    rows.append((x, s, INT32_MAX, *lv))
                    extra.append((x, s, *ev))
            table = synth.Nodes(*(getattr(nodes, f).copy() for f in ("cpu_free", "mem_free", "gpu_free", "avail_min",
                                                                       "part_mask")))
            table.avail_min[many] = INT32_MAX
            bench("(c) the same 1,000 reopened: a base row plus 3 release rows each", list(np.array(rows, np.int64).T),
                  (drained(nodes, many), tline), (table, with_events(tline, many, extra)))
        if a.only in (None, "d"):
            W, x = 16384, int(one[0])
            frm = r.integers(0, H, W)
            rows = [np.full(W, x), frm, frm + r.integers(1, 65, W), r.integers(-1, 65, W), r.integers(-1, 9, W) * 1024 + 1,
                    r.integers(-1, 5, W)]
            rows[4] = np.maximum(rows[4], -1)

            def check(got):
                want = S[x].copy()
                for q in range(W):
                    want[rows[1][q]:rows[2][q]] = [rows[3][q], rows[4][q], rows[5][q]]
                assert np.array_equal(got[x], want), "(d) differs from the restatement of §2q"
                assert np.array_equal(got[:x], S[:x]) and np.array_equal(got[x + 1:], S[x + 1:]), "(d) changed another node"
            bench("(d) 16,384 rows on one node", rows, (nodes, tline), (nodes, tline), check)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln_ in lines:
            fh.write(json.dumps(ln_) + "\n")


if __name__ == "__main__":
    main()

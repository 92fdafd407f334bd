"""fit_place_tl_k_win / fit_when_k_win on the MI355X: one JSON line per
measurement, written to profiles/win_tl_bench.json (and printed).

Config C5 as tools/place_tl_k_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min),
the first 16,384 jobs of its queue with nodes_k = 1 and with nodes_k drawn as config C4 draws it
(kmax 8).  Device ms (stats.ms_device / fit_when_k_win_ms, HIP events on the context's stream): one
warm-up call of each side, then five rounds that ALTERNATE the two sides, a fresh load_timeline
before every placement; the median of 5 with min and max.
  (1) place_tl_k_win_device with open windows (both columns NULL) against place_tl_k_device on the
      same jobs.  The results are asserted equal.  ratio = windowed ms / unwindowed ms: what
      carrying the window costs.
  (2) the same jobs with the window draw of tests/_win_tl_cases.draw_windows; ratio_to_open against
      (1)'s windowed side.
  (3) when_k_win_device against when_k_device on the same jobs, on the timeline as the placement of
      (1) left it: open windows (asserted equal), then the draw.
--ab FILE: JSON lines of the UNWINDOWED tools (tools/place_tl_k_bench.py --only 1,
tools/when_k_bench.py) run at the parent commit and at this one in one GPU call, each tagged
{"side": "parent" | "new", "run": n}; they are summarised (the new medians against the parent's
min-max band over its runs) and appended.

    python tools/win_tl_bench.py [--out profiles/win_tl_bench.json] [--nodes N] [--ab FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd"), os.path.join(ROOT, "tests")]


def stat3(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)


def ms_fields(name, v):
    m = stat3(v)
    return {name + "_ms_median_of_5": m[0], name + "_ms_min": m[1], name + "_ms_max": m[2]}


def ratio(a, b):
    a, b = stat3(a), stat3(b)
    return {"ratio": round(a[0] / b[0], 3), "ratio_low": round(a[1] / b[2], 3), "ratio_high": round(a[2] / b[1], 3)}


def measure(e, label, tline, jobs, kmax, nb, dl):
    import torch

    from fitgpu import ETA_K_DTYPE
    dev = "cuda:0"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [T(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall")] + [T(jobs.part.view(np.int16))]
    nk = T(jobs.nodes_k.view(np.int16))
    dnb, ddl = T(nb), T(dl)
    on, os_ = (torch.empty((jobs.j, kmax), dtype=torch.int32, device=dev), torch.empty(jobs.j, dtype=torch.int32, device=dev))
    wn, ws = torch.empty_like(on), torch.empty_like(os_)
    dn, ds = torch.empty_like(on), torch.empty_like(os_)
    torch.cuda.synchronize()

    def plain():
        e.load_timeline(tline)
        return e.place_tl_k_device(*cols, nk, on, os_, kmax)["ms_device"]

    def opened():
        e.load_timeline(tline)
        return e.place_tl_k_win_device(*cols, nk, None, None, wn, ws, kmax)["ms_device"]

    def drawn():
        e.load_timeline(tline)
        return e.place_tl_k_win_device(*cols, nk, dnb, ddl, dn, ds, kmax)

    plain(), opened(), drawn()  # warm-up: code objects, buffers
    a, b, c = [], [], []
    for _ in range(5):
        a.append(plain())
        b.append(opened())
        st = drawn()
        c.append(st["ms_device"])
    assert torch.equal(on, wn) and torch.equal(os_, ws), "open windows differ from fit_place_tl_k"
    base = {"jobs": jobs.j, "kmax": kmax, "nodes_k": {str(k): int(n) for k, n in zip(*np.unique(jobs.nodes_k, return_counts=True))}}
    lines = [dict(base, what=f"(1) place_tl_k_win_device, open windows, against place_tl_k_device; {label}",
                  placed=int((ws >= 0).sum()), results_equal=True,
                  **ms_fields("place_tl_k_win", b), **ms_fields("place_tl_k", a), **ratio(b, a)),
             dict(base, what=f"(2) place_tl_k_win_device, the test's window draw; {label}", placed=st["placed"],
                  unplaced=st["unplaced"], rejected=st["rejected"], **ms_fields("place_tl_k_win", c),
                  ratio_to_open=ratio(c, b)["ratio"])]
    # (3) the queries, on the timeline as the open placement left it
    e.load_timeline(tline)
    e.place_tl_k_device(*cols, nk, on, os_, kmax)
    r0, r1, r2 = (torch.empty((jobs.j, 10), dtype=torch.int32, device=dev) for _ in range(3))
    q = {"plain": lambda: e.when_k_device(*cols, nk, r0, on, kmax),
         "open": lambda: e.when_k_win_device(*cols, nk, None, None, r1, wn, kmax),
         "drawn": lambda: e.when_k_win_device(*cols, nk, dnb, ddl, r2, dn, kmax)}
    for f in q.values():
        f()
    t = {k: [] for k in q}
    for _ in range(5):
        for k, f in q.items():
            t[k].append(f())
    assert torch.equal(r0, r1) and torch.equal(on, wn), "open windows differ from fit_when_k"
    codes = r2.cpu().numpy().view(ETA_K_DTYPE).reshape(-1)["code"]
    lines.append(dict(base, what=f"(3) when_k_win_device against when_k_device; {label}", results_equal=True,
                      **ms_fields("when_k_win_open", t["open"]), **ms_fields("when_k", t["plain"]),
                      **ratio(t["open"], t["plain"]), **ms_fields("when_k_win_drawn", t["drawn"]),
                      drawn_ratio_to_open=ratio(t["drawn"], t["open"])["ratio"],
                      drawn_codes={str(c): int(n) for c, n in zip(*np.unique(codes, return_counts=True))}))
    return lines


def summarise_ab(path):
    """The unwindowed tools at the parent commit and at this one: per tool line, the parent's band
    over its runs and the new median against it."""
    runs = [json.loads(s) for s in open(path) if s.strip()]
    out = []
    for what in sorted({r["what"] for r in runs}):
        key = "place_tl_k_ms_median_of_5" if "place_tl_k" in what else "when_k_ms_median_of_5"
        parent = [r[key] for r in runs if r["what"] == what and r["side"] == "parent"]
        new = [r[key] for r in runs if r["what"] == what and r["side"] == "new"]
        if not parent or not new:
            continue
        out.append({"what": "unwindowed, parent commit against this one: " + what, "metric": key,
                    "parent_medians": parent, "parent_band": [min(parent), max(parent)], "new_medians": new,
                    "new_inside_parent_band": all(min(parent) <= v <= max(parent) for v in new),
                    # signed distance of each new median from the band, in percent of the band's nearer edge
                    "new_outside_by_pct": [round(100 * (v - max(parent)) / max(parent), 2) if v > max(parent) else
                                           round(100 * (v - min(parent)) / min(parent), 2) if v < min(parent) else 0.0
                                           for v in new]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "win_tl_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--ab", default=None, help="JSON lines of the unwindowed tools at the parent and at this commit")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    import _win_tl_cases as wc
    from fitgpu import Engine, synth
    nodes, tline, jobs, parts = synth.make_c5(a.nodes, 16384)
    wide = synth.gen_jobs(synth.SEEDS["c5"], 16384, parts.p, multi_node=True)
    H, L = int(tline.slots), int(tline.slot_min)
    lines = []
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        for label, jb, kmax in (("nodes_k = 1", jobs, 1), ("nodes_k as C4", wide, 8)):
            nb, dl = wc.draw_windows(jb, H, L, 900 + H)
            lines += measure(e, label, tline, jb, kmax, nb, dl)
    for ln in lines:
        ln.update(nodes=nodes.n, slots=H)
    if a.ab:
        lines += summarise_ab(a.ab)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

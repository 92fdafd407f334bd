"""Dev tool: the k_engine ms and step ms of the runs of a paired A/B.
tools/ab_lines.py DIR TAG WORKLOAD RUNS ARM...  reads DIR/<tag>_<workload>_<arm>_<i>.json, the bench.py
line of run i of each arm (i = 1..RUNS)."""
import json
import os
import statistics
import sys

out, tag, w, n, arms = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5:]
med = {}
for a in arms:
    ks = [json.load(open(os.path.join(out, f"{tag}_{w}_{a}_{i}.json"))) for i in range(1, n + 1)]
    km = [d["kernels"][d["roofline"]["kernel"]]["ms_per_launch"] for d in ks]
    med[a] = (statistics.median(km), max(km) - min(km))
    print(f"{w:4s} {a:7s} kernel ms", km, "step ms", [d["ms_per_step"] for d in ks],
          "rounds", ks[0].get("rounds_per_step"), "stops", ks[0].get("round_stops_per_step"))
if len(arms) == 2:
    (m0, s0), (m1, s1) = med[arms[0]], med[arms[1]]
    print(f"     medians {m0:.4f} -> {m1:.4f} ({m1 - m0:+.4f} ms, {100 * (m1 - m0) / m0:+.2f} %), "
          f"margin 3 x {max(s0, s1):.4f} = {3 * max(s0, s1):.4f}")

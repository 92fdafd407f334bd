"""fit_free_tl on the MI355X: one JSON line, written to profiles/free_tl_bench.json
(and printed).

Config C5 as tools/advance_tl_bench.py sets it up (100k nodes, 16 partitions, 1,024 slots of 5 min),
after fit_place_tl_k_device of its first 16,384 jobs with nodes_k drawn as config C4 draws it (kmax 8):
the state S.  Device ms is fit_free_tl_ms (HIP events on the context's stream) of fit_free_tl_device
for parts = 16: one warm-up call, then the median of 5 with min and max.  The call is read-only, so
every timed call sees S.
The yardstick is the only route there was without the call, timed in the same run on the host clock:
fit_read_timeline (3 x n x H int32 to the host) plus the numpy reduction of the dense timeline, the
restatement of §2k (tests/_free_tl_cases.ref_free_tl, partition by partition over its members).  What
is asserted, once per run, is that the rows of the call equal that reduction byte for byte.
list_bytes is what the call must read: 96 B per header plus 16 B per run beyond the header's four;
out_bytes the rows it writes.  --chunks times the walk at other node counts per workgroup
(FIT_FREE_CHUNK), 0 = the library's choice.

    python tools/free_tl_bench.py [--out profiles/free_tl_bench.json] [--nodes N] [--chunks 0,64,256]
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
PARTS = 16
FIELDS = ("cpu", "mem", "gpu", "wall")
HBM_PEAK = 8.0e12  # bytes/s, MI355X


def stat3(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)


def ref_free_tl(tl, mask, parts, dtype):
    """§2k on the dense [n, H, 3] timeline, one partition's members at a time."""
    H = tl.shape[1]
    out = np.zeros((parts, H), dtype)
    out["max_cpu"] = out["max_mem"] = out["max_gpu"] = -1
    for p in range(parts):
        sub = tl[((mask.astype(np.int64) >> p) & 1) != 0]   # [m, H, 3]
        if not len(sub):
            continue
        is_open = (sub >= 0).all(axis=2)[:, :, None]
        out["nodes"][p] = is_open[:, :, 0].sum(axis=0)
        s = np.where(is_open, sub, 0).sum(axis=0, dtype=np.int64)
        x = np.where(is_open, sub, -1).max(axis=0)
        for c, f in enumerate(("cpu", "mem", "gpu")):
            out[f][p] = s[:, c]
            out["max_" + f][p] = x[:, c]
    return out


def run_counts(dense):
    cnt = np.ones(dense.shape[0], np.int64)
    for lo in range(0, dense.shape[0], 8192):  # in blocks: the comparison's temporaries stay small
        d = dense[lo:lo + 8192]
        cnt[lo:lo + 8192] += (d[:, 1:] != d[:, :-1]).any(axis=2).sum(axis=1)
    return cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "free_tl_bench.json"))
    ap.add_argument("--nodes", type=int, default=None, help="truncate C5 (a rehearsal; the record is the full size)")
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", default="", help="comma-separated FIT_FREE_CHUNK values to time as well")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP runtime starts before the engine's, as in bench.py
    torch.cuda.init()
    dev = "cuda:0"
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    from fitgpu import FREE_DTYPE, Engine, synth
    nodes, tline, jobs, parts = synth.make_c5(a.nodes, a.jobs)
    jobs = synth.gen_jobs(synth.SEEDS["c5"], a.jobs, parts.p, multi_node=True)
    J, H, L, n = jobs.j, int(tline.slots), int(tline.slot_min), nodes.n
    dnodes = [T(x) for x in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min,
                             nodes.part_mask.view(np.int32))]
    dtl = [T(x) for x in (tline.off, tline.slot, tline.cpu, tline.mem, tline.gpu)]
    with Engine(device=0) as e:
        e.load_nodes_device(*dnodes)
        e.load_partitions(parts)
        e.load_timeline_device(H, L, *dtl)
        cols = [T(getattr(jobs, f)) for f in FIELDS]
        part, nk = T(jobs.part.view(np.int16)), T(jobs.nodes_k.view(np.int16))
        on = torch.empty((J, KMAX), dtype=torch.int32, device=dev)
        os_ = torch.empty(J, dtype=torch.int32, device=dev)
        st = e.place_tl_k_device(*cols, part, nk, on, os_, KMAX)
        rows = torch.empty(PARTS * H * 5, dtype=torch.int64, device=dev)

        def timed(chunk=0):
            if chunk:
                os.environ["FIT_FREE_CHUNK"] = str(chunk)
            else:
                os.environ.pop("FIT_FREE_CHUNK", None)
            ms = [e.free_tl_device(PARTS, rows) for _ in range(a.reps + 1)]  # the first is the warm-up
            os.environ.pop("FIT_FREE_CHUNK", None)
            return stat3(ms[1:])

        ms = timed()
        sweep = {str(c): timed(c)[0] for c in (int(x) for x in a.chunks.split(",") if x)}
        got = rows.cpu().numpy().view(FREE_DTYPE).reshape(PARTS, H)
        host = []
        for _ in range(2):  # the host entry point: the same launches plus the rows' copy
            t0 = time.perf_counter()
            got_host = e.free_tl(PARTS)
            host.append((time.perf_counter() - t0) * 1e3)
        # the yardstick: the dense read-back and the reduction on the host
        t0 = time.perf_counter()
        S = e.read_timeline()
        t1 = time.perf_counter()
        want = ref_free_tl(S, nodes.part_mask, PARTS, FREE_DTYPE)
        t2 = time.perf_counter()
        assert got.tobytes() == want.tobytes(), "the rows differ from the restatement of §2k"
        assert got_host.tobytes() == want.tobytes(), "the host entry point's rows differ"
        cnt = run_counts(S)
        member = nodes.part_mask != 0
        list_bytes = int(96 * member.sum() + 16 * np.maximum(cnt[member] - 4, 0).sum())
        out_bytes = PARTS * H * FREE_DTYPE.itemsize
        yard = (t2 - t0) * 1e3
        bps = list_bytes / (ms[0] * 1e-3)
        line = {"parts": PARTS, "free_tl_ms_median_of_%d" % a.reps: ms[0], "free_tl_ms_min": ms[1],
                "free_tl_ms_max": ms[2], "free_tl_host_entry_ms": round(min(host), 4),
                "read_timeline_ms": round((t1 - t0) * 1e3, 2), "numpy_reduce_ms": round((t2 - t1) * 1e3, 2),
                "yardstick_ms": round(yard, 2), "ratio_to_yardstick": round(ms[0] / yard, 7),
                "list_bytes": list_bytes, "out_bytes": out_bytes, "gbytes_per_s": round(bps / 1e9, 1),
                "fraction_of_hbm_peak": round(bps / HBM_PEAK, 4), "chunk_sweep_ms": sweep,
                "runs_in_S": int(cnt[member].sum()), "lists_over_4_runs": int((cnt[member] > 4).sum()),
                "longest_list": int(cnt.max()), "open_nodes_slot0": int(want["nodes"][:, 0].sum()),
                "checked_against_restatement": True, "nodes": n, "slots": H, "queue": J,
                "placed_in_S": int(st["placed"])}
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

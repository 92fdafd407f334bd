"""One fixed pass over every GPU-touching public entry point of libfitgpu.so, for comparing the
HIP calls two builds of the host engine make (profiles/host_fold_hiptrace.txt).

    rocprofv3 --hip-trace --stats --output-format csv -d DIR -o run -- python tools/host_fold_trace.py
    python tools/host_fold_trace.py --table DIR [DIR ...]    # per-API call counts of finished runs

FITGPU_LIB selects the build (fitgpu/_lib.py).  The pass runs twice on the same contexts, so the
second time every buffer is warm; the sizes are those of tests/test_device_entry_gpu.py (k_small,
the engine, a nodes_k column, the backfill).  Everything is sequential and single-threaded: the
number of HIP calls is a function of the library alone."""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slurm-bridge-operator_amd"), os.path.join(ROOT, "tests")]

APIS = ("hipMemcpyAsync", "hipMemsetAsync", "hipLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel",
        "hipStreamSynchronize", "hipEventRecord", "hipMalloc", "hipHostMalloc", "hipFree", "hipHostFree",
        "hipMemcpy", "hipEventQuery", "hipEventElapsedTime", "hipStreamWaitEvent")


def one_pass(e, et, ea):
    from _devarray import DevArray
    from fitgpu import ETA_DTYPE, WHY_DTYPE, Admitter, synth
    dev = lambda obj, fields: [DevArray(np.ascontiguousarray(getattr(obj, f))) for f in fields]  # noqa: E731
    NODE_F = ("cpu_free", "mem_free", "gpu_free", "avail_min", "part_mask")
    JOB_F = ("cpu", "mem", "gpu", "wall", "part")
    for name, n, j, kmax in (("c2", 64, 100, 1), ("c2", 64, 1024, 1), ("c4", 256, 1024, 8)):
        nodes, jobs, parts = synth.make_config(name, n, j)
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.place(jobs, kmax=kmax)
        e.read_nodes()
        e.partition_free(0)
        e.explain(jobs)
        e.load_nodes_device(*dev(nodes, NODE_F))
        cols, k = dev(jobs, JOB_F), DevArray(jobs.nodes_k)
        e.place_device(*cols, k if kmax > 1 else None, DevArray(np.zeros((j, kmax), np.int32)), kmax=kmax)
        e.explain_device(*cols, k, DevArray(np.zeros(j, WHY_DTYPE)))
    nodes, tline, jobs, parts = synth.make_c5(256, 4096)
    et.load_nodes(nodes)
    et.load_partitions(parts)
    et.load_timeline(tline)
    et.when(jobs)
    et.place_tl(jobs)
    et.read_timeline()
    et.load_nodes_device(*dev(nodes, NODE_F))
    et.load_timeline_device(tline.slots, tline.slot_min, *dev(tline, ("off", "slot", "cpu", "mem", "gpu")))
    cols = dev(jobs, JOB_F)
    et.when_device(*cols, DevArray(np.zeros(jobs.j, ETA_DTYPE)))
    et.place_tl_device(*cols, DevArray(np.zeros(jobs.j, np.int32)), DevArray(np.zeros(jobs.j, np.int32)))
    # the admitter (admit.cpp) drives the same engine: one request per batch (no wait, one caller)
    nodes, jobs, parts = synth.make_config("c2", 64, 100)
    ea.load_partitions(parts)
    ea.load_nodes(nodes)
    ea.place(jobs)  # k_small, the batch in the kernel arguments
    # at most 2,048 live jobs under the production choice: the host-driven rounds, plain and backfill
    n2, j2, p2 = synth.make_config("c2", 64, 1024)
    ea.load_nodes(n2)
    ea.place(j2)
    n5, t5, j5, p5 = synth.make_c5(256, 1024)
    ea.load_partitions(p5)
    ea.load_nodes(n5)
    ea.load_timeline(t5)
    ea.place_tl(j5)
    ea.load_partitions(parts)
    with Admitter(ea, max_batch=8, max_wait_us=0) as a:
        a.load_nodes(nodes)
        req = (0, int(jobs.cpu[0]), int(jobs.mem[0]), int(jobs.gpu[0]), int(jobs.wall[0]), int(jobs.part[0]), 1)
        a.explain([req])
        ticket = a.admit(*req)[4]
        a.partition_free(0)
        if ticket > 0:
            a.release(ticket)


def run():
    from fitgpu import Engine
    os.environ.setdefault("FIT_ENGINE", "persistent")  # the engine choice of the GPU tests
    with Engine(device=0) as e, Engine(device=0) as et:
        os.environ.pop("FIT_ENGINE")
        with Engine(device=0) as ea:  # the production choice: k_small for the small batches
            e.set_watchdog_us(0)
            for _ in range(2):
                one_pass(e, et, ea)
    print("host_fold_trace ok")


def table(dirs):
    for d in dirs:
        counts = {}
        for path in glob.glob(os.path.join(d, "**", "*hip_api_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                counts[row["Name"]] = counts.get(row["Name"], 0) + int(row["Calls"])
        print(f"# {d}")
        for api in sorted(counts):
            mark = "*" if api in APIS else " "
            print(f"{mark} {api:36s} {counts[api]}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        table(sys.argv[2:])
    else:
        run()

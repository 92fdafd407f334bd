"""fitgpu — MI355X-native batched job→node placement for slurm-bridge-operator.

Python face of libfitgpu.so (C-ABI: include/fitgpu.h).  The names mirror the reference's Go
functions on the resource-fit path so the tests read like the reference's own:

    ParseDuration                 pkg/slurm-agent/parse.go:36-109
    parse_resources               parse.go:111-190          (parseResources)
    parse_nodes                   slurm.go:343-364 + parse.go:291-308 (Client.Nodes/parseNode)
    parse_partition               parse.go:278-289          (parsePartition)
    parse_partitions_names        parse.go:192-210          (parsePartitionsNames)
    extract_batch_resources       pkg/slurm-bridge-operator/parse.go:30-69
    apply_spec                    pod.go:70-107             (setRequireResourceBySpec + defaults)
    parse_array_len               parse.go:126-135          (parseArrayLen)
    gen_resource_list_for_pod     pod.go:143-162            (genResourceListForPod)
    get_partition_capacity        pkg/slurm-virtual-kubelet/node.go:169-199
    Engine.place                  the fit decision the reference leaves to kube-scheduler/slurmctld

Every compute call goes through the HIP library; nothing here computes a placement.
"""
from __future__ import annotations

import ctypes as C
import threading
import weakref
from dataclasses import dataclass

import numpy as np

from ._lib import (FIT_E_PARSE, FIT_E_STATE, FIT_FLAG_COLLECTIVES, FIT_E_UNLIMITED, FIT_REJECTED, FIT_REQ_ARRAY,
                   FIT_SHARD_AUTO,
                   FIT_SHARD_COMPONENTS, FIT_SHARD_NODES, FIT_TABLE_PIN, FIT_TABLE_STATE, FIT_UNPLACED, FIT_XCHG_ALLGATHER_U64,
                   FIT_XCHG_MAX_I32, FIT_XCHG_MIN_I32, FIT_XCHG_MIN_U64, XCHG_FN, FitAdmitReq, FitAdmitRes, FitError,
                   FitJobResources, FitNode, FitNodeTable, FitOpts, FitPodLabels, FitResources, FitStats, check, lib,
                   FIT_WHY_FITS, FIT_WHY_LIMIT_CPUS, FIT_WHY_LIMIT_MEM, FIT_WHY_LIMIT_TIME, FIT_WHY_NO_NODES,
                   FIT_WHY_PARTITION, FIT_WHY_RESOURCES, FitWhy,
                   FIT_ETA_HORIZON, FIT_ETA_WINDOW, FIT_ETA_LATER, FIT_ETA_LIMIT_CPUS, FIT_ETA_LIMIT_MEM, FIT_ETA_LIMIT_TIME,
                   FIT_ETA_NO_NODES, FIT_ETA_NOW, FIT_ETA_PARTITION, FitEta, FitEtaK, FIT_MAX_K,
                   FIT_ROOM_LIMIT_CPUS, FIT_ROOM_LIMIT_MEM, FIT_ROOM_LIMIT_TIME, FIT_ROOM_NO_NODES, FIT_ROOM_NONE,
                   FIT_ROOM_PARTITION, FIT_ROOM_SOME, FIT_ROOM_UNBOUNDED, FitRoom,
                   FIT_HOLD_HELD, FIT_HOLD_REFUSED, FIT_HOLD_SKIPPED, FitFree,
                   FIT_PRE_EVICT, FIT_PRE_FITS, FIT_PRE_LIMIT_CPUS, FIT_PRE_LIMIT_MEM, FIT_PRE_LIMIT_TIME,
                   FIT_PRE_NO_NODES, FIT_PRE_NONE, FIT_PRE_PARTITION, FitEvict, FitEvictK)

__all__ = [
    "Engine", "FitError", "ErrDurationIsUnlimited", "ParseDuration", "parse_resources", "parse_nodes",
    "parse_partition", "parse_partitions_names", "extract_batch_resources", "apply_spec",
    "parse_array_len", "gen_resource_list_for_pod", "job_demand", "get_partition_capacity",
    "FIT_UNPLACED", "FIT_REJECTED", "Resources", "Node", "JobResources", "TorchHostExchange",
    "FIT_SHARD_AUTO", "FIT_SHARD_NODES", "FIT_SHARD_COMPONENTS", "expand_hostlist", "ingest_nodes",
    "FIT_FLAG_COLLECTIVES", "Admitter", "array_tasks", "pod_demand", "script_with_nodelist",
    "partition_limits", "node_columns", "POD_LABEL_KEYS", "node_names", "set_max_array_size", "FIT_TABLE_STATE",
    "FIT_TABLE_PIN", "why_message", "WHY_DTYPE", "FIT_WHY_FITS", "FIT_WHY_PARTITION", "FIT_WHY_LIMIT_TIME",
    "FIT_WHY_LIMIT_CPUS", "FIT_WHY_LIMIT_MEM", "FIT_WHY_NO_NODES", "FIT_WHY_RESOURCES",
    "when_message", "ETA_DTYPE", "FIT_ETA_NOW", "FIT_ETA_PARTITION", "FIT_ETA_LIMIT_TIME", "FIT_ETA_LIMIT_CPUS",
    "FIT_ETA_LIMIT_MEM", "FIT_ETA_NO_NODES", "FIT_ETA_LATER", "FIT_ETA_HORIZON",
    "FIT_ETA_WINDOW", "when_k_win_message",
    "when_k_message", "ETA_K_DTYPE", "FitEtaK", "FIT_MAX_K",
    "room_message", "ROOM_DTYPE", "FitRoom", "FIT_ROOM_SOME", "FIT_ROOM_PARTITION", "FIT_ROOM_LIMIT_TIME",
    "FIT_ROOM_LIMIT_CPUS", "FIT_ROOM_LIMIT_MEM", "FIT_ROOM_NO_NODES", "FIT_ROOM_NONE", "FIT_ROOM_UNBOUNDED",
    "FIT_HOLD_HELD", "FIT_HOLD_REFUSED", "FIT_HOLD_SKIPPED",
    "free_message", "FREE_DTYPE", "FitFree",
    "preempt_message", "EVICT_DTYPE", "FitEvict", "preempt_k_message", "EVICT_K_DTYPE", "FitEvictK", "FIT_PRE_FITS", "FIT_PRE_PARTITION", "FIT_PRE_LIMIT_TIME",
    "FIT_PRE_LIMIT_CPUS", "FIT_PRE_LIMIT_MEM", "FIT_PRE_NO_NODES", "FIT_PRE_EVICT", "FIT_PRE_NONE",
]


class ErrDurationIsUnlimited(Exception):
    """pkg/slurm-agent/slurm.go:49 — the duration field has value UNLIMITED (or is empty)."""


def _ptr(a) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


# ------------------------------------------------------------------------------- ingest
def ParseDuration(s: str) -> int:
    """Duration in nanoseconds; raises ErrDurationIsUnlimited / ValueError like the Go errors."""
    ns = C.c_int64()
    rc = lib().fit_parse_duration(s.encode(), C.byref(ns))
    if rc == FIT_E_UNLIMITED:
        raise ErrDurationIsUnlimited(s)
    if rc == FIT_E_PARSE:
        raise ValueError(f"invalid duration {s!r}")
    check(rc, "fit_parse_duration")
    return ns.value


@dataclass
class Resources:  # pkg/slurm-agent/slurm.go:104-110 (Features unused on this path)
    Nodes: int
    MemPerNode: int
    CPUPerNode: int
    WallTime: int  # ns, -1 = UNLIMITED


def parse_resources(text: str) -> Resources:
    r = FitResources()
    rc = lib().fit_parse_resources(text.encode(), C.byref(r))
    if rc == FIT_E_PARSE:
        raise ValueError("could not parse partition resources")
    check(rc, "fit_parse_resources")
    return Resources(r.nodes, r.mem_per_node, r.cpu_per_node, r.wall_ns)


@dataclass
class Node:  # pkg/slurm-agent/slurm.go:113-121
    Cpus: int
    Memory: int
    Gpus: int
    AlloCpus: int
    AlloMemory: int
    AlloGpus: int


def parse_nodes(text: str, cap: int | None = None) -> list[Node]:
    cap = cap if cap is not None else text.count("\n\n") + 2
    arr = (FitNode * max(cap, 1))()
    n = check(lib().fit_parse_nodes(text.encode(), arr, cap), "fit_parse_nodes")
    return [Node(a.cpus, a.memory, a.gpus, a.allo_cpus, a.allo_memory, a.allo_gpus) for a in arr[:n]]


def _names(fn, text: str) -> list[str]:
    buflen = len(text.encode()) * 2 + 64
    buf = C.create_string_buffer(buflen)
    n = check(fn(text.encode(), buf, buflen), fn.__name__)
    return [s.decode() for s in buf.raw.split(b"\0")[:n]]


def parse_partition(text: str) -> list[str]:
    return _names(lib().fit_parse_partition, text)


def parse_partitions_names(text: str) -> list[str]:
    return _names(lib().fit_parse_partitions_names, text)


def expand_hostlist(expr: str) -> list[str]:
    """Slurm hostlist expansion (fixes parsePartition's split, parse.go:278-289)."""
    buflen = 1 << 16
    while True:
        buf = C.create_string_buffer(buflen)
        n = lib().fit_expand_hostlist(expr.encode(), buf, buflen)
        if n == FIT_E_PARSE:
            raise ValueError(f"malformed hostlist {expr!r}")
        if n >= 0:
            return [x.decode() for x in buf.raw.split(b"\0")[:n]]
        if buflen > 1 << 28:
            check(n, "fit_expand_hostlist")
        buflen *= 16


def node_names(entries: list[str]) -> list[str]:
    """The Partition RPC's node list (parsePartition's comma split, parse.go:278-289) → the expanded
    node names to send to the Nodes RPC, one engine row each (fit_node_names)."""
    blob = b"".join(e.encode() + b"\0" for e in entries)
    buflen = 1 << 16
    while True:
        buf = C.create_string_buffer(buflen)
        n = lib().fit_node_names(blob, len(entries), buf, buflen)
        if n == FIT_E_PARSE:
            raise ValueError(f"malformed hostlist or a node name listed twice: {entries!r}")
        if n >= 0:
            return [x.decode() for x in buf.raw.split(b"\0")[:n]]
        if buflen > 1 << 28:
            check(n, "fit_node_names")
        buflen *= 16


def release_events(n: int, jobs: list, slots: int, slot_min: int):
    """Release events for Engine.load_timeline from running jobs (fit_release_events): ``jobs`` is a
    list of (node rows, minutes left, cpu, mem MiB, gpus); returns a synth.Timeline."""
    from .synth import Timeline
    m = len(jobs)
    off = np.zeros(m + 1, np.int32)
    for i, j in enumerate(jobs):
        off[i + 1] = off[i] + len(j[0])
    nodes = np.array([x for j in jobs for x in j[0]], np.int32)
    rem = np.array([j[1] for j in jobs], np.int64)
    cols = [np.array([j[k] for j in jobs], np.int32) for k in (2, 3, 4)]
    e = int(off[-1])
    out = [np.zeros(n + 1, np.int32)] + [np.zeros(max(e, 1), np.int32) for _ in range(4)]
    r = lib().fit_release_events(n, m, _ptr(off), _ptr(nodes) if e else None, _ptr(rem), *[_ptr(c) for c in cols],
                                 slots, slot_min, *[_ptr(o) for o in out], e)
    check(r, "fit_release_events")
    return Timeline(slots=slots, slot_min=slot_min, off=out[0], slot=out[1][:r], cpu=out[2][:r],
                    mem=out[3][:r], gpu=out[4][:r])


def ingest_nodes(text: str, partitions: list[str]):
    """`scontrol show nodes` text → (synth.Nodes columns for Engine.load_nodes, node names)
    (Client.Nodes + parseNode, slurm.go:354-363 / parse.go:291-308, plus Gres,
    GresUsed, State, Partitions, NodeName)."""
    from .synth import Nodes
    cap = text.count("\n\n") + 2
    cols = [np.empty(cap, np.int32) for _ in range(4)] + [np.empty(cap, np.uint32)]
    blob = b"".join(p.encode() + b"\0" for p in partitions)
    names_len = len(text.encode()) + 64
    names = C.create_string_buffer(names_len)
    n = lib().fit_ingest_nodes(text.encode(), blob, len(partitions), cap, *[_ptr(c) for c in cols], names,
                               names_len)
    if n == FIT_E_PARSE:
        raise ValueError("malformed Gres count")
    check(n, "fit_ingest_nodes")
    nodes = Nodes(*(c[:n].copy() for c in cols))
    return nodes, [x.decode() for x in names.raw.split(b"\0")[:n]]


@dataclass
class JobResources:  # apis/kubecluster.org/v1alpha1/affinity.go:40-48
    Nodes: int = 0
    CpusPerTask: int = 0
    Ntasks: int = 0
    NtasksPerNode: int = 0
    MemPerCpu: int = 0
    WallTime: int = 0
    Array: str = ""

    def _c(self) -> FitJobResources:
        r = FitJobResources()
        r.nodes, r.cpus_per_task, r.ntasks = self.Nodes, self.CpusPerTask, self.Ntasks
        r.ntasks_per_node, r.mem_per_cpu, r.wall_ns = self.NtasksPerNode, self.MemPerCpu, self.WallTime
        r.array = self.Array.encode()[:63]
        return r

    @staticmethod
    def _py(r: FitJobResources) -> "JobResources":
        return JobResources(r.nodes, r.cpus_per_task, r.ntasks, r.ntasks_per_node, r.mem_per_cpu,
                            r.wall_ns, r.array.decode())


def extract_batch_resources(script: str) -> JobResources:
    r = FitJobResources()
    rc = lib().fit_extract_batch_resources(script.encode(), C.byref(r))
    if rc == FIT_E_PARSE:
        raise ValueError("could not extract required resources")
    check(rc, "fit_extract_batch_resources")
    return JobResources._py(r)


def apply_spec(res: JobResources, nodes=0, cpus_per_task=0, mem_per_cpu=0, ntasks_per_node=0,
               array="", ntasks=0) -> JobResources:
    r = res._c()
    lib().fit_apply_spec(C.byref(r), nodes, cpus_per_task, mem_per_cpu, ntasks_per_node,
                         array.encode(), ntasks)
    return JobResources._py(r)


def parse_array_len(array: str) -> int:
    return lib().fit_array_len(array.encode())


def gen_resource_list_for_pod(res: JobResources) -> dict:
    cpu, mem = C.c_int64(), C.c_int64()
    lib().fit_pod_request(C.byref(res._c()), C.byref(cpu), C.byref(mem))
    return {"cpu": cpu.value, "memory": mem.value}


def job_demand(res: JobResources) -> tuple[int, int, int, int]:
    """(cpus per node, MiB per node, walltime minutes, nodes) — DESIGN.md §2 demand rule."""
    cpu, mem, wall, k = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint16()
    check(lib().fit_job_demand(C.byref(res._c()), C.byref(cpu), C.byref(mem), C.byref(wall),
                               C.byref(k)), "fit_job_demand")
    return cpu.value, mem.value, wall.value, k.value


def get_partition_capacity(nodes: list[Node]) -> dict:
    arr = (FitNode * max(len(nodes), 1))()
    for i, n in enumerate(nodes):
        arr[i] = FitNode(n.Cpus, n.Memory, n.Gpus, n.AlloCpus, n.AlloMemory, n.AlloGpus)
    cpu, mem, gpu, pods = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    lib().fit_partition_capacity(arr, len(nodes), C.byref(cpu), C.byref(mem), C.byref(gpu), C.byref(pods))
    out = {"cpu": cpu.value, "memory": mem.value, "pods": pods.value}
    if gpu.value > 0:
        out["nvidia.com/gpu"] = gpu.value
    return out


# ---------------------------------------------------------------- CreatePod call site
# pkg/common/labels.go:9-14, the keys newSubmitRequestForPod reads (provider.go:74-123)
POD_LABEL_KEYS = {"nodes": "sbo.kubecluster.org/nodes", "cpus_per_task": "sbo.kubecluster.org/cpus-per-task",
                  "mem_per_cpu": "sbo.kubecluster.org/mem-per-cpu",
                  "ntasks_per_node": "sbo.kubecluster.org/ntasks-per-node",
                  "array": "sbo.kubecluster.org/array", "ntasks": "sbo.kubecluster.org/ntask"}


def array_tasks(array: str) -> tuple[int, int]:
    """(distinct task ids, tasks that may run at once) of a Slurm --array expression."""
    n, r = C.c_int64(), C.c_int64()
    rc = lib().fit_array_tasks(array.encode(), C.byref(n), C.byref(r))
    if rc == FIT_E_PARSE:
        raise ValueError(f"malformed array {array!r}")
    check(rc, "fit_array_tasks")
    return n.value, r.value


def set_max_array_size(n: int) -> int:
    """Slurm's MaxArraySize for pod_demand (process-wide; default 1001); returns the previous one."""
    return check(lib().fit_set_max_array_size(n), "fit_set_max_array_size")


def pod_demand(labels: dict, script: str | None, part: int = 0, priority: int = 0) -> list[tuple]:
    """A pod's admission requests from its labels (keys of POD_LABEL_KEYS' values) and script:
    [(priority, cpu, mem_mib, gpu, wall_min, part, nodes_k, flags)] — one per array task that
    may run at once (include/fitgpu.h fit_pod_demand); flags FIT_REQ_ARRAY marks an array job's
    tasks (never pinned by Admitter.script)."""
    byname = {v: k for k, v in POD_LABEL_KEYS.items()}
    vals = {byname[k]: str(v).encode() for k, v in labels.items() if k in byname}
    lab = FitPodLabels(*(vals.get(k) for k in ("nodes", "cpus_per_task", "mem_per_cpu", "ntasks_per_node",
                                               "array", "ntasks")))
    scr = script.encode() if script is not None else None
    n = lib().fit_pod_demand(C.byref(lab), scr, part, priority, None, 0)
    if n == FIT_E_PARSE:
        raise ValueError("malformed #SBATCH header or array expression")
    check(n, "fit_pod_demand")
    out = (FitAdmitReq * n)()
    check(lib().fit_pod_demand(C.byref(lab), scr, part, priority, out, n), "fit_pod_demand")
    return [(r.priority, r.cpu, r.mem_mib, r.gpu, r.wall_min, r.part, r.nodes_k, r.flags) for r in out]


def script_with_nodelist(script: str, names: list[str], nodes: list[int]) -> str:
    """The script with `#SBATCH --nodelist=` for the engine's nodes (fit_script_with_nodelist)."""
    blob = b"".join(x.encode() + b"\0" for x in names)
    outlen = len(script.encode()) + 32 + len(blob) + 1
    buf = C.create_string_buffer(outlen)
    ids = (C.c_int32 * len(nodes))(*nodes)
    n = check(lib().fit_script_with_nodelist(script.encode(), blob, len(names), ids, len(nodes), buf, outlen),
              "fit_script_with_nodelist")
    return buf.raw[:n].decode()


def partition_limits(wall_time_s: int, cpu_per_node: int, mem_per_node: int) -> tuple[int, int, int]:
    """ResourcesResponse fields → (max_time_min, max_cpus_per_node, max_mem_per_node), -1 = none."""
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().fit_partition_limits(wall_time_s, cpu_per_node, mem_per_node, C.byref(a), C.byref(b), C.byref(c)),
          "fit_partition_limits")
    return a.value, b.value, c.value


def node_columns(nodes: list[Node], part_mask: int = 1):
    """NodesResponse rows → synth.Nodes columns (free = total − alloc) for load_nodes."""
    from .synth import Nodes
    n = len(nodes)
    arr = (FitNode * max(n, 1))()
    for i, x in enumerate(nodes):
        arr[i] = FitNode(x.Cpus, x.Memory, x.Gpus, x.AlloCpus, x.AlloMemory, x.AlloGpus)
    cols = [np.empty(max(n, 1), np.int32) for _ in range(4)] + [np.empty(max(n, 1), np.uint32)]
    check(lib().fit_node_columns(arr, n, part_mask, *[_ptr(c) for c in cols]), "fit_node_columns")
    return Nodes(*(c[:n].copy() for c in cols))


# ------------------------------------------------------------------------------- explain
# one fit_why row (include/fitgpu.h), 32 bytes: what Engine.explain / Admitter.explain return
WHY_DTYPE = np.dtype([(n, np.int32) for n, _ in FitWhy._fields_])


def why_message(row) -> str:
    """A fit_why row (an element of an explain() result, or any mapping / object with its fields)
    as one line in kube-scheduler's shape (fit_why_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    w = FitWhy(*(int(get(n)) for n, _ in FitWhy._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_why_message(C.byref(w), buf, len(buf)), "fit_why_message")
    return buf.raw[:n].decode()


# ---------------------------------------------------------------------------------- when
# one fit_eta row (include/fitgpu.h), 32 bytes: what Engine.when returns
ETA_DTYPE = np.dtype([(n, np.int32) for n, _ in FitEta._fields_])


def when_message(row) -> str:
    """A fit_eta row (an element of a when() result, or any mapping / object with its fields) as
    one line of text (fit_when_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    e = FitEta(*(int(get(n)) for n, _ in FitEta._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_when_message(C.byref(e), buf, len(buf)), "fit_when_message")
    return buf.raw[:n].decode()


# -------------------------------------------------------------------------------- when_k
# one fit_eta_k row (include/fitgpu.h), 40 bytes: what Engine.when_k returns
ETA_K_DTYPE = np.dtype([(n, np.int32) for n, _ in FitEtaK._fields_])


def when_k_message(row) -> str:
    """A fit_eta_k row (an element of a when_k() result, or any mapping / object with its fields)
    as one line of text (fit_when_k_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    e = FitEtaK(*(int(get(n)) for n, _ in FitEtaK._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_when_k_message(C.byref(e), buf, len(buf)), "fit_when_k_message")
    return buf.raw[:n].decode()


def when_k_win_message(row) -> str:
    """A fit_eta_k row of when_k_win() as one line of text (fit_when_k_win_message): FIT_ETA_WINDOW's
    own text, when_k_message's for every other code; needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    e = FitEtaK(*(int(get(n)) for n, _ in FitEtaK._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_when_k_win_message(C.byref(e), buf, len(buf)), "fit_when_k_win_message")
    return buf.raw[:n].decode()


# ---------------------------------------------------------------------------------- room
# one fit_room row (include/fitgpu.h), 40 bytes with copies as int64 at offset 16: what Engine.room /
# Admitter.room return
ROOM_DTYPE = np.dtype([(n, np.int64 if t is C.c_int64 else np.int32) for n, t in FitRoom._fields_])


def room_message(row) -> str:
    """A fit_room row (an element of a room() result, or any mapping / object with its fields) as
    one line of text (fit_room_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    r = FitRoom(*(int(get(n)) for n, _ in FitRoom._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_room_message(C.byref(r), buf, len(buf)), "fit_room_message")
    return buf.raw[:n].decode()


# ---------------------------------------------------------------------------------- free
# one fit_free row (include/fitgpu.h), 40 bytes: three int64 sums, then nodes and the three maxima:
# what Engine.free_tl returns
FREE_DTYPE = np.dtype([(n, np.int64 if t is C.c_int64 else np.int32) for n, t in FitFree._fields_])


def free_message(row) -> str:
    """A fit_free row (an element of a free_tl() result, or any mapping / object with its fields) as
    one line of text (fit_free_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    r = FitFree(*(int(get(n)) for n, _ in FitFree._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_free_message(C.byref(r), buf, len(buf)), "fit_free_message")
    return buf.raw[:n].decode()


# ---------------------------------------------------------------------------------- preempt
# one fit_evict row (include/fitgpu.h), 32 bytes of int32: what Engine.preempt returns
EVICT_DTYPE = np.dtype([(n, np.int32) for n, _ in FitEvict._fields_])


def preempt_message(row) -> str:
    """A fit_evict row (an element of a preempt() result, or any mapping / object with its fields)
    as one line of text (fit_preempt_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    r = FitEvict(*(int(get(n)) for n, _ in FitEvict._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_preempt_message(C.byref(r), buf, len(buf)), "fit_preempt_message")
    return buf.raw[:n].decode()


# -------------------------------------------------------------------------------- preempt_k
# one fit_evict_k row (include/fitgpu.h), 40 bytes of int32: what Engine.preempt_k returns
EVICT_K_DTYPE = np.dtype([(n, np.int32) for n, _ in FitEvictK._fields_])


def preempt_k_message(row) -> str:
    """A fit_evict_k row (an element of a preempt_k() result, or any mapping / object with its
    fields) as one line of text (fit_preempt_k_message); needs no device."""
    get = (lambda n: row[n]) if isinstance(row, (np.void, np.ndarray, dict)) else (lambda n: getattr(row, n))
    r = FitEvictK(*(int(get(n)) for n, _ in FitEvictK._fields_))
    buf = C.create_string_buffer(256)
    n = check(lib().fit_preempt_k_message(C.byref(r), buf, len(buf)), "fit_preempt_k_message")
    return buf.raw[:n].decode()


# ------------------------------------------------------------------------------- engine
def lock_dir() -> tuple[str, bool]:
    """fit_lock_dir: the directory of the per-GPU launch lock file and whether it is the shared
    one (FIT_LOCK_DIR, or the /var/run/fitgpu host path) rather than the /tmp fallback."""
    buf = C.create_string_buffer(4096)
    rc = lib().fit_lock_dir(buf, len(buf))
    check(rc, "fit_lock_dir")
    return buf.value.decode(), rc == 0


def nccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(lib().fit_nccl_unique_id(buf), "fit_nccl_unique_id")
    return buf.raw


class TorchHostExchange:
    """Host-side exchange over torch.distributed (e.g. gloo) for the engine's collectives.

    Lets several ranks share one GPU in tests, exercising exactly the multi-rank engine code that
    RCCL drives in production (fit_opts.exchange, include/fitgpu.h)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.fn = XCHG_FN(self._call)

    def _call(self, user, op, buf, count):
        import torch
        try:
            d = self.dist
            if op in (FIT_XCHG_ALLGATHER_U64, FIT_XCHG_MIN_U64):
                n = count * (self.world if op == FIT_XCHG_ALLGATHER_U64 else 1)
                arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int64)), shape=(n,))
                mine = arr[self.rank * count:(self.rank + 1) * count] if op == FIT_XCHG_ALLGATHER_U64 else arr
                parts = [torch.empty(count, dtype=torch.int64) for _ in range(self.world)]
                d.all_gather(parts, torch.from_numpy(mine.copy()), group=self.group)
                if op == FIT_XCHG_ALLGATHER_U64:
                    arr[:] = torch.cat(parts).numpy()
                else:
                    arr[:] = np.minimum.reduce([p.numpy().view(np.uint64) for p in parts]).view(np.int64)
            else:
                arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(count,))
                t = torch.from_numpy(arr.copy())
                d.all_reduce(t, op=d.ReduceOp.MAX if op == FIT_XCHG_MAX_I32 else d.ReduceOp.MIN, group=self.group)
                arr[:] = t.numpy()
            return 0
        except Exception:  # never let a Python exception cross the C boundary
            return -1


class Engine:
    """One placement context on one GPU (optionally one rank of a multi-GPU group)."""

    def __init__(self, device: int = -1, rank: int = 0, world: int = 1, nccl_id: bytes | None = None,
                 window_min: int = 0, window_max: int = 0, shard_mode: int = 0,
                 exchange: "TorchHostExchange | None" = None, flags: int = 0):
        self._idbuf = C.create_string_buffer(nccl_id, 128) if nccl_id else None
        self._xchg = exchange
        o = FitOpts(device, rank, world, C.cast(self._idbuf, C.c_void_p) if self._idbuf else None,
                    shard_mode, window_min, window_max, flags, exchange.fn if exchange else XCHG_FN(), None)
        h = C.c_void_p()
        check(lib().fit_create(C.byref(o), C.byref(h)), "fit_create")
        self._h = h
        self.n = 0
        self._admitters = weakref.WeakSet()  # closed before the context goes (Admitter holds it)

    def close(self):
        for a in list(getattr(self, "_admitters", ())):
            a.close()
        if getattr(self, "_h", None):
            lib().fit_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_nodes(self, nodes):
        cols = [np.ascontiguousarray(nodes.cpu_free, np.int32), np.ascontiguousarray(nodes.mem_free, np.int32),
                np.ascontiguousarray(nodes.gpu_free, np.int32), np.ascontiguousarray(nodes.avail_min, np.int32),
                np.ascontiguousarray(nodes.part_mask, np.uint32)]
        n = len(cols[0])
        check(lib().fit_load_nodes(self._h, n, *[_ptr(c) for c in cols]), "fit_load_nodes")
        self.n = n

    def load_nodes_device(self, cpu, mem, gpu, avail, mask):
        """torch tensors on this context's GPU (int32 / int32 / int32 / int32 / int32-viewed uint32)."""
        n = int(cpu.numel())
        check(lib().fit_load_nodes_device(self._h, n, *[_ptr(t) for t in (cpu, mem, gpu, avail, mask)]),
              "fit_load_nodes_device")
        self.n = n

    def set_watchdog_us(self, us: int):
        """Deadline of every device-side wait of the persistent engines (fit_set_watchdog_us);
        us <= 0 restores the default (10 s)."""
        check(lib().fit_set_watchdog_us(self._h, int(us)), "fit_set_watchdog_us")

    def load_partitions(self, parts):
        cols = [np.ascontiguousarray(a, np.int32) for a in (parts.max_time_min, parts.max_cpus_per_node,
                                                            parts.max_mem_per_node)]
        check(lib().fit_load_partitions(self._h, len(cols[0]), *[_ptr(c) for c in cols]),
              "fit_load_partitions")

    def place(self, jobs, kmax: int = 1, out=None):
        """Host arrays in, placements out[J, kmax] (an int32 array the caller may pass, e.g. pinned)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        j = len(part)
        if out is None:
            out = np.empty((j, kmax), np.int32)
        elif out.dtype != np.int32 or out.size != j * kmax or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous int32 array of J * kmax entries")
        st = FitStats()
        check(lib().fit_place(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(k), kmax, _ptr(out),
                              C.byref(st)), "fit_place")
        return out, st.as_dict()

    def place_device(self, cpu, mem, gpu, wall, part, nodes_k, out, kmax: int = 1):
        """All arguments torch tensors resident on this GPU; writes out[J*kmax]."""
        st = FitStats()
        check(lib().fit_place_device(self._h, int(cpu.numel()), _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall),
                                     _ptr(part), _ptr(nodes_k) if nodes_k is not None else None, kmax,
                                     _ptr(out), C.byref(st)), "fit_place_device")
        return st.as_dict()

    # ---- why a job does not fit ------------------------------------------
    def explain(self, jobs):
        """Every job judged alone against the current node table (fit_explain): a structured
        array of WHY_DTYPE rows (code, need, members, fit, short_*).  Changes nothing."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        out = np.zeros(len(part), WHY_DTYPE)
        check(lib().fit_explain(self._h, len(part), *[_ptr(c) for c in cols], _ptr(part), _ptr(k), _ptr(out)),
              "fit_explain")
        return out

    def explain_device(self, cpu, mem, gpu, wall, part, nodes_k, out):
        """All arguments torch tensors resident on this GPU; writes out (J rows of 8 int32, the
        fields of WHY_DTYPE in order).  Returns the device time of its launches in ms (HIP events
        on the context's stream, fit_explain_ms); 0.0 for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_explain_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall),
                                       _ptr(part), _ptr(nodes_k) if nodes_k is not None else None, _ptr(out)),
              "fit_explain_device")
        if j == 0:
            return 0.0
        ms = C.c_double()
        check(lib().fit_explain_ms(self._h, C.byref(ms)), "fit_explain_ms")
        return ms.value

    # ---- time-windowed backfill ------------------------------------------
    def load_timeline(self, tline):
        """Release events (synth.Timeline) over a horizon of tline.slots slots of tline.slot_min
        minutes, on top of the node table of the last load_nodes."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (tline.off, tline.slot, tline.cpu, tline.mem,
                                                            tline.gpu)]
        check(lib().fit_load_timeline(self._h, int(tline.slots), int(tline.slot_min), *[_ptr(c) for c in cols]),
              "fit_load_timeline")
        self.slots = int(tline.slots)

    def load_timeline_device(self, slots, slot_min, off, slot, cpu, mem, gpu):
        """torch int32 tensors on this GPU (off has n + 1 entries)."""
        check(lib().fit_load_timeline_device(self._h, int(slots), int(slot_min), _ptr(off), int(slot.numel()),
                                             *[_ptr(t) for t in (slot, cpu, mem, gpu)]), "fit_load_timeline_device")
        self.slots = int(slots)

    def place_tl(self, jobs, node=None, start=None):
        """Returns (node[J], start_slot[J], stats); node / start may be caller int32 arrays."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        j = len(part)
        node = np.empty(j, np.int32) if node is None else node
        start = np.empty(j, np.int32) if start is None else start
        for a in (node, start):
            if a.dtype != np.int32 or a.size != j or not a.flags.c_contiguous:
                raise ValueError("node / start must be contiguous int32 arrays of J entries")
        st = FitStats()
        check(lib().fit_place_tl(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(node), _ptr(start),
                                 C.byref(st)), "fit_place_tl")
        return node, start, st.as_dict()

    def place_tl_device(self, cpu, mem, gpu, wall, part, out_node, out_start):
        st = FitStats()
        check(lib().fit_place_tl_device(self._h, int(cpu.numel()), *[_ptr(t) for t in (cpu, mem, gpu, wall, part)],
                                        _ptr(out_node), _ptr(out_start), C.byref(st)), "fit_place_tl_device")
        return st.as_dict()

    # ---- when a pending job can start ------------------------------------
    def when(self, jobs):
        """Every job judged alone against the current timeline (fit_when): a structured array of
        ETA_DTYPE rows (code, dur, start, node, wait_min, members, hosts, now).  Changes nothing;
        jobs.nodes_k plays no part (a backfill job takes one node)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        out = np.zeros(len(part), ETA_DTYPE)
        check(lib().fit_when(self._h, len(part), *[_ptr(c) for c in cols], _ptr(part), _ptr(out)), "fit_when")
        return out

    def when_device(self, cpu, mem, gpu, wall, part, out):
        """All arguments torch tensors resident on this GPU; writes out (J rows of 8 int32, the
        fields of ETA_DTYPE in order).  Returns the device time of its launches in ms (HIP events
        on the context's stream, fit_when_ms); 0.0 for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_when_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part), _ptr(out)),
              "fit_when_device")
        if j == 0:
            return 0.0
        ms = C.c_double()
        check(lib().fit_when_ms(self._h, C.byref(ms)), "fit_when_ms")
        return ms.value

    # ---- when a multi-node job can start ---------------------------------
    def when_k(self, jobs, kmax: int | None = None):
        """Every job judged alone against the current timeline as a job of jobs.nodes_k nodes
        (fit_when_k): (rows, nodes) — a structured array of ETA_K_DTYPE rows (code, dur, need,
        start, wait_min, members, hosts, now, ready, reserved) and nodes[J, kmax], the job's nodes
        in key order for a NOW / LATER row, -1 elsewhere.  kmax None: the largest nodes_k of the
        batch (at least 1).  Changes nothing."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        j = len(part)
        if kmax is None:
            kmax = max(1, int(k.max())) if j else 1
        out = np.zeros(j, ETA_K_DTYPE)
        nodes = np.full((j, max(int(kmax), 0)), -1, np.int32)
        check(lib().fit_when_k(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(k), int(kmax), _ptr(out),
                               _ptr(nodes)), "fit_when_k")
        return out, nodes

    def when_k_device(self, cpu, mem, gpu, wall, part, nodes_k, out, out_node, kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k may be None = all 1); writes
        out (J rows of 10 int32, the fields of ETA_K_DTYPE in order) and out_node (J * kmax int32).
        Returns the device time of its launches in ms (HIP events on the context's stream,
        fit_when_k_ms); 0.0 for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_when_k_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part),
                                      _ptr(nodes_k) if nodes_k is not None else None, int(kmax), _ptr(out),
                                      _ptr(out_node)), "fit_when_k_device")
        if j == 0:
            return 0.0
        ms = C.c_double()
        check(lib().fit_when_k_ms(self._h, C.byref(ms)), "fit_when_k_ms")
        return ms.value

    # ---- priority-order backfill of multi-node jobs ------------------------
    def place_tl_k(self, jobs, kmax: int | None = None):
        """The queue in index order, each job of jobs.nodes_k nodes reserved on the timeline as the
        jobs before it left it (fit_place_tl_k): (nodes[J, kmax], start[J], stats).  A placed job's
        nodes in key order, -1 elsewhere; nodes[q, 0] = FIT_REJECTED for a rejected job; start -1
        when not placed.  kmax None: the largest nodes_k of the batch (at least 1)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        j = len(part)
        if kmax is None:
            kmax = max(1, int(k.max())) if j else 1
        nodes = np.full((j, max(int(kmax), 0)), -1, np.int32)
        start = np.full(j, -1, np.int32)
        st = FitStats()
        check(lib().fit_place_tl_k(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(k), int(kmax), _ptr(nodes),
                                   _ptr(start), C.byref(st)), "fit_place_tl_k")
        return nodes, start, st.as_dict()

    def place_tl_k_device(self, cpu, mem, gpu, wall, part, nodes_k, out_node, out_start, kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k may be None = all 1); writes
        out_node (J * kmax int32) and out_start (J int32).  Returns the stats."""
        st = FitStats()
        check(lib().fit_place_tl_k_device(self._h, int(cpu.numel()), _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall),
                                          _ptr(part), _ptr(nodes_k) if nodes_k is not None else None, int(kmax),
                                          _ptr(out_node), _ptr(out_start), C.byref(st)), "fit_place_tl_k_device")
        return st.as_dict()

    # ---- begin and deadline per job -----------------------------------------
    @staticmethod
    def _win_col(a, j, name):
        """An optional window column from host memory: None, or J contiguous int32."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.int32)
        if a.shape != (j,):
            raise ValueError(f"{name} must have one entry per job")
        return a

    def when_k_win(self, jobs, not_before=None, deadline=None, kmax: int | None = None):
        """when_k with a window of allowed starts per job (fit_when_k_win): not_before[J] and
        deadline[J] in slots, either None (all 0 / none); a start s is allowed when
        clamp(not_before, 0, H) <= s and s + dur <= clamp(deadline, 0, H).  Returns (rows, nodes) as
        when_k; a job without a start inside a window that is not the whole range has code
        FIT_ETA_WINDOW.  Changes nothing."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        j = len(part)
        nb, dl = self._win_col(not_before, j, "not_before"), self._win_col(deadline, j, "deadline")
        if kmax is None:
            kmax = max(1, int(k.max())) if j else 1
        out = np.zeros(j, ETA_K_DTYPE)
        nodes = np.full((j, max(int(kmax), 0)), -1, np.int32)
        check(lib().fit_when_k_win(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(k), int(kmax),
                                   _ptr(nb) if nb is not None else None, _ptr(dl) if dl is not None else None,
                                   _ptr(out), _ptr(nodes)), "fit_when_k_win")
        return out, nodes

    def when_k_win_device(self, cpu, mem, gpu, wall, part, nodes_k, not_before, deadline, out, out_node,
                          kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k, not_before, deadline may each be
        None); writes out and out_node as when_k_device.  Returns the device time of its launches in
        ms (fit_when_k_win_ms); 0.0 for no jobs."""
        j = int(cpu.numel())
        opt = lambda t: _ptr(t) if t is not None else None  # noqa: E731
        check(lib().fit_when_k_win_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part),
                                          opt(nodes_k), int(kmax), opt(not_before), opt(deadline), _ptr(out),
                                          _ptr(out_node)), "fit_when_k_win_device")
        if j == 0:
            return 0.0
        ms = C.c_double()
        check(lib().fit_when_k_win_ms(self._h, C.byref(ms)), "fit_when_k_win_ms")
        return ms.value

    def place_tl_k_win(self, jobs, not_before=None, deadline=None, kmax: int | None = None):
        """place_tl_k with when_k_win's window per job (fit_place_tl_k_win): (nodes[J, kmax],
        start[J], stats) as place_tl_k.  A job without an allowed start is unplaced and consumes
        nothing."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        j = len(part)
        nb, dl = self._win_col(not_before, j, "not_before"), self._win_col(deadline, j, "deadline")
        if kmax is None:
            kmax = max(1, int(k.max())) if j else 1
        nodes = np.full((j, max(int(kmax), 0)), -1, np.int32)
        start = np.full(j, -1, np.int32)
        st = FitStats()
        check(lib().fit_place_tl_k_win(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(k), int(kmax),
                                       _ptr(nb) if nb is not None else None, _ptr(dl) if dl is not None else None,
                                       _ptr(nodes), _ptr(start), C.byref(st)), "fit_place_tl_k_win")
        return nodes, start, st.as_dict()

    def place_tl_k_win_device(self, cpu, mem, gpu, wall, part, nodes_k, not_before, deadline, out_node, out_start,
                              kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k, not_before, deadline may each be
        None); writes out_node (J * kmax int32) and out_start (J int32).  Returns the stats."""
        st = FitStats()
        opt = lambda t: _ptr(t) if t is not None else None  # noqa: E731
        check(lib().fit_place_tl_k_win_device(self._h, int(cpu.numel()), _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall),
                                              _ptr(part), opt(nodes_k), int(kmax), opt(not_before), opt(deadline),
                                              _ptr(out_node), _ptr(out_start), C.byref(st)),
              "fit_place_tl_k_win_device")
        return st.as_dict()

    # ---- hand reservations back to the timeline ----------------------------
    def unplace_tl(self, jobs, node, start, kmax: int | None = None):
        """Add the rows' demand windows back to the current timeline (fit_unplace_tl): jobs as given
        to place_tl_k / place_tl, node[J, kmax] (or node[J] at kmax 1) and start[J] as they came
        back; rows with start < 0 are skipped, so a placement's outputs go in verbatim.  kmax None:
        node's second dimension (1 for a flat array).  Returns the (row, node) windows added."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        node = np.ascontiguousarray(node, np.int32)
        start = np.ascontiguousarray(start, np.int32)
        j = len(start)
        if kmax is None:
            kmax = node.shape[1] if node.ndim == 2 else 1
        # a kmax outside 1..FIT_MAX_K is the library's error (FIT_E_INVAL), before it reads node
        if any(len(c) != j for c in cols) or len(k) != j or (1 <= kmax <= FIT_MAX_K and node.size != j * kmax):
            raise ValueError("jobs, node (J * kmax) and start (J) disagree on J")
        applied = C.c_int64()
        check(lib().fit_unplace_tl(self._h, j, *[_ptr(c) for c in cols], _ptr(k), int(kmax), _ptr(node), _ptr(start),
                                   C.byref(applied)), "fit_unplace_tl")
        return applied.value

    def unplace_tl_device(self, cpu, mem, gpu, wall, nodes_k, node, start, kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k may be None = all 1; node has
        J * kmax int32 entries).  Returns the (row, node) windows added."""
        applied = C.c_int64()
        check(lib().fit_unplace_tl_device(self._h, int(start.numel()), _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall),
                                          _ptr(nodes_k) if nodes_k is not None else None, int(kmax), _ptr(node),
                                          _ptr(start), C.byref(applied)), "fit_unplace_tl_device")
        return applied.value

    def unplace_tl_ms(self):
        """Device time in ms of the last successful unplace_tl / unplace_tl_device (HIP events on the
        context's stream, fit_unplace_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_unplace_tl_ms(self._h, C.byref(ms)), "fit_unplace_tl_ms")
        return ms.value

    # ---- move the timeline forward with the clock ---------------------------
    def advance_tl(self, a: int, tail=None):
        """Move the current timeline left by a slots (fit_advance_tl).  tail: int32 [n, 3] (cpu, mem,
        gpu per node in the caller's order), the level of the a new slots at the far end wherever
        slot H - 1 is not -1; None: every column continues its slot H - 1 value, which is exact only
        when no reservation and no pending release reaches the old horizon edge."""
        if tail is None:
            check(lib().fit_advance_tl(self._h, int(a), None, None, None), "fit_advance_tl")
            return
        tail = np.asarray(tail, np.int32)
        if tail.shape != (self.n, 3):
            raise ValueError("tail must be [n, 3]")
        cols = [np.ascontiguousarray(tail[:, i]) for i in range(3)]
        check(lib().fit_advance_tl(self._h, int(a), *[_ptr(c) for c in cols]), "fit_advance_tl")

    def advance_tl_device(self, a: int, cpu, mem, gpu):
        """The tails as torch tensors resident on this GPU, n int32 entries each (all three None:
        continue slot H - 1)."""
        check(lib().fit_advance_tl_device(self._h, int(a), *[_ptr(t) if t is not None else None
                                                             for t in (cpu, mem, gpu)]), "fit_advance_tl_device")

    def advance_tl_ms(self):
        """Device time in ms of the last successful advance_tl / advance_tl_device with a > 0 (HIP
        events on the context's stream, fit_advance_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_advance_tl_ms(self._h, C.byref(ms)), "fit_advance_tl_ms")
        return ms.value

    # ---- re-apply recorded reservations to the timeline ----------------------
    def hold_tl(self, jobs, node, start, kmax: int | None = None):
        """Subtract the rows' demand windows from the current timeline at their recorded nodes and
        start slots (fit_hold_tl), unless they no longer fit: jobs, node[J, kmax] (or node[J] at kmax 1)
        and start[J] as unplace_tl takes them; rows with start < 0 are skipped, so a placement's outputs
        go in verbatim.  kmax None: node's second dimension (1 for a flat array).  Returns (state[J]
        of FIT_HOLD_HELD / FIT_HOLD_REFUSED / FIT_HOLD_SKIPPED, the nodes of the held rows, the
        refused rows)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        k = np.ascontiguousarray(jobs.nodes_k, np.uint16)
        node = np.ascontiguousarray(node, np.int32)
        start = np.ascontiguousarray(start, np.int32)
        j = len(start)
        if kmax is None:
            kmax = node.shape[1] if node.ndim == 2 else 1
        # a kmax outside 1..FIT_MAX_K is the library's error (FIT_E_INVAL), before it reads node
        if any(len(c) != j for c in cols) or len(k) != j or (1 <= kmax <= FIT_MAX_K and node.size != j * kmax):
            raise ValueError("jobs, node (J * kmax) and start (J) disagree on J")
        state = np.full(j, FIT_HOLD_SKIPPED, np.int32)
        applied, refused = C.c_int64(), C.c_int64()
        check(lib().fit_hold_tl(self._h, j, *[_ptr(c) for c in cols], _ptr(k), int(kmax), _ptr(node), _ptr(start),
                                _ptr(state), C.byref(applied), C.byref(refused)), "fit_hold_tl")
        return state, applied.value, refused.value

    def hold_tl_device(self, cpu, mem, gpu, wall, nodes_k, node, start, out_state, kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k may be None = all 1; node has
        J * kmax int32 entries); writes out_state (J int32).  Returns (the nodes of the held rows, the
        refused rows)."""
        applied, refused = C.c_int64(), C.c_int64()
        check(lib().fit_hold_tl_device(self._h, int(start.numel()), _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall),
                                       _ptr(nodes_k) if nodes_k is not None else None, int(kmax), _ptr(node),
                                       _ptr(start), _ptr(out_state), C.byref(applied), C.byref(refused)),
              "fit_hold_tl_device")
        return applied.value, refused.value

    def hold_tl_ms(self):
        """Device time in ms of the last successful hold_tl / hold_tl_device (HIP events on the
        context's stream, fit_hold_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_hold_tl_ms(self._h, C.byref(ms)), "fit_hold_tl_ms")
        return ms.value

    # ---- how many more copies of a job fit now ---------------------------
    def room(self, jobs):
        """Every job judged alone against the current node table (fit_room): a structured array of
        ROOM_DTYPE rows (code, members, nodes, best, copies, best_node, by_gpu, by_cpu, by_mem).
        Changes nothing; jobs.nodes_k plays no part (the row counts node shares)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        out = np.zeros(len(part), ROOM_DTYPE)
        check(lib().fit_room(self._h, len(part), *[_ptr(c) for c in cols], _ptr(part), _ptr(out)), "fit_room")
        return out

    def room_device(self, cpu, mem, gpu, wall, part, out):
        """All arguments torch tensors resident on this GPU; writes out (J rows of 40 bytes,
        ROOM_DTYPE's layout, 8-byte aligned: an int64 tensor of J * 5 words will do).  Returns the
        device time of its launches in ms (HIP events on the context's stream, fit_room_ms); 0.0
        for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_room_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part), _ptr(out)),
              "fit_room_device")
        if j == 0:
            return 0.0
        ms = C.c_double()
        check(lib().fit_room_ms(self._h, C.byref(ms)), "fit_room_ms")
        return ms.value

    # ---- which running jobs to evict so that a pending job fits ---------------
    def load_victims(self, victims):
        """The preemptible running jobs per node (fit_load_victims): `victims` has off (n + 1), prio,
        cpu, mem, gpu — a CSR by node id, each node's entries in eviction order (priority
        non-decreasing) — or is None: every list empty.  After load_nodes, which drops them."""
        if victims is None:
            check(lib().fit_load_victims(self._h, None, None, None, None, None), "fit_load_victims")
            return
        cols = [np.ascontiguousarray(getattr(victims, f), np.int32) for f in ("off", "prio", "cpu", "mem", "gpu")]
        if len(cols[0]) != self.n + 1 or any(len(c) != len(cols[1]) for c in cols[2:]) or (
                len(cols[0]) and int(cols[0].max()) > len(cols[1])):
            raise ValueError("victims: off must have n + 1 entries that index equally long columns")
        check(lib().fit_load_victims(self._h, *[_ptr(c) if len(c) else None for c in cols]), "fit_load_victims")

    def load_victims_device(self, off, prio, cpu, mem, gpu):
        """torch int32 tensors on this GPU (off has n + 1 entries, the others off[n]); off None: every
        list empty.  The lists are validated by a kernel."""
        if off is None:
            check(lib().fit_load_victims_device(self._h, None, 0, None, None, None, None), "fit_load_victims_device")
            return
        check(lib().fit_load_victims_device(self._h, _ptr(off), int(prio.numel()),
                                            *[_ptr(t) if t.numel() else None for t in (prio, cpu, mem, gpu)]),
              "fit_load_victims_device")

    def preempt(self, jobs, prio):
        """Every job judged alone against the current node table and the loaded victims
        (fit_preempt): a structured array of EVICT_DTYPE rows (code, node, victims, top_prio, members,
        fit, able, outranked).  prio: the jobs' priorities (int32).  Changes nothing; jobs.nodes_k
        plays no part (each job takes one node)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        prio = np.ascontiguousarray(prio, np.int32)
        if len(prio) != len(part):
            raise ValueError("prio must have one entry per job")
        out = np.zeros(len(part), EVICT_DTYPE)
        check(lib().fit_preempt(self._h, len(part), *[_ptr(c) for c in cols], _ptr(part), _ptr(prio), _ptr(out)),
              "fit_preempt")
        return out

    def preempt_device(self, cpu, mem, gpu, wall, part, prio, out):
        """All arguments torch tensors resident on this GPU; writes out (J rows of 8 int32, the fields
        of EVICT_DTYPE in order).  Returns the device time of its launches in ms (HIP events on the
        context's stream, fit_preempt_ms); 0.0 for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_preempt_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part),
                                       _ptr(prio), _ptr(out)), "fit_preempt_device")
        if j == 0:
            return 0.0
        return self.preempt_ms()

    def preempt_ms(self):
        """Device time in ms of the last successful preempt_device (fit_preempt_ms)."""
        ms = C.c_double()
        check(lib().fit_preempt_ms(self._h, C.byref(ms)), "fit_preempt_ms")
        return ms.value

    # ---- which running jobs to evict so that a job starts now on the timeline --
    def load_victims_tl(self, victims):
        """The preemptible running jobs per node for the loaded timeline (fit_load_victims_tl):
        load_victims' CSR plus `end`, the slot at which each job hands its resources back anyway
        (0 <= end <= H) — or None: every list empty.  After load_timeline, which drops them;
        advance_tl keeps them and moves their ends along."""
        if victims is None:
            check(lib().fit_load_victims_tl(self._h, None, None, None, None, None, None), "fit_load_victims_tl")
            return
        cols = [np.ascontiguousarray(getattr(victims, f), np.int32) for f in ("off", "prio", "end", "cpu", "mem", "gpu")]
        if len(cols[0]) != self.n + 1 or any(len(c) != len(cols[1]) for c in cols[2:]) or (
                len(cols[0]) and int(cols[0].max()) > len(cols[1])):
            raise ValueError("victims: off must have n + 1 entries that index equally long columns")
        check(lib().fit_load_victims_tl(self._h, *[_ptr(c) if len(c) else None for c in cols]), "fit_load_victims_tl")

    def load_victims_tl_device(self, off, prio, end, cpu, mem, gpu):
        """torch int32 tensors on this GPU (off has n + 1 entries, the others off[n]); off None: every
        list empty.  The lists are validated by a kernel."""
        if off is None:
            check(lib().fit_load_victims_tl_device(self._h, None, 0, None, None, None, None, None),
                  "fit_load_victims_tl_device")
            return
        check(lib().fit_load_victims_tl_device(self._h, _ptr(off), int(prio.numel()),
                                               *[_ptr(t) if t.numel() else None for t in (prio, end, cpu, mem, gpu)]),
              "fit_load_victims_tl_device")

    def preempt_tl(self, jobs, prio):
        """Every job judged alone, for a start now, against the current timeline (reservations
        included) and the lists of load_victims_tl (fit_preempt_tl): EVICT_DTYPE rows, as preempt's.
        Changes nothing; jobs.nodes_k plays no part (each job takes one node)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        prio = np.ascontiguousarray(prio, np.int32)
        if len(prio) != len(part):
            raise ValueError("prio must have one entry per job")
        out = np.zeros(len(part), EVICT_DTYPE)
        check(lib().fit_preempt_tl(self._h, len(part), *[_ptr(c) for c in cols], _ptr(part), _ptr(prio), _ptr(out)),
              "fit_preempt_tl")
        return out

    def preempt_tl_device(self, cpu, mem, gpu, wall, part, prio, out):
        """All arguments torch tensors resident on this GPU; writes out (J rows of 8 int32, the fields
        of EVICT_DTYPE in order).  Returns the device time of its launches in ms (fit_preempt_tl_ms);
        0.0 for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_preempt_tl_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part),
                                          _ptr(prio), _ptr(out)), "fit_preempt_tl_device")
        if j == 0:
            return 0.0
        return self.preempt_tl_ms()

    def preempt_tl_ms(self):
        """Device time in ms of the last successful preempt_tl_device (fit_preempt_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_preempt_tl_ms(self._h, C.byref(ms)), "fit_preempt_tl_ms")
        return ms.value

    # ---- which victims to evict so that a multi-node job fits -----------------
    def preempt_k(self, jobs, prio, kmax: int | None = None):
        """Every job judged alone against the current node table and the loaded victims, on
        max(jobs.nodes_k, 1) distinct nodes at once (fit_preempt_k): (rows[J] of EVICT_K_DTYPE,
        nodes[J, kmax], victims[J, kmax]).  A FITS or EVICT row's picks in key order with the entries
        of each node's list to evict (0: it fits now); -1 and 0 elsewhere.  Changes nothing.  kmax
        None: the largest nodes_k of the batch (at least 1)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = None if jobs.nodes_k is None else np.ascontiguousarray(jobs.nodes_k, np.uint16)  # None: all 1
        prio = np.ascontiguousarray(prio, np.int32)
        j = len(part)
        if len(prio) != j or (k is not None and len(k) != j):
            raise ValueError("prio and nodes_k must have one entry per job")
        if kmax is None:
            kmax = max(1, int(k.max())) if j and k is not None else 1
        out = np.zeros(j, EVICT_K_DTYPE)
        nodes = np.full((j, max(int(kmax), 0)), -1, np.int32)
        victims = np.zeros((j, max(int(kmax), 0)), np.int32)
        check(lib().fit_preempt_k(self._h, j, *[_ptr(c) for c in cols], _ptr(part), _ptr(k) if k is not None else None,
                                  _ptr(prio), int(kmax), _ptr(out), _ptr(nodes), _ptr(victims)), "fit_preempt_k")
        return out, nodes, victims

    def preempt_k_device(self, cpu, mem, gpu, wall, part, nodes_k, prio, out, out_node, out_victims, kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k may be None = all 1); writes out
        (J rows of 10 int32, the fields of EVICT_K_DTYPE in order), out_node and out_victims (J * kmax
        int32 each).  Returns the device time of its launches in ms (HIP events on the context's
        stream, fit_preempt_k_ms); 0.0 for no jobs."""
        j = int(cpu.numel())
        check(lib().fit_preempt_k_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part),
                                         _ptr(nodes_k) if nodes_k is not None else None, _ptr(prio), int(kmax),
                                         _ptr(out), _ptr(out_node), _ptr(out_victims)), "fit_preempt_k_device")
        if j == 0:
            return 0.0
        return self.preempt_k_ms()

    def preempt_k_ms(self):
        """Device time in ms of the last successful preempt_k_device (fit_preempt_k_ms)."""
        ms = C.c_double()
        check(lib().fit_preempt_k_ms(self._h, C.byref(ms)), "fit_preempt_k_ms")
        return ms.value

    # ---- victims for a multi-node job on the timeline ------------------------
    def preempt_tl_k(self, jobs, prio, kmax: int | None = None):
        """Every job judged alone against the current timeline (reservations included) and the lists of
        load_victims_tl, for a start now on max(jobs.nodes_k, 1) distinct nodes at once
        (fit_preempt_tl_k): (rows[J] of EVICT_K_DTYPE, nodes[J, kmax], victims[J, kmax]), as
        preempt_k's.  Changes nothing.  kmax None: the largest nodes_k of the batch (at least 1)."""
        cols = [np.ascontiguousarray(a, np.int32) for a in (jobs.cpu, jobs.mem, jobs.gpu, jobs.wall)]
        part = np.ascontiguousarray(jobs.part, np.uint16)
        k = None if jobs.nodes_k is None else np.ascontiguousarray(jobs.nodes_k, np.uint16)  # None: all 1
        prio = np.ascontiguousarray(prio, np.int32)
        j = len(part)
        if len(prio) != j or (k is not None and len(k) != j):
            raise ValueError("prio and nodes_k must have one entry per job")
        if kmax is None:
            kmax = max(1, int(k.max())) if j and k is not None else 1
        out = np.zeros(j, EVICT_K_DTYPE)
        nodes = np.full((j, max(int(kmax), 0)), -1, np.int32)
        victims = np.zeros((j, max(int(kmax), 0)), np.int32)
        check(lib().fit_preempt_tl_k(self._h, j, *[_ptr(c) for c in cols], _ptr(part),
                                     _ptr(k) if k is not None else None, _ptr(prio), int(kmax), _ptr(out), _ptr(nodes),
                                     _ptr(victims)), "fit_preempt_tl_k")
        return out, nodes, victims

    def preempt_tl_k_device(self, cpu, mem, gpu, wall, part, nodes_k, prio, out, out_node, out_victims, kmax: int = 1):
        """All arguments torch tensors resident on this GPU (nodes_k may be None = all 1); writes out
        (J rows of 10 int32, the fields of EVICT_K_DTYPE in order), out_node and out_victims (J * kmax
        int32 each).  Returns the device time of its launches in ms (fit_preempt_tl_k_ms); 0.0 for no
        jobs."""
        j = int(cpu.numel())
        check(lib().fit_preempt_tl_k_device(self._h, j, _ptr(cpu), _ptr(mem), _ptr(gpu), _ptr(wall), _ptr(part),
                                            _ptr(nodes_k) if nodes_k is not None else None, _ptr(prio), int(kmax),
                                            _ptr(out), _ptr(out_node), _ptr(out_victims)), "fit_preempt_tl_k_device")
        if j == 0:
            return 0.0
        return self.preempt_tl_k_ms()

    def preempt_tl_k_ms(self):
        """Device time in ms of the last successful preempt_tl_k_device (fit_preempt_tl_k_ms)."""
        ms = C.c_double()
        check(lib().fit_preempt_tl_k_ms(self._h, C.byref(ms)), "fit_preempt_tl_k_ms")
        return ms.value

    # ---- report evicted victims: off the lists, onto the timeline -------------
    def evicted_tl(self, node, pos):
        """Report evicted entries (fit_evicted_tl): row i says that entry pos[i] of node[i]'s list
        (caller's node id; position in the list as it is before the call) is gone.  Its amounts go back
        to the slots [0, max(end - shift, 0)) of its node and it leaves the list; the timeline, the
        other entries and the shift stay loaded."""
        node = np.ascontiguousarray(node, np.int32)
        pos = np.ascontiguousarray(pos, np.int32)
        if node.ndim != 1 or node.shape != pos.shape:
            raise ValueError("node and pos must be flat arrays of one length")
        check(lib().fit_evicted_tl(self._h, len(node), _ptr(node) if len(node) else None,
                                   _ptr(pos) if len(pos) else None), "fit_evicted_tl")

    def evicted_tl_device(self, node, pos):
        """node and pos torch int32 tensors resident on this GPU; the rows are judged by a kernel.
        Returns the device time of its launches in ms (fit_evicted_tl_ms); 0.0 for no rows."""
        m = int(node.numel())
        check(lib().fit_evicted_tl_device(self._h, m, _ptr(node) if m else None, _ptr(pos) if m else None),
              "fit_evicted_tl_device")
        if m == 0:
            return 0.0
        return self.evicted_tl_ms()

    def evicted_tl_ms(self):
        """Device time in ms of the last successful evicted_tl / evicted_tl_device with rows (HIP events
        on the context's stream, fit_evicted_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_evicted_tl_ms(self._h, C.byref(ms)), "fit_evicted_tl_ms")
        return ms.value

    def read_victims_tl(self):
        """The current lists of load_victims_tl by the caller's node id (fit_read_victims_tl): a
        synth.VictimsTL with every end as the queries read it, max(end - shift, 0); the list of a node
        in no partition is empty.  Changes nothing."""
        from .synth import VictimsTL
        off = np.zeros(self.n + 1, np.int32)
        check(lib().fit_read_victims_tl(self._h, _ptr(off), 0, None, None, None, None, None), "fit_read_victims_tl")
        nv = int(off[-1])
        cols = [np.zeros(nv, np.int32) for _ in range(5)]
        if nv:
            check(lib().fit_read_victims_tl(self._h, _ptr(off), nv, *[_ptr(c) for c in cols]), "fit_read_victims_tl")
        return VictimsTL(off, *cols)

    # ---- a node changes outside the plan: overwrite windows of the timeline ----
    def set_tl(self, node, frm, to, levels):
        """Overwrite windows of the current timeline (fit_set_tl): row i sets the slots
        [frm[i], min(to[i], H)) of node[i] (caller's node id) to levels[i] = (cpu, mem, gpu), each
        >= -1, -1 closing the column; rows with frm < 0 are skipped, and where rows overlap the one with
        the largest index stands.  levels is int32 [m, 3].  Returns (applied, ignored): the live rows
        whose node has a run list, and those on a node that was loaded in no partition."""
        node = np.ascontiguousarray(node, np.int32)
        frm = np.ascontiguousarray(frm, np.int32)
        to = np.ascontiguousarray(to, np.int32)
        levels = np.asarray(levels, np.int32)
        m = len(node) if node.ndim == 1 else -1
        if m < 0 or frm.shape != (m,) or to.shape != (m,) or levels.shape != (m, 3):
            raise ValueError("node, frm and to must be flat arrays of one length m, levels [m, 3]")
        cols = [node, frm, to] + [np.ascontiguousarray(levels[:, i]) for i in range(3)]
        applied, ignored = C.c_int64(), C.c_int64()
        check(lib().fit_set_tl(self._h, m, *[_ptr(c) if m else None for c in cols], C.byref(applied),
                               C.byref(ignored)), "fit_set_tl")
        return applied.value, ignored.value

    def set_tl_device(self, node, frm, to, cpu, mem, gpu):
        """The six columns as torch int32 tensors resident on this GPU, m entries each; the rows are
        judged by a kernel.  Returns (applied, ignored)."""
        m = int(node.numel())
        applied, ignored = C.c_int64(), C.c_int64()
        check(lib().fit_set_tl_device(self._h, m, *[_ptr(t) if m else None for t in (node, frm, to, cpu, mem, gpu)],
                                      C.byref(applied), C.byref(ignored)), "fit_set_tl_device")
        return applied.value, ignored.value

    def set_tl_ms(self):
        """Device time in ms of the last successful set_tl / set_tl_device with a live row (HIP events
        on the context's stream, fit_set_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_set_tl_ms(self._h, C.byref(ms)), "fit_set_tl_ms")
        return ms.value

    # ---- free capacity per partition and slot --------------------------------
    def free_tl(self, parts: int):
        """The capacity profile of the current timeline (fit_free_tl): a structured array of
        FREE_DTYPE rows [parts, H] (cpu, mem, gpu, nodes, max_cpu, max_mem, max_gpu), row [p, t] over
        the nodes with mask bit p that are open at slot t.  Changes nothing."""
        parts = int(parts)
        # parts outside 1..32 or no timeline is the library's error, before it writes a row
        out = np.zeros((min(max(parts, 1), 32), max(getattr(self, "slots", 0), 1)), FREE_DTYPE)
        check(lib().fit_free_tl(self._h, parts, _ptr(out)), "fit_free_tl")
        return out

    def free_tl_device(self, parts: int, out):
        """The rows written into out, a torch tensor resident on this GPU (parts * H rows of 40 bytes,
        FREE_DTYPE's layout, 8-byte aligned: an int64 tensor of parts * H * 5 words will do).  Returns
        the device time of its launches in ms (HIP events on the context's stream, fit_free_tl_ms)."""
        check(lib().fit_free_tl_device(self._h, int(parts), _ptr(out)), "fit_free_tl_device")
        return self.free_tl_ms()

    def free_tl_ms(self):
        """Device time in ms of the last successful free_tl / free_tl_device (HIP events on the
        context's stream, fit_free_tl_ms)."""
        ms = C.c_double()
        check(lib().fit_free_tl_ms(self._h, C.byref(ms)), "fit_free_tl_ms")
        return ms.value

    def read_timeline(self):
        """Dense [n, slots, 3] int32 (cpu, mem, gpu)."""
        c, m, g = (np.empty((self.n, self.slots), np.int32) for _ in range(3))
        check(lib().fit_read_timeline(self._h, _ptr(c), _ptr(m), _ptr(g)), "fit_read_timeline")
        return np.stack([c, m, g], axis=2)

    def read_nodes(self):
        c, m, g = (np.empty(self.n, np.int32) for _ in range(3))
        check(lib().fit_read_nodes(self._h, _ptr(c), _ptr(m), _ptr(g)), "fit_read_nodes")
        return c, m, g

    def partition_free(self, p: int):
        c, m, g = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().fit_partition_free(self._h, p, C.byref(c), C.byref(m), C.byref(g)), "fit_partition_free")
        return {"cpu": c.value, "mem_mib": m.value, "gpu": g.value}


class Admitter:
    """Batched admission over one Engine (include/fitgpu.h "batched admission"; the CreatePod
    call site of pkg/slurm-virtual-kubelet/provider.go:35-60).  `admit` blocks the calling thread
    until its batch is placed (ctypes releases the GIL, so threads admit concurrently, as the 10
    PodSyncWorkers do) and returns (nodes, batch, batch_jobs, order, ticket); nodes[0] is
    FIT_UNPLACED / FIT_REJECTED when the pod cannot be placed now.

    Lifetime: close() (also Engine.close()) stops new calls, waits for the calls already inside
    (their batches are still placed), then destroys the native admitter — a caller can never hold
    a handle that is being freed."""

    def __init__(self, engine: Engine, max_batch: int = 1024, max_wait_us: int = 2000):
        self._engine = engine  # keeps the context alive
        h = C.c_void_p()
        check(lib().fit_admitter_create(engine._h, max_batch, max_wait_us, C.byref(h)), "fit_admitter_create")
        self._h = h
        self._cv = threading.Condition()
        self._users = 0
        engine._admitters.add(self)

    def _enter(self):
        with self._cv:
            if not self._h:
                raise FitError(FIT_E_STATE, "Admitter closed")
            self._users += 1
            return self._h

    def _leave(self):
        with self._cv:
            self._users -= 1
            self._cv.notify_all()

    def _call(self, fn, *args):
        h = self._enter()
        try:
            return fn(h, *args)
        finally:
            self._leave()

    @staticmethod
    def _res(r, nodes_k):
        k = max(nodes_k, 1)
        nodes = [r.node[i] for i in range(k)] if r.node[0] >= 0 else [r.node[0]]
        return nodes, r.batch, r.batch_jobs, r.order, r.ticket

    def admit(self, priority: int, cpu: int, mem_mib: int, gpu: int = 0, wall_min: int = 0,
              part: int = 0, nodes_k: int = 1):
        q = FitAdmitReq(priority, cpu, mem_mib, gpu, wall_min, part, nodes_k)
        r = FitAdmitRes()
        check(self._call(lambda h: lib().fit_admit(h, C.byref(q), C.byref(r))), "fit_admit")
        return self._res(r, nodes_k)

    def admit_group(self, reqs: list[tuple]):
        """All-or-nothing admission of (priority, cpu, mem, gpu, wall, part, k) requests (the
        tasks of one array job, pod_demand's output); one result per request."""
        n = len(reqs)
        q = (FitAdmitReq * n)(*[FitAdmitReq(*r) for r in reqs])
        r = (FitAdmitRes * n)()
        check(self._call(lambda h: lib().fit_admit_group(h, q, n, r)), "fit_admit_group")
        return [self._res(r[i], reqs[i][6]) for i in range(n)]

    def explain(self, reqs: list[tuple]):
        """fit_admitter_explain of (priority, cpu, mem, gpu, wall, part, k) requests (admit_group's
        form) against the table the next batch would see, open reservations included: WHY_DTYPE rows."""
        n = len(reqs)
        q = (FitAdmitReq * max(n, 1))(*[FitAdmitReq(*r) for r in reqs])
        out = np.zeros(n, WHY_DTYPE)
        check(self._call(lambda h: lib().fit_admitter_explain(h, q, n, _ptr(out))), "fit_admitter_explain")
        return out

    def room(self, reqs: list[tuple]):
        """fit_admitter_room of (priority, cpu, mem, gpu, wall, part, k) requests against the table
        the next batch would see, open reservations included: ROOM_DTYPE rows.  Priority and k are
        ignored."""
        n = len(reqs)
        q = (FitAdmitReq * max(n, 1))(*[FitAdmitReq(*r) for r in reqs])
        out = np.zeros(n, ROOM_DTYPE)
        check(self._call(lambda h: lib().fit_admitter_room(h, q, n, _ptr(out))), "fit_admitter_room")
        return out

    def load_nodes(self, nodes):
        cols = [np.ascontiguousarray(nodes.cpu_free, np.int32), np.ascontiguousarray(nodes.mem_free, np.int32),
                np.ascontiguousarray(nodes.gpu_free, np.int32), np.ascontiguousarray(nodes.avail_min, np.int32),
                np.ascontiguousarray(nodes.part_mask, np.uint32)]
        check(self._call(lambda h: lib().fit_admitter_load_nodes(h, len(cols[0]), *[_ptr(c) for c in cols])),
              "fit_admitter_load_nodes")
        self._engine.n = len(cols[0])

    def load_table(self, nodes, names: list[str] | None = None, state: bool = False, pin: bool = False,
                   generation: int = 0):
        """fit_admitter_load_table: the node table with its names (reservations follow nodes by
        name; pinning needs them), whether part_mask carries node State (FIT_TABLE_STATE: pinned)
        and whether to pin without State (FIT_TABLE_PIN)."""
        cols = [np.ascontiguousarray(nodes.cpu_free, np.int32), np.ascontiguousarray(nodes.mem_free, np.int32),
                np.ascontiguousarray(nodes.gpu_free, np.int32), np.ascontiguousarray(nodes.avail_min, np.int32),
                np.ascontiguousarray(nodes.part_mask, np.uint32)]
        blob = b"".join(x.encode() + b"\0" for x in names) if names is not None else None
        t = FitNodeTable(len(cols[0]), *[c.ctypes.data for c in cols], blob,
                         (FIT_TABLE_STATE if state else 0) | (FIT_TABLE_PIN if pin else 0), generation)
        check(self._call(lambda h: lib().fit_admitter_load_table(h, C.byref(t))), "fit_admitter_load_table")
        self._engine.n = len(cols[0])

    def generation(self) -> int:
        return check(self._call(lambda h: lib().fit_admitter_generation(h)), "fit_admitter_generation")

    def script(self, tickets: list[int], script: str) -> tuple[str, bool]:
        """(script to submit, pinned): fit_admitter_script."""
        t = (C.c_int64 * len(tickets))(*tickets)
        outlen = len(script.encode()) + 64 + 4096 * 8
        buf = C.create_string_buffer(outlen)
        pinned = C.c_int32()
        n = check(self._call(lambda h: lib().fit_admitter_script(h, t, len(tickets), script.encode(), buf, outlen,
                                                                 C.byref(pinned))), "fit_admitter_script")
        return buf.raw[:n].decode(), bool(pinned.value)

    def partition_free(self, p: int):
        c, m, g = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._call(lambda h: lib().fit_admitter_partition_free(h, p, C.byref(c), C.byref(m), C.byref(g))),
              "fit_admitter_partition_free")
        return {"cpu": c.value, "mem_mib": m.value, "gpu": g.value}

    def confirm(self, ticket: int):
        check(self._call(lambda h: lib().fit_admitter_confirm(h, ticket)), "fit_admitter_confirm")

    def release(self, ticket: int):
        check(self._call(lambda h: lib().fit_admitter_release(h, ticket)), "fit_admitter_release")

    def set_ttl(self, loads: int):
        check(self._call(lambda h: lib().fit_admitter_set_ttl(h, loads)), "fit_admitter_set_ttl")

    def reservations(self) -> int:
        return check(self._call(lambda h: lib().fit_admitter_reservations(h)), "fit_admitter_reservations")

    def pending(self) -> int:
        return check(self._call(lambda h: lib().fit_admitter_pending(h)), "fit_admitter_pending")

    def close(self):
        cv = getattr(self, "_cv", None)
        if cv is None:
            return
        with cv:
            h, self._h = self._h, None  # no new calls
            while self._users:
                cv.wait()  # calls already inside finish (their batches are placed)
        if h:
            lib().fit_admitter_destroy(h)

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

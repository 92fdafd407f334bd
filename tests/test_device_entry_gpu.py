"""The *_device entry points (fit_load_nodes_device, fit_place_device, fit_load_timeline_device,
fit_place_tl_device) against the host entry points on the same inputs: the same placements and the
same final node table or timelines, exactly.  The sizes are the smallest that reach each path of
the host engine: k_small (at most 128 jobs), the rounds / persistent engine, a nodes_k column
(kmax 8), and the backfill."""
import numpy as np
import pytest

from _devarray import DevArray
from fitgpu import Engine, synth

pytestmark = pytest.mark.gpu

STAT_KEYS = ("jobs", "placed", "unplaced", "rejected", "engine", "components", "shard_mode")


def place_host(nodes, jobs, parts, kmax):
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        out, st = e.place(jobs, kmax=kmax)
        return out, st, e.read_nodes()


def place_device(nodes, jobs, parts, kmax, with_k):
    with Engine(device=0) as e:
        ncols = [DevArray(a) for a in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min,
                                       nodes.part_mask)]
        e.load_nodes_device(*ncols)
        e.load_partitions(parts)
        jcols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")]
        k = DevArray(jobs.nodes_k) if with_k else None
        out = DevArray(np.full((jobs.j, kmax), -7, np.int32))
        st = e.place_device(*jcols, k, out, kmax=kmax)
        return out.numpy(), st, e.read_nodes()


def check_place(name, n, j, kmax, with_k, engines):
    nodes, jobs, parts = synth.make_config(name, n, j)
    if not with_k:
        assert (jobs.nodes_k <= 1).all()  # a null nodes_k means one node per job
    out, st, fin = place_host(nodes, jobs, parts, kmax)
    dout, dst, dfin = place_device(nodes, jobs, parts, kmax, with_k)
    assert st["engine"] in engines and st["placed"] > 0
    assert np.array_equal(out, dout), "placements of fit_place and fit_place_device differ"
    assert all(np.array_equal(a, b) for a, b in zip(fin, dfin)), "final node tables differ"
    assert [st[k] for k in STAT_KEYS] == [dst[k] for k in STAT_KEYS]
    # the table did change, so the comparison of the final state says something
    assert not np.array_equal(fin[0], nodes.cpu_free)


@pytest.mark.auto_engine
def test_place_device_direct():
    """100 jobs under the production engine choice: k_small, from device columns (the host entry
    point carries the same batch in the kernel arguments)."""
    check_place("c2", 64, 100, 1, False, (2,))


def test_place_device_engine():
    check_place("c2", 64, 1024, 1, False, (0, 1))


def test_place_device_nodes_k():
    check_place("c4", 256, 1024, 8, True, (0, 1, 3))


def test_place_tl_device():
    nodes, tline, jobs, parts = synth.make_c5(256, 4096)
    with Engine(device=0) as e:
        e.load_nodes(nodes)
        e.load_partitions(parts)
        e.load_timeline(tline)
        node, start, st = e.place_tl(jobs)
        fin = e.read_timeline()
    with Engine(device=0) as e:
        ncols = [DevArray(a) for a in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.avail_min,
                                       nodes.part_mask)]
        e.load_nodes_device(*ncols)
        e.load_partitions(parts)
        tcols = [DevArray(np.ascontiguousarray(a, np.int32)) for a in (tline.off, tline.slot, tline.cpu, tline.mem,
                                                                       tline.gpu)]
        assert tcols[1].numel() > 0  # there are release events to copy
        e.load_timeline_device(tline.slots, tline.slot_min, *tcols)
        before = e.read_timeline()
        jcols = [DevArray(getattr(jobs, f)) for f in ("cpu", "mem", "gpu", "wall", "part")]
        dnode, dstart = (DevArray(np.full(jobs.j, -7, np.int32)) for _ in range(2))
        dst = e.place_tl_device(*jcols, dnode, dstart)
        dfin = e.read_timeline()
    assert st["placed"] > 0 and (start > 0).any()
    assert np.array_equal(node, dnode.numpy()) and np.array_equal(start, dstart.numpy())
    assert np.array_equal(fin, dfin), "final timelines differ"
    assert not np.array_equal(before, dfin)
    assert [st[k] for k in STAT_KEYS] == [dst[k] for k in STAT_KEYS]

"""The edge-case generator (tests/_edge_cases.py) earns its keep, on the CPU: for every seed the GPU
module uses, the oracle's own placements show that the inputs reach the corner they aim at (capped
fields, scores of exactly 0 and 0xFFFFFFFF, placed and unplaced jobs at the int32 extremes, starts in
later slots), and a plain numpy best fit with the key as a parameter shows that each plausible
mistake in one of the kernels' hand-written copies of the key — a cap off by one, a missing cap, a
missing `>> 10`, the wrong tie-break, a score of 0 read as "no node" — changes the placements of at
least one case of the family aimed at it.  The CPU round models agree with the oracle on all of them."""
import functools

import numpy as np
import pytest

from _edge_cases import edge_case, score
from fitgpu import synth
from oracle import pyoracle as po

SEEDS = list(range(24))     # tests/test_edges_gpu.py: 6 per family, 2 per level of family 0
TL_SEEDS = list(range(12))  # 3 per family
INF = np.uint64(2**64 - 1)
U32 = np.uint64(0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def case(seed):
    nodes, jobs, parts, kmax = edge_case(seed)
    ref, rst, rfin = po.ref_place(nodes, jobs, parts, kmax=kmax)
    for a in (ref, *rfin):
        a.setflags(write=False)
    return nodes, jobs, parts, kmax, ref, rst, rfin


@functools.lru_cache(maxsize=None)
def tl_case(seed):
    nodes, tl, jobs, parts = edge_case(seed, timeline=True)
    rn, rs, rst, rfin = po.ref_place_tl(nodes, tl, jobs, parts)
    return nodes, tl, jobs, parts, rn, rs, rst, rfin


def picks(seed):
    """The oracle's placements replayed: the (gpu, cpu, mem) residual of every placed node pick at
    the moment of choice (all k picks of a job are chosen on the state before it)."""
    nodes, jobs, _, _, ref, _, _ = case(seed)
    free = np.stack([nodes.gpu_free, nodes.cpu_free, nodes.mem_free]).astype(np.int64)
    dem = np.stack([jobs.gpu, jobs.cpu, jobs.mem]).astype(np.int64)
    res = []
    for q in np.flatnonzero(ref[:, 0] >= 0):
        x = ref[q, :max(int(jobs.nodes_k[q]), 1)]
        res.append(free[:, x] - dem[:, q, None])
        free[:, x] -= dem[:, q, None]
    assert np.array_equal(free[1].astype(np.int32), case(seed)[6][0])  # the replay is the oracle's state
    return np.concatenate(res, axis=1) if res else np.zeros((3, 0), np.int64)


# ------------------------------------------------------------------ the inputs reach their corner
@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 4 == 0])
def test_caps_family_wins_on_capped_fields(seed):
    gr, cr, mr = picks(seed)
    capped = (gr > 255) | (cr > 4095) | ((mr >> 10) > 4095)
    level = (seed // 4) % 3
    straddle = [gr, cr, mr >> 10][level]
    cap = [255, 4095, 4095][level]
    print(f"seed {seed} level {level}: {capped.size} picks, {capped.mean():.1%} with a capped field, "
          f"{(straddle > cap).mean():.1%} beyond the level's own cap, {(straddle <= cap).mean():.1%} at or below")
    assert capped.size and capped.mean() >= 0.10
    # the level's own field is met on both sides of its cap
    assert (straddle > cap).any() and (straddle <= cap).any()


@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 4 == 1])
def test_zero_family_wins_on_score_zero(seed):
    sc = score(*picks(seed))
    print(f"seed {seed}: {sc.size} picks, {(sc == 0).mean():.1%} of score 0")
    assert sc.size and (sc == 0).mean() >= 0.10


@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 4 == 2])
def test_extremes_family_places_some_and_not_others(seed):
    rst = case(seed)[5]
    print(f"seed {seed}: {rst['placed']} placed, {rst['unplaced']} unplaced")
    assert rst["placed"] >= 1 and rst["unplaced"] >= 1 and rst["rejected"] == 0


@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 4 == 3])
def test_capped_family_scores_all_ones(seed):
    sc = score(*picks(seed))
    print(f"seed {seed}: {sc.size} picks")
    assert sc.size and (sc == 0xFFFFFFFF).all()


@pytest.mark.parametrize("seed", TL_SEEDS)
def test_timeline_cases_start_later(seed):
    rn, rs = tl_case(seed)[4:6]
    placed = rn >= 0
    print(f"seed {seed}: {placed.sum()} placed of {rn.size}, {(rs[placed] > 0).mean() if placed.any() else 0:.1%} "
          f"start after slot 0, latest start {rs.max()}")
    assert placed.any() and (rs[placed] > 0).mean() >= 0.10


def test_zero256_case_is_seed_1():
    nodes, jobs, _, kmax, ref, rst, rfin = case(1)
    assert nodes.n == 256 and len(set(zip(nodes.cpu_free, nodes.mem_free, nodes.gpu_free, nodes.part_mask))) == 1
    assert (score(*picks(1)) == 0).all() and not any(a.any() for a in rfin)  # every node filled to (0, 0, 0)
    assert rst["unplaced"] > 0


# ------------------------------------------------- a wrong key would be noticed (numpy best fit)
def _u32(a):
    return np.asarray(a, np.int64).astype(np.uint64) & U32


def make_key(gcap=255, ccap=4095, mcap=4095, shift=10, highest_id=False, zero_infeasible=False):
    """The SPEC §2 key with its constants as parameters, in the kernels' 32-bit arithmetic."""
    def key(gr, cr, mr, ids):
        g = np.minimum(_u32(gr), np.uint64(gcap))
        c = np.minimum(_u32(cr), np.uint64(ccap))
        m = _u32(mr) >> np.uint64(shift)
        if mcap is not None:
            m = np.minimum(m, np.uint64(mcap))
        sc = ((g << np.uint64(24)) | (c << np.uint64(12)) | m) & U32
        low = (U32 - np.uint64(1) - ids) if highest_id else ids
        k = (sc << np.uint64(32)) | low
        return np.where(sc == 0, INF, k) if zero_infeasible else k
    return key


def seq_place(nodes, jobs, kmax, key):
    """Sequential best fit in plain numpy (unlimited partitions): out[J, kmax], final (cpu, mem, gpu)."""
    cf, mf, gf, av = (np.asarray(a, np.int64).copy() for a in (nodes.cpu_free, nodes.mem_free, nodes.gpu_free,
                                                                nodes.avail_min))
    mask = np.asarray(nodes.part_mask, np.uint32)
    ids = np.arange(nodes.n, dtype=np.uint64)
    out = np.full((jobs.j, kmax), -1, np.int32)
    for q in range(jobs.j):
        c, m, g, w = int(jobs.cpu[q]), int(jobs.mem[q]), int(jobs.gpu[q]), int(jobs.wall[q])
        k = max(int(jobs.nodes_k[q]), 1)
        x = np.flatnonzero((cf >= c) & (mf >= m) & (gf >= g) & (av >= w) & ((mask >> np.uint32(jobs.part[q])) & 1 != 0))
        if x.size < k:
            continue
        keys = key(gf[x] - g, cf[x] - c, mf[x] - m, ids[x])
        order = np.argsort(keys, kind="stable")[:k]
        if keys[order[-1]] == INF:
            continue
        x = x[order]
        out[q, :k] = x
        cf[x] -= c
        mf[x] -= m
        gf[x] -= g
    return out, (cf.astype(np.int32), mf.astype(np.int32), gf.astype(np.int32))


@pytest.mark.parametrize("seed", SEEDS)
def test_numpy_best_fit_is_the_oracle(seed):
    nodes, jobs, _, kmax, ref, _, rfin = case(seed)
    out, fin = seq_place(nodes, jobs, kmax, make_key())
    assert np.array_equal(out, ref)
    assert all(np.array_equal(a, b) for a, b in zip(fin, rfin))


# wrong key -> the family whose cases must notice it
WRONG = {"cpu cap 4096": (dict(ccap=4096), 0), "gpu cap 256": (dict(gcap=256), 0),
         "memory uncapped": (dict(mcap=None), 0), "memory without >> 10": (dict(shift=0), 1),
         "ties to the highest id": (dict(highest_id=True), 3), "score 0 infeasible": (dict(zero_infeasible=True), 1)}


@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_key_changes_the_placements(name):
    kw, fam = WRONG[name]
    seen = []
    for seed in (s for s in SEEDS if s % 4 == fam):
        nodes, jobs, _, kmax, ref, _, _ = case(seed)
        if not np.array_equal(seq_place(nodes, jobs, kmax, make_key(**kw))[0], ref):
            seen.append(seed)
    print(f"{name}: family {fam}, noticed by seeds {seen}")
    assert seen


# ------------------------------------------------------------------ the CPU models on these inputs
TINY = dict(slice=64, ks=2, km=4, ucap=8, wmin=1, wmax=16)


@pytest.mark.parametrize("seed", SEEDS)
def test_round_models_on_k1_projection(seed):
    nodes, jobs, parts = case(seed)[:3]
    one = synth.Jobs(jobs.cpu, jobs.mem, jobs.gpu, jobs.wall, jobs.part, np.ones(jobs.j, np.uint16))
    ref, _, rfin = po.ref_place(nodes, one, parts)
    for out, fin in ([po.model_place(nodes, one, parts, **prm)[::2] for prm in ({}, TINY)] +
                     [po.cpu_place(nodes, one, parts, threads=2, variant=v)[::2] for v in ("rounds", "component", "split")]):
        assert np.array_equal(out, ref[:, 0])
        assert all(np.array_equal(a, b) for a, b in zip(fin, rfin))


@pytest.mark.parametrize("seed", SEEDS)
def test_cpu_baseline_with_multi_node_jobs(seed):
    nodes, jobs, parts, kmax, ref, rst, rfin = case(seed)
    out, st, fin = po.cpu_place_k(nodes, jobs, parts, kmax, threads=2)
    assert np.array_equal(out, ref) and st["placed"] == rst["placed"]
    assert all(np.array_equal(a, b) for a, b in zip(fin, rfin))


@pytest.mark.parametrize("seed", TL_SEEDS)
def test_rle_backfill_on_timeline_cases(seed):
    nodes, tl, jobs, parts, rn, rs, rst, rfin = tl_case(seed)
    node, start, st, fin = po.cpu_place_tl(nodes, tl, jobs, parts, rle=True)
    assert np.array_equal(node, rn) and np.array_equal(start, rs)
    assert np.array_equal(fin, rfin) and st["placed"] == rst["placed"]

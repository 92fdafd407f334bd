"""tools/recycle_model.c — the CPU round model with the recycling of exhausted dirty rows
 — reproduces the sequential oracle bit for bit under tests/test_model.py's
parameter sets with dirty capacities 1, 3 and 8 and retired lists of 0, 1 and 4 rows, and with no
retired list it counts exactly what oracle/round_model.c counts."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

from fitgpu import synth
from oracle import pyoracle as po
from test_model import P1, PARAMS, _jobs, _nodes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import recycle_model as rm  # noqa: E402

COMBOS = [dict(prm, ucap=u, rcap=r) for prm, u, r in itertools.product(PARAMS, (1, 3, 8), (0, 1, 4))]
IDS = [f"p{i // 9}-u{c['ucap']}-r{c['rcap']}" for i, c in enumerate(COMBOS)]


def _exact_fit():
    rng = np.random.default_rng(5)
    return _nodes(40, rng.permutation(40) + 1, 4096), _jobs(40, rng.permutation(40) + 1, 64), P1


def _zero_and_ties():
    rng = np.random.default_rng(1)
    return (_nodes(50, rng.integers(0, 3, 50), rng.integers(0, 3000, 50)),
            _jobs(400, rng.integers(0, 2, 400), rng.integers(0, 1500, 400)), P1)


def _overlap_negative():
    rng = np.random.default_rng(2)
    masks = rng.choice([1, 2, 3, 4, 12, 0], 120)
    n = _nodes(120, rng.integers(-3, 40, 120), rng.integers(-100, 80000, 120), rng.integers(-1, 9, 120),
               rng.choice([synth.INT32_MAX, 100, 2000, -5], 120), masks)
    j = _jobs(1500, rng.integers(0, 9, 1500), rng.integers(0, 9000, 1500), rng.integers(0, 3, 1500),
              rng.integers(0, 3000, 1500), rng.integers(0, 4, 1500))
    parts = synth.Partitions(np.array([-1, 1000, -1, 60], np.int32), np.array([-1, -1, 4, -1], np.int32),
                             np.array([-1, -1, -1, 5000], np.int32))
    return n, j, parts


INPUTS = {"c2": lambda: synth.make_config("c2", 300, 3000), "c3": lambda: synth.make_config("c3", 1000, 6000),
          "identical": lambda: (_nodes(200, 4, 4096), _jobs(300, 4, 4096), P1), "zero": _zero_and_ties,
          "overlap": _overlap_negative, "exact": _exact_fit}


@functools.lru_cache(maxsize=None)
def _input(name):
    """An input and the oracle's answer, computed once for all parameter combinations."""
    nodes, jobs, parts = INPUTS[name]()
    ref, _, rfin = po.ref_place(nodes, jobs, parts)
    return nodes, jobs, parts, ref[:, 0].copy(), rfin


def _same(name, prm, tmp):
    nodes, jobs, parts, ref, rfin = _input(name)
    out, st, fin = rm.recycle_place(nodes, jobs, parts, build_dir=tmp, **prm)
    assert np.array_equal(out, ref)
    for a, b in zip(fin, rfin):
        assert np.array_equal(a, b)
    return st


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("recycle_model"))


@pytest.mark.parametrize("prm", COMBOS, ids=IDS)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_model_with_recycling_is_exact(name, prm, tmp):
    st = _same(name, prm, tmp)
    if prm["rcap"] == 0:
        assert st["recycled"] == 0


@pytest.mark.parametrize("prm", COMBOS[::3], ids=IDS[::3])  # the rcap = 0 combinations
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_no_retired_list_counts_what_the_round_model_counts(name, prm, tmp):
    nodes, jobs, parts, _, _ = _input(name)
    st = _same(name, prm, tmp)
    kw = {k: v for k, v in prm.items() if k != "rcap"}
    _, mst, _ = po.model_place(nodes, jobs, parts, **kw)
    assert {k: st[k] for k in mst} == mst


def test_exact_fit_recycles(tmp):
    # 40 exact-fit jobs in one window, 8 rows: each full set holds 8 dead rows, 4 may be retired
    prm = dict(PARAMS[0], ucap=8)
    base = _same("exact", dict(prm, rcap=0), tmp)
    st = _same("exact", dict(prm, rcap=4), tmp)
    assert base["stops_ucap"] >= 1 and st["recycled"] >= 4
    assert st["rounds"] < base["rounds"]

"""The periodic minimum spanning tree on the CPU path: the brute-force oracle K.mst_periodic_cpu
against a plain numpy Kruskal over all pairs under the minimum image (mst_periodic_ref.py),
mst_labels against the periodic friends-of-friends oracle, the CPU-index path of the engine with
its periodic core distances, and the argument errors. Data, pair weights and reference trees are
computed once per module."""
import math

import numpy as np
import pytest
import torch

from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

import mst_periodic_ref
import mst_ref
import periodic_knn_ref
from datasets import GENERATORS, uniform

INF = math.inf
N = 1200
PERIODS = {"L1": 1.0, "xy": (1.0, 1.0, INF), "half": 0.5}  # half: the coordinates are not inside one period
_DATA: dict = {}
_CORE: dict = {}
_REF: dict = {}


def data(name):
    if name not in _DATA:
        _DATA[name] = GENERATORS[name](N, seed=21)
    return _DATA[name]


def core5(p, period):
    """The 5th smallest reference pd2 of every finite row (by its bits, self counted), 0 elsewhere."""
    v = periodic_knn_ref.pd2(p, p, periodic_knn_ref.as_period(period))
    finite = np.isfinite(periodic_knn_ref._np(p)).all(axis=1)
    v = np.where(finite[None, :], v, np.float32(np.inf))
    c = np.sort(v.view(np.uint32), axis=1)[:, 4].view(np.float32)
    return torch.from_numpy(np.where(finite, c, np.float32(0)).astype(np.float32))


def case(name, per, core):
    key = (name, per, core)
    if key not in _REF:
        p = data(name)
        if core and (name, per) not in _CORE:
            _CORE[(name, per)] = core5(p, PERIODS[per])
        c = _CORE[(name, per)] if core else None
        _REF[key] = (p, c, mst_periodic_ref.mst(p, PERIODS[per], c))
    return _REF[key]


def check(got, want):
    rows, d2 = got
    assert rows.dtype == torch.int32 and d2.dtype == torch.float32
    assert rows.shape == want[0].shape and d2.shape == want[1].shape
    assert np.array_equal(rows.numpy(), want[0])
    assert np.array_equal(d2.numpy().view(np.uint32), want[1].view(np.uint32))


def wrapped_edges(p, rows, d2, core=None):
    """Edges whose weight differs in its bits from the open-box weight of the same pair."""
    w = mst_ref.pair_weights(p, core)[rows[:, 0], rows[:, 1]]
    return int((w.view(np.uint32) != np.asarray(d2).view(np.uint32)).sum())


@pytest.mark.parametrize("core", [False, True])
@pytest.mark.parametrize("per", sorted(PERIODS))
@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_oracle_against_reference(name, per, core):
    p, c, want = case(name, per, core)
    assert want[1].shape[0] == N - 1
    got = K.mst_periodic_cpu(p, PERIODS[per], c)
    check(got, want)
    rows = got[0]
    assert bool((rows[:, 0] < rows[:, 1]).all())
    key = [(int(b), int(lo), int(hi)) for b, (lo, hi) in zip(got[1].view(torch.int32).tolist(), rows.tolist())]
    assert all(x < y for x, y in zip(key, key[1:]))
    # the period must matter: some edge of the tree wraps
    nwrap = wrapped_edges(p, want[0], want[1], c)
    print(f"{name} {per} core={core}: {nwrap} wrapped edges")
    assert nwrap >= 1
    # the engine on a CPU index, and from the points
    check(E.mst_edges(E.build_index(p), c, period=PERIODS[per]), want)
    check(E.mst_points(p, c, period=PERIODS[per]), want)


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_small_sets(n):
    p = uniform(n, seed=7)
    for period in PERIODS.values():
        want = mst_periodic_ref.mst(p, period)
        assert want[0].shape == (max(n - 1, 0), 2)
        check(K.mst_periodic_cpu(p, period), want)
        check(E.mst_points(p, period=period), want)
        check(E.mst_edges(E.build_index(p), period=period), want)
        if n == 65:  # (two points need not wrap; 64 edges among 65 uniform points do)
            assert wrapped_edges(p, want[0], want[1]) >= 1


def test_nan_and_inf_rows():
    p = uniform(400, seed=4)
    p[17] = math.nan
    p[40, 1] = math.nan
    p[99, 0] = math.inf
    p[250, 2] = -math.inf
    finite = torch.isfinite(p).all(dim=1)
    for period in PERIODS.values():
        for c in (None, core5(p, period)):
            want = mst_periodic_ref.mst(p, period, c)
            assert want[1].shape[0] == int(finite.sum()) - 1
            got = K.mst_periodic_cpu(p, period, c)
            check(got, want)
            assert bool(finite[got[0].long()].all())
            check(E.mst_points(p, c, period=period), want)


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_open_period_is_the_open_tree(name):
    p = data(name)
    want = K.mst_cpu(p)
    got = K.mst_periodic_cpu(p, (INF, INF, INF))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    got = E.mst_points(p, period=INF)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


@pytest.mark.parametrize("per", ["L1", "xy"])
@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_labels_equal_periodic_friends_of_friends(name, per):
    p, period = data(name), PERIODS[per]
    rows, d2 = K.mst_periodic_cpu(p, period)
    bound = K.period_cut2_bound(K.check_period("test", period))
    scale = N ** (-1.0 / 3.0)
    on_edge = float(d2[d2.shape[0] // 2])  # exactly an edge's d2: the strict < leaves that edge out
    cuts = [(E.cut2_of(0.5 * scale), 0.5 * scale, False), (on_edge, on_edge, True),
            (E.cut2_of(2.0 * scale), 2.0 * scale, False)]
    for cut2, eps, squared in cuts:
        assert cut2 <= bound
        want = K.cluster_periodic_cpu(p, cut2, 1, period)[0]
        got = E.mst_labels(rows, d2, N, eps, squared=squared)
        assert torch.equal(got, want), f"cut2 = {cut2}: {int((got != want).sum())} labels differ"
        assert torch.equal(K.mst_labels_cpu(rows, d2, N, cut2), want)
        assert int((d2 < cut2).sum()) == N - int(got.unique().numel())


def test_engine_core_distances():
    p = data("uniform")
    index = E.build_index(p)
    got = E.mst_core_d2(index, 5, period=1.0)
    want = core5(p, 1.0)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, E.mst_core_d2(index, 5))
    check(E.mst_edges(index, got, period=1.0), case("uniform", "L1", True)[2])
    q = p.clone()
    q[5] = math.nan
    got = E.mst_core_d2(E.build_index(q), 5, period=(1.0, 1.0, INF))
    assert float(got[5]) == 0.0
    assert torch.equal(got.view(torch.int32), core5(q, (1.0, 1.0, INF)).view(torch.int32))


def test_value_errors():
    p = uniform(50, seed=9)
    index = E.build_index(p)
    for bad in (0, 0.0, -1, math.nan, (1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, 1.0, 1.0), "x"):
        with pytest.raises(ValueError):
            E.mst_edges(index, period=bad)
        with pytest.raises(ValueError):
            E.mst_points(p, period=bad)
        with pytest.raises(ValueError):
            E.mst_points(torch.empty((0, 3)), period=bad)
        with pytest.raises(ValueError):
            E.mst_core_d2(index, 5, period=bad)
        with pytest.raises(ValueError):
            K.mst_periodic_cpu(p, bad)
    lined = E.LocalIndex(index.n, index.pts, index.perm, index.nodes, index.qnodes, index.depth, index.box, line=True)
    with pytest.raises(ValueError):
        E.mst_edges(lined, period=1.0)
    with pytest.raises(ValueError):
        E.mst_core_d2(lined, 5, period=1.0)
    with pytest.raises(ValueError):
        E.mst_edges(index, torch.zeros(49), period=1.0)
    with pytest.raises(ValueError):
        K.mst_periodic_cpu(p, 1.0, torch.full((50,), math.inf))

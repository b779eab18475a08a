"""The periodic minimum spanning tree on the GPU (mst.hip under a period): the edges of
mst_edges(..., period=) equal to the brute-force oracle K.mst_periodic_cpu bit for bit, with the
device error word at 0, the periodic core distances of mst_core_d2, and mst_labels equal to the
periodic friends-of-friends labels of cluster_labels. Data sets, indexes and oracle results are
computed once per module."""
import math

import numpy as np
import pytest
import torch

import mst_ref
from datasets import GENERATORS, lattice, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of kWalkStep = 6
PERIODS = {"L1": 1.0, "xz": (1.0, INF, 1.0)}

_DATA: dict = {}
_INDEX: dict = {}
_ORACLE: dict = {}
_CORE: dict = {}


def data(name):
    if name not in _DATA:
        if name == "lattice":  # spacing 1 / 16, period 16 spacings: every face point has a wrapped neighbour
            _DATA[name] = lattice(16)
        elif name == "shifted":  # the period away from the data: no coordinate inside [0, 1)
            _DATA[name] = (data("uniform") + 7.25).contiguous()
        elif name == "shifted_wrapped":
            _DATA[name] = E.wrap_points(data("shifted"), 1.0)
        else:
            _DATA[name] = GENERATORS[name](N, seed=21)
    return _DATA[name]


def index_of(name, grid="auto"):
    key = (name, grid)
    if key not in _INDEX:
        old = E.GRID
        E.GRID = grid
        try:
            _INDEX[key] = E.build_index(data(name).to(DEV), grid=True)
        finally:
            E.GRID = old
    return _INDEX[key]


def core_of(name, per):
    """The oracle's squared periodic 5th-neighbour distances (CPU tensor)."""
    if (name, per) not in _CORE:
        p = data(name)
        _CORE[(name, per)] = K.kth_periodic_cpu(p, p, 5, INF, PERIODS[per])
    return _CORE[(name, per)]


def oracle(name, per, core=False):
    key = (name, per, core)
    if key not in _ORACLE:
        _ORACLE[key] = K.mst_periodic_cpu(data(name), PERIODS[per], core_of(name, per) if core else None)
    return _ORACLE[key]


def run(index, core=None, **kw):
    rows, d2 = E.mst_edges(index, core, **kw)
    assert E.LAST_MST_ERRORS[0] == 0
    assert rows.dtype == torch.int32 and d2.dtype == torch.float32 and rows.device.type == "cuda"
    assert rows.dim() == 2 and rows.shape[1] == 2 and rows.shape[0] == d2.shape[0]
    return rows.cpu(), d2.cpu()


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def describe(got, want):
    if got[1].shape != want[1].shape:
        return f"{got[1].shape[0]} edges, the oracle has {want[1].shape[0]}"
    bad = ((got[0] != want[0]).any(dim=1) | (got[1] != want[1])).nonzero().flatten()
    i = bad[:5]
    return (f"{bad.numel()} edges differ (first {i.tolist()}: {got[0][i].tolist()} {got[1][i].tolist()} vs "
            f"{want[0][i].tolist()} {want[1][i].tolist()})")


@pytest.mark.parametrize("per", sorted(PERIODS))
@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "lattice", "planar"])
def test_matches_oracle(name, per):
    want = oracle(name, per)
    assert want[1].shape[0] == data(name).shape[0] - 1
    got = run(index_of(name), period=PERIODS[per])
    assert same(got, want), describe(got, want)


def test_lattice_wraps_at_the_lattice_distance():
    """Every edge of the periodic lattice tree has the lattice distance, and some cross a face."""
    rows, d2 = oracle("lattice", "L1")
    assert d2.unique().numel() == 1
    p = data("lattice")
    assert bool(((p[rows[:, 0].long()] - p[rows[:, 1].long()]).abs().max(dim=1).values > 0.5).any())


@pytest.mark.parametrize("name", ["shifted", "shifted_wrapped"])
def test_period_away_from_the_data(name):
    want = oracle(name, "L1")
    assert not same(want, K.mst_cpu(data(name)))
    got = run(index_of(name), period=1.0)
    assert same(got, want), describe(got, want)


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_mutual_reachability_matches_oracle(name):
    index = index_of(name)
    core = core_of(name, "L1")
    got_core = E.mst_core_d2(index, 5, period=1.0)
    assert E.LAST_PERIODIC_KNN_ERRORS[0] == 0
    assert got_core.dtype == torch.float32 and got_core.device.type == "cuda"
    assert torch.equal(got_core.cpu().view(torch.int32), core.view(torch.int32))
    if name == "uniform":  # (points near a face have wrapped neighbours; the blobs need not)
        assert not torch.equal(got_core, E.mst_core_d2(index, 5))
    want = oracle(name, "L1", core=True)
    assert float(want[1].min()) >= float(core.min()) and not same(want, oracle(name, "L1"))
    got = run(index, got_core, period=1.0)
    assert same(got, want), describe(got, want)


def wrapped_edges(p, rows, d2):
    w = mst_ref.pair_weights(p)[rows[:, 0].numpy(), rows[:, 1].numpy()]
    return int((w.view(np.uint32) != d2.numpy().view(np.uint32)).sum())


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 4097])
def test_edge_sizes(n):
    # (two uniform points need not wrap: these two do, across the x face)
    p = torch.tensor([[0.05, 0.5, 0.5], [0.95, 0.6, 0.4]]) if n == 2 else uniform(n, seed=30 + n)
    want = K.mst_periodic_cpu(p, 1.0)
    if 2 <= n <= 64:  # one bucket: a wrapped pair is found in the own bucket of a shifted image
        assert wrapped_edges(p, *want) >= 1
    got = run(E.build_index(p.to(DEV)), period=1.0)
    assert got[1].shape[0] == n - 1
    assert same(got, want), describe(got, want)
    got = E.mst_points(p.to(DEV), period=1.0)
    assert same((got[0].cpu(), got[1].cpu()), want)


def test_nan_and_inf_points():
    p = data("uniform")[:5000].clone()
    bad = (1234, 77, 4000, 4001)
    p[1234] = math.nan
    p[77, 1] = math.nan
    p[4000, 0] = math.inf
    p[4001, 2] = -math.inf
    want = K.mst_periodic_cpu(p, 1.0)
    got = run(E.build_index(p.to(DEV)), period=1.0)
    assert got[1].shape[0] == 5000 - len(bad) - 1
    assert not bool(torch.isin(got[0], torch.tensor(bad, dtype=torch.int32)).any())
    assert same(got, want), describe(got, want)
    # the periodic core distances of such a set: 0 for a row that is no vertex
    core = K.kth_periodic_cpu(p, p, 5, INF, 1.0)
    core[list(bad)] = 0.0
    index = E.build_index(p.to(DEV), grid=True)
    got_core = E.mst_core_d2(index, 5, period=1.0)
    assert E.LAST_PERIODIC_KNN_ERRORS[0] == 0
    assert torch.equal(got_core.cpu().view(torch.int32), core.view(torch.int32))
    want = K.mst_periodic_cpu(p, 1.0, core)
    got = run(index, got_core, period=1.0)
    assert same(got, want), describe(got, want)
    # a set without a vertex, one with a single vertex, one with two (a pair that wraps)
    q = torch.full((70, 3), math.nan)
    assert run(E.build_index(q.to(DEV)), period=1.0)[1].shape == (0,)
    q[33] = 0.5
    assert run(E.build_index(q.to(DEV)), period=1.0)[1].shape == (0,)
    q[33] = torch.tensor([0.5, 0.03, 0.5])
    q[68] = torch.tensor([0.5, 0.97, 0.5])
    got = run(E.build_index(q.to(DEV)), period=1.0)
    want = K.mst_periodic_cpu(q, 1.0)
    assert got[0].tolist() == [[33, 68]] and same(got, want)
    assert float(got[1][0]) < 0.01  # (the open-box pair is 0.94 apart)


@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_identities(name):
    index = index_of(name)
    open_tree = run(index)
    got = run(index, period=(INF, INF, INF))
    assert same(got, open_tree), describe(got, open_tree)
    got = run(index, period=1e6)  # no pair of the unit box wraps
    assert same(got, open_tree), describe(got, open_tree)
    core = E.mst_core_d2(index, 5)
    assert torch.equal(E.mst_core_d2(index, 5, period=INF).view(torch.int32), core.view(torch.int32))
    assert torch.equal(E.mst_core_d2(index, 5, period=1e6).view(torch.int32), core.view(torch.int32))


def eps_of(p, f):
    extent = float((p.max(0).values - p.min(0).values).max())
    return f * extent * p.shape[0] ** (-1.0 / 3.0)


@pytest.mark.parametrize("per", sorted(PERIODS))
@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_labels_equal_cluster_labels(name, per):
    index, period = index_of(name), PERIODS[per]
    rows, d2 = E.mst_edges(index, period=period)
    for f in (0.5, 0.9, 2.0):
        eps = eps_of(data(name), f)
        want = E.cluster_labels(index, eps, 1, period=period)[0]
        got = E.mst_labels(rows, d2, index.n, eps)
        assert E.LAST_MST_ERRORS[0] == 0
        assert got.dtype == torch.int32 and got.device.type == "cuda"
        assert torch.equal(got, want), f"f = {f}: {int((got != want).sum())} labels differ"
        assert torch.equal(E.mst_labels(rows.cpu(), d2.cpu(), index.n, eps), want.cpu())
    # a cutoff exactly on an edge's d2: the strict < leaves it out
    mid = float(d2[d2.shape[0] // 2])
    got = E.mst_labels(rows, d2, index.n, mid, squared=True)
    assert torch.equal(got, E.cluster_labels(index, mid, 1, squared=True, period=period)[0])
    assert int(got.unique().numel()) == index.n - int((d2 < mid).sum())


def test_reproducible_and_grid_independent():
    for name, core in (("uniform", False), ("clustered", True), ("lattice", False)):
        c = core_of(name, "L1").to(DEV) if core else None
        a = run(index_of(name, "on"), c, period=1.0)
        b = run(index_of(name, "on"), c, period=1.0)
        off = run(index_of(name, "off"), c, period=1.0)
        assert same(a, b) and same(a, off)
        assert same(a, oracle(name, "L1", core))


def test_rounds_and_stats():
    n = N
    for period, images in ((1.0, True), (1e6, False)):
        stats = E.KnnStats()
        E.reset_kernels_used()
        got = run(index_of("uniform"), stats=stats, period=period)
        assert "mst" in E.kernels_used()
        c = stats.counters
        print(period, c)
        comps = c["mst_components"]
        assert c["mst_rounds"] == len(comps) <= math.ceil(math.log2(n))
        assert comps[0] == n
        for before, after in zip(comps, comps[1:] + [1]):
            assert 2 * after <= before
        assert c["mst_evals"] > 0 and c["mst_buckets"] > 0 and c["mst_nodes"] > 0 and "mst_cas_retries" in c
        assert (c["mst_images"] > 0) == images
        if images:
            assert same(got, oracle("uniform", "L1"))
    stats = E.KnnStats()
    run(index_of("uniform"), stats=stats)
    assert stats.counters["mst_images"] == 0


def test_refuses_bad_arguments_before_any_kernel():
    index = index_of("uniform")
    E.reset_kernels_used()
    for bad in (0, -1, math.nan, (1.0, 1.0), (1.0, 0.0, 1.0)):
        with pytest.raises(ValueError):
            E.mst_edges(index, period=bad)
        with pytest.raises(ValueError):
            E.mst_points(data("uniform").to(DEV), period=bad)
        with pytest.raises(ValueError):
            E.mst_core_d2(index, 5, period=bad)
    with pytest.raises(ValueError):
        E.mst_edges(index, torch.zeros(index.n - 1, device=DEV), period=1.0)
    p = GENERATORS["tilted_plane"](70_000, seed=5).to(DEV)
    idx = E.build_index(p, frame=E.flat_frame(p))
    assert idx.qrot is not None
    with pytest.raises(ValueError):
        E.mst_edges(idx, period=1.0)
    with pytest.raises(ValueError):
        E.mst_core_d2(idx, 5, period=1.0)
    assert "mst" not in E.kernels_used() and "knn_periodic" not in E.kernels_used()

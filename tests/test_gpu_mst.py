"""The minimum spanning tree on the GPU (mst.hip): the edges of mst_edges equal to the brute-force
oracle K.mst_cpu bit for bit, with the device error word at 0, and mst_labels equal to the
friends-of-friends labels of cluster_labels. Data sets and oracle results are computed once per
module."""
import math

import pytest
import torch

from datasets import GENERATORS, lattice, uniform
from mpi_cuda_largescaleknn_amd._native import NativeError
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of kWalkStep = 6

_DATA: dict = {}
_INDEX: dict = {}
_ORACLE: dict = {}
_CORE: dict = {}


def data(name):
    if name not in _DATA:
        _DATA[name] = lattice(16) if name == "lattice" else GENERATORS[name](N, seed=21)
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


def core_of(name):
    """Squared 5th-neighbour distances from the engine's neighbour lists (CPU tensor)."""
    if name not in _CORE:
        dist = E.knn_neighbors(data(name).to(DEV), 5)[1][:, 4]
        _CORE[name] = (dist * dist).cpu()
    return _CORE[name]


def oracle(name, core=False):
    key = (name, core)
    if key not in _ORACLE:
        _ORACLE[key] = K.mst_cpu(data(name), core_of(name) if core else None)
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


@pytest.mark.parametrize("name", ["uniform", "clustered", "mixed_scale", "duplicates", "line", "planar", "lattice"])
def test_matches_oracle(name):
    want = oracle(name)
    assert want[1].shape[0] == data(name).shape[0] - 1
    got = run(index_of(name))
    assert same(got, want), describe(got, want)


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_mutual_reachability_matches_oracle(name):
    core = core_of(name)
    want = oracle(name, core=True)
    assert float(want[1].min()) >= float(core.min()) and not same(want, oracle(name))
    got = run(index_of(name), core.to(DEV))
    assert same(got, want), describe(got, want)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097])
def test_edge_sizes(n):
    p = uniform(n, seed=30 + n)
    want = K.mst_cpu(p)
    got = run(E.build_index(p.to(DEV)))
    assert got[1].shape[0] == n - 1
    assert same(got, want), describe(got, want)
    got = E.mst_points(p.to(DEV))
    assert same((got[0].cpu(), got[1].cpu()), want)


def test_nan_and_inf_points():
    p = data("uniform")[:5000].clone()
    bad = (1234, 77, 4000, 4001)
    p[1234] = math.nan
    p[77, 1] = math.nan
    p[4000, 0] = math.inf
    p[4001, 2] = -math.inf
    want = K.mst_cpu(p)
    got = run(E.build_index(p.to(DEV)))
    assert got[1].shape[0] == 5000 - len(bad) - 1
    assert not bool(torch.isin(got[0], torch.tensor(bad, dtype=torch.int32)).any())
    assert same(got, want), describe(got, want)
    # a set without a vertex, and one with a single vertex
    q = torch.full((70, 3), math.nan)
    assert run(E.build_index(q.to(DEV)))[1].shape == (0,)
    q[33] = 0.5
    assert run(E.build_index(q.to(DEV)))[1].shape == (0,)
    q[68] = 0.25
    got = run(E.build_index(q.to(DEV)))
    assert got[0].tolist() == [[33, 68]] and same(got, K.mst_cpu(q))


def eps_of(p, f):
    extent = float((p.max(0).values - p.min(0).values).max())
    return f * extent * p.shape[0] ** (-1.0 / 3.0)


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_labels_equal_cluster_labels(name):
    index = index_of(name)
    rows, d2 = E.mst_edges(index)
    for f in (0.5, 0.9, 2.0):
        eps = eps_of(data(name), f)
        want = E.cluster_labels(index, eps, 1)[0]
        got = E.mst_labels(rows, d2, index.n, eps)
        assert E.LAST_MST_ERRORS[0] == 0
        assert got.dtype == torch.int32 and got.device.type == "cuda"
        assert torch.equal(got, want), f"f = {f}: {int((got != want).sum())} labels differ"
        # the host form over the same edges
        assert torch.equal(E.mst_labels(rows.cpu(), d2.cpu(), index.n, eps), want.cpu())
    # a cutoff exactly on an edge's d2: the strict < leaves it out
    mid = float(d2[d2.shape[0] // 2])
    got = E.mst_labels(rows, d2, index.n, mid, squared=True)
    assert torch.equal(got, E.cluster_labels(index, mid, 1, squared=True)[0])
    assert int(got.unique().numel()) == index.n - int((d2 < mid).sum())


def test_reproducible_and_grid_independent():
    for name, core in (("uniform", False), ("clustered", True), ("lattice", False)):
        c = core_of(name).to(DEV) if core else None
        a = run(index_of(name, "on"), c)
        b = run(index_of(name, "on"), c)
        off = run(index_of(name, "off"), c)
        assert same(a, b) and same(a, off)
        assert same(a, oracle(name, core))


@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "lattice"])
def test_rounds_and_stats(name):
    stats = E.KnnStats()
    E.reset_kernels_used()
    got = run(index_of(name), stats=stats)
    assert "mst" in E.kernels_used()
    c = stats.counters
    print(c)
    n = data(name).shape[0]
    comps = c["mst_components"]
    assert c["mst_rounds"] == len(comps) <= math.ceil(math.log2(n))
    assert comps[0] == n
    for before, after in zip(comps, comps[1:] + [1]):
        assert 2 * after <= before
    for nm in ("mst_evals", "mst_nodes", "mst_buckets", "mst_cas_retries"):
        assert nm in c
    assert c["mst_evals"] > 0 and c["mst_buckets"] > 0 and c["mst_nodes"] > 0
    assert same(got, oracle(name))


def test_refuses_bad_arguments_before_any_kernel():
    index = index_of("uniform")
    n = index.n
    E.reset_kernels_used()
    bad = [torch.zeros(n - 1, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n),
           torch.full((n,), -1.0, device=DEV), torch.full((n,), math.nan, device=DEV),
           torch.full((n,), math.inf, device=DEV)]
    for core in bad:
        with pytest.raises(ValueError):
            E.mst_edges(index, core)
    p = GENERATORS["tilted_plane"](70_000, seed=5).to(DEV)
    idx = E.build_index(p, frame=E.flat_frame(p))
    assert idx.qrot is not None
    with pytest.raises(ValueError):
        E.mst_edges(idx)
    assert "mst" not in E.kernels_used()
    rows, d2 = E.mst_edges(index)
    for eps in (-1.0, math.nan):
        with pytest.raises(ValueError):
            E.mst_labels(rows, d2, n, eps)
    with pytest.raises(ValueError):
        E.mst_labels(rows, d2.cpu(), n, 0.1)
    with pytest.raises(ValueError):
        E.mst_labels(rows, d2, n - 1, 0.1)
    # an edge that names a row outside [0, n): refused by the hook, nothing is written out of bounds
    out_of_range = rows.clone()
    out_of_range[0, 1] = n
    with pytest.raises(NativeError):
        E.mst_labels(out_of_range, d2, n, math.inf)
    assert E.LAST_MST_ERRORS[0] != 0
    E.mst_labels(rows, d2, n, 0.1)
    assert E.LAST_MST_ERRORS[0] == 0

"""Density clustering on the GPU (cluster.hip): labels and core flags of cluster_labels equal
to the brute-force oracle K.cluster_cpu, with the device error word at 0. Data sets and oracle
results are computed once per module."""
import math
import os

import numpy as np
import pytest
import torch

from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd.apps import cluster as cluster_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of kWalkStep = 6

# (generator, f, min_pts) -> (clusters, core points) of the oracle: the regime each case is
# meant to be in. eps = f * extent * n^(-1/3).
REGIMES = {
    ("uniform", 0.5, 1): (9137, N),          # mostly singletons
    ("uniform", 0.5, 5): (19, 21),
    ("uniform", 0.9, 1): (1335, N),          # near percolation: the largest has 6155 points
    ("uniform", 0.9, 5): (574, 4059),        # the rest border or noise: the border walk
    ("uniform", 2.0, 1): (1, N),             # one giant component
    ("uniform", 2.0, 5): (1, N - 1),         # one point is not core
    ("mixed_scale", 0.9, 1): (2524, N),
    ("mixed_scale", 0.9, 5): (161, 6366),
    ("clustered", 0.5, 1): (20, N),
    ("clustered", 0.5, 5): (19, 11996),
    ("duplicates", 0.5, 1): (50, N),         # exact copies: clique nodes above the bucket level
    ("duplicates", 0.5, 5): (50, N),
    ("line", 0.5, 1): (1, N),                # one 12 000-point chain: deep union trees
    ("line", 0.5, 5): (1, N),
    ("planar", 0.9, 1): (1, N),
    ("planar", 0.9, 5): (1, N),
    ("tilted_plane", 0.9, 1): (1, N),
    ("tilted_plane", 0.9, 5): (1, N),
}

_DATA: dict = {}
_INDEX: dict = {}
_ORACLE: dict = {}


def data(name):
    if name not in _DATA:
        _DATA[name] = GENERATORS[name](N, seed=21)
    return _DATA[name]


def eps_of(p, f):
    extent = float((p.max(0).values - p.min(0).values).max())
    return f * extent * p.shape[0] ** (-1.0 / 3.0)


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


def oracle(name, f, min_pts):
    key = (name, f, min_pts)
    if key not in _ORACLE:
        p = data(name)
        _ORACLE[key] = K.cluster_cpu(p, E.cut2_of(eps_of(p, f)), min_pts)
    return _ORACLE[key]


def run(index, eps, min_pts, **kw):
    labels, core = E.cluster_labels(index, eps, min_pts, **kw)
    assert E.LAST_CLUSTER_ERRORS[0] == 0
    assert labels.dtype == torch.int32 and core.dtype == torch.bool and labels.device.type == "cuda"
    return labels.cpu(), core.cpu()


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def describe(got, want):
    bl = (got[0] != want[0]).nonzero().flatten()
    bc = (got[1] != want[1]).nonzero().flatten()
    return (f"{bl.numel()} labels differ (first rows {bl[:5].tolist()}: {got[0][bl[:5]].tolist()} vs "
            f"{want[0][bl[:5]].tolist()}), {bc.numel()} core flags differ (first rows {bc[:5].tolist()})")


@pytest.mark.parametrize("name,f,min_pts", sorted(REGIMES))
def test_matches_oracle(name, f, min_pts):
    want = oracle(name, f, min_pts)
    # the oracle's own result is in the regime the case is meant to cover
    assert (E.compact_labels(want[0])[1], int(want[1].sum())) == REGIMES[(name, f, min_pts)]
    got = run(index_of(name), eps_of(data(name), f), min_pts)
    assert same(got, want), describe(got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("min_pts", [1, 3])
def test_edge_sizes(n, min_pts):
    p = uniform(n, seed=30 + n)
    eps = 0.9 * n ** (-1.0 / 3.0)
    want = K.cluster_cpu(p, E.cut2_of(eps), min_pts)
    got = run(E.build_index(p.to(DEV)), eps, min_pts)
    assert same(got, want), describe(got, want)


@pytest.mark.parametrize("min_pts", [1, 100])
def test_many_exact_copies(min_pts):
    """Two sites with 70 000 copies each and 1 000 scattered points: O(n) through the clique
    nodes. Checked against the closed form, not the quadratic oracle."""
    m, extra = 70_000, 1_000
    g = torch.Generator().manual_seed(5)
    bases = torch.tensor([[0.25, 0.25, 0.25], [0.75, 0.5, 0.75]])
    p = torch.cat([bases[0].repeat(m, 1), bases[1].repeat(m, 1), uniform(extra, seed=6)])
    site = torch.cat([torch.zeros(m), torch.ones(m), torch.full((extra,), 2.0)]).long()
    order = torch.randperm(p.shape[0], generator=g)
    p, site = p[order].contiguous(), site[order]
    n = p.shape[0]
    eps = 1e-3
    # the closed form holds: every scattered point has itself within eps and nothing else
    assert bool((K.radius_count_cpu(p, p[site == 2], E.cut2_of(eps)) == 1).all())
    want = torch.arange(n, dtype=torch.int32) if min_pts == 1 else torch.full((n,), -1, dtype=torch.int32)
    for s in (0, 1):
        want[site == s] = int((site == s).nonzero()[0])
    stats = E.KnnStats()
    got = run(E.build_index(p.to(DEV)), eps, min_pts, stats=stats)
    assert torch.equal(got[0], want)
    assert torch.equal(got[1], (site < 2) if min_pts > 1 else torch.ones(n, dtype=torch.bool))
    c = stats.counters
    print(c)
    assert c["cluster_evals"] < 64 * n and c["cluster_clique_accepts"] > 0


def test_strict_comparison():
    p = torch.tensor([[0.1, 0.2, 0.3], [0.4, 0.6, 0.35]])
    off, idx, d2s = K.radius_cpu(p, p[:1], math.inf)
    d2 = float(d2s[idx.tolist().index(1)])  # the oracle's own dist2 of the pair
    index = E.build_index(p.to(DEV))
    assert run(index, d2, 1, squared=True)[0].tolist() == [0, 1]
    got = run(index, d2, 2, squared=True)
    assert got[0].tolist() == [-1, -1] and got[1].tolist() == [False, False]
    above = float(np.nextafter(np.float32(d2), np.float32(np.inf)))
    got = run(index, above, 2, squared=True)
    assert got[0].tolist() == [0, 0] and got[1].tolist() == [True, True]
    # eps = 0 and eps = inf
    q = data("uniform")[:3000].contiguous()
    index = E.build_index(q.to(DEV))
    for eps in (0.0, math.inf):
        for min_pts in (1, 4):
            want = K.cluster_cpu(q, E.cut2_of(eps), min_pts)
            got = run(index, eps, min_pts)
            assert same(got, want), describe(got, want)


@pytest.mark.parametrize("min_pts", [1, 3])
def test_nan_and_inf_points(min_pts):
    p = data("uniform")[:5000].clone()
    p[1234] = math.nan
    p[77, 1] = math.nan
    p[4000, 0] = math.inf
    eps = eps_of(data("uniform")[:5000], 0.9)
    want = K.cluster_cpu(p, E.cut2_of(eps), min_pts)
    for row in (1234, 77, 4000):
        assert not bool(want[1][row]) and int(want[0][row]) == (row if min_pts == 1 else -1)
    got = run(E.build_index(p.to(DEV)), eps, min_pts)
    assert same(got, want), describe(got, want)


def test_reproducible_and_grid_independent():
    for name, f, min_pts in (("uniform", 0.9, 5), ("uniform", 2.0, 1), ("clustered", 0.5, 5)):
        eps = eps_of(data(name), f)
        a = run(index_of(name, "on"), eps, min_pts)
        b = run(index_of(name, "on"), eps, min_pts)
        c = run(index_of(name, "off"), eps, min_pts)
        assert same(a, b) and same(a, c)
        assert same(a, oracle(name, f, min_pts))
        # both forms of the hook walk (each pair united from one side, or from both)
        assert E.CLUSTER_HALF
        E.CLUSTER_HALF = False
        try:
            d = run(index_of(name, "on"), eps, min_pts)
        finally:
            E.CLUSTER_HALF = True
        assert same(a, d)


def test_cluster_points_and_kernels_used():
    p = data("uniform")
    eps = eps_of(p, 0.9)
    E.reset_kernels_used()
    a = E.cluster_points(p.to(DEV), eps, 5)
    assert "cluster" in E.kernels_used()
    b = E.cluster_labels(E.build_index(p.to(DEV)), eps, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert same((a[0].cpu(), a[1].cpu()), oracle("uniform", 0.9, 5))
    stats = E.KnnStats()
    E.cluster_labels(index_of("uniform"), eps, 5, stats=stats)
    for nm in ("cluster_evals", "cluster_nodes", "cluster_buckets", "cluster_clique_accepts", "cluster_cas_retries"):
        assert nm in stats.counters
    assert stats.counters["cluster_evals"] > 0 and stats.counters["cluster_buckets"] > 0
    got = E.cluster_points(torch.empty((0, 3), device=DEV), 0.1, 2)
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[0].device.type == "cuda"


def test_refuses_bad_arguments_and_rotated_index():
    p = GENERATORS["tilted_plane"](70_000, seed=5).to(DEV)
    idx = E.build_index(p, frame=E.flat_frame(p))
    assert idx.qrot is not None
    with pytest.raises(ValueError):
        E.cluster_labels(idx, 0.01, 2)
    index = index_of("uniform")
    for eps, min_pts in ((-1.0, 1), (math.nan, 1), (0.1, 0)):
        with pytest.raises(ValueError):
            E.cluster_labels(index, eps, min_pts)


def test_app_round_trip(tmp_path, capsys):
    p = data("uniform")
    eps = eps_of(p, 0.9)
    fp = str(tmp_path / "p.float3")
    io.write_points(fp, p)
    pre = str(tmp_path / "cl")
    assert cluster_app.main([fp, "-r", repr(eps), "--min-pts", "5", "-o", pre, "--device", "cuda",
                             "--stats", str(tmp_path / "s.json")]) == 0
    want = oracle("uniform", 0.9, 5)
    assert f"{N} points: 574 clusters, {int((want[0] < 0).sum())} noise points" in capsys.readouterr().out
    assert torch.equal(io.read_array(pre + ".labels", torch.int32), want[0])
    assert os.path.getsize(pre + ".core") == N
    assert tools.main(["ccheck", fp, pre, "-r", repr(eps), "--min-pts", "5"]) == 0
    assert "0 core flag mismatches, 0 label mismatches" in capsys.readouterr().out

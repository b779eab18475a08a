"""Periodic density clustering on the GPU (periodic.hip around the init / label passes of
cluster.hip): labels and core flags of cluster_labels with `period=` equal to the brute-force
oracle K.cluster_periodic_cpu, with the device error word at 0. Data sets and oracle results are
computed once per module."""
import math

import pytest
import torch

from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from test_periodic_cpu import closed_forms

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of kWalkStep = 6

CASES = [("uniform", 0.5), ("uniform", 0.9), ("uniform", 2.0), ("clustered", 0.5), ("duplicates", 0.5)]

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# Seeds at which the period changes the number of clusters in every case below (asserted there
# on the oracle's own results): with min_pts = 5 at f = 0.5 only some twenty tiny clusters exist,
# and few seeds put one of them across a face.
SEEDS = {"uniform": 33, "clustered": 31, "duplicates": 38}


def data(name):
    def make():
        if name == "duplicates":  # 400 sites of 30 copies
            return GENERATORS[name](N, seed=SEEDS[name], ndistinct=400).contiguous()
        return E.wrap_points(GENERATORS[name](N, seed=SEEDS[name]), 1.0).contiguous()
    return cached(("data", name), make)


def eps_of(f):
    """f mean spacings of N points in the unit box."""
    return f * N ** (-1.0 / 3.0)


def index_of(name):
    return cached(("index", name), lambda: E.build_index(data(name).to(DEV)))


def oracle(name, f, min_pts):
    return cached(("oracle", name, f, min_pts),
                  lambda: K.cluster_periodic_cpu(data(name), E.cut2_of(eps_of(f)), min_pts, 1.0))


def run(index, eps, min_pts, period=1.0, **kw):
    labels, core = E.cluster_labels(index, eps, min_pts, period=period, **kw)
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


def n_clusters(labels):
    return E.compact_labels(labels)[1]


@pytest.mark.parametrize("min_pts", [1, 5])
@pytest.mark.parametrize("name,f", CASES)
def test_matches_oracle(name, f, min_pts):
    want = oracle(name, f, min_pts)
    # the period matters for the oracle's own result (or everything is one component anyway)
    open_box = K.cluster_cpu(data(name), E.cut2_of(eps_of(f)), min_pts)
    if f == 2.0:
        assert n_clusters(want[0]) == 1 and n_clusters(open_box[0]) == 1
    else:
        assert n_clusters(want[0]) != n_clusters(open_box[0])
    got = run(index_of(name), eps_of(f), min_pts)
    assert same(got, want), describe(got, want)


def test_closed_forms_on_the_gpu():
    def cluster(p, eps, period):
        if period is None:
            return E.cluster_points(p.to(DEV), eps, 1)[0].cpu()
        return run(E.build_index(p.to(DEV)), eps, 1, period=period)[0]

    closed_forms(cluster)
    one = torch.tensor([[0.3, 0.9, 0.0]], device=DEV)
    assert E.radius_query_counts(one, one, 0.5, period=1.0).tolist() == [1]
    assert run(E.build_index(one), 0.5, 1)[0].tolist() == [0]


@pytest.mark.parametrize("min_pts", [1, 3])
def test_anisotropic_period_and_far_origin(min_pts):
    p = (uniform(N, seed=32) * torch.tensor([1.0, 2.0, 1.0])).contiguous()
    eps = 0.9 * (2.0 / N) ** (1.0 / 3.0)
    for pts, per in ((p, (1.0, 2.0, INF)), ((data("uniform") + 4096.0).contiguous(), 1.0)):
        want = K.cluster_periodic_cpu(pts, E.cut2_of(eps), min_pts, per)
        assert not torch.equal(want[0], K.cluster_cpu(pts, E.cut2_of(eps), min_pts)[0])
        got = run(E.build_index(pts.to(DEV)), eps, min_pts, period=per)
        assert same(got, want), describe(got, want)


@pytest.mark.parametrize("min_pts", [1, 3])
def test_nan_and_inf_points(min_pts):
    p = data("uniform")[:5000].clone()
    p[1234] = math.nan
    p[77, 1] = math.nan
    p[4000, 0] = INF
    eps = 0.9 * 5000 ** (-1.0 / 3.0)
    want = K.cluster_periodic_cpu(p, E.cut2_of(eps), min_pts, 1.0)
    for row in (1234, 77, 4000):
        assert not bool(want[1][row]) and int(want[0][row]) == (row if min_pts == 1 else -1)
    got = run(E.build_index(p.to(DEV)), eps, min_pts)
    assert same(got, want), describe(got, want)


def test_open_period_equals_the_open_box_kernels():
    index = index_of("uniform")
    for f, min_pts in ((0.9, 1), (0.9, 5), (2.0, 1)):
        got = run(index, eps_of(f), min_pts, period=INF)
        want = E.cluster_labels(index, eps_of(f), min_pts)
        assert same(got, (want[0].cpu(), want[1].cpu()))
    assert "cluster_periodic" in E.kernels_used()


@pytest.mark.parametrize("min_pts", [1, 100])
def test_many_exact_copies_across_a_face(min_pts):
    """Two sites of 70 000 exact copies at x = 0.001 and x = 0.999 and 1 000 scattered points:
    one cluster under the period (the sites are 0.002 apart through the face), O(n) through the
    clique nodes; the scattered points are a lattice, each alone within eps. Checked against the closed form, not the quadratic oracle."""
    m, extra = 70_000, 1_000
    g = torch.Generator().manual_seed(5)
    bases = torch.tensor([[0.001, 0.5, 0.5], [0.999, 0.5, 0.5]])
    t = torch.arange(10, dtype=torch.float32)  # a 10^3 lattice, 0.08 apart and away from the sites
    scattered = torch.stack(torch.meshgrid(0.1 + 0.08 * t, 0.04 + 0.09 * t, 0.04 + 0.09 * t, indexing="ij"), -1).view(-1, 3)
    p = torch.cat([bases[0].repeat(m, 1), bases[1].repeat(m, 1), scattered])
    site = torch.cat([torch.zeros(m), torch.ones(m), torch.full((extra,), 2.0)]).long()
    order = torch.randperm(p.shape[0], generator=g)
    p, site = p[order].contiguous(), site[order]
    n = p.shape[0]
    eps = 0.01
    # the closed form holds: every scattered point has itself within eps and nothing else
    assert bool((K.radius_periodic_count_cpu(p, p[site == 2], E.cut2_of(eps), 1.0) == 1).all())
    want = torch.arange(n, dtype=torch.int32) if min_pts == 1 else torch.full((n,), -1, dtype=torch.int32)
    want[site < 2] = int((site < 2).nonzero()[0])
    stats = E.KnnStats()
    index = E.build_index(p.to(DEV))
    got = run(index, eps, min_pts, stats=stats)
    assert torch.equal(got[0], want)
    assert torch.equal(got[1], (site < 2) if min_pts > 1 else torch.ones(n, dtype=torch.bool))
    print(stats.counters)
    assert stats.counters["cluster_clique_accepts"] > 0
    # without the period the two sites are two clusters
    assert n_clusters(E.cluster_labels(index, eps, min_pts)[0].cpu()) == n_clusters(got[0]) + 1


def test_labels_do_not_depend_on_the_order_of_the_unions():
    """Near percolation, five runs in one process: identical labels whatever order the atomics
    of the hooks land in."""
    index = index_of("uniform")
    first = run(index, eps_of(0.9), 1)
    assert same(first, oracle("uniform", 0.9, 1))
    for _ in range(4):
        assert same(run(index, eps_of(0.9), 1), first)


def test_refuses_bad_arguments_and_rotated_index():
    p = GENERATORS["tilted_plane"](70_000, seed=5).to(DEV)
    idx = E.build_index(p, frame=E.flat_frame(p))
    assert idx.qrot is not None
    with pytest.raises(ValueError):
        E.cluster_labels(idx, 0.01, 2, period=1.0)
    with pytest.raises(ValueError):
        E.radius_counts(idx, p[:10].contiguous(), 0.01, period=1.0)
    index = index_of("uniform")
    for eps, per in ((0.6, 1.0), (0.1, 0.0), (0.1, (1.0, 1.0)), (0.1, math.nan)):
        with pytest.raises(ValueError):
            E.cluster_labels(index, eps, 1, period=per)
    with pytest.raises(ValueError, match="not supported"):
        E.point_radius_counts(index, data("uniform")[:10].to(DEV), torch.full((N,), 0.05, device=DEV), period=1.0)

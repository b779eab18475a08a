"""The minimum spanning tree on the CPU path: the brute-force oracle K.mst_cpu against a plain
numpy Kruskal over all pairs (mst_ref.py), mst_labels against the friends-of-friends oracle, the
argument errors and the CPU-index path of the engine."""
import math

import numpy as np
import pytest
import torch

import mpi_cuda_largescaleknn_amd as pkg
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

import mst_ref
from datasets import lattice, line, uniform


def sites(nsites=20, copies=30, seed=3):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand((nsites, 3), generator=g).repeat_interleave(copies, 0)
    return p[torch.randperm(p.shape[0], generator=g)].contiguous()


def with_bad_rows(n=400, seed=4):
    p = uniform(n, seed=seed)
    p[17] = math.nan
    p[40, 1] = math.nan
    p[99, 0] = math.inf
    p[250, 2] = -math.inf
    return p


def core5(p):
    """Squared 5th-neighbour distances of the finite rows (the oracle's own), 0 elsewhere."""
    c = K.kth_cpu(p, p, 5, math.inf)
    c[~torch.isfinite(p).all(dim=1)] = 0.0
    return c


CASES = {
    "uniform": lambda: (uniform(1000, seed=1), None),
    "duplicates": lambda: (sites(), None),
    "lattice": lambda: (lattice(8), None),
    "line": lambda: (line(700, seed=2), None),
    "core_k5": lambda: (uniform(800, seed=5), "k5"),
    "nan_inf": lambda: (with_bad_rows(), None),
    "nan_inf_core_k5": lambda: (with_bad_rows(), "k5"),
}


def check(got, want):
    rows, d2 = got
    assert rows.dtype == torch.int32 and d2.dtype == torch.float32
    assert rows.shape == want[0].shape and d2.shape == want[1].shape
    assert np.array_equal(rows.numpy(), want[0])
    assert np.array_equal(d2.numpy().view(np.uint32), want[1].view(np.uint32))


def test_exported():
    assert pkg.mst_edges is E.mst_edges and pkg.mst_points is E.mst_points and pkg.mst_labels is E.mst_labels


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_against_reference(name):
    p, core = CASES[name]()
    core = core5(p) if core else None
    want = mst_ref.mst(p, core)
    finite = torch.isfinite(p).all(dim=1)
    assert want[1].shape[0] == int(finite.sum()) - 1
    got = K.mst_cpu(p, core)
    check(got, want)
    rows = got[0]
    # every row is (lo, hi), no edge touches a row that is no vertex, keys ascend strictly
    assert bool((rows[:, 0] < rows[:, 1]).all()) and bool(finite[rows.long()].all())
    key = [(int(b), int(lo), int(hi)) for b, (lo, hi) in zip(got[1].view(torch.int32).tolist(), rows.tolist())]
    assert all(x < y for x, y in zip(key, key[1:]))
    # the engine on a CPU index, and from the points
    check(E.mst_edges(E.build_index(p), core), want)
    check(E.mst_points(p, core), want)


def test_lattice_ties_are_decided_by_the_key():
    """Every nearest distance of the lattice ties: all edges have one weight, and the tree is the
    one Kruskal builds from the pairs at that weight in (lo, hi) order."""
    rows, d2 = K.mst_cpu(lattice(8))
    assert d2.unique().numel() == 1 and rows.shape[0] == 511
    assert rows[0].tolist() == [0, 1]


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_sets(n):
    p = uniform(n, seed=7)
    want = mst_ref.mst(p)
    assert want[0].shape == (max(n - 1, 0), 2)
    check(K.mst_cpu(p), want)
    check(E.mst_points(p), want)
    check(E.mst_edges(E.build_index(p)), want)
    check(E.mst_points(p, torch.zeros(n)), want)


def test_core_distances_change_the_weights_only_upwards():
    p = uniform(500, seed=8)
    plain = K.mst_cpu(p)
    core = core5(p)
    mr = K.mst_cpu(p, core)
    assert float(mr[1].min()) >= float(core.min()) and float(mr[1].sum()) > float(plain[1].sum())
    check(K.mst_cpu(p, torch.zeros(500)), (plain[0].numpy(), plain[1].numpy()))
    # -0 is 0: the max of the contract compares bits
    check(K.mst_cpu(p, -torch.zeros(500)), (plain[0].numpy(), plain[1].numpy()))
    check(E.mst_points(p, -torch.zeros(500)), (plain[0].numpy(), plain[1].numpy()))
    index = E.build_index(p)
    got = E.mst_core_d2(index, 5)
    assert torch.equal(got, core)


@pytest.mark.parametrize("name", ["uniform", "nan_inf"])
def test_labels_equal_friends_of_friends(name):
    p, _ = CASES[name]()
    n = p.shape[0]
    rows, d2 = K.mst_cpu(p)
    on_edge = float(d2[d2.shape[0] // 2])  # exactly an edge's d2: the strict < leaves that edge out
    scale = float(np.sqrt(np.median(d2.numpy())))
    cuts = [(E.cut2_of(0.7 * scale), 0.7 * scale, False), (on_edge, on_edge, True),
            (E.cut2_of(1.6 * scale), 1.6 * scale, False)]
    groups = []
    for cut2, eps, squared in cuts:
        want = K.cluster_cpu(p, cut2, 1)[0]
        got = E.mst_labels(rows, d2, n, eps, squared=squared)
        assert got.dtype == torch.int32 and torch.equal(got, want)
        assert int((d2 < cut2).sum()) == n - int(got.unique().numel())
        groups.append(int(got.unique().numel()))
    assert n > groups[0] > groups[1] > groups[2] > 1  # three different, non-trivial cuts
    above = float(np.nextafter(np.float32(on_edge), np.float32(np.inf)))
    assert int(E.mst_labels(rows, d2, n, above, squared=True).unique().numel()) < groups[1]
    # eps = 0 cuts every edge, eps = inf none
    assert torch.equal(E.mst_labels(rows, d2, n, 0.0), torch.arange(n, dtype=torch.int32))
    assert torch.equal(E.mst_labels(rows, d2, n, math.inf), K.cluster_cpu(p, math.inf, 1)[0])


def test_labels_of_nothing():
    rows, d2 = K.mst_cpu(uniform(0))
    assert E.mst_labels(rows, d2, 0, 0.1).shape == (0,)
    assert E.mst_labels(rows, d2, 3, 0.1).tolist() == [0, 1, 2]


def test_value_errors():
    p = uniform(50, seed=9)
    index = E.build_index(p)
    bad = [torch.zeros(49), torch.zeros(50, dtype=torch.float64), torch.zeros((50, 1)), [0.0] * 50,
           torch.full((50,), -1.0), torch.full((50,), math.nan), torch.full((50,), math.inf)]
    one = torch.zeros(50)
    one[7] = -1e-30
    for core in bad + [one]:
        with pytest.raises(ValueError):
            E.mst_edges(index, core)
        with pytest.raises(ValueError):
            E.mst_points(p, core)
    with pytest.raises(ValueError):
        E.mst_points(p.double())
    with pytest.raises(ValueError):
        E.mst_points(torch.empty((0, 3)), torch.zeros(1))
    with pytest.raises(ValueError):
        K.mst_cpu(p, torch.full((50,), math.inf))
    with pytest.raises(ValueError):
        E.mst_core_d2(index, 0)
    lined = E.LocalIndex(index.n, index.pts, index.perm, index.nodes, index.qnodes, index.depth, index.box, line=True)
    with pytest.raises(ValueError):
        E.mst_edges(lined)
    rows, d2 = K.mst_cpu(p)
    for eps in (-1.0, math.nan):
        with pytest.raises(ValueError):
            E.mst_labels(rows, d2, 50, eps)
    for r, d, n in ((rows.long(), d2, 50), (rows, d2.double(), 50), (rows[:-1], d2, 50), (rows.flatten(), d2, 50),
                    (rows, d2, 49), (rows, d2, -1), (rows, d2, 2.5)):
        with pytest.raises(ValueError):
            E.mst_labels(r, d, n, 0.1)
    out_of_range = rows.clone()
    out_of_range[0, 1] = 50
    with pytest.raises(ValueError):
        E.mst_labels(out_of_range, d2, 50, math.inf)

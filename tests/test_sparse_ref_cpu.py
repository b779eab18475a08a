"""The sparse exact reference (sparse_ref.py) held to the all-pairs oracles at a size they can do,
before it judges a kernel at sizes they cannot (test_gpu_tree_stages.py): labels equal to
K.cluster_cpu / K.cluster_periodic_cpu exactly, tree weights equal to the sorted d2 of K.mst_cpu /
K.mst_periodic_cpu bit for bit, in the open box and under a period."""
import math

import numpy as np
import pytest
import torch

import sparse_ref as S
from datasets import uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

N = 3000
INF = math.inf
PERIODS = pytest.mark.parametrize("period", (None, 1.0), ids=("open", "L1"))
# The graph of the pairs within MST_F mean spacings must be connected and hold the whole tree
# (mst_weights asserts both): 2.5 does for these 3000 points, open and periodic, with and
# without core distances (80 489 pairs in the open box, 98 268 under the period).
MST_F = 2.5

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def data():
    return cached("data", lambda: uniform(N, seed=71))


def eps_of(f):
    return f * N ** (-1.0 / 3.0)


def core_of(period):
    """The oracle's squared 5th-neighbour distances (itself counted)."""
    p = data()
    return cached(("core", period), lambda: K.kth_cpu(p, p, 5, INF) if period is None else
                  K.kth_periodic_cpu(p, p, 5, INF, period))


@PERIODS
@pytest.mark.parametrize("f", (0.5, 0.9, 2.0))
def test_pairs_within_counts_what_the_brute_force_counts(f, period):
    p = data()
    cut2 = E.cut2_of(eps_of(f))
    a, b, d2 = S.pairs_within(p, cut2, period)
    counts = K.radius_count_cpu(p, p, cut2) if period is None else K.radius_periodic_count_cpu(p, p, cut2, period)
    got = 1 + np.bincount(a, minlength=N) + np.bincount(b, minlength=N)
    assert np.array_equal(got, counts.numpy())
    assert bool((a < b).all()) and bool((d2 < np.float32(cut2)).all())
    assert np.array_equal(d2.view(np.uint32), S.pair_d2(p, b, a, period).view(np.uint32))  # symmetric in its bits


@PERIODS
@pytest.mark.parametrize("min_pts", (1, 5))
@pytest.mark.parametrize("f", (0.7, 0.9))
def test_labels_equal_the_oracle(f, min_pts, period):
    p = data()
    cut2 = E.cut2_of(eps_of(f))
    want = K.cluster_cpu(p, cut2, min_pts) if period is None else K.cluster_periodic_cpu(p, cut2, min_pts, period)
    fn = (lambda: S.fof_labels(p, cut2, period)) if min_pts == 1 else (lambda: S.dbscan_labels(p, cut2, min_pts, period))
    labels, core, nclusters = fn()
    assert labels.dtype == np.int32 and np.array_equal(core, want[1].numpy())
    bad = np.nonzero(labels != want[0].numpy())[0]
    assert bad.size == 0, f"{bad.size} labels differ, first rows {bad[:5].tolist()}"
    assert nclusters == E.compact_labels(want[0])[1]
    if min_pts == 1:
        assert bool(core.all()) and 1 < nclusters < N
    else:  # core, border and noise points all occur
        border = ~core & (labels >= 0)
        assert core.any() and border.any() and bool((labels == -1).any())


def test_the_period_changes_the_labels():
    p = data()
    cut2 = E.cut2_of(eps_of(0.9))
    assert S.fof_labels(p, cut2)[2] != S.fof_labels(p, cut2, 1.0)[2]


@PERIODS
@pytest.mark.parametrize("with_core", (False, True), ids=("plain", "core"))
def test_tree_weights_equal_the_oracle(with_core, period):
    p = data()
    core = core_of(period) if with_core else None
    rows, d2 = K.mst_cpu(p, core) if period is None else K.mst_periodic_cpu(p, period, core)
    assert d2.shape[0] == N - 1
    got, npairs = S.mst_weights(p, eps_of(MST_F), core, period)
    assert got.dtype == np.float32 and npairs > N
    assert np.array_equal(got.view(np.uint32), np.sort(d2.numpy()).view(np.uint32))
    # the oracle's rows weigh what pair_weights says, and span the set
    w = S.pair_weights(p, rows[:, 0].numpy(), rows[:, 1].numpy(), core, period)
    assert np.array_equal(w.view(np.uint32), d2.numpy().view(np.uint32))
    assert S.components_of_edges(rows, N) == 1


def test_tree_weights_refuse_a_graph_that_does_not_hold_the_tree():
    p = data()
    with pytest.raises(AssertionError, match="raise r"):
        S.mst_weights(p, eps_of(0.9))
    q = p.clone()
    q[17] = q[5]  # an exact copy: a zero weight
    with pytest.raises(AssertionError, match="zero weight"):
        S.mst_weights(q, eps_of(MST_F))


def test_fof_labels_equal_the_cut_of_the_oracle_tree():
    """The identity the GPU module leans on for mst_labels: the tree cut below eps is friends-of-friends."""
    p = data()
    rows, d2 = K.mst_periodic_cpu(p, 1.0)
    cut2 = E.cut2_of(eps_of(0.9))
    want = K.mst_labels_cpu(rows, d2, N, cut2)
    assert np.array_equal(S.fof_labels(p, cut2, 1.0)[0], want.numpy())
    assert torch.equal(want, K.cluster_periodic_cpu(p, cut2, 1, 1.0)[0])

"""A sparse exact reference of the self-form contracts (friends-of-friends / DBSCAN labels and
the minimum spanning tree's weights) for point sets too large for the all-pairs oracles
K.cluster_cpu / K.mst_cpu and their periodic forms. numpy and scipy only.

Candidate pairs come from a float64 k-d tree at a slightly widened radius; every candidate's
weight is then recomputed in float32 with the project's canonical arithmetic (fma_sq and the
minimum image of periodic_knn_ref.py) and compared strictly against the squared cutoff, so the
kept set is the contract's, not the k-d tree's. The widening only has to exceed the float32
rounding of d2 (open box: a few ulp; under a period the rounding of q - p before the wrap, about
1e-7 absolute for coordinates in [0, 1)); pairs_within asserts that a second, wider query keeps
the same set. test_sparse_ref_cpu.py holds this module to the all-pairs oracles at a size they
can do."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
from scipy.spatial import cKDTree

from periodic_knn_ref import _np, as_period, fma_sq, wrap

MARGIN = 1e-4  # relative widening of the candidate radius (and twice that for the check)


def _points(points):
    p = np.ascontiguousarray(_np(points), dtype=np.float32)
    assert p.ndim == 2 and p.shape[1] == 3 and np.isfinite(p).all(), "finite float32 [n, 3] points"
    return p


def _boxsize(period):
    if period is None:
        return None
    per = as_period(period)
    assert len(per) == 3 and all(np.isfinite(L) and L > 0 for L in per), "finite periods only"
    return per


def pair_d2(points, a, b, period=None):
    """float32 [m]: the canonical squared distance of the rows a[i], b[i] (under `period` the
    minimum image of the float32 difference): fmaf(dz, dz, fmaf(dy, dy, dx * dx))."""
    p = _points(points)
    per = _boxsize(period)
    d = []
    for ax in range(3):
        dd = (p[a, ax] - p[b, ax]).astype(np.float32)
        d.append(dd if per is None else wrap(dd, per[ax]))
    return fma_sq(d[2], fma_sq(d[1], (d[0] * d[0]).astype(np.float32)))


def pair_weights(points, a, b, core=None, period=None):
    """float32 [m]: pair_d2, with core distances max(d2, core[a], core[b])."""
    w = pair_d2(points, a, b, period)
    if core is not None:
        c = _np(core).astype(np.float32)
        w = np.maximum(np.maximum(w, c[a]), c[b])
    return w


def _kept(p, tree, cut2, period, margin):
    r = float(np.sqrt(np.float64(cut2)))
    cand = tree.query_pairs(r * (1.0 + margin), output_type="ndarray")
    a, b = cand[:, 0].astype(np.int64), cand[:, 1].astype(np.int64)
    d2 = pair_d2(p, a, b, period)
    keep = d2 < np.float32(cut2)
    return a[keep], b[keep], d2[keep]


def pairs_within(points, cut2, period=None):
    """(a, b, d2): every pair of rows a < b whose canonical float32 squared distance is below
    cut2 (strict), in the k-d tree's order. Under `period` (one value or three, finite) the
    coordinates must lie in [0, period)."""
    p = _points(points)
    cut2 = np.float32(cut2)
    assert np.isfinite(cut2) and cut2 > 0
    tree = cKDTree(p.astype(np.float64), boxsize=_boxsize(period))
    a, b, d2 = _kept(p, tree, cut2, period, MARGIN)
    # The candidates of the wider query contain those of the narrower one and a pair is kept by
    # its own weight alone, so the wider query's kept set contains this one: equal sizes, equal sets.
    wider = _kept(p, tree, cut2, period, 2.0 * MARGIN)[0]
    assert a.shape == wider.shape, f"the candidate margin lost {wider.shape[0] - a.shape[0]} pairs"
    return a, b, d2


def _labels(p, cut2, min_pts, period):
    return _labels_of_pairs(p.shape[0], *pairs_within(p, cut2, period), min_pts)


def dense_labels(weights, cut2, min_pts):
    """dbscan_labels from the all-pairs weights (float32 [n, n], symmetric, 0 on the diagonal)
    instead of a k-d tree, for inputs the tree does not take: coordinates outside [0, period),
    squared distances that are denormal or overflow. cut2 > 0, so every point links to itself."""
    w = np.asarray(weights, dtype=np.float32)
    assert np.float32(cut2) > 0 and w.ndim == 2 and w.shape[0] == w.shape[1]
    a, b = np.triu_indices(w.shape[0], k=1)
    keep = w[a, b] < np.float32(cut2)
    return _labels_of_pairs(w.shape[0], a[keep], b[keep], w[a, b][keep], int(min_pts))


def _labels_of_pairs(n, a, b, d2, min_pts):
    # a point is linked to itself and its exact copies (d2 = 0 < cut2); the copies are pairs
    counts = 1 + np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    core = counts >= min_pts
    cc = core[a] & core[b]
    ones = np.ones(int(cc.sum()), dtype=np.int8)
    ncomp, comp = connected_components(coo_matrix((ones, (a[cc], b[cc])), shape=(n, n)).tocsr(), directed=False)
    rows = np.arange(n, dtype=np.int64)
    smallest = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(smallest, comp[core], rows[core])  # the smallest row among a component's core points
    labels = np.full(n, -1, dtype=np.int64)
    labels[core] = smallest[comp[core]]
    # border points: the label of the nearest core point by (d2 bits, row)
    src = np.concatenate([a, b])
    dst = np.concatenate([b, a])
    bits = np.concatenate([d2, d2]).view(np.uint32)
    sel = ~core[src] & core[dst]
    src, dst, bits = src[sel], dst[sel], bits[sel]
    order = np.lexsort((dst, bits, src))  # (the last key is the primary one)
    src, dst = src[order], dst[order]
    first = np.ones(src.shape[0], dtype=bool)
    first[1:] = src[1:] != src[:-1]
    labels[src[first]] = labels[dst[first]]
    return labels.astype(np.int32), core, int(np.unique(labels[core]).size)


def dbscan_labels(points, cut2, min_pts, period=None):
    """(labels int32 [n], core bool [n], number of clusters): the contract of K.cluster_cpu's
    docstring. core: at least min_pts points, itself and exact copies included, with d2 < cut2
    (strict); a core point's label is the smallest row among the core points of its component
    under the core-core links; a non-core point takes the label of its nearest core point by (d2
    bits, row) within cut2, else -1."""
    assert min_pts >= 1
    return _labels(_points(points), cut2, int(min_pts), period)


def fof_labels(points, cut2, period=None):
    """dbscan_labels with min_pts = 1: every point is a core point, there is no noise."""
    return _labels(_points(points), cut2, 1, period)


def components_of_edges(rows, n):
    """The number of connected components of n vertices under the edges rows [m, 2]."""
    rows = _np(rows).astype(np.int64)
    ones = np.ones(rows.shape[0], dtype=np.int8)
    return connected_components(coo_matrix((ones, (rows[:, 0], rows[:, 1])), shape=(n, n)).tocsr(),
                                directed=False)[0]


def mst_weights(points, r, core=None, period=None, pairs=None):
    """(w float32 [n - 1] ascending, number of pairs in the graph): the weights of the minimum
    spanning tree of the graph of the pairs with d2 < fl(r * r), each weighing max(d2, core[a],
    core[b]). It asserts one connected component, no zero weight (scipy reads 0 as no edge) and
    a largest tree weight below fl(r * r): every pair left out of the graph has d2 >= fl(r * r)
    and so weighs more than every tree edge, the graph's tree is a minimum spanning tree of all
    pairs, and the sorted weights of all minimum spanning trees coincide. pairs: the result of
    pairs_within(points, fl(r * r), period), when the caller has it already."""
    p = _points(points)
    n = p.shape[0]
    r32 = np.float32(r)
    cut2 = np.float32(r32 * r32)
    a, b, d2 = pairs_within(p, cut2, period) if pairs is None else pairs
    w = d2
    if core is not None:
        c = _np(core).astype(np.float32)
        w = np.maximum(np.maximum(d2, c[a]), c[b])
    assert w.size and float(w.min()) > 0.0, "a zero weight (exact copies): scipy would drop the edge"
    tree = minimum_spanning_tree(coo_matrix((w.astype(np.float64), (a, b)), shape=(n, n)).tocsr())
    tw = np.sort(tree.data.astype(np.float32))
    assert tw.shape[0] == n - 1, f"the graph at r = {r} has {n - tw.shape[0]} components, raise r"
    assert float(tw[-1]) < float(cut2), f"the largest tree weight {tw[-1]} is not below r^2 = {cut2}, raise r"
    return tw, int(a.shape[0])

"""A plain numpy reference of the periodic minimum-spanning-tree contract, for the tests of the
oracle K.mst_periodic_cpu (and through it of the GPU path).

The contract, literally: vertices are the rows with three finite coordinates; the weight of the
pair {a, b} is pd2(a, b), the float32 minimum-image squared distance of periodic_knn_ref.pd2
(symmetric in its bits), with core distances max(pd2, core[a], core[b]); edges are ordered by
(bits of w, lo, hi), lo < hi the rows. There is no bound on an edge's length and no requirement
that the coordinates lie inside one period. Kruskal over all pairs in that order: for n up to
~1500."""
import numpy as np

from periodic_knn_ref import _np, as_period, pd2


def pair_weights(points, period, core=None):
    """(w float32 [n, n]) of every pair of rows under `period` (one value or three)."""
    w = pd2(points, points, as_period(period))
    if core is not None:
        c = _np(core).astype(np.float32)
        w = np.maximum(np.maximum(w, c[:, None]), c[None, :])
    return w


def mst(points, period, core=None):
    """(rows int32 [m, 2], d2 float32 [m]) ascending by (bits of w, lo, hi)."""
    p = _np(points).astype(np.float32)
    n = p.shape[0]
    finite = np.isfinite(p).all(axis=1) if n else np.zeros(0, dtype=bool)
    want = max(int(finite.sum()) - 1, 0)
    rows = np.zeros((want, 2), dtype=np.int32)
    d2 = np.zeros(want, dtype=np.float32)
    if want == 0:
        return rows, d2
    w = pair_weights(p, period, core)
    lo, hi = np.triu_indices(n, k=1)
    ok = finite[lo] & finite[hi]
    lo, hi = lo[ok], hi[ok]
    bits = w[lo, hi].view(np.uint32)
    order = np.lexsort((hi, lo, bits))  # (the last key is the primary one)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    m = 0
    for e in order:
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a == b:
            continue
        parent[max(a, b)] = min(a, b)
        rows[m] = (lo[e], hi[e])
        d2[m] = w[lo[e], hi[e]]
        m += 1
        if m == want:
            break
    assert m == want
    return rows, d2

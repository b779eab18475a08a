"""A plain numpy reference of the weighted radius profile, for the tests of the oracle
(K.weighted_profile_cpu) and through it of the GPU path. Written on its own: nothing of the C++
oracle is used.

The contract, literally: d2 of a pair as in radius_profile_ref.py (float32, the canonical
operation order, under a period the minimum image of each axis' difference as the README
states it); WP[q, b] = the sum of w[p] over {p : d2(q, p) < c_b}, strict (a NaN d2 passes no
test), in int64; WS[b] = the sum over q of wq[q] * WP[q, b], in int64."""
import numpy as np

from radius_profile_ref import _np, dist2


def weighted_profile(points, queries, cut2s, weights, period=None) -> np.ndarray:
    """int64 [nq, B]: column b sums the weights of the pairs with d2 < cut2s[b]."""
    v = dist2(points, queries, period)
    c = np.asarray(cut2s, dtype=np.float32)
    w = _np(weights).astype(np.int64)
    assert w.shape == (v.shape[1],)
    with np.errstate(invalid="ignore"):
        cols = [np.where(v < cb, w[None, :], np.int64(0)).sum(1, dtype=np.int64) for cb in c]
    return np.stack(cols, axis=1).astype(np.int64).reshape(v.shape[0], c.size)


def weighted_pair_sums(points, queries, cut2s, weights, period=None, query_weights=None) -> np.ndarray:
    """int64 [B]: the column sums of weighted_profile, each row times its query weight."""
    prof = weighted_profile(points, queries, cut2s, weights, period)
    if query_weights is not None:
        prof = prof * _np(query_weights).astype(np.int64)[:, None]
    return prof.sum(0, dtype=np.int64)

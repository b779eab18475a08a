"""A plain numpy reference of the two-sided radius search, for the tests of the oracle
(K.radius_reach_count_cpu / K.radius_reach_cpu) and of the GPU path.

The contract, literally: with cq[q] and cp[p] the squared cutoffs (float32), p is in row q iff
    either:  d2 < max(cq[q], cp[p])        both:  d2 < min(cq[q], cp[p])
strictly, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of d = q - p in float32, under a period of
its minimum image (periodic_knn_ref.pd2: per axis d > h: d - L, d < -h: d + L, h = 0.5f * L; an
open box is the period (inf, inf, inf), which never wraps). A NaN d2 passes no comparison. Rows
ascend by (bits of d2, row of the points)."""
import numpy as np

from periodic_knn_ref import _np, as_period, pd2

OPEN = (np.inf, np.inf, np.inf)


def cutoffs(qcut2, pcut2, rule: str) -> np.ndarray:
    """float32 [nq, n]: the cutoff of every pair."""
    cq = _np(qcut2).astype(np.float32)[:, None]
    cp = _np(pcut2).astype(np.float32)[None, :]
    if rule == "either":
        return np.maximum(cq, cp)
    if rule == "both":
        return np.minimum(cq, cp)
    raise KeyError(rule)


def selected(points, queries, qcut2, pcut2, rule: str, period=None) -> tuple:
    """(mask bool [nq, n], d2 float32 [nq, n])."""
    per = OPEN if period is None else as_period(period)
    v = pd2(points, queries, per)
    with np.errstate(invalid="ignore"):
        return v < cutoffs(qcut2, pcut2, rule), v


def reach(points, queries, qcut2, pcut2, rule: str, period=None) -> tuple:
    """(counts int32 [nq], offsets int64 [nq + 1], idx int32 [total], d2 float32 [total])."""
    m, v = selected(points, queries, qcut2, pcut2, rule, period)
    nq = m.shape[0]
    counts = m.sum(1).astype(np.int32)
    offsets = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    idx = np.empty(int(offsets[nq]), dtype=np.int32)
    d2 = np.empty(int(offsets[nq]), dtype=np.float32)
    for r in range(nq):
        ok = np.nonzero(m[r])[0]
        order = ok[np.argsort(v[r, ok].view(np.uint32), kind="stable")]  # (ok ascends: ties by row)
        idx[offsets[r]:offsets[r + 1]] = order
        d2[offsets[r]:offsets[r + 1]] = v[r, order]
    return counts, offsets, idx, d2


def wraps(points, queries, period) -> np.ndarray:
    """bool [nq, n]: the pair's wrap vector is not zero (some axis takes a branch)."""
    p = _np(points).astype(np.float32)
    q = _np(queries).astype(np.float32)
    out = np.zeros((q.shape[0], p.shape[0]), dtype=bool)
    for a, L in enumerate(as_period(period)):
        h = np.float32(0.5) * np.float32(L)
        with np.errstate(invalid="ignore"):
            d = (q[:, None, a] - p[None, :, a]).astype(np.float32)
            out |= (d > h) | (d < -h)
    return out

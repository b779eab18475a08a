"""A plain numpy reference of the periodic k-NN contract, for the tests of the oracles
(K.kth_periodic_cpu / K.knn_periodic_cpu) and of the GPU path.

The contract, literally: per axis, in float32, d = q - p; h = 0.5f * L; d > h: d = d - L; else
d < -h: d = d + L (L = inf never wraps); pd2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)). The k-th
value of a query is the k-th smallest pd2 by its bits among those < cut2, or cut2 when fewer
than k qualify; its list the first k of {(pd2, row) : pd2 < cut2} ascending by (bits, row),
unfilled slots -1 / cut2.

fmaf(a, a, c) is a single rounding of the exact a * a + c. Here: the float64 product of two
float32 is exact (48 bits); the float64 sum with c is rounded to odd (its two-sum error tells
whether it was inexact), and a value rounded to odd at 53 bits rounds to float32 (24 bits) as
the exact value would."""
import numpy as np


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def fma_sq(a: np.ndarray, c: np.ndarray) -> np.ndarray:
    """float32 fmaf(a, a, c) for float32 a and c >= 0."""
    p = a.astype(np.float64) ** 2
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)  # exact: s + err = p + c64
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    with np.errstate(invalid="ignore"):
        s = np.where((err != 0) & even & np.isfinite(s), np.nextafter(s, toward), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def wrap(d: np.ndarray, L) -> np.ndarray:
    """One axis of the minimum image, float32 throughout."""
    L = np.float32(L)
    h = np.float32(0.5) * L
    with np.errstate(invalid="ignore", over="ignore"):
        down = (d - L).astype(np.float32)
        up = (d + L).astype(np.float32)
    return np.where(d > h, down, np.where(d < -h, up, d)).astype(np.float32)


def pd2(points, queries, period) -> np.ndarray:
    """float32 [nq, n]: the periodic squared distance of every pair; period: three values."""
    p = _np(points).astype(np.float32)
    q = _np(queries).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [wrap((q[:, None, a] - p[None, :, a]).astype(np.float32), period[a]) for a in range(3)]
        xx = (d[0] * d[0]).astype(np.float32)
        return fma_sq(d[2], fma_sq(d[1], xx))


def knn_periodic(points, queries, k, cut2, period):
    """(idx int32 [nq, k], d2 float32 [nq, k]) by a stable sort of every row by the bits of
    pd2 (rows ascending among equal bits); d2[:, k - 1] is the k-th value."""
    v = pd2(points, queries, period)
    nq, n = v.shape
    c2 = np.float32(cut2)
    idx = np.full((nq, k), -1, dtype=np.int32)
    d2 = np.full((nq, k), c2, dtype=np.float32)
    for r in range(nq):
        with np.errstate(invalid="ignore"):
            ok = np.nonzero(v[r] < c2)[0]  # (a NaN fails the comparison: no neighbour)
        bits = v[r, ok].view(np.uint32)
        order = ok[np.argsort(bits, kind="stable")][:k]
        idx[r, :order.size] = order
        d2[r, :order.size] = v[r, order]
    return idx, d2


def as_period(period):
    return (period,) * 3 if isinstance(period, (int, float)) else tuple(period)

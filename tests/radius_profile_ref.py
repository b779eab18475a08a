"""A plain numpy reference of the radius profile, for the tests of the oracle
(K.radius_profile_cpu) and through it of the GPU path. Written on its own: nothing of the C++
oracle is used.

The contract, literally: per axis, in float32, d = q - p; under a period h = 0.5f * L; d > h: d
= d - L; else d < -h: d = d + L (L = inf never wraps); d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
P[q, b] = #{p : d2(q, p) < c_b}, strict (a NaN d2 passes no test). The fma is emulated as in
periodic_knn_ref.py (fma_sq)."""
import numpy as np

from periodic_knn_ref import fma_sq, wrap


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def dist2(points, queries, period=None) -> np.ndarray:
    """float32 [nq, n]: the (periodic) squared distance of every pair."""
    p = _np(points).astype(np.float32).reshape(-1, 3)
    q = _np(queries).astype(np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [(q[:, None, a] - p[None, :, a]).astype(np.float32) for a in range(3)]
        if period is not None:
            d = [wrap(d[a], period[a]) for a in range(3)]
        xx = (d[0] * d[0]).astype(np.float32)
        return fma_sq(d[2], fma_sq(d[1], xx))


def radius_profile(points, queries, cut2s, period=None) -> np.ndarray:
    """int32 [nq, B]: column b counts the pairs with d2 < cut2s[b]."""
    v = dist2(points, queries, period)
    c = np.asarray(cut2s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.stack([(v < cb).sum(1) for cb in c], axis=1).astype(np.int32).reshape(v.shape[0], c.size)

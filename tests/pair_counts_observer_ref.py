"""A plain numpy reference of the anisotropic pair counts with the line of sight of an observer
(los='midpoint'), for the tests of the oracle (K.pair_counts_2d_observer_cpu) and through it of the
GPU path. Written from the contract alone: nothing of the C++ oracle is used.

The contract, literally, per pair (query q, point p) and observer o, all float32:
    dx = q.x - p.x, dy, dz likewise
    lx = (q.x - o.x) + (p.x - o.x), ly, lz
    sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx))
    ll = fmaf(lz, lz, fmaf(ly, ly, lx * lx)),  d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx))
    par2  = (sl / ll) * sl
    perp2 = d2 - par2;  if perp2 < 0: perp2 = 0        (a NaN stays a NaN)
(rp, pi): S[i, j] = #{pairs : perp2 < a2[i] and par2 < b2[j]};
(s, mu):  S[i, j] = #{pairs : d2 < a2[i] and par2 < fl(b2[j] * d2)}; strict: a NaN passes no test.

The general float32 fma. The product of two float32 values has at most 48 significant bits and an
exponent far inside the float64 range, so a64 * b64 is exact. Its float64 sum with c is rounded
once to 53 bits; TwoSum gives the exact error of that rounding, and where the sum is inexact and its
last bit even it is moved to the odd neighbour on the error's side (rounding to odd). A value
rounded to odd at 53 bits rounds to any format of at most 51 bits, float32 and its denormals among
them, exactly as the unrounded a * b + c would: the one conversion to float32 is the single
rounding of fmaf. (fma_sq of periodic_knn_ref.py is this with a == b and c >= 0.)"""
import numpy as np

from periodic_knn_ref import fma_sq


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """float32 fmaf(a, b, c) for float32 operands of any sign."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # exact: s + err = p + c64
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where((err != 0) & ~np.isnan(err) & even & np.isfinite(s), np.nextafter(s, toward), s)
        return s.astype(np.float32)


def components(points, queries, observer):
    """float32 [nq, n] each: (par2, perp2, d2) of every pair."""
    p = _np(points).astype(np.float32).reshape(-1, 3)
    q = _np(queries).astype(np.float32).reshape(-1, 3)
    o = np.asarray(observer, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        d = [(q[:, None, a] - p[None, :, a]).astype(np.float32) for a in range(3)]
        l = [((q[:, None, a] - o[a]).astype(np.float32) + (p[None, :, a] - o[a]).astype(np.float32)).astype(np.float32)
             for a in range(3)]
        sl = fma32(d[2], l[2], fma32(d[1], l[1], (d[0] * l[0]).astype(np.float32)))
        ll = fma_sq(l[2], fma_sq(l[1], (l[0] * l[0]).astype(np.float32)))
        d2 = fma_sq(d[2], fma_sq(d[1], (d[0] * d[0]).astype(np.float32)))
        par2 = ((sl / ll).astype(np.float32) * sl).astype(np.float32)
        perp2 = (d2 - par2).astype(np.float32)
        perp2 = np.where(perp2 < 0, np.float32(0), perp2)
    return par2, perp2, d2


def _cells(par2, perp2, d2, a2, b2, mode):
    """bool [nq, n] per cell (i, j): the pairs S[i, j] takes."""
    a2 = np.asarray(a2, dtype=np.float32)
    b2 = np.asarray(b2, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, ca in enumerate(a2):
            first = (perp2 if mode == "rppi" else d2) < ca
            for j, cb in enumerate(b2):
                second = par2 < cb if mode == "rppi" else par2 < (cb * d2).astype(np.float32)
                yield i, j, first & second


def pair_counts_2d_observer(points, queries, a2, b2, mode, observer) -> np.ndarray:
    """int64 [Ba, Bb], straight from the definition of S: one count per cell."""
    par2, perp2, d2 = components(points, queries, observer)
    out = np.zeros((len(a2), len(b2)), dtype=np.int64)
    for i, j, take in _cells(par2, perp2, d2, a2, b2, mode):
        out[i, j] = np.count_nonzero(take)
    return out


def weighted_pair_sums_2d_observer(points, queries, a2, b2, mode, observer, weights, query_weights=None) -> list:
    """[Ba][Bb] Python integers: the sum of wq[q] * w[p] over the pairs of each cell."""
    par2, perp2, d2 = components(points, queries, observer)
    w = [int(v) for v in _np(weights)]
    wq = [1] * par2.shape[0] if query_weights is None else [int(v) for v in _np(query_weights)]
    out = [[0] * len(b2) for _ in range(len(a2))]
    for i, j, take in _cells(par2, perp2, d2, a2, b2, mode):
        out[i][j] = sum(wq[qi] * w[pi] for qi, pi in zip(*np.nonzero(take)))
    return out

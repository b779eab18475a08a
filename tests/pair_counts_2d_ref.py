"""A plain numpy reference of the anisotropic pair counts, for the tests of the oracle
(K.pair_counts_2d_cpu) and through it of the GPU path. Written from the contract alone: nothing of
the C++ oracle is used.

The contract, literally: per axis, in float32, d = q - p; under a period its minimum image (wrap
of periodic_knn_ref.py). los picks dl, the other two in ascending axis order are da, db; par2 = dl
* dl, perp2 = fmaf(db, db, da * da), d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)).
(rp, pi): S[i, j] = #{pairs : perp2 < a2[i] and par2 < b2[j]};
(s, mu):  S[i, j] = #{pairs : d2 < a2[i] and par2 < fl(b2[j] * d2)}; strict: a NaN passes no test."""
import numpy as np

from periodic_knn_ref import fma_sq, wrap


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def components(points, queries, los, period=None):
    """float32 [nq, n] each: (par2, perp2, d2) of every pair."""
    p = _np(points).astype(np.float32).reshape(-1, 3)
    q = _np(queries).astype(np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [(q[:, None, a] - p[None, :, a]).astype(np.float32) for a in range(3)]
        if period is not None:
            d = [wrap(d[a], period[a]) for a in range(3)]
        a, b = [x for x in range(3) if x != los]
        par2 = (d[los] * d[los]).astype(np.float32)
        perp2 = fma_sq(d[b], (d[a] * d[a]).astype(np.float32))
        d2 = fma_sq(d[2], fma_sq(d[1], (d[0] * d[0]).astype(np.float32)))
    return par2, perp2, d2


def pair_counts_2d(points, queries, a2, b2, mode, los=2, period=None) -> np.ndarray:
    """int64 [Ba, Bb], straight from the definition of S: one count per cell."""
    par2, perp2, d2 = components(points, queries, los, period)
    a2 = np.asarray(a2, dtype=np.float32)
    b2 = np.asarray(b2, dtype=np.float32)
    out = np.zeros((a2.size, b2.size), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, ca in enumerate(a2):
            first = (perp2 if mode == "rppi" else d2) < ca
            for j, cb in enumerate(b2):
                second = par2 < cb if mode == "rppi" else par2 < (cb * d2).astype(np.float32)
                out[i, j] = np.count_nonzero(first & second)
    return out

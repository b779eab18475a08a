"""A plain numpy reference of the weighted anisotropic pair sums, for the tests of the oracle
(K.weighted_pair_sums_2d_cpu) and through it of the GPU path. Written from the contract alone:
nothing of the C++ oracle is used, the float32 arithmetic is spelled out here and the sums are
Python integers, which cannot wrap.

The contract: per axis, in float32, d = q - p; under a period L its minimum image (h = 0.5f * L; d >
h: d - L; d < -h: d + L). los picks dl, the other two axes in ascending order are da, db:
    par2 = dl * dl,  perp2 = fmaf(db, db, da * da),  d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)).
(rp, pi): WS[i, j] = sum {wq[q] * w[p] : perp2 < a2[i] and par2 < b2[j]};
(s, mu):  WS[i, j] = sum {wq[q] * w[p] : d2 < a2[i] and par2 < fl(b2[j] * d2)};
strict tests: a NaN passes none. wq = None means all ones."""
import numpy as np

F = np.float32


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _fma_square(a, c):
    """float32 fmaf(a, a, c) of float32 a and c >= 0: a * a is exact in float64, the float64 sum is
    made sticky (round to odd: an inexact even result moves one step toward the lost part) so that
    the second rounding, to float32, is the single rounding of the exact a * a + c."""
    p = a.astype(np.float64) * a.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    lost = (p - (s - t)) + (c - t)  # s + lost == p + c exactly (two-sum)
    even = (s.view(np.int64) & 1) == 0
    with np.errstate(invalid="ignore"):
        fix = (lost != 0) & even & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(F)


def _image(d, L):
    L = F(L)
    h = F(0.5) * L
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(d > h, (d - L).astype(F), np.where(d < -h, (d + L).astype(F), d)).astype(F)


def components(points, queries, los, period=None):
    """float32 [nq, n] each: (par2, perp2, d2) of every pair."""
    p = _np(points).astype(F).reshape(-1, 3)
    q = _np(queries).astype(F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [(q[:, None, a] - p[None, :, a]).astype(F) for a in range(3)]
        if period is not None:
            d = [_image(d[a], period[a]) for a in range(3)]
        a, b = [x for x in range(3) if x != los]
        par2 = (d[los] * d[los]).astype(F)
        perp2 = _fma_square(d[b], (d[a] * d[a]).astype(F))
        d2 = _fma_square(d[2], _fma_square(d[1], (d[0] * d[0]).astype(F)))
    return par2, perp2, d2


def weighted_pair_sums_2d(points, queries, a2, b2, weights, mode, los=2, period=None, query_weights=None):
    """A [Ba][Bb] nested list of Python ints, straight from the definition: one sum per cell."""
    par2, perp2, d2 = components(points, queries, los, period)
    nq, n = par2.shape
    w = [int(v) for v in _np(weights).reshape(-1)]
    wq = [1] * nq if query_weights is None else [int(v) for v in _np(query_weights).reshape(-1)]
    assert len(w) == n and len(wq) == nq
    prod = np.empty((nq, n), dtype=object)  # Python ints: wq[q] * w[p]
    for qi in range(nq):
        for pi in range(n):
            prod[qi, pi] = wq[qi] * w[pi]
    a2 = np.asarray(a2, dtype=F)
    b2 = np.asarray(b2, dtype=F)
    out = [[0] * b2.size for _ in range(a2.size)]
    with np.errstate(invalid="ignore", over="ignore"):
        for i, ca in enumerate(a2):
            first = (perp2 if mode == "rppi" else d2) < ca
            for j, cb in enumerate(b2):
                second = par2 < cb if mode == "rppi" else par2 < (cb * d2).astype(F)
                out[i][j] = sum(prod[first & second].tolist(), 0)
    return out


def as_int64(cells):
    """The nested list as an int64 array (every value must fit: the caller's bound)."""
    flat = [v for row in cells for v in row]
    assert all(-(1 << 63) <= v < (1 << 63) for v in flat)
    return np.array(cells, dtype=np.int64)

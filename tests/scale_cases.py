"""The transforms of the scale tests, in one place: the point sets of datasets.py scaled by
exact powers of two, moved far from the origin, and wrapped into boxes whose periods are no
powers of two. test_scale_cpu.py pins the host oracles on them, test_gpu_scales.py runs every
kernel family on them against those oracles.

  SCALES   s: every coordinate times 2^s, exactly (np.ldexp). Squared distances scale by 2^2s:
             +-40  no d2 leaves the normal range, every float operation is exactly covariant
             -60   the k-th d2 straddles the denormal boundary (2^-126)
             -70   every d2 of near neighbours is denormal
             -80   every d2 underflows to 0: distinct points at distance 0
             +62   d2 near 2^124: 16 x and the product of two d2 overflow
             +70   every non-zero d2 is inf
  OFFSETS  added to the unscaled set: +1000 on every axis; (+2^20, -3e5, +1000), where x keeps
           four bits below the unit and most points collapse to copies; -4096 on every axis
  PERIODS  data = wrap_points(base * L + origin, L, origin) for periods that are no powers of
           two, origins 0, -L / 2 and +1000 (an open axis spans the longest finite period)
"""
import math
from functools import lru_cache

import numpy as np
import torch

from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E

INF = math.inf
BASES = ("uniform", "clustered", "tilted_plane", "line", "duplicates")
SCALES = (40, -40, -60, -70, -80, 62, 70)
COVARIANT = (40, -40)  # (no d2 leaves the normal range)
OFFSETS = {
    "p1000": (1000.0, 1000.0, 1000.0),
    "quant": (float(2 ** 20), -3e5, 1000.0),
    "m4096": (-4096.0, -4096.0, -4096.0),
}
L33 = float(np.float32(100.0 / 3.0))
PERIODS = {
    "L0.7": (0.7, 0.7, 0.7),
    "L1000": (1000.0, 1000.0, 1000.0),
    "L33": (L33, L33, L33),
    "L205x75xinf": (205.0, 75.0, INF),
    "L0.7x1x2.5": (0.7, 1.0, 2.5),
}
ORIGINS = ("zero", "half", "p1000")

# every (kind, value) transform of the open-box tests, the exactly covariant ones first
TRANSFORMS = [("scale", s) for s in SCALES] + [("offset", o) for o in OFFSETS]
PERIOD_CASES = [(p, o) for p in PERIODS for o in ORIGINS]


def tid(t) -> str:
    return f"s{t[1]:+d}" if t[0] == "scale" else str(t[1])


@lru_cache(maxsize=None)
def base(name: str, n: int, seed: int = 0) -> torch.Tensor:
    """A generator's points (shared: never written to)."""
    return GENERATORS[name](n, seed=seed).contiguous()


def scaled(p: torch.Tensor, s: int) -> torch.Tensor:
    """p x 2^s, exactly."""
    return torch.from_numpy(np.ldexp(p.numpy(), s)).contiguous()


def shifted(p: torch.Tensor, name: str) -> torch.Tensor:
    return (p + torch.tensor(OFFSETS[name], dtype=torch.float32)).contiguous()


def apply(p: torch.Tensor, t) -> torch.Tensor:
    return scaled(p, t[1]) if t[0] == "scale" else shifted(p, t[1])


def radius(r: float, t) -> float:
    """The radius r of the unit set under the transform: x 2^s, unchanged by an offset."""
    return math.ldexp(r, t[1]) if t[0] == "scale" else r


def radii(r: torch.Tensor, t) -> torch.Tensor:
    """radius() for a float32 tensor of radii."""
    return scaled(r.float(), t[1]) if t[0] == "scale" else r.float().contiguous()


@lru_cache(maxsize=None)
def points(name: str, n: int, t, seed: int = 0) -> torch.Tensor:
    return apply(base(name, n, seed), t)


@lru_cache(maxsize=None)
def foreign(name: str, nq: int, t, n: int, seed: int = 1) -> torch.Tensor:
    """Queries under the transform of their points: a second seed of the same generator, every
    eighth one moved outside the set's box (up to one extent beyond each face), and the last
    eighth exact copies of (transformed) points."""
    q = base(name, nq, seed).clone()
    g = torch.Generator().manual_seed(seed + 100)
    out = torch.arange(0, nq, 8)
    q[out] = torch.rand((out.numel(), 3), generator=g) * 3.0 - 1.0
    q = apply(q, t)
    m = nq // 8
    q[nq - m:] = points(name, n, t)[torch.randint(0, n, (m,), generator=g)]
    return q.contiguous()


def r_for(count: float, n: int, volume: float = 1.0) -> float:
    """The radius whose ball holds `count` of n uniform points in `volume`."""
    return (3.0 * count * volume / (4.0 * math.pi * n)) ** (1.0 / 3.0)


# ------------------------------------------------------------------------------- periods
def finite_axes(per) -> list:
    return [v for v in per if math.isfinite(v)]


def origin_of(per, origin: str) -> tuple:
    if origin == "zero":
        return (0.0, 0.0, 0.0)
    if origin == "p1000":
        return (1000.0, 1000.0, 1000.0)
    return tuple(-0.5 * v if math.isfinite(v) else 0.0 for v in per)


@lru_cache(maxsize=None)
def periodic_points(name: str, n: int, pname: str, origin: str, seed: int = 0) -> torch.Tensor:
    """wrap_points(base * L + origin, L, origin); an open axis spans the longest finite period."""
    per = PERIODS[pname]
    span = torch.tensor([v if math.isfinite(v) else max(finite_axes(per)) for v in per], dtype=torch.float32)
    org = origin_of(per, origin)
    p = base(name, n, seed) * span + torch.tensor(org, dtype=torch.float32)
    return E.wrap_points(p.contiguous(), per, org).contiguous()


def period_radius(pname: str, fraction: float) -> float:
    """fraction x the shortest finite axis; 0.5 gives exactly period_radius_bound."""
    per = PERIODS[pname]
    if fraction == 0.5:
        return E.period_radius_bound(tuple(float(np.float32(v)) for v in per), False)
    return fraction * min(finite_axes(per))


def float_above(x: float) -> float:
    """The next float32 above x."""
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))

"""Plain references for the k-th-distance select kernels (knn_rows.hip, knn_grid.hip) and
the inputs that drive each recovery branch of their radix select.

Nothing here shares code with the kernels or with the host oracle (K.kth_cpu): the references
are plain numpy (bracket_counts_torch: the same sum with torch tensors, for whole cases on a
GPU); torch and `datasets` only build the inputs.

  kth_bracket  float64 counting test of a returned distance (no selection at all)
  kth_plain    the canonical float32 d² rebuilt with numpy, k-th by np.partition
  status_bits  the QS_* status-word values the GPU test expects (checked against the
               two enums in the .hip sources by name)
  CASES        one input per branch of the select, shared by test_select_ref_cpu.py (which
               pins the host oracle to the references on them) and test_gpu_select_paths.py
"""
import math
import re
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path

import numpy as np
import torch

from datasets import lattice, uniform

EPS = 2.0 ** -20
_HIP = Path(__file__).resolve().parents[1] / "mpi_cuda_largescaleknn_amd" / "csrc" / "hip"


# ------------------------------------------------------------------------ status words
status_bits = {
    "rows": {"QS_OVERFLOW": 1, "QS_UNDERFLOW": 2, "QS_REFINE": 4, "QS_LIST_INVALID": 8, "QS_COLLECTED": 16,
             "QS_DONE_BAND1": 32, "QS_DONE_CUT": 64, "QS_DONE_ZERO": 128, "QS_LIMIT": 256, "QS_MISMATCH": 512,
             "QS_HINT": 1024, "QS_BINOVF": 2048, "QS_FAIL": 4096},
    "grid": {"QS_OVERFLOW": 1, "QS_UNDERFLOW": 2, "QS_REFINE": 4, "QS_COLLECTED": 16, "QS_DONE_BAND1": 32,
             "QS_DONE_CUT": 64, "QS_LIMIT": 256, "QS_MISMATCH": 512, "QS_HINT": 1024, "QS_BINOVF": 2048,
             "QS_FAIL": 4096},
}


def parse_status_enum(kernel: str) -> dict:
    """The QS_* enumerators of knn_rows.hip / knn_grid.hip, read from the source text."""
    src = (_HIP / f"knn_{kernel}.hip").read_text()
    m = re.search(r"enum[^{;]*\{([^}]*QS_OVERFLOW[^}]*)\}", src)
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return {nm: int(v, 0) for nm, v in re.findall(r"(QS_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", body)}


# --------------------------------------------------------------------------- references
def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _rows_per_chunk(n: int) -> int:
    return max(1, (1 << 23) // max(n, 1))


def _finalize(cut2: float) -> np.float32:
    c = np.float32(cut2)
    return c if np.isinf(c) else np.float32(np.sqrt(np.float64(c)))


def bracket_counts(points, queries, v):
    """(#{D < v²(1 − 2⁻²⁰)}, #{D <= v²(1 + 2⁻²⁰)}) per row, D in float64."""
    p = _np(points).astype(np.float64)
    q = _np(queries).astype(np.float64)
    v2 = _np(v).astype(np.float64) ** 2
    lo = np.zeros(q.shape[0], dtype=np.int64)
    hi = np.zeros(q.shape[0], dtype=np.int64)
    step = _rows_per_chunk(p.shape[0])
    for a in range(0, q.shape[0], step):
        d = q[a:a + step, None, :] - p[None, :, :]
        D = (d * d).sum(axis=2)
        t = v2[a:a + step, None]
        lo[a:a + step] = (D < t * (1.0 - EPS)).sum(axis=1)
        hi[a:a + step] = (D <= t * (1.0 + EPS)).sum(axis=1)
    return lo, hi


def kth_bracket(points, queries, v, k, cut2=math.inf, count_fn=None):
    """Per row: is the float32 distance v[j] a right k-th-neighbour distance of queries[j]
    among points? D = Σ (q − p)² is taken in float64 from the float32 inputs with float64
    differences; there is no tree and no selection. Row j is right iff

        #{D < v_j² (1 − 2⁻²⁰)}  <  k  <=  #{D <= v_j² (1 + 2⁻²⁰)}.

    Margin: the canonical float32 d² = fma(dz, dz, fma(dy, dy, dx·dx)) rounds three
    subtractions, one product and two fmas. A rounded difference d(1 + e), |e| <= 2⁻²⁴,
    squares to d²(1 + 2e + e²): below 2⁻²³ + 2⁻⁴⁸ relative per term, and as the terms are
    non-negative the same bound holds for their sum. The product and the two fmas add one
    rounding of 2⁻²⁴ each on a non-negative partial sum: 3·2⁻²⁴. Together below
    2⁻²³ + 3·2⁻²⁴ + (second order) < 2⁻²², and sqrtf adds 2⁻²⁴ on the distance, 2⁻²³ on
    its square: under 2⁻²¹ in all, so 2⁻²⁰ covers it with a factor two to spare.

    v = inf is right iff fewer than k points exist (no cutoff given). With a cutoff, v equal
    to finalize(cut2) is right iff the lower count at the cutoff is < k; a smaller v must
    pass the bracket. NaN is never right. count_fn: a drop-in for bracket_counts."""
    count_fn = count_fn or bracket_counts
    v = _np(v).astype(np.float32)
    n = _np(points).shape[0]
    ok = np.zeros(v.shape[0], dtype=bool)
    fin = _finalize(cut2)
    at_cut = (v == fin) & ~np.isnan(v)
    if np.isinf(fin):
        ok[at_cut] = n < k
    elif at_cut.any():
        lo, _ = count_fn(points, _np(queries)[at_cut], np.full(int(at_cut.sum()), fin, dtype=np.float32))
        ok[at_cut] = lo < k
    rest = ~at_cut & ~np.isnan(v) & (v < fin) & (v >= 0)
    if rest.any():
        lo, hi = count_fn(points, _np(queries)[rest], v[rest])
        ok[rest] = (lo < k) & (k <= hi)
    return ok


def _round_f32(a: np.ndarray, b: np.ndarray):
    """(float32(a + b), near-tie mask) for float64 a, b >= 0: the sum is rounded to float64
    and then to float32. Where the float64 sum is inexact (its two-sum error is not 0) and
    lies within one float64 ulp of the midpoint of two float32 values, the single rounding of
    a real fmaf may go the other way. An exact sum rounds once, as fmaf does."""
    s = a + b
    bb = s - a
    inexact = ((a - (s - bb)) + (b - bb)) != 0.0
    r, tie = _tie_f32(s)
    return r, tie & inexact


def _tie_f32(s: np.ndarray):
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    e = s - r64  # exact (Sterbenz: s and r64 within a factor two, or r64 = 0)
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.spacing(r).astype(np.float64)
        down = r64 - np.nextafter(r, np.float32(0)).astype(np.float64)
    half = 0.5 * np.where(e >= 0, up, down)
    tie = np.abs(np.abs(e) - half) <= np.spacing(s)
    return r, tie & np.isfinite(s)


def canonical_d2(points, queries):
    """float32 d² [nq, n] as the kernels and the oracle define it, and the near-tie mask.
    fmaf(a, a, c) is emulated as the float64 a·a (exact: 48 bits) plus c, rounded to
    float64 and then to float32."""
    p = _np(points).astype(np.float32)
    q = _np(queries).astype(np.float32)
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    xx = dx * dx
    s1, t1 = _round_f32(dy.astype(np.float64) ** 2, xx.astype(np.float64))
    s2, t2 = _round_f32(dz.astype(np.float64) ** 2, s1.astype(np.float64))
    return s2, t1 | t2


def kth_plain(points, queries, k, cut2=math.inf):
    """(values float32 [nq], undecided bool [nq], ties int64 [nq]): the k-th smallest
    canonical float32 d² by np.partition, candidates at or above cut2 not counted (fewer
    than k left: cut2), then sqrt in float32 (inf stays). A row is undecided when a
    near-tie candidate (see _round_f32) lies within 4 float32 steps of the k-th value:
    rounding it the other way moves it by one step, and that could change the k-th. ties:
    how many candidates equal the k-th value exactly (0 where the cutoff is returned)."""
    p = _np(points).astype(np.float32)
    q = _np(queries).astype(np.float32)
    n, nq = p.shape[0], q.shape[0]
    c2 = np.float32(cut2)
    out = np.empty(nq, dtype=np.float32)
    und = np.zeros(nq, dtype=bool)
    ties = np.zeros(nq, dtype=np.int64)
    step = _rows_per_chunk(n)
    for a in range(0, nq, step):
        d2, tie = canonical_d2(p, q[a:a + step])
        live = d2 < c2
        cnt = live.sum(axis=1)
        d2c = np.where(live, d2, np.float32(np.inf))
        if k <= n:
            kth = np.partition(d2c, k - 1, axis=1)[:, k - 1]
        else:
            kth = np.full(d2.shape[0], np.inf, dtype=np.float32)
        found = cnt >= k
        kth = np.where(found, kth, c2).astype(np.float32)
        ties[a:a + step] = np.where(found, (d2c == kth[:, None]).sum(axis=1), 0)
        ref_bits = np.where(found, kth, c2).view(np.int32).astype(np.int64)
        near = np.abs(d2.view(np.int32).astype(np.int64) - ref_bits[:, None]) <= 4
        und[a:a + step] = (tie & near).any(axis=1)
        with np.errstate(invalid="ignore"):
            out[a:a + step] = np.where(np.isinf(kth), kth, np.sqrt(kth.astype(np.float64)).astype(np.float32))
    return out, und, ties


# ------------------------------------------------------------------------------- inputs
@dataclass(frozen=True)
class Case:
    name: str
    k: int
    foreign: bool       # queries are not the points: E.query_points; else E.query on the index
    kernels: tuple      # the kernels the branch exists in
    sample: int = 512   # rows the CPU test takes (at most 2048)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _unit_dirs(n, g):
    d = torch.randn((n, 3), generator=g)
    return d / d.norm(dim=1, keepdim=True)


def _shuffle(p, g):
    return p[torch.randperm(p.shape[0], generator=g)].contiguous()


def _copies(nsites, ncopies, seed):
    g = _g(seed)
    sites = torch.rand((nsites, 3), generator=g)
    return sites, _shuffle(sites.repeat_interleave(ncopies, dim=0), g)


def _shell(n, lo, hi, g):
    return _unit_dirs(n, g) * (lo + (hi - lo) * torch.rand((n, 1), generator=g))


@lru_cache(maxsize=None)
def case_input(name: str):
    """(points float32 [n, 3], queries float32 [nq, 3] or None for self queries)."""
    if name == "overflow":  # 300 clumps of 24: the 8-NN estimate is the clump's, the k-th lies in other clumps
        g = _g(101)
        c = torch.rand((300, 3), generator=g)
        return _shuffle(c.repeat_interleave(24, dim=0) + 1e-4 * (torch.rand((7200, 3), generator=g) - 0.5), g), None
    if name == "zero_fail":  # every site 12 times: the zero probe finds 12 < k zeros
        return _copies(2000, 12, 102)[1], None
    if name == "zero_ok":  # every site 200 times: the zero probe finds k zeros
        return _copies(100, 200, 103)[1], None
    if name == "underflow1":  # a dense core inside sparse data: sparse groups near the core start too high
        g = _g(104)
        core = 0.5 + 1e-2 * (torch.rand((4000, 3), generator=g) - 0.5)
        return _shuffle(torch.cat([core, torch.rand((4000, 3), generator=g)]), g), None
    if name == "underflow2":  # distinct foreign queries exactly on sites with 20 >= k copies
        sites, p = _copies(1000, 20, 105)
        return p, sites.clone()
    if name == "band1":  # six exact ties at the 7th value, twenty at the 27th (i / 16: exact coordinates,
        return lattice(16), None  # so equal distances are equal bits, which i / 24 does not give)
    if name == "ties":  # 512 exact lattice sites, 32 copies each: 192 equal values around the k-th
        g = _g(106)
        return _shuffle(lattice(8).repeat_interleave(32, dim=0), g), None
    if name == "refine":  # 200 points and 64 queries at the centre of a shell of 4000: k reaches the shell
        g = _g(107)
        near = 1e-3 * (torch.rand((200, 3), generator=g) - 0.5)
        q = 1e-3 * (torch.rand((64, 3), generator=g) - 0.5)
        return _shuffle(torch.cat([_shell(4000, 0.97, 1.03, g), near]), g), q
    if name == "crowd_hi":
        # a shell of 6000 around 512 queries, inside sparse far data: the range from the located
        # bucket's points reaches the shell in a middle bin, which then holds thousands of values
        g = _g(108)
        q = 1e-3 * (torch.rand((512, 3), generator=g) - 0.5)
        far = 100.0 * (torch.rand((3000, 3), generator=g) - 0.5)
        far = far[far.norm(dim=1) > 8.0]
        return _shuffle(torch.cat([_shell(6000, 0.94, 1.06, g), far]), g), q
    if name == "crowd_lo":
        # the same shell; 24 queries at its centre share their two groups of 64 curve-sorted
        # queries with 104 decoy queries 50 away, whichever side of them the decoys sort on. A
        # group's located bucket is that of its median query, a decoy: the 24 take their first
        # range from far points, orders of magnitude above the shell, which saturates bin 0
        g = _g(109)
        real = 1e-3 * (torch.rand((24, 3), generator=g) - 0.5)
        decoy = 30.0 + (torch.rand((104, 3), generator=g) - 0.5)
        far = 100.0 * (torch.rand((3000, 3), generator=g) - 0.5)
        far = far[far.norm(dim=1) > 8.0]
        return _shuffle(torch.cat([_shell(6000, 0.94, 1.06, g), far]), g), torch.cat([real, decoy]).contiguous()
    if name == "binwrap":  # 70 000 copies of A, 64 distinct points at nearly one distance from it
        g = _g(110)
        a = torch.tensor([[0.5, 0.5, 0.5]])
        ring = a + _unit_dirs(64, g) * (0.25 + 1e-3 * torch.rand((64, 1), generator=g))
        return _shuffle(torch.cat([a.repeat(70_000, 1), ring]), g), None
    if name == "walk":  # 300 000 points in a 1e-3 cube, 64 sparse points whose k-th lies in it
        g = _g(111)
        core = 0.5 + 1e-3 * (torch.rand((300_000, 3), generator=g) - 0.5)
        sparse = 0.5 + _unit_dirs(64, g) * (0.8 + 0.4 * torch.rand((64, 1), generator=g))
        return torch.cat([sparse, core]).contiguous(), None  # (rows 0..63: the sparse points)
    if name == "hint":  # every wave 64 copies of one site: estimate 0, neighbours far, k > 64
        return _copies(300, 64, 112)[1], None
    if name == "uniform":  # init_d2 and the cutoffs
        return uniform(20000, seed=113), None
    if name == "tiny":  # k == n and k > n
        return uniform(100, seed=114), None
    raise KeyError(name)


BOTH = ("rows", "grid")
CASES = [
    Case("overflow", 100, False, BOTH),
    Case("zero_fail", 16, False, BOTH),
    Case("zero_fail", 100, False, BOTH),
    Case("zero_ok", 100, False, BOTH),
    Case("underflow1", 16, False, BOTH),
    Case("underflow2", 16, True, BOTH),
    Case("band1", 7, False, BOTH),
    Case("band1", 27, False, BOTH),
    Case("ties", 100, False, BOTH),
    Case("refine", 250, True, BOTH),
    Case("crowd_hi", 16, True, ("rows",)),
    Case("crowd_lo", 16, True, ("rows",)),
    Case("binwrap", 100, False, BOTH, sample=256),
    Case("walk", 100, False, BOTH, sample=128),
    Case("hint", 100, False, BOTH),
    Case("uniform", 16, False, BOTH, sample=256),
    Case("tiny", 100, False, BOTH),
    Case("tiny", 101, False, BOTH),
]


@lru_cache(maxsize=None)
def uniform_cutoffs(k: int) -> tuple:
    """Squared cutoffs for the `uniform` input: the canonical k-th d² of one of its points
    (the median of its first 512 rows), one float above it and one float below it."""
    p, _ = case_input("uniform")
    m = np.float32(np.sort(canonical_kth_d2(p, p[:512], k))[256])
    return float(m), float(np.nextafter(m, np.float32(np.inf))), float(np.nextafter(m, np.float32(0)))


def canonical_kth_d2(points, queries, k) -> np.ndarray:
    """The k-th smallest canonical float32 d² per row (no cutoff, no sqrt)."""
    out = []
    step = _rows_per_chunk(_np(points).shape[0])
    q = _np(queries)
    for a in range(0, q.shape[0], step):
        out.append(np.partition(canonical_d2(points, q[a:a + step])[0], k - 1, axis=1)[:, k - 1])
    return np.concatenate(out)


def case_id(c: Case) -> str:
    return f"{c.name}-k{c.k}"


def sample_rows(c: Case) -> torch.Tensor:
    """The query rows the references are taken on: all, or a fixed sample of c.sample rows
    (walk: 8 of the sparse points, the rest from the core)."""
    p, q = case_input(c.name)
    nq = (q if q is not None else p).shape[0]
    if nq <= c.sample:
        return torch.arange(nq)
    if c.name == "walk":
        return torch.cat([torch.arange(8), 64 + torch.randperm(nq - 64, generator=_g(7))[:c.sample - 8]])
    return torch.randperm(nq, generator=_g(7))[:c.sample].sort().values


def bracket_counts_torch(points, queries, v, device="cpu"):
    """bracket_counts with torch float64 tensors on `device` (the same plain sum, chunked):
    the whole query set of a case in a fraction of a second on a GPU."""
    p = torch.as_tensor(_np(points)).to(device=device, dtype=torch.float64)
    q = torch.as_tensor(_np(queries)).to(device=device, dtype=torch.float64)
    v2 = torch.as_tensor(_np(v)).to(device=device, dtype=torch.float64) ** 2
    lo = torch.zeros(q.shape[0], dtype=torch.int64, device=device)
    hi = torch.zeros(q.shape[0], dtype=torch.int64, device=device)
    step = max(1, (1 << 25) // max(p.shape[0], 1))
    for a in range(0, q.shape[0], step):
        d = q[a:a + step, None, :] - p[None, :, :]
        D = (d * d).sum(dim=2)
        t = v2[a:a + step, None]
        lo[a:a + step] = (D < t * (1.0 - EPS)).sum(dim=1)
        hi[a:a + step] = (D <= t * (1.0 + EPS)).sum(dim=1)
    return lo.cpu().numpy(), hi.cpu().numpy()

"""Anisotropic pair counts on the CPU: the brute-force oracle K.pair_counts_2d_cpu against a plain
numpy reference written from the contract (pair_counts_2d_ref.py), shell_counts_2d, every argument
error and the public functions through a CPU index. Everything is an integer: no tolerance."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import pair_counts_2d_ref as R
from datasets import uniform
from mpi_cuda_largescaleknn_amd import (pair_counts_rppi, pair_counts_smu, pair_query_counts_rppi,
                                        pair_query_counts_smu, pair_self_counts_rppi, pair_self_counts_smu,
                                        shell_counts_2d)
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

INF = math.inf
N, NQ = 600, 200
PERIODS = (None, (1.0, 1.0, 1.0), (1.0, INF, 0.5))
# duplicated edges, a zero and (open box) inf; within the bound 0.25 of the shortest period used
RP = (0.0, 0.03, 0.08, 0.08, 0.15, 0.25)
PI = (0.02, 0.05, 0.05, 0.11, 0.2, 0.25)
S = (0.04, 0.09, 0.09, 0.17, 0.25)
MU = (0.0, 0.2, 0.5, 0.5, 0.9, 1.0, INF)

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def case():
    """600 points in the unit box and 200 queries: half of them data points (d2 == 0 pairs), one
    with a NaN coordinate and one with an infinite one."""
    def make():
        p = uniform(N, seed=71).contiguous()
        q = torch.cat([p[:NQ // 2], uniform(NQ - NQ // 2, seed=72)]).contiguous()
        q[NQ // 2 + 3, 1] = float("nan")
        q[NQ // 2 + 7, 2] = INF
        q[5, 0] = -INF
        return p, q
    return cached("case", make)


def edges(mode, period, squared):
    first, second = (RP, PI) if mode == "rppi" else (S, MU)
    if period is None:
        first = first + (INF,)
        if mode == "rppi":
            second = second + (INF,)
    if squared:
        first = tuple(E.cut2_of(r) for r in first)
        if mode == "rppi":
            second = tuple(E.cut2_of(r) for r in second)
    return first, second


def cut2s(mode, first, second, squared):
    a2 = [float(np.float32(r)) if squared else E.cut2_of(r) for r in first]
    b2 = [float(np.float32(r)) if squared and mode == "rppi" else E.cut2_of(r) for r in second]
    return a2, b2


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso", "aniso"))
@pytest.mark.parametrize("los", (0, 1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_oracle_equals_the_numpy_reference(mode, los, period):
    p, q = case()
    if period is not None and not math.isfinite(period[los]) and mode == "rppi":
        first, second = edges(mode, None, False)  # an open line of sight admits every pi
        first = first[:-1]
    else:
        first, second = edges(mode, period, False)
    a2, b2 = cut2s(mode, first, second, False)
    got = K.pair_counts_2d_cpu(p, q, a2, b2, mode, los, period)
    assert got.dtype == torch.int64 and got.shape == (len(a2), len(b2))
    want = R.pair_counts_2d(p, q, a2, b2, mode, los, period)
    assert np.array_equal(got.numpy(), want)
    assert want[-1, -1] > 0
    # cumulative on both axes, duplicated edges give equal rows / columns
    assert bool((got[1:] >= got[:-1]).all()) and bool((got[:, 1:] >= got[:, :-1]).all())
    assert torch.equal(got[2], got[3]) if mode == "rppi" else torch.equal(got[1], got[2])


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_non_finite_queries_count_nothing(mode):
    p, q = case()
    bad = ~torch.isfinite(q).all(1)
    assert int(bad.sum()) == 3
    first, second = edges(mode, None, False)
    a2, b2 = cut2s(mode, first, second, False)
    assert int(K.pair_counts_2d_cpu(p, q[bad], a2, b2, mode, 2).sum()) == 0
    assert torch.equal(K.pair_counts_2d_cpu(p, q, a2, b2, mode, 2), K.pair_counts_2d_cpu(p, q[~bad], a2, b2, mode, 2))


def test_open_period_equals_the_open_box():
    p, q = case()
    for mode in ("rppi", "smu"):
        first, second = edges(mode, None, False)
        a2, b2 = cut2s(mode, first, second, False)
        assert torch.equal(K.pair_counts_2d_cpu(p, q, a2, b2, mode, 1, (INF, INF, INF)),
                           K.pair_counts_2d_cpu(p, q, a2, b2, mode, 1))


def test_smu_consequences_of_the_strict_product():
    """d2 == 0 pairs count in no column; mu < 1 excludes pairs along the line of sight, inf takes
    them in."""
    p = torch.tensor([[0.5, 0.5, 0.5], [0.5, 0.5, 0.6], [0.6, 0.5, 0.5]])
    got = pair_self_counts_smu(p, [1.0], [1.0, INF])
    # ordered pairs: 6 in all; the two along z have par2 == d2 and fail par2 < 1 * d2
    assert got.tolist() == [[4, 6]]
    assert pair_self_counts_rppi(p, [1.0], [1.0]).tolist() == [[9]]  # with the three self pairs


# ---------------------------------------------------------------- 2. the API on a CPU index
def api_case():
    p, q = case()
    return p, q, cached("index", lambda: E.build_index(p))


@pytest.mark.parametrize("squared", (False, True), ids=("radii", "squared"))
@pytest.mark.parametrize("period", PERIODS[:2], ids=("open", "iso"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_api_on_a_cpu_index(mode, period, squared):
    p, q, index = api_case()
    first, second = edges(mode, period, squared)
    a2, b2 = cut2s(mode, first, second, squared)
    want = torch.from_numpy(R.pair_counts_2d(p, q, a2, b2, mode, 2, period))
    fn, fq, fs = ((pair_counts_rppi, pair_query_counts_rppi, pair_self_counts_rppi) if mode == "rppi" else
                  (pair_counts_smu, pair_query_counts_smu, pair_self_counts_smu))
    E.reset_kernels_used()
    got = fn(index, q, first, second, squared=squared, period=period)
    assert E.kernels_used() == ["cpu"]
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(fn(index, q, torch.tensor(first, dtype=torch.float64), list(second), los="z",
                          squared=squared, period=period), want)
    assert torch.equal(fq(p, q, first, second, squared=squared, period=period), want)
    self_want = torch.from_numpy(R.pair_counts_2d(p, p, a2, b2, mode, 2, period))
    assert torch.equal(fs(p, first, second, squared=squared, period=period), self_want)
    # los by name, against the reference on that axis
    assert torch.equal(fn(index, q, first, second, los="x", squared=squared, period=period),
                       torch.from_numpy(R.pair_counts_2d(p, q, a2, b2, mode, 0, period)))


def test_nothing_to_count_gives_zeros():
    p, q, index = api_case()
    none = torch.empty((0, 3))
    zeros = torch.zeros((2, 3), dtype=torch.int64)
    assert torch.equal(pair_counts_rppi(index, none, (0.1, 0.2), (0.1, 0.2, 0.3)), zeros)
    assert torch.equal(pair_query_counts_rppi(none, q, (0.1, 0.2), (0.1, 0.2, 0.3)), zeros)
    assert torch.equal(pair_query_counts_smu(none, q, (0.1, 0.2), (0.1, 0.2, 0.3)), zeros)
    assert torch.equal(pair_self_counts_smu(none, (0.1, 0.2), (0.1, 0.2, 0.3)), zeros)
    assert torch.equal(pair_counts_smu(index, none, (0.1, 0.2), (0.1, 0.2, 0.3)), zeros)


def test_shell_counts_2d():
    g = torch.Generator().manual_seed(3)
    D = torch.randint(0, 1000, (5, 7), generator=g, dtype=torch.int64)
    S2 = D.cumsum(0).cumsum(1)
    assert torch.equal(shell_counts_2d(S2), D)
    assert torch.equal(shell_counts_2d(S2[:1, :1]), D[:1, :1])
    assert torch.equal(S2, D.cumsum(0).cumsum(1))  # (the argument is left alone)
    with pytest.raises(ValueError):
        shell_counts_2d(S2[0])
    p, q, index = api_case()
    a2, b2 = cut2s("rppi", RP, PI, False)
    par2, perp2, _ = R.components(p, q, 2)
    S3 = pair_counts_rppi(index, q, RP, PI)
    cells = shell_counts_2d(S3)
    for i in (1, 2, 4):
        for j in (0, 3):
            with np.errstate(invalid="ignore"):
                want = np.count_nonzero((perp2 < np.float32(a2[i])) & ~(perp2 < np.float32(a2[i - 1])) &
                                        (par2 < np.float32(b2[j])) &
                                        (~(par2 < np.float32(b2[j - 1])) if j else True))
            assert int(cells[i, j]) == want


# ---------------------------------------------------------------- 3. argument errors
@pytest.mark.parametrize("fn", (pair_counts_rppi, pair_counts_smu))
def test_argument_errors(fn):
    p, q, index = api_case()
    ok = (0.1, 0.2)
    E.reset_kernels_used()
    for bad in ((0.2, 0.1), (-0.1, 0.2), (0.1, float("nan")), (), "ab", torch.tensor([1, 2]),
                torch.tensor([[0.1, 0.2]])):
        with pytest.raises(ValueError):
            fn(index, q, bad, ok)
        with pytest.raises(ValueError):
            fn(index, q, ok, bad)
    for los in (3, -1, "w", 1.0, None, True):
        with pytest.raises(ValueError, match="los"):
            fn(index, q, ok, ok, los=los)
    # too many edges on one axis; too many cells
    with pytest.raises(ValueError, match="2048"):
        fn(index, q, [0.1] * 2049, ok)
    with pytest.raises(ValueError, match="65536"):
        fn(index, q, [0.1] * 257, [0.1] * 256)
    fn(index, q[:2], [0.1] * 256, [0.1] * 256)
    with pytest.raises(ValueError, match="period"):
        fn(index, q, ok, ok, period=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="float32"):
        fn(index, q.double(), ok, ok)
    for other in (dataclasses.replace(index, line=True), dataclasses.replace(index, qrot=torch.eye(3))):
        with pytest.raises(ValueError, match="not supported"):
            fn(other, q, ok, ok)
    assert E.kernels_used() == ["cpu"]  # (the one call that was valid)


def test_period_bounds_per_component():
    p, q, index = api_case()
    per = (1.0, 0.6, 0.4)  # bounds 0.5, 0.3, 0.2
    # (rp, pi): pi against the line of sight alone, rp against the shorter perpendicular axis
    pair_counts_rppi(index, q, (0.3,), (0.2,), los=2, period=per)
    with pytest.raises(ValueError, match="line-of-sight"):
        pair_counts_rppi(index, q, (0.3,), (0.21,), los=2, period=per)
    with pytest.raises(ValueError, match="perpendicular"):
        pair_counts_rppi(index, q, (0.31,), (0.2,), los=2, period=per)
    pair_counts_rppi(index, q, (0.2,), (0.5,), los=0, period=per)
    with pytest.raises(ValueError, match="perpendicular"):
        pair_counts_rppi(index, q, (0.21,), (0.5,), los=0, period=per)
    with pytest.raises(ValueError, match="line-of-sight"):
        pair_counts_rppi(index, q, (0.2,), (0.51,), los=0, period=per)
    # squared cutoffs against the squared bounds
    pair_counts_rppi(index, q, (E.cut2_of(0.3),), (E.cut2_of(0.2),), los=2, squared=True, period=per)
    with pytest.raises(ValueError, match="line-of-sight"):
        pair_counts_rppi(index, q, (E.cut2_of(0.3),), (0.05,), los=2, squared=True, period=per)
    # an open axis bounds nothing
    pair_counts_rppi(index, q, (0.3,), (7.0, INF), los=2, period=(1.0, 0.6, INF))
    pair_counts_rppi(index, q, (0.3, INF), (0.2,), los=2, period=(INF, INF, 0.4))
    # (s, mu): s against both, mu against nothing
    pair_counts_smu(index, q, (0.2,), (0.5, 1.0, INF), los=0, period=per)
    with pytest.raises(ValueError, match="perpendicular"):
        pair_counts_smu(index, q, (0.21,), (0.5,), los=0, period=per)
    with pytest.raises(ValueError, match="line-of-sight"):
        pair_counts_smu(index, q, (0.21,), (0.5,), los=2, period=(1.0, 0.6, 0.4))
    with pytest.raises(ValueError):
        pair_counts_smu(index, q, (0.1,), (0.5, -1.0), period=per)


def test_oracle_argument_errors():
    p, q = case()
    with pytest.raises(ValueError):
        K.pair_counts_2d_cpu(p, q, [0.2, 0.1], [0.1], "rppi")
    with pytest.raises(ValueError):
        K.pair_counts_2d_cpu(p, q, [0.1], [], "rppi")
    with pytest.raises(ValueError, match="mode"):
        K.pair_counts_2d_cpu(p, q, [0.1], [0.1], "other")
    with pytest.raises(ValueError, match="los"):
        K.pair_counts_2d_cpu(p, q, [0.1], [0.1], "smu", 3)

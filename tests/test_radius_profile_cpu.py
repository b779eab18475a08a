"""Radius profiles on the CPU: the brute-force oracle K.radius_profile_cpu against a plain numpy
reference and against the single-radius oracles, column by column, and the public functions
(radius_profile, pair_counts and their *_query_* / *_self_* forms) through a CPU index. Every
row is compared; everything is an integer, so there is no tolerance."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import radius_profile_ref as R
from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd import (pair_counts, pair_query_counts, pair_self_counts, radius_profile,
                                        radius_query_profile, radius_self_profile)
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

INF = math.inf
SIZES = (1, 63, 64, 65, 1000)
RADII = (0.0, 0.02, 0.07, 0.07, 0.15, 0.3, 0.5)  # 0.5 = the bound of period 1
PERIODS = (None, (1.0, 1.0, 1.0), (1.0, INF, 0.75))

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def cut2s_of(radii):
    return [E.cut2_of(r) for r in radii]


def radii_for(period):
    """RADII within the period's bound (the anisotropic one admits 0.375), + inf on the open box."""
    if period is None:
        return RADII + (INF,)
    bound = E.period_radius_bound(period, False)
    return tuple(min(r, bound) for r in RADII)


def check_columns(p, q, cut2s, period, got):
    """Every column against the single-radius oracle at that cutoff."""
    for b, c in enumerate(cut2s):
        if period is None:
            want = K.radius_count_cpu(p, q, c)
        else:
            want = K.radius_periodic_count_cpu(p, q, c, period)
        assert torch.equal(got[:, b], want), f"column {b} (cut2 {c})"


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso", "aniso"))
@pytest.mark.parametrize("nq", SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_oracle_equals_the_numpy_reference_at_every_size(n, nq, period):
    p, q = uniform(n, seed=41), uniform(nq, seed=42)
    cut2s = cut2s_of(radii_for(period))
    got = K.radius_profile_cpu(p, q, cut2s, period)
    assert got.dtype == torch.int32 and got.shape == (nq, len(cut2s))
    assert np.array_equal(got.numpy(), R.radius_profile(p, q, cut2s, period))
    check_columns(p, q, cut2s, period, got)
    assert torch.equal(K.pair_counts_cpu(p, q, cut2s, period), got.sum(0, dtype=torch.int64))


@pytest.mark.parametrize("period", PERIODS[:2], ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "clustered", "duplicates", "planar"))
def test_oracle_equals_the_numpy_reference_on_every_dataset(name, period):
    p = GENERATORS[name](1000, seed=43)
    g = torch.Generator().manual_seed(44)
    q = torch.cat([p[torch.randint(0, 1000, (500,), generator=g)], uniform(500, seed=45)]).contiguous()
    cut2s = cut2s_of(radii_for(period))
    got = K.radius_profile_cpu(p, q, cut2s, period)
    assert np.array_equal(got.numpy(), R.radius_profile(p, q, cut2s, period))
    check_columns(p, q, cut2s, period, got)
    pairs = K.pair_counts_cpu(p, q, cut2s, period)
    assert pairs.dtype == torch.int64 and torch.equal(pairs, got.sum(0, dtype=torch.int64))


# ---------------------------------------------------------------- 2. the public functions, CPU index
def api_case():
    def make():
        p = GENERATORS["clustered"](1000, seed=46)
        q = torch.cat([p[:300], uniform(300, seed=47)]).contiguous()
        return p, q, E.build_index(p)
    return cached("api", make)


@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso", "aniso"))
def test_api_columns_equal_radius_counts(period):
    p, q, index = api_case()
    radii = radii_for(period)
    E.reset_kernels_used()
    stats = E.KnnStats()
    prof = radius_profile(index, q, radii, period=period, stats=stats)
    assert E.kernels_used() == ["cpu"]
    assert prof.dtype == torch.int32 and prof.shape == (q.shape[0], len(radii))
    for b, r in enumerate(radii):
        assert torch.equal(prof[:, b], E.radius_counts(index, q, r, period=period)), f"column {b}"
    assert bool((prof[:, 1:] >= prof[:, :-1]).all())  # cumulative
    assert torch.equal(prof[:, 2], prof[:, 3])  # the duplicated radius
    assert int(prof[:, 0].abs().sum()) == 0  # r = 0
    assert np.array_equal(prof.numpy(), R.radius_profile(p, q, cut2s_of(radii), period))
    pairs = pair_counts(index, q, radii, period=period)
    assert pairs.dtype == torch.int64 and torch.equal(pairs, prof.sum(0, dtype=torch.int64))
    # the forms that build the index themselves; radii as tensors
    assert torch.equal(radius_query_profile(p, q, torch.tensor(radii, dtype=torch.float64), period=period), prof)
    assert torch.equal(pair_query_counts(p, q, torch.tensor(radii, dtype=torch.float32), period=period), pairs)
    self_prof = radius_self_profile(p, radii, period=period)
    assert torch.equal(self_prof, radius_profile(index, p, radii, period=period))
    assert torch.equal(pair_self_counts(p, radii, period=period), self_prof.sum(0, dtype=torch.int64))
    # squared cutoffs handed in as they are
    assert torch.equal(radius_profile(index, q, cut2s_of(radii), squared=True, period=period), prof)


def test_infinite_radius_counts_every_point_and_bad_queries_count_nothing():
    p, q, index = api_case()
    q = q.clone()
    q[5, 0] = math.nan
    q[6, 2] = INF
    q[7] = -INF
    radii = (0.0, 0.05, INF, INF)
    prof = radius_profile(index, q, radii)
    finite = torch.isfinite(q).all(dim=1)
    assert int(finite.sum()) == q.shape[0] - 3
    assert bool((prof[finite][:, 2:] == p.shape[0]).all())
    assert int(prof[~finite].abs().sum()) == 0
    assert torch.equal(pair_counts(index, q, radii), prof.sum(0, dtype=torch.int64))
    # under a period an open axis still admits no infinite radius: the finite ones bound it
    per = (1.0, 1.0, 1.0)
    pp = radius_profile(index, q, (0.0, 0.5), period=per)
    assert int(pp[~finite].abs().sum()) == 0 and int(pp[:, 0].abs().sum()) == 0
    assert torch.equal(radius_profile(index, q, radii, period=(INF, INF, INF)), prof)


def test_empty_inputs_give_zeros_of_the_right_shape():
    p, q, index = api_case()
    none = torch.empty((0, 3), dtype=torch.float32)
    assert radius_profile(index, none, (0.1, 0.2)).shape == (0, 2)
    assert torch.equal(pair_counts(index, none, (0.1, 0.2)), torch.zeros(2, dtype=torch.int64))
    got = radius_query_profile(none, q, (0.1, 0.2, 0.3))
    assert got.dtype == torch.int32 and got.shape == (q.shape[0], 3) and int(got.abs().sum()) == 0
    assert torch.equal(pair_query_counts(none, q, (0.1, 0.2, 0.3)), torch.zeros(3, dtype=torch.int64))
    assert radius_self_profile(none, (0.1,)).shape == (0, 1)
    assert torch.equal(pair_self_counts(none, (0.1,)), torch.zeros(1, dtype=torch.int64))


BAD = [
    (dict(radii=()), "at least one"),
    (dict(radii=torch.empty(0)), "at least one"),
    (dict(radii=(0.1, -0.2)), ">= 0"),
    (dict(radii=(0.1, math.nan)), ">= 0"),
    (dict(radii=(0.2, 0.1)), "ascend"),
    (dict(radii=(0.1, 0.6), period=1.0), "half the period"),
    (dict(radii=(0.1, 0.26), period=1.0, squared=True), "half the period"),
    (dict(radii=(0.1, INF), period=(1.0, INF, INF)), "half the period"),
    (dict(radii=(0.1,), period=0.0), "period"),
    (dict(radii=(0.1,), period=(1.0, 2.0)), "period"),
    (dict(radii=torch.tensor([1, 2])), "float32 / float64"),
    (dict(radii="abc"), "sequence of numbers"),
]


@pytest.mark.parametrize("fn", (radius_profile, pair_counts), ids=("profile", "pairs"))
@pytest.mark.parametrize("kw,msg", BAD, ids=[m + str(i) for i, (_, m) in enumerate(BAD)])
def test_bad_arguments_raise_before_anything_runs(fn, kw, msg):
    p, q, index = api_case()
    E.reset_kernels_used()
    with pytest.raises(ValueError, match=msg):
        fn(index, q, **kw)
    with pytest.raises(ValueError, match=msg):  # also where there is nothing to index
        (radius_query_profile if fn is radius_profile else pair_query_counts)(q[:0], q, **kw)
    assert E.kernels_used() == []


@pytest.mark.parametrize("fn", (radius_profile, pair_counts), ids=("profile", "pairs"))
def test_bad_queries_and_unsupported_indexes_raise(fn):
    p, q, index = api_case()
    E.reset_kernels_used()
    with pytest.raises(ValueError, match="float32"):
        fn(index, q.double(), (0.1,))
    with pytest.raises(ValueError, match="float32"):
        fn(index, q[:, :2], (0.1,))
    # (rotated-frame and line-keyed indexes are built on the GPU only: the flags alone decide)
    for other in (dataclasses.replace(index, line=True), dataclasses.replace(index, qrot=torch.eye(3))):
        with pytest.raises(ValueError, match="not supported"):
            fn(other, q, (0.1,))
    assert E.kernels_used() == []


# ---------------------------------------------------------------- 3. cutoffs on existing values
@pytest.mark.parametrize("period", PERIODS[:2], ids=("open", "iso"))
def test_cutoffs_placed_exactly_on_distances_separate_as_the_oracle_does(period):
    p, q, index = api_case()
    v = R.dist2(p, q[:40], period)  # float32 [40, n]: the bit patterns of real pairs
    pick = np.sort(v.reshape(-1))[[50, 700, 2000, 5000]]
    assert np.all(pick > 0) and np.all(pick < 0.2)  # (below the squared bound of period 1)
    cuts = []
    for d2 in pick:
        cuts += [np.nextafter(d2, np.float32(0)), d2, np.nextafter(d2, np.float32(1))]
    cuts = np.unique(np.asarray(cuts, dtype=np.float32))  # ascending
    cut2s = [float(c) for c in cuts]
    got = radius_profile(index, q, cut2s, squared=True, period=period)
    want = R.radius_profile(p, q, cut2s, period)
    assert np.array_equal(got.numpy(), want)
    check_columns(p, q, cut2s, period, got)
    for d2 in pick:  # strict: the pair at d2 is out at the cutoff d2 and in one float above
        b = int(np.searchsorted(cuts, d2))
        hits = int((v == d2).sum())
        assert hits >= 1 and int((want[:40, b + 1] - want[:40, b]).sum()) == hits

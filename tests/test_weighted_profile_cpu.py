"""Weighted radius profiles on the CPU: the brute-force oracle K.weighted_profile_cpu /
K.weighted_pair_sums_cpu against a plain numpy reference, the public functions through a CPU
index, every argument error with both overflow bounds at their edges, and fixed_point_weights.
Every row is compared; everything is an integer, so there is no tolerance."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import weighted_profile_ref as R
from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd import (PointWeights, fixed_point_weights, prepare_point_weights,
                                        weighted_pair_query_sums, weighted_pair_self_sums, weighted_pair_sums,
                                        weighted_profile, weighted_query_profile, weighted_self_profile)
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

INF = math.inf
SIZES = (1, 63, 64, 65, 1000)
RADII = (0.0, 0.02, 0.07, 0.07, 0.15, 0.3, 0.5)  # 0.5 = the bound of period 1
ISO = (1.0, 1.0, 1.0)
PERIODS = (None, ISO)
KINDS = ("pm2^20", "ones", "zeros", "one huge")

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def cut2s_of(radii):
    return [E.cut2_of(r) for r in radii]


def radii_for(period):
    return RADII + (INF,) if period is None else RADII


def weights_of(kind, n, seed=60):
    g = torch.Generator().manual_seed(seed + n)
    if kind == "pm2^20":
        return torch.randint(-(1 << 20), (1 << 20) + 1, (n,), generator=g, dtype=torch.int64)
    if kind == "ones":
        return torch.ones(n, dtype=torch.int64)
    if kind == "zeros":
        return torch.zeros(n, dtype=torch.int64)
    w = torch.zeros(n, dtype=torch.int64)  # one huge (negative) weight, as large as n admits, the rest 0
    w[int(torch.randint(0, n, (1,), generator=g))] = -(((1 << 62) - 1) // n)
    return w


def check_oracle(p, q, period):
    cut2s = cut2s_of(radii_for(period))
    n, nq = p.shape[0], q.shape[0]
    wq = torch.randint(-1000, 1001, (nq,), generator=torch.Generator().manual_seed(61), dtype=torch.int64)
    for kind in KINDS:
        w = weights_of(kind, n)
        got = K.weighted_profile_cpu(p, q, cut2s, w, period)
        assert got.dtype == torch.int64 and got.shape == (nq, len(cut2s)), kind
        assert np.array_equal(got.numpy(), R.weighted_profile(p, q, cut2s, w, period)), kind
        pairs = K.weighted_pair_sums_cpu(p, q, cut2s, w, period)
        assert pairs.dtype == torch.int64 and torch.equal(pairs, got.sum(0, dtype=torch.int64)), kind
        if kind != "one huge":  # (its products with a query weight leave int64: not a valid input)
            pairs = K.weighted_pair_sums_cpu(p, q, cut2s, w, period, query_weights=wq)
            assert np.array_equal(pairs.numpy(), R.weighted_pair_sums(p, q, cut2s, w, period, wq)), kind
        if kind == "ones":
            assert torch.equal(got, K.radius_profile_cpu(p, q, cut2s, period).long())
            assert torch.equal(K.weighted_pair_sums_cpu(p, q, cut2s, w, period),
                               K.pair_counts_cpu(p, q, cut2s, period))
        if kind == "zeros":
            assert int(got.abs().sum()) == 0


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso"))
@pytest.mark.parametrize("nq", SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_oracle_equals_the_numpy_reference_at_every_size(n, nq, period):
    check_oracle(uniform(n, seed=41), uniform(nq, seed=42), period)


@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "clustered", "duplicates", "planar"))
def test_oracle_equals_the_numpy_reference_on_every_dataset(name, period):
    p = GENERATORS[name](1000, seed=43)
    g = torch.Generator().manual_seed(44)
    q = torch.cat([p[torch.randint(0, 1000, (500,), generator=g)], uniform(500, seed=45)]).contiguous()
    check_oracle(p, q, period)


# ---------------------------------------------------------------- 2. the public functions, CPU index
def api_case():
    def make():
        p = GENERATORS["clustered"](1000, seed=46)
        q = torch.cat([p[:300], uniform(300, seed=47)]).contiguous()
        return p, q, E.build_index(p), weights_of("pm2^20", 1000)
    return cached("api", make)


@pytest.mark.parametrize("period", (None, ISO, (1.0, INF, 0.75)), ids=("open", "iso", "aniso"))
def test_api_returns_the_oracle(period):
    p, q, index, w = api_case()
    radii = RADII + (INF,) if period is None else tuple(min(r, E.period_radius_bound(period, False)) for r in RADII)
    cut2s = cut2s_of(radii)
    E.reset_kernels_used()
    stats = E.KnnStats()
    prof = weighted_profile(index, q, radii, w, period=period, stats=stats)
    assert E.kernels_used() == ["cpu"]
    assert prof.dtype == torch.int64 and prof.shape == (q.shape[0], len(radii))
    assert torch.equal(prof, K.weighted_profile_cpu(p, q, cut2s, w, period))  # (p in input order: w too)
    assert np.array_equal(prof.numpy(), R.weighted_profile(p, q, cut2s, w, period))
    assert torch.equal(prof[:, 2], prof[:, 3]) and int(prof[:, 0].abs().sum()) == 0
    wq = torch.randint(-50, 51, (q.shape[0],), generator=torch.Generator().manual_seed(62), dtype=torch.int64)
    pairs = weighted_pair_sums(index, q, radii, w, period=period)
    assert pairs.dtype == torch.int64 and torch.equal(pairs, prof.sum(0, dtype=torch.int64))
    pairs_q = weighted_pair_sums(index, q, radii, w, query_weights=wq, period=period)
    assert torch.equal(pairs_q, (prof * wq[:, None]).sum(0, dtype=torch.int64))
    assert torch.equal(pairs_q, K.weighted_pair_sums_cpu(p, q, cut2s, w, period, query_weights=wq))
    # prepared weights; the forms that build the index themselves; radii as a tensor; squared cutoffs
    pw = prepare_point_weights(index, w)
    assert isinstance(pw, PointWeights) and pw.abs_sum == int(w.abs().sum())
    assert torch.equal(pw.sorted, w[index.perm[:index.n].long()])
    assert torch.equal(weighted_profile(index, q, radii, pw, period=period), prof)
    assert torch.equal(weighted_pair_sums(index, q, radii, pw, query_weights=wq, period=period), pairs_q)
    assert torch.equal(weighted_query_profile(p, q, torch.tensor(radii, dtype=torch.float64), w, period=period), prof)
    assert torch.equal(weighted_pair_query_sums(p, q, radii, w, query_weights=wq, period=period), pairs_q)
    self_prof = weighted_self_profile(p, radii, w, period=period)
    assert torch.equal(self_prof, weighted_profile(index, p, radii, w, period=period))
    assert torch.equal(weighted_pair_self_sums(p, radii, w, period=period),
                       (self_prof * w[:, None]).sum(0, dtype=torch.int64))  # `weights` on both sides
    ones = torch.ones(p.shape[0], dtype=torch.int64)
    assert torch.equal(weighted_pair_self_sums(p, radii, w, query_weights=ones, period=period),
                       self_prof.sum(0, dtype=torch.int64))
    assert torch.equal(weighted_profile(index, q, cut2s, w, squared=True, period=period), prof)
    # unit weights: radius_profile and pair_counts
    assert torch.equal(weighted_profile(index, q, radii, ones, period=period),
                       E.radius_profile(index, q, radii, period=period).long())
    assert torch.equal(weighted_pair_sums(index, q, radii, ones, period=period),
                       E.pair_counts(index, q, radii, period=period))


def test_infinite_radius_sums_every_weight_and_bad_queries_sum_nothing():
    p, q, index, w = api_case()
    q = q.clone()
    q[5, 0] = math.nan
    q[6, 2] = INF
    q[7] = -INF
    prof = weighted_profile(index, q, (0.0, 0.05, INF), w)
    finite = torch.isfinite(q).all(dim=1)
    assert bool((prof[finite][:, 2] == int(w.sum())).all())
    assert int(prof[~finite].abs().sum()) == 0 and int(prof[:, 0].abs().sum()) == 0
    assert torch.equal(weighted_profile(index, q, (0.0, 0.05, INF), w, period=(INF, INF, INF)), prof)


def test_empty_inputs_give_zeros_of_the_right_shape():
    p, q, index, w = api_case()
    none = torch.empty((0, 3), dtype=torch.float32)
    w0 = torch.empty(0, dtype=torch.int64)
    got = weighted_profile(index, none, (0.1, 0.2), w)
    assert got.shape == (0, 2) and got.dtype == torch.int64
    assert torch.equal(weighted_pair_sums(index, none, (0.1, 0.2), w, query_weights=w0),
                       torch.zeros(2, dtype=torch.int64))
    got = weighted_query_profile(none, q, (0.1, 0.2, 0.3), w0)
    assert got.dtype == torch.int64 and got.shape == (q.shape[0], 3) and int(got.abs().sum()) == 0
    assert torch.equal(weighted_pair_query_sums(none, q, (0.1, 0.2, 0.3), w0), torch.zeros(3, dtype=torch.int64))
    assert weighted_self_profile(none, (0.1,), w0).shape == (0, 1)
    assert torch.equal(weighted_pair_self_sums(none, (0.1,), w0), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):  # the weights are checked all the same
        weighted_query_profile(none, q, (0.1,), w)


# ---------------------------------------------------------------- 3. errors
BAD_RADII = [
    (dict(radii=()), "at least one"),
    (dict(radii=(0.1, -0.2)), ">= 0"),
    (dict(radii=(0.1, math.nan)), ">= 0"),
    (dict(radii=(0.2, 0.1)), "ascend"),
    (dict(radii=(0.1, 0.6), period=1.0), "half the period"),
    (dict(radii=(0.1, 0.26), period=1.0, squared=True), "half the period"),
    (dict(radii=(0.1,), period=0.0), "period"),
    (dict(radii=(0.1,), period=(1.0, 2.0)), "period"),
    (dict(radii=torch.tensor([1, 2])), "float32 / float64"),
    (dict(radii="abc"), "sequence of numbers"),
]


@pytest.mark.parametrize("fn", (weighted_profile, weighted_pair_sums), ids=("profile", "pairs"))
@pytest.mark.parametrize("kw,msg", BAD_RADII, ids=[m + str(i) for i, (_, m) in enumerate(BAD_RADII)])
def test_every_argument_error_of_radius_profile_is_raised(fn, kw, msg):
    p, q, index, w = api_case()
    E.reset_kernels_used()
    with pytest.raises(ValueError, match=msg):
        fn(index, q, weights=w, **kw)
    with pytest.raises(ValueError, match=msg):  # also where there is nothing to index
        (weighted_query_profile if fn is weighted_profile else weighted_pair_query_sums)(
            q[:0], q, weights=w[:0], **kw)
    assert E.kernels_used() == []


@pytest.mark.parametrize("fn", (weighted_profile, weighted_pair_sums), ids=("profile", "pairs"))
def test_bad_weights_queries_and_indexes_raise(fn):
    p, q, index, w = api_case()
    E.reset_kernels_used()
    for bad in (w.int(), w.double(), w[:-1], w[:, None], w.tolist(), None):
        with pytest.raises(ValueError, match="int64"):
            fn(index, q, (0.1,), bad)
    with pytest.raises(ValueError, match="int64"):
        prepare_point_weights(index, w.float())
    other = E.build_index(p[:500])
    with pytest.raises(ValueError, match="another index"):
        fn(index, q, (0.1,), prepare_point_weights(other, w[:500]))
    with pytest.raises(ValueError, match="float32"):
        fn(index, q.double(), (0.1,), w)
    for unsupported in (dataclasses.replace(index, line=True), dataclasses.replace(index, qrot=torch.eye(3))):
        with pytest.raises(ValueError, match="not supported"):
            fn(unsupported, q, (0.1,), w)
    wq = torch.ones(q.shape[0], dtype=torch.int64)
    for bad in (wq.int(), wq[:-1], wq.double()):
        with pytest.raises(ValueError, match="query_weights"):
            weighted_pair_sums(index, q, (0.1,), w, query_weights=bad)
    assert E.kernels_used() == []


def test_both_overflow_bounds_at_their_edges():
    third = ((1 << 62) - 1) // 3
    assert third * 3 == (1 << 62) - 1
    p3, p4 = uniform(3, seed=48), uniform(4, seed=48)
    i3, i4 = E.build_index(p3), E.build_index(p4)
    q = uniform(5, seed=49)
    # max|w| * n = 2^62 - 1 passes (and the sums are exact), 2^62 raises, whatever the sign
    w3 = torch.tensor([third, -1, 5], dtype=torch.int64)
    got = weighted_profile(i3, q, (INF,), w3)
    assert got[:, 0].tolist() == [third + 4] * 5
    assert prepare_point_weights(i3, -w3).abs_sum == third + 6
    for w4 in ([1 << 60, 0, 0, 0], [0, 0, -(1 << 60), 1], [-(1 << 63), 0, 0, 0]):
        with pytest.raises(ValueError, match="2\\^62"):
            weighted_profile(i4, q, (INF,), torch.tensor(w4, dtype=torch.int64))
        with pytest.raises(ValueError, match="2\\^62"):
            prepare_point_weights(i4, torch.tensor(w4, dtype=torch.int64))
    assert weighted_profile(i4, q, (INF,), torch.tensor([(1 << 60) - 1, 0, 0, 0]))[0, 0] == (1 << 60) - 1
    # A_p * A_q = 2^63 - 1 passes, 2^63 raises
    w = torch.tensor([0, 1, 0], dtype=torch.int64)  # A_p = 1
    q2 = p3[1:3].contiguous()
    ok = torch.tensor([1 << 62, -((1 << 62) - 1)], dtype=torch.int64)  # A_q = 2^63 - 1
    assert weighted_pair_sums(i3, q2, (INF,), w, query_weights=ok).tolist() == [1]
    assert weighted_pair_sums(i3, q2, (1e-3, INF), w, query_weights=ok).tolist() == [1 << 62, 1]
    for bad in ([1 << 62, 1 << 62], [-(1 << 62), 1 << 62], [-(1 << 63), 0]):  # A_q >= 2^63
        with pytest.raises(ValueError, match="2\\^63"):
            weighted_pair_sums(i3, q2, (INF,), w, query_weights=torch.tensor(bad, dtype=torch.int64))
    # without query weights A_q = nq
    big = torch.tensor([(1 << 60) + 1, 0, -(1 << 60)], dtype=torch.int64)  # A_p = 2^61 + 1, max * n < 2^62
    assert weighted_profile(i3, q, (INF,), big)[0, 0] == 1
    assert weighted_pair_sums(i3, q[:3], (INF,), big).tolist() == [3]  # 3 * (2^61 + 1) < 2^63
    with pytest.raises(ValueError, match="2\\^63"):
        weighted_pair_sums(i3, q[:4], (INF,), big)  # 4 * (2^61 + 1) > 2^63
    w2 = torch.tensor([1 << 60, -(1 << 60), 0], dtype=torch.int64)  # A_p = 2^61
    assert weighted_pair_sums(i3, q[:3], (INF,), w2).tolist() == [0]
    with pytest.raises(ValueError, match="2\\^63"):
        weighted_pair_sums(i3, q[:4], (INF,), w2)  # 4 * 2^61 = 2^63 exactly


# ---------------------------------------------------------------- 4. fixed_point_weights
def test_fixed_point_weights_are_exact_when_the_spread_fits():
    g = torch.Generator().manual_seed(63)
    # float32 masses with 24-bit mantissas over 2^10 of dynamic range: 34 bits of spread
    w = (torch.rand(1000, generator=g) + 0.5) * torch.pow(2.0, torch.randint(-5, 6, (1000,), generator=g).float())
    w[::3] *= -1
    for dtype in (torch.float32, torch.float64):
        fix, s = fixed_point_weights(w.to(dtype))
        assert fix.dtype == torch.int64 and fix.shape == w.shape
        assert torch.equal(torch.ldexp(fix.double(), torch.tensor(s)), w.double())  # w_fix * 2^s == w
        e_a = math.frexp(float(w.abs().max()))[1]
        assert s == e_a + 10 - 62  # ceil(log2(1000)) = 10
        assert int(fix.abs().sum()) <= 1 << 62
    # the result feeds the weighted functions: the physical sum is result * 2^s
    p = uniform(1000, seed=64)
    fix, s = fixed_point_weights(w)
    total = weighted_self_profile(p, (INF,), fix)[0, 0]
    assert math.ldexp(int(total), s) == float(w.double().sum())


@pytest.mark.parametrize("bits", (1, 8, 31, 62))
@pytest.mark.parametrize("n_terms", (1, 3, 1 << 20))
def test_fixed_point_sum_guarantee(n_terms, bits):
    """sum |w_fix| <= 2^bits for any n_terms weights no larger than the largest one: the bound per
    weight is 2^(bits - ceil(log2 n_terms)), reached by the largest itself."""
    n = min(n_terms, 4096)
    w = torch.full((n,), 0.999999, dtype=torch.float64)  # all at the maximum, just under 2^eA
    w[1::2] *= -1
    fix, s = fixed_point_weights(w, n_terms=n_terms, bits=bits)
    e_n = (n_terms - 1).bit_length()
    assert s == 0 + e_n - bits
    assert int(fix.abs().max()) * n_terms <= 1 << bits
    if n == n_terms:
        assert int(fix.abs().sum()) <= 1 << bits
    err = (torch.ldexp(fix.double(), torch.tensor(s)) - w).abs().max()
    assert float(err) <= math.ldexp(1.0, s - 1)
    exact_max = torch.tensor([1.0, -0.25], dtype=torch.float32)  # A = 2^0 has frexp exponent 1
    fix, s = fixed_point_weights(exact_max, n_terms=n_terms, bits=bits)
    assert s == 1 + e_n - bits and int(fix.abs().max()) * n_terms <= 1 << bits


def test_fixed_point_ties_round_to_even_and_special_values():
    # with A = 4 (eA = 3), n_terms = 1 and bits = 3 the quantum is 2^0: halves are ties
    w = torch.tensor([4.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 0.49, 0.51], dtype=torch.float64)
    fix, s = fixed_point_weights(w, n_terms=1, bits=3)
    assert s == 0 and fix.tolist() == [4, 0, 2, 2, 0, -2, -2, 4, 0, 1]
    fix, s = fixed_point_weights(torch.zeros(5, dtype=torch.float32))
    assert s == 0 and fix.dtype == torch.int64 and fix.tolist() == [0] * 5
    fix, s = fixed_point_weights(torch.empty(0, dtype=torch.float64))
    assert s == 0 and fix.shape == (0,)
    # the extremes of float64's range scale exactly
    fix, s = fixed_point_weights(torch.tensor([1e300, -5e299], dtype=torch.float64))
    assert math.ldexp(int(fix[0]), s) == 1e300 and math.ldexp(int(fix[1]), s) == -5e299
    fix, s = fixed_point_weights(torch.tensor([1e-300, 3e-301], dtype=torch.float64))
    assert math.ldexp(int(fix[0]), s) == 1e-300 and math.ldexp(int(fix[1]), s) == 3e-301
    for bad in (math.nan, INF, -INF):
        with pytest.raises(ValueError, match="finite"):
            fixed_point_weights(torch.tensor([1.0, bad]))
    for bits in (0, 63, -1, 2.5, True):
        with pytest.raises(ValueError, match="bits"):
            fixed_point_weights(torch.ones(3), bits=bits)
    with pytest.raises(ValueError, match="n_terms"):
        fixed_point_weights(torch.ones(3), n_terms=0)
    for bad in (torch.ones(3, dtype=torch.int64), torch.ones((2, 2)), [1.0, 2.0]):
        with pytest.raises(ValueError, match="float32 / float64"):
            fixed_point_weights(bad)

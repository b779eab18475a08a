"""Weighted anisotropic pair sums on the CPU: the brute-force oracle K.weighted_pair_sums_2d_cpu
against a plain numpy reference with Python-integer sums (weighted_pair_sums_2d_ref.py), the
identities the sums must obey (unit weights, linearity, data minus randoms), every argument error
and the six public functions through a CPU index. Everything is an integer: no tolerance."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import weighted_pair_sums_2d_ref as R
from datasets import uniform
from mpi_cuda_largescaleknn_amd import (prepare_point_weights, shell_counts_2d, weighted_pair_query_sums_rppi,
                                        weighted_pair_query_sums_smu, weighted_pair_self_sums_rppi,
                                        weighted_pair_self_sums_smu, weighted_pair_sums_rppi,
                                        weighted_pair_sums_smu)
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

INF = math.inf
N, NQ = 300, 120
PERIODS = (None, (1.0, 1.0, 1.0), (1.0, INF, 0.8))
# duplicated edges, a zero and (open box) inf; within the bound 0.4 of the shortest period used
RP = (0.0, 0.05, 0.12, 0.12, 0.25, 0.4)
PI = (0.03, 0.08, 0.08, 0.2, 0.4)
S = (0.06, 0.15, 0.15, 0.3, 0.4)
MU = (0.0, 0.2, 0.5, 0.5, 0.9, 1.0, INF)

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def case():
    """300 points in the unit box and 120 queries: half of them data points (d2 == 0 pairs), one
    with a NaN coordinate and one with an infinite one; point weights in +-2^34, query weights in
    +-2^4."""
    def make():
        p = uniform(N, seed=81).contiguous()
        q = torch.cat([p[:NQ // 2], uniform(NQ - NQ // 2, seed=82)]).contiguous()
        q[NQ // 2 + 3, 1] = float("nan")
        q[NQ // 2 + 7, 2] = INF
        g = torch.Generator().manual_seed(83)
        w = torch.randint(-(1 << 34), (1 << 34) + 1, (N,), generator=g, dtype=torch.int64)
        wq = torch.randint(-16, 17, (NQ,), generator=g, dtype=torch.int64)
        return p, q, w, wq
    return cached("case", make)


def edges(mode, period):
    first, second = (RP, PI) if mode == "rppi" else (S, MU)
    if period is None:
        first = first + (INF,)
        if mode == "rppi":
            second = second + (INF,)
    return first, second


def cut2s(first, second):
    return [E.cut2_of(r) for r in first], [E.cut2_of(r) for r in second]


def ref(p, q, a2, b2, w, mode, los, period, wq):
    return torch.from_numpy(R.as_int64(R.weighted_pair_sums_2d(p, q, a2, b2, w, mode, los, period, wq)))


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso", "aniso"))
@pytest.mark.parametrize("los", (0, 1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_oracle_equals_the_numpy_reference(mode, los, period):
    p, q, w, wq = case()
    if period is not None and not math.isfinite(period[los]) and mode == "rppi":
        first, second = edges(mode, None)  # an open line of sight admits every pi
        first = first[:-1]
    else:
        first, second = edges(mode, period)
    a2, b2 = cut2s(first, second)
    assert bool((w < 0).any()) and bool((wq < 0).any()) and int(w.abs().max()) > 1 << 32
    got = K.weighted_pair_sums_2d_cpu(p, q, a2, b2, w, mode, los, period, query_weights=wq)
    assert got.dtype == torch.int64 and got.shape == (len(a2), len(b2))
    assert torch.equal(got, ref(p, q, a2, b2, w, mode, los, period, wq))
    assert int(got[-1, -1]) != 0
    got1 = K.weighted_pair_sums_2d_cpu(p, q, a2, b2, w, mode, los, period)
    assert torch.equal(got1, ref(p, q, a2, b2, w, mode, los, period, None))
    # duplicated edges give equal rows
    assert torch.equal(got[2], got[3]) if mode == "rppi" else torch.equal(got[1], got[2])


@pytest.mark.parametrize("period", PERIODS, ids=("open", "iso", "aniso"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_unit_weights_are_the_counts(mode, period):
    p, q, _, _ = case()
    a2, b2 = cut2s(*edges(mode, PERIODS[1]))
    ones = torch.ones(N, dtype=torch.int64)
    want = K.pair_counts_2d_cpu(p, q, a2, b2, mode, 0, period)
    assert torch.equal(K.weighted_pair_sums_2d_cpu(p, q, a2, b2, ones, mode, 0, period), want)
    assert torch.equal(K.weighted_pair_sums_2d_cpu(p, q, a2, b2, ones, mode, 0, period,
                                                   query_weights=torch.ones(NQ, dtype=torch.int64)), want)


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_linearity(mode):
    p, q, w1, wq = case()
    g = torch.Generator().manual_seed(84)
    w2 = torch.randint(-(1 << 30), 1 << 30, (N,), generator=g, dtype=torch.int64)
    a2, b2 = cut2s(*edges(mode, PERIODS[1]))

    def ws(w, wq_):
        return K.weighted_pair_sums_2d_cpu(p, q, a2, b2, w, mode, 2, PERIODS[1], query_weights=wq_)
    assert torch.equal(ws(w1 + w2, wq), ws(w1, wq) + ws(w2, wq))
    assert torch.equal(ws(w1, -7 * wq), -7 * ws(w1, wq))
    assert torch.equal(ws(w1, None), ws(w1, torch.ones(NQ, dtype=torch.int64)))


@pytest.mark.parametrize("period", PERIODS[:2], ids=("open", "iso"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_data_minus_randoms(mode, period):
    """D u R with weights (+1, -1), queried with itself: DD - DR - RD + RR of four counts."""
    d, r = uniform(170, seed=85).contiguous(), uniform(230, seed=86).contiguous()
    both = torch.cat([d, r])
    w = torch.cat([torch.ones(170, dtype=torch.int64), -torch.ones(230, dtype=torch.int64)])
    a2, b2 = cut2s(*edges(mode, PERIODS[1]))

    def c(points, queries):
        return K.pair_counts_2d_cpu(points, queries, a2, b2, mode, 1, period)
    want = c(d, d) - c(r, d) - c(d, r) + c(r, r)
    assert torch.equal(K.weighted_pair_sums_2d_cpu(both, both, a2, b2, w, mode, 1, period, query_weights=w), want)
    fs = weighted_pair_self_sums_rppi if mode == "rppi" else weighted_pair_self_sums_smu
    first, second = edges(mode, PERIODS[1])
    assert torch.equal(fs(both, first, second, w, los=1, period=period), want)


def test_non_finite_queries_add_nothing_and_zero_distance_pairs():
    p, q, w, wq = case()
    bad = ~torch.isfinite(q).all(1)
    assert int(bad.sum()) == 2
    for mode in ("rppi", "smu"):
        a2, b2 = cut2s(*edges(mode, None))
        assert int(K.weighted_pair_sums_2d_cpu(p, q[bad], a2, b2, w, mode, 2, None,
                                               query_weights=wq[bad]).abs().sum()) == 0
    # (s, mu): a pair at distance 0 adds nowhere; (rp, pi): a point with itself adds w^2
    pts = torch.tensor([[0.5, 0.5, 0.5], [0.5, 0.5, 0.6], [0.6, 0.5, 0.5]])
    w3 = torch.tensor([2, -3, 5])
    assert weighted_pair_self_sums_rppi(pts, [1.0], [1.0], w3).tolist() == [[(2 - 3 + 5) ** 2]]
    # ordered pairs with d2 > 0: all six for mu = inf; mu = 1 leaves out the two along z
    assert weighted_pair_self_sums_smu(pts, [1.0], [1.0, INF], w3).tolist() == \
        [[2 * (2 * 5 - 3 * 5), 2 * (2 * -3 + 2 * 5 - 3 * 5)]]


# ---------------------------------------------------------------- 2. the API on a CPU index
def api_case():
    p, q, w, wq = case()
    return p, q, w, wq, cached("index", lambda: E.build_index(p))


@pytest.mark.parametrize("squared", (False, True), ids=("radii", "squared"))
@pytest.mark.parametrize("period", PERIODS[:2], ids=("open", "iso"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_api_on_a_cpu_index(mode, period, squared):
    p, q, w, wq, index = api_case()
    first, second = edges(mode, period)
    a2, b2 = cut2s(first, second)
    if squared:
        first = a2
        second = b2 if mode == "rppi" else second
    fn, fq, fs = ((weighted_pair_sums_rppi, weighted_pair_query_sums_rppi, weighted_pair_self_sums_rppi)
                  if mode == "rppi" else
                  (weighted_pair_sums_smu, weighted_pair_query_sums_smu, weighted_pair_self_sums_smu))
    want = ref(p, q, a2, b2, w, mode, 2, period, wq)
    E.reset_kernels_used()
    got = fn(index, q, first, second, w, query_weights=wq, squared=squared, period=period)
    assert E.kernels_used() == ["cpu"]
    assert got.dtype == torch.int64 and got.shape == want.shape and torch.equal(got, want)
    # the prepared weights, the queries in two chunks
    pw = prepare_point_weights(index, w)
    parts = [fn(index, q[s], first, second, pw, query_weights=wq[s], squared=squared, period=period)
             for s in (slice(0, 50), slice(50, NQ))]
    assert torch.equal(parts[0] + parts[1], want)
    assert torch.equal(fq(p, q, first, second, w, query_weights=wq, squared=squared, period=period), want)
    assert torch.equal(fn(index, q, first, second, w, los="x", squared=squared, period=period),
                       ref(p, q, a2, b2, w, mode, 0, period, None))
    # self forms: weights on both sides unless query weights are given
    ws = w >> 14  # +-2^20: (sum |w|)^2 < 2^63
    assert torch.equal(fs(p, first, second, ws, squared=squared, period=period),
                       K.weighted_pair_sums_2d_cpu(p, p, a2, b2, ws, mode, 2, period, query_weights=ws))
    one = torch.ones(N, dtype=torch.int64)
    assert torch.equal(fs(p, first, second, w, query_weights=one, squared=squared, period=period),
                       K.weighted_pair_sums_2d_cpu(p, p, a2, b2, w, mode, 2, period))
    # shell_counts_2d applies as is: the cells sum back to the last entry
    assert int(shell_counts_2d(got).sum()) == int(got[-1, -1])


def test_nothing_to_sum_gives_zeros():
    p, q, w, wq, index = api_case()
    none = torch.empty((0, 3))
    w0 = torch.empty(0, dtype=torch.int64)
    zeros = torch.zeros((2, 3), dtype=torch.int64)
    ea, eb = (0.1, 0.2), (0.1, 0.2, 0.3)
    for fn, fq, fs in ((weighted_pair_sums_rppi, weighted_pair_query_sums_rppi, weighted_pair_self_sums_rppi),
                       (weighted_pair_sums_smu, weighted_pair_query_sums_smu, weighted_pair_self_sums_smu)):
        assert torch.equal(fn(index, none, ea, eb, w), zeros)
        assert torch.equal(fn(index, none, ea, eb, w, query_weights=w0), zeros)
        assert torch.equal(fq(none, q, ea, eb, w0, query_weights=wq), zeros)
        assert torch.equal(fq(none, q, ea, eb, w0), zeros)
        assert torch.equal(fs(none, ea, eb, w0), zeros)
        with pytest.raises(ValueError, match="weights"):
            fq(none, q, ea, eb, w)  # 300 weights for no point
        with pytest.raises(ValueError, match="query_weights"):
            fn(index, none, ea, eb, w, query_weights=wq)


# ---------------------------------------------------------------- 3. argument errors
@pytest.mark.parametrize("fn", (weighted_pair_sums_rppi, weighted_pair_sums_smu))
def test_weight_errors(fn):
    p, q, w, wq, index = api_case()
    ok = (0.1, 0.2)
    name = fn.__name__
    E.reset_kernels_used()
    for bad in (w.float(), w.int(), w[:-1], w[:, None], w.tolist(), None):
        with pytest.raises(ValueError, match=name):
            fn(index, q, ok, ok, bad)
    for bad in (wq.double(), wq[:-1], wq[None, :], wq.tolist()):
        with pytest.raises(ValueError, match=name + ".*query_weights"):
            fn(index, q, ok, ok, w, query_weights=bad)
    if torch.cuda.is_available():  # the device of either weight tensor
        with pytest.raises(ValueError, match=name):
            fn(index, q, ok, ok, w.cuda())
        with pytest.raises(ValueError, match=name):
            fn(index, q, ok, ok, w, query_weights=wq.cuda())
    else:
        meta = torch.empty(N, dtype=torch.int64, device="meta")
        with pytest.raises(ValueError, match=name):
            fn(index, q, ok, ok, meta)
        with pytest.raises(ValueError, match=name):
            fn(index, q, ok, ok, w, query_weights=torch.empty(NQ, dtype=torch.int64, device="meta"))
    # max|w| * n >= 2^62
    big = torch.ones(N, dtype=torch.int64)
    big[7] = -((1 << 62) // N + 1)
    with pytest.raises(ValueError, match=name + ".*2\\^62"):
        fn(index, q, ok, ok, big)
    big = torch.full((N,), (1 << 62) // N - 1, dtype=torch.int64)  # sum |w| just below 2^62
    # (sum |w|) * (sum |wq|) >= 2^63: with query weights, and with nq in their place
    with pytest.raises(ValueError, match=name + ".*2\\^63"):
        fn(index, q, ok, ok, big, query_weights=torch.full((NQ,), -1, dtype=torch.int64))
    with pytest.raises(ValueError, match=name + ".*2\\^63"):
        fn(index, q, ok, ok, big)
    heavy = torch.zeros(NQ, dtype=torch.int64)
    heavy[0] = 1 << 40
    with pytest.raises(ValueError, match=name + ".*2\\^63"):
        fn(index, q, ok, ok, w, query_weights=heavy)
    fn(index, q[:1], ok, ok, big)  # one query: sum |w| < 2^62 stands alone
    # weights prepared for another index
    other = E.build_index(p.clone())
    with pytest.raises(ValueError, match=name + ".*another index"):
        fn(index, q, ok, ok, prepare_point_weights(other, w))
    # the errors of the unweighted functions, and the unsupported indexes
    for bad in ((0.2, 0.1), (-0.1, 0.2), (), [0.1] * 2049):
        with pytest.raises(ValueError, match=name):
            fn(index, q, bad, ok, w)
    with pytest.raises(ValueError, match="65536"):
        fn(index, q, [0.1] * 257, [0.1] * 256, w)
    with pytest.raises(ValueError, match="los"):
        fn(index, q, ok, ok, w, los=3)
    with pytest.raises(ValueError, match="half the period"):
        fn(index, q, (0.6,), ok, w, period=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="float32"):
        fn(index, q.double(), ok, ok, w)
    for odd in (dataclasses.replace(index, line=True), dataclasses.replace(index, qrot=torch.eye(3))):
        with pytest.raises(ValueError, match="not supported"):
            fn(odd, q, ok, ok, w)
    assert E.kernels_used() == ["cpu"]  # (the one call that was valid)


def test_query_and_self_forms_name_themselves():
    p, q, w, wq, _ = api_case()
    ok = (0.1, 0.2)
    for fq in (weighted_pair_query_sums_rppi, weighted_pair_query_sums_smu):
        with pytest.raises(ValueError, match=fq.__name__):
            fq(p, q, ok, ok, w[:-1])
        with pytest.raises(ValueError, match=fq.__name__):
            fq(p, q, ok, ok, w, query_weights=wq[:-1])
    for fs in (weighted_pair_self_sums_rppi, weighted_pair_self_sums_smu):
        with pytest.raises(ValueError, match=fs.__name__):
            fs(p, ok, ok, w.float())
        with pytest.raises(ValueError, match=fs.__name__ + ".*2\\^63"):
            fs(p, ok, ok, torch.full((N,), 1 << 31, dtype=torch.int64))


def test_oracle_argument_errors():
    p, q, w, wq = case()
    with pytest.raises(ValueError):
        K.weighted_pair_sums_2d_cpu(p, q, [0.2, 0.1], [0.1], w, "rppi")
    with pytest.raises(ValueError, match="mode"):
        K.weighted_pair_sums_2d_cpu(p, q, [0.1], [0.1], w, "other")
    with pytest.raises(ValueError, match="los"):
        K.weighted_pair_sums_2d_cpu(p, q, [0.1], [0.1], w, "smu", 3)
    with pytest.raises(ValueError, match="weights"):
        K.weighted_pair_sums_2d_cpu(p, q, [0.1], [0.1], w[:-1], "smu")
    with pytest.raises(ValueError, match="query_weights"):
        K.weighted_pair_sums_2d_cpu(p, q, [0.1], [0.1], w, "smu", query_weights=wq.float())

"""Anisotropic pair counts with the line of sight of an observer (los='midpoint') on the CPU: the
brute-force oracles K.pair_counts_2d_observer_cpu / K.weighted_pair_sums_2d_observer_cpu against a
plain numpy reference written from the contract (pair_counts_observer_ref.py), the consequences the
contract names, every argument error, and hipKNN_pairs / lsknn_tools pcheck on the CPU device.
Everything is an integer: no tolerance."""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import pair_counts_observer_ref as R
from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.apps import pairs as pairs_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

INF = math.inf
N, NQ = 600, 200
NW, NQW = 300, 100  # the weighted reference sums Python integers pair by pair
RP = (0.0, 0.03, 0.08, 0.08, 0.15, 0.25, INF)
PI = (0.02, 0.05, 0.05, 0.11, 0.2, INF)
S = (0.04, 0.09, 0.09, 0.17, 0.25, INF)
MU = (0.0, 0.2, 0.5, 0.5, 0.9, 1.0, INF)
DATASETS = ("uniform", "clustered", "duplicates")
OBSERVERS = ("far", "corner", "centre", "on_point")
FNS = {
    "rppi": (E.pair_counts_rppi, E.pair_query_counts_rppi, E.pair_self_counts_rppi, E.weighted_pair_sums_rppi,
             E.weighted_pair_query_sums_rppi, E.weighted_pair_self_sums_rppi),
    "smu": (E.pair_counts_smu, E.pair_query_counts_smu, E.pair_self_counts_smu, E.weighted_pair_sums_smu,
            E.weighted_pair_query_sums_smu, E.weighted_pair_self_sums_smu),
}

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def data(name, n=N):
    def make():
        if name == "duplicates":
            return GENERATORS[name](n, seed=81, ndistinct=max(1, n // 30)).contiguous()
        return GENERATORS[name](n, seed=81).contiguous()
    return cached(("data", name, n), make)


def queries(name, n=N, nq=NQ):
    """Half of them data points (d2 == 0 pairs), half random over the data's range."""
    def make():
        p = data(name, n)
        g = torch.Generator().manual_seed(82)
        lo, hi = p.min(0).values, p.max(0).values
        rnd = lo + (hi - lo) * torch.rand((nq - nq // 2, 3), generator=g)
        return torch.cat([p[torch.randint(0, n, (nq // 2,), generator=g)], rnd]).contiguous()
    return cached(("queries", name, n, nq), make)


def observer(kind, p):
    lo, hi = p.min(0).values, p.max(0).values
    if kind == "far":
        return (0.5, 0.5, -3.0)
    if kind == "corner":
        return tuple(lo.tolist())
    if kind == "centre":
        return tuple((0.5 * (lo + hi)).tolist())
    return tuple(p[7].tolist())  # exactly on a data point


def cut2s(mode):
    first, second = (RP, PI) if mode == "rppi" else (S, MU)
    return first, second, [E.cut2_of(r) for r in first], [E.cut2_of(r) for r in second]


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("obs", OBSERVERS)
@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_oracle_equals_the_numpy_reference(mode, name, obs):
    p, q = data(name), queries(name)
    o = observer(obs, p)
    _, _, a2, b2 = cut2s(mode)
    got = K.pair_counts_2d_observer_cpu(p, q, a2, b2, mode, o)
    want = R.pair_counts_2d_observer(p, q, a2, b2, mode, o)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert int(got[-1, -1]) > N and int(got[0, 0]) < int(got[-1, -1])


@pytest.mark.parametrize("with_wq", (False, True), ids=("w", "w_wq"))
@pytest.mark.parametrize("obs", OBSERVERS)
@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_weighted_oracle_equals_the_numpy_reference(mode, name, obs, with_wq):
    p, q = data(name, NW), queries(name, NW, NQW)
    o = observer(obs, p)
    g = torch.Generator().manual_seed(83)
    w = torch.randint(-(1 << 34), (1 << 34) + 1, (NW,), generator=g, dtype=torch.int64)
    wq = torch.randint(-16, 17, (NQW,), generator=g, dtype=torch.int64) if with_wq else None
    _, _, a2, b2 = cut2s(mode)
    got = K.weighted_pair_sums_2d_observer_cpu(p, q, a2, b2, w, mode, o, query_weights=wq)
    want = R.weighted_pair_sums_2d_observer(p, q, a2, b2, mode, o, w, wq)
    assert got.tolist() == want and want[-1][-1] != 0


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_unit_weights_give_the_counts(mode):
    p, q = data("clustered"), queries("clustered")
    o = observer("centre", p)
    first, second, a2, b2 = cut2s(mode)
    one, oneq = torch.ones(N, dtype=torch.int64), torch.ones(NQ, dtype=torch.int64)
    want = K.pair_counts_2d_observer_cpu(p, q, a2, b2, mode, o)
    assert torch.equal(K.weighted_pair_sums_2d_observer_cpu(p, q, a2, b2, one, mode, o), want)
    assert torch.equal(K.weighted_pair_sums_2d_observer_cpu(p, q, a2, b2, one, mode, o, query_weights=oneq), want)
    index = E.build_index(p)
    counts, _, _, sums, _, _ = FNS[mode]
    assert torch.equal(counts(index, q, first, second, los="midpoint", observer=o), want)
    assert torch.equal(sums(index, q, first, second, one, los="MidPoint", observer=o), want)


# ---------------------------------------------------------------- 2. what the contract implies
@pytest.mark.parametrize("obs", OBSERVERS)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_swapping_the_two_sets_changes_no_bit(mode, obs):
    """Swapping q and p negates sl exactly and leaves ll and d2 alone."""
    a, b = data("clustered"), queries("clustered")
    o = observer(obs, a)
    first, second, _, _ = cut2s(mode)
    fn = FNS[mode][1]
    ab = fn(a, b, first, second, los="midpoint", observer=o)
    ba = fn(b, a, first, second, los="midpoint", observer=o)
    assert torch.equal(ab, ba) and int(ab[-1, -1]) > 0


def grid_case():
    """Coordinates on the grid of multiples of 2^-10 in [0, 1): every difference and sum of the
    contract is exact. 50 queries are 2 o - p for 50 of the points (their pair's midpoint is the
    observer, l == 0 exactly), 50 are other grid positions, 20 are copies of points."""
    def make():
        g = torch.Generator().manual_seed(84)
        pi_ = torch.randint(0, 1024, (200, 3), generator=g)
        oi = torch.tensor([512, 300, 700])
        qi = torch.cat([2 * oi - pi_[:50], torch.randint(0, 1024, (50, 3), generator=g), pi_[100:120]])
        centred = int(((qi[:, None, :] + pi_[None, :, :]) == 2 * oi).all(-1).sum())
        same = int((qi[:, None, :] == pi_[None, :, :]).all(-1).sum())
        both = int((((qi[:, None, :] + pi_[None, :, :]) == 2 * oi).all(-1) &
                    (qi[:, None, :] == pi_[None, :, :]).all(-1)).sum())
        scale = 2.0 ** -10
        return (pi_.float() * scale).contiguous(), (qi.float() * scale).contiguous(), \
            tuple((oi.float() * scale).tolist()), centred, same, both
    return cached("grid", make)


def test_a_pair_whose_midpoint_is_the_observer_counts_nowhere():
    p, q, o, centred, same, both = grid_case()
    assert centred >= 50 and same >= 20
    nq, n = q.shape[0], p.shape[0]
    every = E.pair_query_counts_rppi(p, q, [INF], [INF], los="midpoint", observer=o)
    assert int(every[0, 0]) == nq * n - centred  # ll == 0: 0 / 0, a NaN passes no test
    every = E.pair_query_counts_smu(p, q, [INF], [INF], los="midpoint", observer=o)
    assert int(every[0, 0]) == nq * n - centred - same + both  # and d2 == 0 counts in no (s, mu) cell
    for mode in ("rppi", "smu"):
        first, second, a2, b2 = cut2s(mode)
        got = FNS[mode][1](p, q, first, second, los="midpoint", observer=o)
        assert np.array_equal(got.numpy(), R.pair_counts_2d_observer(p, q, a2, b2, mode, o))
        par2 = R.components(p, q, o)[0]
        assert int(np.isnan(par2).sum()) == centred


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_non_finite_queries_count_nothing(mode):
    p, q = data("uniform"), queries("uniform")
    o = observer("far", p)
    first, second, a2, b2 = cut2s(mode)
    bad = q[:6].clone()
    bad[0, 0] = float("nan")
    bad[1, 1] = INF
    bad[2, 2] = -INF
    bad[3] = float("nan")
    bad[4] = INF
    bad[5, 0], bad[5, 1] = INF, -INF
    fn = FNS[mode][1]
    assert int(fn(p, bad, first, second, los="midpoint", observer=o).abs().sum()) == 0
    assert int(K.pair_counts_2d_observer_cpu(p, bad, a2, b2, mode, o).abs().sum()) == 0
    assert int(R.pair_counts_2d_observer(p, bad, a2, b2, mode, o).sum()) == 0
    mixed = torch.cat([q[:50], bad, q[50:]])
    assert torch.equal(fn(p, mixed, first, second, los="midpoint", observer=o),
                       fn(p, q, first, second, los="midpoint", observer=o))


def test_self_pairs_and_exact_copies():
    """A point with itself and exact copies (d2 == 0): par2 = perp2 = 0, in every (rp, pi) cell with
    cutoffs above 0 and in no (s, mu) cell."""
    p = data("duplicates")
    o = observer("far", p)
    same = int((p[:, None, :] == p[None, :, :]).all(-1).sum())
    assert same > N  # every point with itself, and the copies
    tiny = 2.0 ** -149
    got = E.pair_self_counts_rppi(p, [0.0, tiny, INF], [0.0, tiny, INF], squared=True, los="midpoint", observer=o)
    assert got[0].tolist() == [0, 0, 0] and got[:, 0].tolist() == [0, 0, 0]
    assert int(got[1, 1]) == same and int(got[2, 2]) == N * N
    assert torch.equal(got, E.pair_query_counts_rppi(p, p, [0.0, tiny, INF], [0.0, tiny, INF], squared=True,
                                                     los="midpoint", observer=o))
    got = E.pair_self_counts_smu(p, [tiny, INF], [1.0, INF], squared=True, los="midpoint", observer=o)
    assert got[0].tolist() == [0, 0] and int(got[1, 1]) == N * N - same
    # weighted: w[p]^2 for a point with itself
    w = torch.arange(1, N + 1, dtype=torch.int64)
    ws = E.weighted_pair_self_sums_rppi(p, [tiny], [tiny], w, squared=True, los="midpoint", observer=o)
    eq = (p[:, None, :] == p[None, :, :]).all(-1)
    assert int(ws[0, 0]) == int((w[:, None] * w[None, :])[eq].sum())
    ws = E.weighted_pair_self_sums_smu(p, [tiny], [INF], w, squared=True, los="midpoint", observer=o)
    assert int(ws[0, 0]) == 0


def test_every_mu_gives_pair_counts():
    """Queries that are no data points, the observer far outside: no pair has d2 == 0 or a
    non-finite par2 (checked first), so par2 < inf * d2 holds for every pair and the column mu =
    inf is the isotropic pair count, bit for bit (the two d2 are the same canonical dist2)."""
    p = data("clustered")
    q = queries("clustered")[NQ // 2:]
    o = observer("far", p)
    par2, _, d2 = R.components(p, q, o)
    assert not (d2 == 0).any() and np.isfinite(par2).all()
    s = [0.02, 0.05, 0.11, 0.2, 0.4, INF]
    index = E.build_index(p)
    got = E.pair_counts_smu(index, q, s, [0.5, INF], los="midpoint", observer=o)
    want = E.pair_counts(index, q, s)
    assert torch.equal(got[:, 1], want) and int(want[-1]) == p.shape[0] * q.shape[0]
    assert int(got[-1, 0]) < int(got[-1, 1])


# ---------------------------------------------------------------- 3. argument errors
@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_argument_errors(mode, k):
    p, q = data("uniform"), queries("uniform")
    ok = (0.1, 0.2)
    w = torch.ones(N, dtype=torch.int64)
    fn = FNS[mode][k]
    if k in (0, 3):
        index = E.build_index(p)
        args = (index, q, ok, ok)
    elif k in (1, 4):
        args = (p, q, ok, ok)
    else:
        args = (p, ok, ok)
    if k >= 3:
        args = args + (w,)
    E.reset_kernels_used()
    for bad in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, float("nan")), (0.0, INF, 0.0), (0.0, 0.0, 1e39), 1.0,
                "abc", (0.0, None, 0.0)):
        with pytest.raises(ValueError, match="observer"):
            fn(*args, los="midpoint", observer=bad)
    for los in (0, 1, 2, "x", "Y", "z"):
        with pytest.raises(ValueError, match="observer"):
            fn(*args, los=los, observer=(0.0, 0.0, 0.0))
    for period in (1.0, (1.0, 1.0, 1.0), (INF, INF, INF)):
        with pytest.raises(ValueError, match="period"):
            fn(*args, los="midpoint", period=period)
    for los in ("mid", "midpoints", "observer", 3, None):
        with pytest.raises(ValueError, match="los"):
            fn(*args, los=los)
    if k in (0, 3):
        for other in (dataclasses.replace(index, line=True), dataclasses.replace(index, qrot=torch.eye(3))):
            with pytest.raises(ValueError, match="not supported"):
                fn(other, *args[1:], los="midpoint")
    assert E.kernels_used() == []  # nothing ran
    got = fn(*args, los="Midpoint")  # the observer defaults to the origin
    assert torch.equal(got, fn(*args, los="midpoint", observer=torch.zeros(3)))
    assert torch.equal(got, fn(*args, los="midpoint", observer=[0, 0, 0]))


def test_oracle_argument_errors():
    p, q = data("uniform"), queries("uniform")
    with pytest.raises(ValueError, match="observer"):
        K.pair_counts_2d_observer_cpu(p, q, [0.1], [0.1], "rppi", (0.0, 0.0))
    with pytest.raises(ValueError, match="observer"):
        K.weighted_pair_sums_2d_observer_cpu(p, q, [0.1], [0.1], torch.ones(N, dtype=torch.int64), "smu",
                                             (0.0, INF, 0.0))
    with pytest.raises(ValueError, match="mode"):
        K.pair_counts_2d_observer_cpu(p, q, [0.1], [0.1], "other")
    with pytest.raises(ValueError):
        K.pair_counts_2d_observer_cpu(p, q, [0.2, 0.1], [0.1], "rppi")


# ---------------------------------------------------------------- 4. hipKNN_pairs and pcheck
MODES = {"rppi": ["--rp", "0,0.03,0.08,0.08,0.2", "--pi", "0.02,0.1,0.25,inf"],
         "smu": ["--s", "0.05,0.1,0.1,0.25", "--mu", "0,0.3,0.6,1,inf"]}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("obspairs")
    p, q = data("uniform"), queries("uniform")
    g = torch.Generator().manual_seed(85)
    w = torch.randint(-(1 << 34), (1 << 34) + 1, (N,), generator=g, dtype=torch.int64)
    wq = torch.randint(-16, 17, (NQ,), generator=g, dtype=torch.int64)
    io.write_points(str(d / "p.float3"), p)
    io.write_points(str(d / "q.float3"), q)
    io.write_array(str(d / "w.i64"), w, 0, truncate=True)
    io.write_array(str(d / "wq.i64"), wq, 0, truncate=True)
    return d, p, q, w, wq


@pytest.mark.parametrize("weights", ("none", "w", "w_wq"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_the_cli_round_trip(files, mode, weights, capsys):
    d, p, q, w, wq = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    pre = str(d / f"out_{mode}_{weights}")
    edges = MODES[mode]
    first, second = ([float(v) for v in edges[i].split(",")] for i in (1, 3))
    wopts = [] if weights == "none" else ["--weights", str(d / "w.i64")]
    if weights == "w_wq":
        wopts += ["--query-weights", str(d / "wq.i64")]
    o = (0.25, 0.5, -2.0)
    los = ["--los", "Midpoint", "--observer", "0.25,0.5,-2"]
    assert pairs_app.main([fp, fq, "-o", pre, "--device", "cpu", "--chunk", "70", "--stats", pre + ".json"] + edges +
                          los + wopts) == 0
    a2 = [E.cut2_of(r) for r in first]
    b2 = [E.cut2_of(r) for r in second]
    if weights == "none":
        want = K.pair_counts_2d_observer_cpu(p, q, a2, b2, mode, o)
    else:
        want = K.weighted_pair_sums_2d_observer_cpu(p, q, a2, b2, w, mode, o,
                                                    query_weights=wq if weights == "w_wq" else None)
    ext = ".pairs2d" if weights == "none" else ".wpairs2d"
    got = io.read_array(pre + ext, torch.int64)
    assert torch.equal(got.view(len(first), len(second)), want) and int(want[-1, -1]) != 0
    assert not os.path.exists(pre + (".wpairs2d" if weights == "none" else ".pairs2d"))
    capsys.readouterr()
    check = ["pcheck", fp, fq, pre] + edges + los + wopts
    assert tools.main(check) == 0
    assert f"checked {want.numel()} cells: 0 mismatches" in capsys.readouterr().out
    # another observer, and an axis: the check fails
    assert tools.main(["pcheck", fp, fq, pre] + edges + ["--los", "midpoint", "--observer", "0.25,0.5,-2.5"] +
                      wopts) == 1
    assert tools.main(["pcheck", fp, fq, pre] + edges + ["--los", "z"] + wopts) == 1
    # the default observer is the origin
    assert pairs_app.main([fp, fq, "-o", pre + "_origin", "--device", "cpu", "--los", "midpoint"] + edges + wopts) == 0
    assert tools.main(["pcheck", fp, fq, pre + "_origin", "--los", "midpoint", "--observer", "0,0,0"] + edges +
                      wopts) == 0
    capsys.readouterr()


def test_the_cli_refuses_a_period_and_a_stray_observer(files, capsys):
    d = files[0]
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    base = [fp, fq, "-o", str(d / "bad"), "--device", "cpu", "--rp", "0.1", "--pi", "0.1"]
    assert pairs_app.main(base + ["--los", "midpoint", "--period", "1"]) == 1
    assert "period" in capsys.readouterr().err
    assert pairs_app.main(base + ["--los", "y", "--observer", "0,0,0"]) == 1
    assert "observer" in capsys.readouterr().err
    assert pairs_app.main(base + ["--los", "midpoint", "--observer", "0,0"]) == 1
    assert "observer" in capsys.readouterr().err
    assert pairs_app.main(base + ["--los", "midpoint", "--observer", "0,nan,0"]) == 1
    assert "observer" in capsys.readouterr().err
    assert not (d / "bad.pairs2d").exists()
    assert tools.main(["pcheck", fp, fq, str(d / "bad"), "--rp", "0.1", "--pi", "0.1", "--los", "midpoint",
                       "--period", "1"]) == 1
    assert "period" in capsys.readouterr().out

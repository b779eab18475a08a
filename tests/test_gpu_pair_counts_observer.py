"""Anisotropic pair counts with the line of sight of an observer (los='midpoint') on the GPU: the
observer instances of pair_counts_2d.hip, the whole [B1, B2] array bit for bit against the
brute-force oracles K.pair_counts_2d_observer_cpu / K.weighted_pair_sums_2d_observer_cpu. Data,
indexes and queries are computed once per module; everything is an integer, so there is no
tolerance."""
import math

import pytest
import torch

import scale_cases as SC
from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of the walk
NQ = 1500
MU = (0.1, 0.3, 0.5, 0.5, 0.8, 1.0, INF)
DATASETS = ("uniform", "clustered", "duplicates")
OBSERVERS = ("far", "corner", "centre", "on_point")
MID = "midpoint"

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def r_for(count, n=N, volume=1.0):
    """The radius whose ball holds `count` of n uniform points in `volume`."""
    return (3.0 * count * volume / (4.0 * math.pi * n)) ** (1.0 / 3.0)


def radii_of(B, n=N, top=None):
    """B ascending radii for expected counts from ~1 to ~n / 4 (log-spaced), the third one doubled."""
    top = r_for(n / 4.0, n) if top is None else top
    lo = min(r_for(1.0, n), top)
    r = [lo * (top / lo) ** (i / max(B - 1, 1)) for i in range(B)]
    r[-1] = top
    if B > 3:
        r[3] = r[2]
    return r


def data(name, n=N):
    def make():
        if name == "duplicates":
            return GENERATORS[name](n, seed=51, ndistinct=max(1, n // 30)).contiguous()
        return E.wrap_points(GENERATORS[name](n, seed=51), 1.0).contiguous()
    return cached(("data", name, n), make)


def queries(name, nq=NQ, n=N):
    """Half of them data points, half random over the data's range."""
    def make():
        p = data(name, n)
        g = torch.Generator().manual_seed(52)
        lo, hi = p.min(0).values, p.max(0).values
        rnd = lo + (hi - lo) * torch.rand((nq - nq // 2, 3), generator=g)
        q = torch.cat([p[torch.randint(0, p.shape[0], (nq // 2,), generator=g)], rnd])
        return q[torch.randperm(nq, generator=g)].contiguous()
    return cached(("queries", name, nq, n), make)


def index_of(name, n=N):
    return cached(("index", name, n), lambda: E.build_index(data(name, n).to(DEV)))


def observer(kind, p):
    lo, hi = p.min(0).values, p.max(0).values
    if kind == "far":
        return (0.5, 0.5, -3.0)
    if kind == "corner":
        return tuple(lo.tolist())
    if kind == "centre":
        return tuple((0.5 * (lo + hi)).tolist())
    return tuple(p[7].tolist())  # exactly on a data point


def grid(mode, B1, B2, n=N):
    if mode == "rppi":
        return radii_of(B1, n), radii_of(B2, n)
    mu = list(MU) if B2 == len(MU) else [(j + 1) / B2 for j in range(B2 - 1)] + [INF]
    return radii_of(B1, n), mu


def cut2s(first, second):
    return [E.cut2_of(r) for r in first], [E.cut2_of(r) for r in second]


def same_cells(got, want):
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} of {want.numel()} cells differ from the oracle, first "
                               f"{[(tuple(c), int(got[tuple(c)]), int(want[tuple(c)])) for c in bad[:4].tolist()]}")


def check(mode, index, p, q, first, second, o, stats=None):
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    got = fn(index, q.to(DEV), first, second, los=MID, observer=o, stats=stats)
    assert got.dtype == torch.int64 and got.shape == (len(first), len(second)) and got.device.type == "cuda"
    got = got.cpu()
    same_cells(got, K.pair_counts_2d_observer_cpu(p, q, *cut2s(first, second), mode, o))
    return got


def check_weighted(mode, index, p, q, first, second, o, w, wq=None, weights=None, stats=None):
    fn = E.weighted_pair_sums_rppi if mode == "rppi" else E.weighted_pair_sums_smu
    got = fn(index, q.to(DEV), first, second, w.to(DEV) if weights is None else weights,
             query_weights=None if wq is None else wq.to(DEV), los=MID, observer=o, stats=stats)
    assert got.dtype == torch.int64 and got.shape == (len(first), len(second)) and got.device.type == "cuda"
    got = got.cpu()
    same_cells(got, K.weighted_pair_sums_2d_observer_cpu(p, q, *cut2s(first, second), w, mode, o, query_weights=wq))
    return got


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("obs", OBSERVERS)
@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_equals_the_oracle(mode, name, obs):
    E.reset_kernels_used()
    first, second = grid(mode, 5, 7)
    stats = E.KnnStats()
    p = data(name)
    got = check(mode, index_of(name), p, queries(name), first, second, observer(obs, p), stats=stats)
    assert "pair_counts_2d_observer" in E.kernels_used()
    assert int(got[-1, -1]) > N and int(got[0, 0]) < int(got[-1, -1])
    assert stats.counters["radius_evals"] > 0 and stats.counters["radius_nodes"] > 0
    assert stats.counters["radius_box_accepts"] == 0


# ---------------------------------------------------------------- 2. slices and their cull radius
@pytest.mark.parametrize("shape", ((40, 60), (3, 1500), (2048, 1)), ids=str)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_grid_sizes_and_slices(mode, shape):
    """40 x 60 = 2400 cells > 2048: two slices of whole rows; 3 x 1500: one row per slice; 2048 x
    1: one slice of 2048 rows. Every slice has its own cull radius."""
    first, second = grid(mode, *shape)
    p = data("uniform")
    check(mode, index_of("uniform"), p, queries("uniform"), first, second, observer("far", p))


def test_cutoff_extremes():
    """An edge list that ends in inf on either axis (the cull radius is inf: every node is kept),
    and lists of zeros alone (nothing counts)."""
    p, q, index = data("duplicates"), queries("duplicates"), index_of("duplicates")
    o = observer("centre", p)
    got = check("rppi", index, p, q, [0.0, 0.05, 0.05, 0.3, INF], [0.0, 0.01, 0.2, INF, INF], o)
    assert int(got[-1, -1]) > NQ * N // 2
    check("rppi", index, p, q, [0.05, 0.3, INF], [0.01, 0.2], o)
    check("rppi", index, p, q, [0.05, 0.3], [0.01, 0.2, INF], o)
    check("smu", index, p, q, [0.0, 0.05, INF], [0.0, 0.5, 1.0, INF], o)
    check("smu", index, p, q, [0.05, 0.3], [0.5, INF, INF], o)
    for mode, first, second in (("rppi", [0.0], [0.0, 0.0]), ("rppi", [0.0, 0.0], [0.3]), ("rppi", [0.3], [0.0]),
                                ("smu", [0.0, 0.0], [0.5, INF]), ("smu", [0.3], [0.0])):
        assert int(check(mode, index, p, q, first, second, o).abs().sum()) == 0


@pytest.mark.parametrize("n", (40, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_small_sets(mode, n):
    """One bucket (n = 40) and two (n = 65); with the last edges inf every pair is evaluated."""
    p = data("uniform", n)
    q = torch.cat([p, queries("uniform", 100, n)])
    first, second = grid(mode, 5, 7, n)
    first[-1] = INF
    if mode == "rppi":
        second[-1] = INF
    o = observer("far", p)
    got = check(mode, index_of("uniform", n), p, q, first, second, o)
    same = int((q[:, None, :] == p[None, :, :]).all(-1).sum())
    assert same >= n and int(got[-1, -1]) == (n * (n + 100) if mode == "rppi" else n * (n + 100) - same)
    w = torch.arange(n, dtype=torch.int64) - n // 2  # negative weights too
    check_weighted(mode, index_of("uniform", n), p, q, first, second, o, w)


# ---------------------------------------------------------------- 3. weighted
def weights_of(n=N, nq=NQ):
    def make():
        g = torch.Generator().manual_seed(53)
        w = torch.randint(-(1 << 34), (1 << 34) + 1, (n,), generator=g, dtype=torch.int64)
        wq = torch.randint(-16, 17, (nq,), generator=g, dtype=torch.int64)
        return w, wq
    return cached(("weights", n, nq), make)


@pytest.mark.parametrize("with_wq", (False, True), ids=("w", "w_wq"))
@pytest.mark.parametrize("name", ("clustered", "duplicates"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_weighted_equals_the_oracle(mode, name, with_wq):
    """Negative weights on both sides."""
    E.reset_kernels_used()
    w, wq = weights_of()
    first, second = grid(mode, 5, 7)
    p = data(name)
    stats = E.KnnStats()
    got = check_weighted(mode, index_of(name), p, queries(name), first, second, observer("corner", p), w,
                         wq if with_wq else None, stats=stats)
    assert "weighted_pair_sums_2d_observer" in E.kernels_used()
    assert int(got[-1, -1]) != 0 and bool((w < 0).any()) and bool((wq < 0).any())
    assert stats.counters["radius_evals"] > 0 and stats.counters["radius_box_accepts"] == 0


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_prepared_weights_and_two_slices(mode):
    w, wq = weights_of()
    index, p = index_of("uniform"), data("uniform")
    pw = E.prepare_point_weights(index, w.to(DEV))
    first, second = grid(mode, 40, 60)
    check_weighted(mode, index, p, queries("uniform"), first, second, observer("on_point", p), w, wq, weights=pw)


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_unit_weights_give_the_counts_and_the_same_walk(mode):
    index, p, q = index_of("clustered"), data("clustered"), queries("clustered").to(DEV)
    o = observer("centre", p)
    first, second = grid(mode, 5, 7)
    counts, sums = (E.pair_counts_rppi, E.weighted_pair_sums_rppi) if mode == "rppi" else \
        (E.pair_counts_smu, E.weighted_pair_sums_smu)
    sc, sw = E.KnnStats(), E.KnnStats()
    want = counts(index, q, first, second, los=MID, observer=o, stats=sc)
    one = torch.ones(N, dtype=torch.int64, device=DEV)
    got = sums(index, q, first, second, one, query_weights=torch.ones(NQ, dtype=torch.int64, device=DEV), los=MID,
               observer=o, stats=sw)
    assert torch.equal(got, want) and int(want[-1, -1]) > N
    names = [k for k in sc.counters if k.startswith("radius_")]
    assert names and all(sc.counters[k] == sw.counters[k] for k in names)


# ---------------------------------------------------------------- 4. the CPU checks on the device
@pytest.mark.parametrize("obs", ("far", "on_point"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_swapping_the_two_sets_changes_no_bit(mode, obs):
    a, b = data("clustered"), queries("clustered")
    o = observer(obs, a)
    first, second = grid(mode, 5, 7)
    fn = E.pair_query_counts_rppi if mode == "rppi" else E.pair_query_counts_smu
    ab = fn(a.to(DEV), b.to(DEV), first, second, los=MID, observer=o)
    ba = fn(b.to(DEV), a.to(DEV), first, second, los=MID, observer=o)
    assert torch.equal(ab, ba) and int(ab[-1, -1]) > 0


def test_every_mu_gives_pair_counts():
    """Queries that are no data points, the observer far outside: no pair has d2 == 0 or a
    non-finite par2 (checked on the CPU first), so the column mu = inf is the isotropic pair count
    of the same index, bit for bit."""
    p = data("clustered")
    g = torch.Generator().manual_seed(54)
    q = torch.rand((NQ // 2, 3), generator=g)
    o = observer("far", p)
    tiny = 2.0 ** -149
    assert int(K.pair_counts_cpu(p, q, [tiny])[0]) == 0  # no d2 == 0
    every = K.pair_counts_2d_observer_cpu(p, q, [INF], [INF], "rppi", o)
    assert int(every[0, 0]) == p.shape[0] * q.shape[0]  # every par2 finite
    R = radii_of(9)
    index = index_of("clustered")
    got = E.pair_counts_smu(index, q.to(DEV), R, [0.5, INF], los=MID, observer=o)
    want = E.pair_counts(index, q.to(DEV), R)
    assert torch.equal(got[:, 1], want) and int(want[-1]) > 0 and int(got[-1, 0]) < int(got[-1, 1])


def test_a_pair_whose_midpoint_is_the_observer_counts_nowhere():
    """Coordinates on the grid of multiples of 2^-10: 2 o - p is exact, l == 0 for those pairs."""
    g = torch.Generator().manual_seed(55)
    pi_ = torch.randint(0, 1024, (3000, 3), generator=g)
    oi = torch.tensor([512, 300, 700])
    qi = torch.cat([2 * oi - pi_[:200], torch.randint(0, 1024, (200, 3), generator=g), pi_[1000:1100]])
    centred = int(((qi[:, None, :] + pi_[None, :, :]) == 2 * oi).all(-1).sum())
    assert centred >= 200
    p, q = (pi_.float() * 2.0 ** -10).contiguous(), (qi.float() * 2.0 ** -10).contiguous()
    o = tuple((oi.float() * 2.0 ** -10).tolist())
    index = E.build_index(p.to(DEV))
    got = check("rppi", index, p, q, [0.05, 0.3, INF], [0.05, INF], o)
    assert int(got[-1, -1]) == q.shape[0] * p.shape[0] - centred
    check("smu", index, p, q, [0.05, 0.3, INF], [0.5, 1.0, INF], o)


def test_non_finite_queries_and_the_self_form():
    p = data("uniform")
    o = observer("far", p)
    q = queries("uniform").clone()
    q[3, 0] = float("nan")
    q[70, 2] = INF
    q[200, 1] = -INF
    bad = q[[3, 70, 200]]
    for mode in ("rppi", "smu"):
        first, second = grid(mode, 5, 7)
        check(mode, index_of("uniform"), p, q, first, second, o)
        assert int(check(mode, index_of("uniform"), p, bad, first, second, o).abs().sum()) == 0
    first, second = grid("rppi", 3, 3)
    got = E.pair_self_counts_rppi(p.to(DEV), first, second, los=MID, observer=o).cpu()
    same_cells(got, K.pair_counts_2d_observer_cpu(p, p, *cut2s(first, second), "rppi", o))
    assert int(got[0, 0]) >= N  # every point with itself
    first, second = grid("smu", 3, 7)
    got = E.pair_self_counts_smu(p.to(DEV), first, second, los=MID, observer=o).cpu()
    same_cells(got, K.pair_counts_2d_observer_cpu(p, p, *cut2s(first, second), "smu", o))


# ---------------------------------------------------------------- 5. scales and offsets
@pytest.mark.parametrize("t", (("scale", 40), ("scale", -60), ("scale", -70), ("offset", "p1000"), ("offset", "quant")),
                         ids=SC.tid)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_scales_and_offsets(mode, t):
    """The observer moves with the data. 2^-60, 2^-70: d2 and par2 straddle, or lie in, the
    denormal range on both sides; a far offset leaves few bits to the differences while l is
    large. The division and the denormals must agree with the host's."""
    n, nq = 4000, 600
    p = SC.points("clustered", n, t)
    q = SC.foreign("clustered", nq, t, n)
    o = tuple(SC.apply(torch.tensor([[0.5, 0.5, -3.0], [0.25, 0.5, 0.75]]), t)[0 if mode == "rppi" else 1].tolist())
    first = [SC.radius(r, t) for r in radii_of(5, n)]
    second = [SC.radius(r, t) for r in radii_of(7, n)] if mode == "rppi" else list(MU)
    index = cached(("scaled", t), lambda: E.build_index(p.to(DEV)))
    got = check(mode, index, p, q, first, second, o)
    assert int(got[-1, -1]) > 0

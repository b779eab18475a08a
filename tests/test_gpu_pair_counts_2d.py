"""Anisotropic pair counts on the GPU (pair_counts_2d.hip): pair_counts_rppi / pair_counts_smu, the
whole [B1, B2] array bit for bit against the brute-force oracle K.pair_counts_2d_cpu, and against
pair_counts on the same GPU index where the two must agree. Data, indexes and queries are
computed once per module; everything is an integer, so there is no tolerance."""
import math

import pytest
import torch

from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of the walk
NQ = 1500
ISO = (1.0, 1.0, 1.0)
MU = (0.1, 0.3, 0.5, 0.5, 0.8, 1.0, INF)

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


def queries(name, nq=NQ):
    """Half of them data points, half random over the data's range, six of those moved to within
    0.001 of a face of the unit box each."""
    def make():
        p = data(name)
        g = torch.Generator().manual_seed(52)
        lo, hi = p.min(0).values, p.max(0).values
        rnd = lo + (hi - lo) * torch.rand((nq - nq // 2, 3), generator=g)
        for f in range(min(6, rnd.shape[0])):
            rnd[f, f % 3] = 0.001 if f < 3 else 0.999
        q = torch.cat([p[torch.randint(0, p.shape[0], (nq // 2,), generator=g)], rnd])
        return q[torch.randperm(nq, generator=g)].contiguous()
    return cached(("queries", name, nq), make)


def index_of(name, n=N):
    return cached(("index", name, n), lambda: E.build_index(data(name, n).to(DEV)))


def grid(mode, B1, B2, period):
    top = 0.5 if period else None
    if mode == "rppi":
        return radii_of(B1, top=top), radii_of(B2, top=top)
    mu = list(MU) if B2 == len(MU) else [(j + 1) / B2 for j in range(B2 - 1)] + [INF]
    return radii_of(B1, top=top), mu


def oracle(mode, p, q, first, second, los, period):
    a2 = [E.cut2_of(r) for r in first]
    b2 = [E.cut2_of(r) for r in second]
    return K.pair_counts_2d_cpu(p, q, a2, b2, mode, los, period)


def check(mode, index, p, q, first, second, los=2, period=None, stats=None):
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    got = fn(index, q.to(DEV), first, second, los=los, period=period, stats=stats)
    assert got.dtype == torch.int64 and got.shape == (len(first), len(second)) and got.device.type == "cuda"
    got = got.cpu()
    want = oracle(mode, p, q, first, second, los, period)
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} of {want.numel()} cells differ from the oracle, first "
                               f"{[(tuple(c), int(got[tuple(c)]), int(want[tuple(c)])) for c in bad[:4].tolist()]}")
    return got


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "clustered", "duplicates"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_equals_the_oracle(mode, name, period):
    E.reset_kernels_used()
    first, second = grid(mode, 5, 7, period)
    stats = E.KnnStats()
    got = check(mode, index_of(name), data(name), queries(name), first, second, period=period, stats=stats)
    assert "pair_counts_2d" in E.kernels_used()
    assert int(got[-1, -1]) > N and int(got[0, 0]) < int(got[-1, -1])
    assert stats.counters["radius_evals"] > 0 and stats.counters["radius_nodes"] > 0
    if period:
        assert stats.counters["radius_images"] > (NQ + 63) // 64  # queries near every face: more than one image
    if mode == "smu":
        assert stats.counters["radius_box_accepts"] == 0


@pytest.mark.parametrize("los", (0, 1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_every_line_of_sight(mode, los):
    first, second = grid(mode, 5, 7, ISO)
    if mode == "rppi":
        second = [0.01, 0.03, 0.07, 0.07, 0.2, 0.35, 0.5]  # a grid that is not symmetric in the axes
    p, q, index = data("clustered"), queries("clustered"), index_of("clustered")
    got = check(mode, index, p, q, first, second, los=los, period=ISO)
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    assert torch.equal(fn(index, q.to(DEV), first, second, los="xyz"[los], period=ISO).cpu(), got)


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("shape", ((1, 1), (40, 60), (60, 40), (2048, 1), (1, 2048)), ids=str)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_grid_sizes_and_slices(mode, shape, period):
    """1 x 1; 40 x 60 = 2400 cells > 2048: two slices of whole rows; 2048 x 1: one slice of 2048
    rows; 1 x 2048: one row that fills the slice."""
    first, second = grid(mode, *shape, period)
    check(mode, index_of("uniform"), data("uniform"), queries("uniform"), first, second, period=period)


def test_duplicated_and_extreme_edges():
    p, q, index = data("duplicates"), queries("duplicates"), index_of("duplicates")
    check("rppi", index, p, q, [0.0, 0.0, 0.05, 0.05, 0.3, INF], [0.0, 0.01, 0.01, 0.2, INF, INF])
    check("rppi", index, p, q, [0.0], [0.3])
    check("rppi", index, p, q, [0.3], [0.0])
    check("smu", index, p, q, [0.0, 0.05, 0.05, INF], [0.0, 0.0, 0.5, 1.0, 1.0, INF, INF])
    check("smu", index, p, q, [0.3], [0.0])


# ---------------------------------------------------------------- 2. whole-box acceptance
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
def test_coarse_grid_accepts_whole_boxes(period):
    stats = E.KnnStats()
    top = 0.5 if period else r_for(N / 4.0)
    check("rppi", index_of("uniform"), data("uniform"), queries("uniform"), [0.5 * top, top], [0.6 * top, top],
          period=period, stats=stats)
    assert stats.counters["radius_box_accepts"] > 0


@pytest.mark.parametrize("los", (1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_non_cubic_period_with_an_open_axis(mode, los):
    per = (1.0, INF, 0.8)  # bounds 0.5, none, 0.4
    first, second = grid(mode, 5, 7, None)
    first = [min(r, 0.4) for r in first]
    if mode == "rppi" and los == 2:
        second = [min(r, 0.4) for r in second]
    stats = E.KnnStats()
    check(mode, index_of("uniform"), data("uniform"), queries("uniform"), first, second, los=los, period=per,
          stats=stats)
    assert stats.counters["radius_images"] > (NQ + 63) // 64


# ---------------------------------------------------------------- 3. edge sizes
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("nq", (1, 64, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_query_counts_at_the_group_edge(mode, nq, period):
    first, second = grid(mode, 5, 7, period)
    check(mode, index_of("uniform"), data("uniform"), queries("uniform", nq), first, second, period=period)


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("n", (1, 64, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_point_counts_at_the_bucket_edge(mode, n, period):
    p = data("uniform", n)
    q = torch.cat([p, queries("uniform", 100)])
    first, second = grid(mode, 5, 7, period)
    if period is None:
        first[-1] = second[-1] = INF
    got = check(mode, index_of("uniform", n), p, q, first, second, period=period)
    if period is None:  # every pair; (s, mu): but those at distance 0
        same = int((q[:, None, :] == p[None, :, :]).all(-1).sum())
        assert same >= n and int(got[-1, -1]) == (n * (n + 100) if mode == "rppi" else n * (n + 100) - same)


def test_non_finite_queries_and_the_self_form():
    p = data("uniform")
    q = queries("uniform").clone()
    q[3, 0] = float("nan")
    q[70, 2] = INF
    q[200, 1] = -INF
    for mode in ("rppi", "smu"):
        first, second = grid(mode, 5, 7, ISO)
        check(mode, index_of("uniform"), p, q, first, second, period=ISO)
    first, second = grid("rppi", 3, 3, ISO)
    got = E.pair_self_counts_rppi(p.to(DEV), first, second, period=ISO).cpu()
    assert torch.equal(got, oracle("rppi", p, p, first, second, 2, ISO))
    assert int(got[0, 0]) >= N  # every point with itself
    first, second = grid("smu", 3, 7, None)
    got = E.pair_query_counts_smu(p.to(DEV), p.to(DEV), first, second, los="x").cpu()
    assert torch.equal(got, oracle("smu", p, p, first, second, 0, None))
    assert torch.equal(got, E.pair_self_counts_smu(p.to(DEV), first, second, los=0).cpu())


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_two_runs_give_the_same_bits(mode):
    first, second = grid(mode, 40, 60, ISO)
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    q = queries("clustered").to(DEV)
    a = fn(index_of("clustered"), q, first, second, period=ISO)
    b = fn(index_of("clustered"), q, first, second, period=ISO)
    assert torch.equal(a, b)
    D = E.shell_counts_2d(a)
    assert bool((D >= 0).all()) and int(D.sum()) == int(a[-1, -1])


# ---------------------------------------------------------------- 4. against pair_counts on the same index
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("los", (0, 1, 2))
def test_a_plane_across_the_line_of_sight_gives_pair_counts(los, period):
    """Points and queries whose line-of-sight coordinate is one constant have par2 = 0 and, the
    fma of a zero being exact, d2 == perp2 bit for bit: the first column of (rp, pi) is the
    isotropic pair count."""
    p = data("clustered").clone()
    q = queries("clustered").clone()
    p[:, los] = 0.25
    q[:, los] = 0.25
    index = E.build_index(p.to(DEV))
    R = radii_of(9, top=0.5 if period else None)
    got = E.pair_counts_rppi(index, q.to(DEV), R, [0.5 if period else 1.0], los=los, period=period)
    want = E.pair_counts(index, q.to(DEV), R, period=period)
    assert got.shape == (9, 1) and torch.equal(got[:, 0], want) and int(want[-1]) > 0


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "duplicates"))
def test_every_mu_gives_pair_counts_without_the_zero_distances(name, period):
    """par2 < inf * d2 holds for every pair with d2 > 0: column mu = inf is the isotropic pair count
    less the pairs at distance 0 (those below the smallest positive float32)."""
    index, q = index_of(name), queries(name).to(DEV)
    R = radii_of(9, top=0.5 if period else None)
    got = E.pair_counts_smu(index, q, R, [INF], los=1, period=period)
    zero = E.pair_counts(index, q, [2.0 ** -149], squared=True, period=period)[0]
    want = E.pair_counts(index, q, R, period=period) - zero
    assert int(zero) >= NQ // 2 and torch.equal(got[:, 0], want)

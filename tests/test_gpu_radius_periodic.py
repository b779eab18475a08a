"""Periodic radius search on the GPU (periodic.hip): counts and CSR lists of radius_counts /
radius_neighbors with `period=` bit for bit against the brute-force oracle of the minimum
image, K.radius_periodic_cpu. Data, indexes and oracle results are computed once per module."""
import math

import pytest
import torch

from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
OPEN = (INF, INF, INF)
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of kWalkStep = 6
NQ = 1500


def r_for(count, n=N, volume=1.0):
    """The radius whose ball holds `count` of n uniform points in `volume`."""
    return (3.0 * count * volume / (4.0 * math.pi * n)) ** (1.0 / 3.0)


R4, R30 = r_for(4), r_for(30)  # 0.043, 0.084

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def data(name):
    """A generator's points wrapped into the unit box; `far`: the uniform ones at 4096;
    `aniso`: [0, 1) x [0, 2) x [0, 1); `unwrapped`: [-0.5, 1.5)^3 as they are."""
    def make():
        if name == "far":
            return (data("uniform") + 4096.0).contiguous()
        if name == "aniso":
            return (uniform(N, seed=32) * torch.tensor([1.0, 2.0, 1.0])).contiguous()
        if name == "unwrapped":
            return (uniform(N, seed=33) * 2.0 - 0.5).contiguous()
        if name == "duplicates":  # 400 sites of 30 copies: enough sites for some to face each other across a face
            return GENERATORS[name](N, seed=31, ndistinct=400).contiguous()
        return E.wrap_points(GENERATORS[name](N, seed=31), 1.0).contiguous()
    return cached(("data", name), make)


def queries(name):
    """Queries over the data's own range: half of them data points, half random."""
    def make():
        p = data(name)
        g = torch.Generator().manual_seed(34)
        lo, hi = p.min(0).values, p.max(0).values
        q = torch.cat([p[torch.randint(0, p.shape[0], (NQ // 2,), generator=g)],
                       lo + (hi - lo) * torch.rand((NQ - NQ // 2, 3), generator=g)])
        return q[torch.randperm(NQ, generator=g)].contiguous()
    return cached(("queries", name), make)


def index_of(name):
    return cached(("index", name), lambda: E.build_index(data(name).to(DEV)))


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def oracle(name, r, period, qcut2=None, key=None):
    def make():
        cut2 = 0.0 if qcut2 is not None else E.cut2_of(r)
        o, i, d2 = K.radius_periodic_cpu(data(name), queries(name), cut2, period, qcut2)
        return o, i, final(d2)
    return cached(("oracle", name, r if key is None else key, period), make)


def counts_of(lists):
    return (lists[0][1:] - lists[0][:-1]).int()


def run(index, q, r, period, **kw):
    offsets, idx, dist = E.radius_neighbors(index, q.to(DEV) if isinstance(q, torch.Tensor) else q, r, period=period, **kw)
    assert E.LAST_RADIUS_ERRORS[0] == 0  # the device error word of the fill pass
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    return offsets.cpu(), idx.cpu(), dist.cpu()


def run_counts(index, q, r, period, **kw):
    c = E.radius_counts(index, q.to(DEV), r, period=period, **kw)
    assert c.dtype == torch.int32 and c.shape == (q.shape[0],)
    return c.cpu()


def same(got, ref):
    return all(torch.equal(g, w) for g, w in zip(got, ref)) and \
        torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32))


def report(got, ref):
    if not torch.equal(got[0], ref[0]):
        bad = (counts_of(got) != counts_of(ref)).nonzero().flatten()
        return f"{bad.numel()} of {ref[0].numel() - 1} rows differ in length, first {bad[:5].tolist()}"
    bad = ((got[1] != ref[1]) | (got[2] != ref[2])).nonzero().flatten()
    return f"{bad.numel()} of {ref[1].numel()} pairs differ"


def rows_as_sets(lists):
    """Every row ordered by id (ids are distinct within a row)."""
    o, i, d = lists
    rows = torch.repeat_interleave(torch.arange(o.numel() - 1), counts_of(lists).long())
    order = torch.argsort(rows * (1 << 31) + i.long())
    return o, i[order], d[order]


def check_all(name, r, period, ref=None):
    """Counts, sorted lists and unsorted lists of one case against the oracle."""
    ref = oracle(name, r, period) if ref is None else ref
    index, q = index_of(name), queries(name)
    c = run_counts(index, q, r, period)
    assert torch.equal(c, counts_of(ref)), f"{name} r={r}: {int((c != counts_of(ref)).sum())} counts differ"
    got = run(index, q, r, period)
    assert same(got, ref), f"{name} r={r}: {report(got, ref)}"
    got = rows_as_sets(run(index, q, r, period, sort=False))
    assert same(got, rows_as_sets(ref)), f"{name} r={r} unsorted: {report(got, rows_as_sets(ref))}"
    return ref


def open_total(name, r):
    return int(K.radius_count_cpu(data(name), queries(name), E.cut2_of(r)).sum())


# ---------------------------------------------------------------- 1. isotropic
@pytest.mark.parametrize("r", [R4, R30])
@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "planar"])
def test_isotropic_period(name, r):
    ref = check_all(name, r, 1.0)
    assert int(ref[0][-1]) > open_total(name, r)  # the case really wraps


# ---------------------------------------------------------------- 2. anisotropic and open axes
def test_anisotropic_period_with_an_open_axis():
    per = (1.0, 2.0, INF)
    r = r_for(30, volume=2.0)
    ref = check_all("aniso", r, per)
    assert int(ref[0][-1]) > open_total("aniso", r)
    # the open axis does not wrap: fewer pairs than with all three axes periodic
    assert int(ref[0][-1]) < int(K.radius_periodic_count_cpu(data("aniso"), queries("aniso"), E.cut2_of(r),
                                                             (1.0, 2.0, 1.0)).sum())


# ---------------------------------------------------------------- 3. far from the origin
def test_far_from_the_origin():
    """Coordinates near 4096, where one ulp is 2^-11 (about 1 % of the smaller radius): the box
    arithmetic on fl(q + s L) and the wrapped difference round differently, the case the
    conservative cull exists for."""
    for r in (R4, R30):
        ref = check_all("far", r, 1.0)
        assert int(ref[0][-1]) > open_total("far", r)


# ---------------------------------------------------------------- 4. unwrapped input
def test_unwrapped_input_is_taken_literally():
    """Uniform in [-0.5, 1.5)^3 with L = 1: a single wrap per axis, as the contract says, not
    the physical distance; the oracle is the same literal formula."""
    r = r_for(30, volume=8.0)
    ref = check_all("unwrapped", r, 1.0)
    assert int(ref[0][-1]) != open_total("unwrapped", r)


# ---------------------------------------------------------------- 5. per-query radii
def test_per_query_radii():
    g = torch.Generator().manual_seed(35)
    rad = (R30 / 8.0) * 16.0 ** torch.rand(NQ, generator=g)  # log-uniform in [r/8, 2r]
    assert float(rad.max()) <= 0.5
    qc = rad * rad
    ref = oracle("uniform", None, 1.0, qcut2=qc, key="var")
    index, q = index_of("uniform"), queries("uniform")
    assert int(ref[0][-1]) > int(K.radius_var_count_cpu(data("uniform"), q, qc, None).sum())
    assert torch.equal(run_counts(index, q, rad.to(DEV), 1.0), counts_of(ref))
    got = run(index, q, rad.to(DEV), 1.0)
    assert same(got, ref), report(got, ref)
    got = run(index, q, qc.to(DEV), 1.0, squared=True)
    assert same(got, ref), report(got, ref)
    # one lane reaches half the box, its 63 neighbours in the group a few points each
    rad2 = torch.full((NQ,), R4 / 2.0)
    rad2[777] = 0.5
    ref = oracle("uniform", None, 1.0, qcut2=rad2 * rad2, key="var_half")
    assert int(counts_of(ref)[777]) > N // 3
    assert torch.equal(run_counts(index, q, rad2.to(DEV), 1.0), counts_of(ref))
    got = run(index, q, rad2.to(DEV), 1.0)
    assert same(got, ref), report(got, ref)


# ---------------------------------------------------------------- 6. limits
def test_radius_of_half_the_box():
    """r = L / 2 on 4 097 points: every lane reaches half the box in every direction, so whole
    nodes are accepted under a wrap (and the stats say so)."""
    p = uniform(4097, seed=36)
    q = p[:640].contiguous()
    o, i, d2 = K.radius_periodic_cpu(p, q, E.cut2_of(0.5), 1.0)
    ref = (o, i, final(d2))
    index = E.build_index(p.to(DEV))
    stats = E.KnnStats()
    assert torch.equal(run_counts(index, q, 0.5, 1.0, stats=stats), counts_of(ref))
    print(stats.counters)
    assert stats.counters["radius_box_accepts"] > 0
    # 10 groups that span much of the box: at r = L / 2 an axis may wrap either way, up to 27 images
    assert 10 < stats.counters["radius_images"] <= 27 * 10
    got = run(index, q, 0.5, 1.0)
    assert same(got, ref), report(got, ref)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_edge_sizes(n):
    p = uniform(n, seed=40 + n)
    q = torch.cat([p[:200], uniform(100, seed=41)]).contiguous()
    index = E.build_index(p.to(DEV))
    for r in (0.5 * n ** (-1.0 / 3.0), 0.5):
        o, i, d2 = K.radius_periodic_cpu(p, q, E.cut2_of(r), 1.0)
        ref = (o, i, final(d2))
        assert torch.equal(run_counts(index, q, r, 1.0), counts_of(ref))
        got = run(index, q, r, 1.0)
        assert same(got, ref), f"n={n} r={r}: {report(got, ref)}"
        # nq = 1
        got = run(index, q[:1].contiguous(), r, 1.0)
        assert torch.equal(got[1], ref[1][:int(ref[0][1])]) and torch.equal(got[2], ref[2][:int(ref[0][1])])
    if n == 1:  # one point, L = 1, r = 0.5: itself
        assert run_counts(index, p, 0.5, 1.0).tolist() == [1]


def test_nan_queries_and_nan_points():
    p = data("uniform")
    index, q = index_of("uniform"), queries("uniform")[:300].clone()
    q[7, 2] = math.nan
    q[100] = math.nan
    q[201, 0] = -INF
    o, i, d2 = K.radius_periodic_cpu(p, q, E.cut2_of(R30), 1.0)
    ref = (o, i, final(d2))
    got = run(index, q, R30, 1.0)
    assert same(got, ref), report(got, ref)
    c = counts_of(got)
    assert c[7] == 0 and c[100] == 0 and c[201] == 0
    # NaN / infinite coordinates among the indexed points: in no row, every other pair unchanged
    p2 = p[:5000].clone()
    p2[1234] = math.nan
    p2[77, 1] = math.nan
    p2[4000, 0] = INF
    q2 = queries("uniform")[:300].contiguous()
    o, i, d2 = K.radius_periodic_cpu(p2, q2, E.cut2_of(R30), 1.0)
    ref = (o, i, final(d2))
    assert not any(row in ref[1].tolist() for row in (1234, 77, 4000))
    index2 = E.build_index(p2.to(DEV))
    assert torch.equal(run_counts(index2, q2, R30, 1.0), counts_of(ref))
    got = run(index2, q2, R30, 1.0)
    assert same(got, ref), report(got, ref)


# ---------------------------------------------------------------- 7. open period
@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_open_period_equals_the_open_box_kernels(name):
    index, q = index_of(name), queries(name).to(DEV)
    for r in (R4, R30, INF):
        assert torch.equal(E.radius_counts(index, q, r, period=OPEN), E.radius_counts(index, q, r))
        if r == INF:
            continue
        a, b = E.radius_neighbors(index, q, r, period=OPEN), E.radius_neighbors(index, q, r)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    g = torch.Generator().manual_seed(37)
    rad = ((R30 / 8.0) * 16.0 ** torch.rand(NQ, generator=g)).to(DEV)
    a, b = E.radius_neighbors(index, q, rad, period=OPEN), E.radius_neighbors(index, q, rad)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert "radius_periodic" in E.kernels_used()


# ---------------------------------------------------------------- 8. stats
def test_image_statistics():
    index, p = index_of("uniform"), data("uniform").to(DEV)
    groups = (N + 63) // 64
    s_open, s_per, s_ref = E.KnnStats(), E.KnnStats(), E.KnnStats()
    c_open = E.radius_counts(index, p, R4, stats=s_open, period=OPEN)
    E.radius_counts(index, p, R4, stats=s_per, period=1.0)
    assert torch.equal(c_open, E.radius_counts(index, p, R4, stats=s_ref))
    print(s_open.counters, s_per.counters)
    assert s_open.counters["radius_images"] == groups
    # the one image of an open period is the open-box walk itself
    for nm in ("radius_evals", "radius_nodes", "radius_buckets", "radius_box_accepts"):
        assert s_open.counters[nm] == s_ref.counters[nm]
    assert groups < s_per.counters["radius_images"] < 8 * groups

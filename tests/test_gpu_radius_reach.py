"""Two-sided radius search on the GPU (radius_reach.hip): reach_counts / reach_neighbors under
both rules, in the open box and under a period, bit for bit against the brute-force oracle
K.radius_reach_count_cpu / K.radius_reach_cpu, with the device error word checked after every
fill. Data, indexes and query sets are built once."""
import math

import pytest
import torch

import scale_cases as S
from datasets import GENERATORS, lattice, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 30_000
INF = math.inf
NAMES = sorted(GENERATORS) + ["lattice"]
RULES = ("either", "both")
ANISO = (1.0, 0.7, INF)

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def data(name, period=None):
    """A generator's points; with a period wrapped into it (the unit cube holds them otherwise)."""
    def make():
        p = lattice(32) if name == "lattice" else GENERATORS[name](N, seed=21)
        return p if period is None else E.wrap_points(p, period).contiguous()
    return cached(("data", name, period), make)


def index_of(name, period=None):
    return cached(("index", name, period), lambda: E.build_index(data(name, period).to(DEV), grid=True))


def rand_in(lo, hi, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand((n, 3), generator=g)).contiguous()


def queries(name, kind):
    """in_box: 2000 queries in the data's box; scaled3: 3000 in the box scaled 3x about its centre."""
    def make():
        p = data(name)
        lo, hi = p.min(0).values, p.max(0).values
        c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        return rand_in(lo, hi, 2000, 1) if kind == "in_box" else rand_in(c - 3 * half, c + 3 * half, 3000, 2)
    return cached(("queries", name, kind), make)


def band_queries(period):
    """1500 queries in the period's cell ([0, 1) on an open axis) and 700 whose every axis lies, one
    time in three each, within 0.02 of the lower face, of the upper face, or anywhere: the bands
    of all faces, edges and corners."""
    def make():
        g = torch.Generator().manual_seed(60)
        span = torch.tensor([v if math.isfinite(v) else 1.0 for v in K.check_period("test", period)])
        u = torch.rand((700, 3), generator=g)
        where = torch.randint(0, 3, (700, 3), generator=g)
        near = 0.02 * torch.rand((700, 3), generator=g)
        band = torch.where(where == 0, near, torch.where(where == 1, span - near, u * span))
        return torch.cat([torch.rand((1500, 3), generator=g) * span, band]).contiguous()
    return cached(("band", period), make)


def loguniform(m, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(m, generator=g)).float()


def reach_radii(m, lo, hi, seed, top=None):
    """Log-uniform in [lo, hi] with three entries at 0 and, with `top`, three at exactly `top`."""
    r = loguniform(m, lo, hi, seed)
    where = torch.randperm(m, generator=torch.Generator().manual_seed(seed + 1))
    r[where[:3]] = 0.0
    if top is not None:
        r[where[3:6]] = top
    return r.contiguous()


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def oracle(p, q, rq, rp, rule, period=None, squared=False):
    """The oracle's lists with final distances; radii as distances unless `squared`."""
    c = (lambda r: r) if squared else (lambda r: r * r)  # (the float32 product = cut2_of)
    offsets, idx, d2 = K.radius_reach_cpu(p, q, c(rq), c(rp), rule, period)
    return offsets, idx, final(d2)


def counts_of(lists):
    return (lists[0][1:] - lists[0][:-1]).int()


def dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def run(index, q, rq, rp, rule, period=None, **kw):
    per = {} if period is None else {"period": period}
    offsets, idx, dist = E.reach_neighbors(index, q.to(DEV), dev(rq), dev(rp), rule=rule, **per, **kw)
    assert E.LAST_RADIUS_ERRORS[0] == 0  # the device error word of the fill pass
    nq = q.shape[0]
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert offsets.shape == (nq + 1,) and idx.shape == dist.shape == (int(offsets[-1]),)
    return offsets.cpu(), idx.cpu(), dist.cpu()


def run_counts(index, q, rq, rp, rule, period=None, **kw):
    per = {} if period is None else {"period": period}
    c = E.reach_counts(index, q.to(DEV), dev(rq), dev(rp), rule=rule, **per, **kw)
    assert c.dtype == torch.int32 and c.shape == (q.shape[0],)
    return c.cpu()


def same(got, ref):
    return all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, ref)) \
        and torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32))


def report(got, ref):
    if not torch.equal(got[0], ref[0]):
        bad = (counts_of(got) != counts_of(ref)).nonzero().flatten()
        return f"{bad.numel()} of {ref[0].numel() - 1} rows differ in length, first {bad[:5].tolist()}"
    bad = ((got[1] != ref[1]) | (got[2] != ref[2])).nonzero().flatten()
    rows_bad = torch.unique(torch.searchsorted(ref[0], bad, right=True) - 1)
    return f"{bad.numel()} of {ref[1].numel()} pairs differ, in {rows_bad.numel()} rows, first {rows_bad[:5].tolist()}"


def by_id(lists):
    """Every row re-ordered by id (ids are distinct within a row): rows as sets."""
    offsets, idx, dist = lists
    row = torch.repeat_interleave(torch.arange(offsets.numel() - 1), counts_of(lists).long())
    order = torch.argsort(row * (1 << 31) + idx.long())
    return offsets, idx[order], dist[order]


def check(index, p, q, rq, rp, rule, period=None, what="", stats=None):
    """Counts and lists of the device against the oracle; (lists, oracle counts)."""
    ref = oracle(p, q, rq, rp, rule, period)
    c = run_counts(index, q, rq, rp, rule, period, stats=stats)
    assert torch.equal(c, counts_of(ref)), f"{what}/{rule}: {int((c != counts_of(ref)).sum())} counts differ"
    got = run(index, q, rq, rp, rule, period)
    assert same(got, ref), f"{what}/{rule}: {report(got, ref)}"
    return got, c


def conditions(p, q, rq, rp, rule, period, c):
    """What makes a case say something, from the oracle: a pair that only the wrap selects; rows
    that neither one-sided search gives (c: the oracle's counts of the case)."""
    qc, pc = rq * rq, rp * rp
    if period is not None:
        assert int(c.sum()) > int(K.radius_reach_count_cpu(p, q, qc, pc, rule).sum())
    gather = K.radius_reach_count_cpu(p, q, qc, torch.zeros_like(pc), "either", period)
    scatter = K.radius_reach_count_cpu(p, q, torch.zeros_like(qc), pc, "either", period)
    if rule == "either":
        assert bool((c != gather).any()) and bool((c != scatter).any())
    else:
        assert bool((c > 0).any()) and bool(((c < gather) & (c < scatter)).any())


@pytest.mark.parametrize("nq", [1, 63, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_shapes(n, nq):
    p = uniform(n, seed=40 + n)
    q = (uniform(nq, seed=50 + nq) * 1.4 - 0.2).contiguous()
    g = torch.Generator().manual_seed(n * 100 + nq)
    index = E.build_index(p.to(DEV), grid=True)
    rq, rp = 0.5 * torch.rand(nq, generator=g), 0.5 * torch.rand(n, generator=g)
    for period in (None, 1.0):
        for rule in RULES:
            check(index, p, q, rq, rp, rule, period, what=f"n={n} nq={nq} period={period}")


@pytest.mark.parametrize("kind", ["in_box", "scaled3"])
@pytest.mark.parametrize("name", NAMES)
def test_every_data_set(name, kind):
    p, index, q = data(name), index_of(name), queries(name, kind)
    rq, rp = reach_radii(q.shape[0], 1e-4, 0.05, 91), reach_radii(p.shape[0], 1e-4, 0.05, 93)
    for rule in RULES:
        check(index, p, q, rq, rp, rule, what=f"{name}/{kind}")


@pytest.mark.parametrize("period", [1.0, ANISO], ids=["L1", "L1x0.7xinf"])
@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_periodic(name, period):
    p, index, q = data(name, period), index_of(name, period), band_queries(period)
    top = E.period_radius_bound(K.check_period("test", period), False)
    rq, rp = reach_radii(q.shape[0], 0.002, 0.2, 61, top=top), reach_radii(p.shape[0], 0.002, 0.2, 63, top=top)
    for rule in RULES:
        stats = E.KnnStats()
        _, c = check(index, p, q, rq, rp, rule, period, what=name, stats=stats)
        conditions(p, q, rq, rp, rule, period, c)
        groups = (q.shape[0] + 63) // 64
        assert stats.counters["radius_images"] > groups
        assert set(stats.counters) == {"radius_evals", "radius_nodes", "radius_buckets", "radius_box_accepts",
                                       "radius_images"}
    # the open run of the same inputs says something too
    for rule in RULES:
        conditions(p, q, rq, rp, rule, None, check(index, p, q, rq, rp, rule, what=f"{name}/open")[1])


@pytest.mark.parametrize("period", [None, 1.0], ids=["open", "L1"])
def test_one_dominant_point(period):
    """Tiny radii everywhere but one point, next to the x = 0 face, at the bound: the node
    annotation alone keeps it reachable from far groups and, under the period, across the face."""
    p, index, q = data("uniform", 1.0), index_of("uniform", 1.0), queries("uniform", "in_box")
    big = int(p[:, 0].argmin())
    rp = torch.full((p.shape[0],), 1e-4)
    rp[big] = 0.5
    rq = torch.full((q.shape[0],), 1e-4)
    got, c = check(index, p, q, rq, rp, "either", period, what="dominant")
    reached = int((got[1] == big).sum())
    across = int((q[:, 0] - p[big, 0] > 0.5).sum())  # queries nearer to its image below x = 0
    assert across > 100
    if period is None:
        assert reached > 50
    else:
        open_rows = int((oracle(p, q, rq, rp, "either")[1] == big).sum())
        assert reached > open_rows + 50
    # under `both` the one wide ball changes nothing: the tiny query radii decide
    _, cb = check(index, p, q, rq, rp, "both", period, what="dominant")
    assert torch.equal(cb, K.radius_reach_count_cpu(p, q, rq * rq, torch.full_like(rp, 1e-4) ** 2, "both", period))


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_whole_box_acceptance(name):
    p, index, q = data(name, 1.0), index_of(name, 1.0), queries(name, "in_box")
    rp = reach_radii(p.shape[0], 1e-4, 0.05, 95)
    for period, wide in ((None, 2.0), (1.0, 0.45)):
        rq = torch.where(torch.arange(q.shape[0]) % 2 == 0, torch.tensor(wide), torch.tensor(0.0))
        stats = E.KnnStats()
        c = run_counts(index, q, rq, rp, "either", period, stats=stats)
        assert torch.equal(c, K.radius_reach_count_cpu(p, q, rq * rq, rp * rp, "either", period))
        assert stats.counters["radius_box_accepts"] > 0 and stats.counters["radius_nodes"] > 0
        if period is None:  # the wide lanes take the root whole
            assert bool((c[rq > 0] == p.shape[0]).all())
            assert set(stats.counters) == {"radius_evals", "radius_nodes", "radius_buckets", "radius_box_accepts"}
        stats = E.KnnStats()
        c = run_counts(index, q, rq, rp, "both", period, stats=stats)
        assert torch.equal(c, K.radius_reach_count_cpu(p, q, rq * rq, rp * rp, "both", period))
        assert stats.counters["radius_box_accepts"] == 0 and stats.counters["radius_nodes"] > 0
        assert bool((c[rq == 0] == 0).all()) and int(c.sum()) > 0


@pytest.mark.parametrize("period", [None, 1.0], ids=["open", "L1"])
def test_paths(period):
    p, index, q = data("clustered", 1.0), index_of("clustered", 1.0), queries("clustered", "in_box")
    rq, rp = reach_radii(q.shape[0], 1e-3, 0.1, 71), reach_radii(p.shape[0], 1e-3, 0.1, 73)
    kept = [t.clone() for t in (index.nodes, index.pts, index.perm)]
    for rule in RULES:
        ref, c = check(index, p, q, rq, rp, rule, period, what="paths")
        assert torch.equal(c, counts_of(ref)) and int(c.sum()) > 0
        # unsorted rows are the same sets; two runs are bit-identical
        assert same(by_id(run(index, q, rq, rp, rule, period, sort=False)), by_id(ref))
        assert same(run(index, q, rq, rp, rule, period), ref)
        assert torch.equal(run_counts(index, q, rq, rp, rule, period), c)
        # prepared radii and chunked queries; squared cutoffs
        prep = E.prepare_point_radii(index, rp.to(DEV))
        assert prep.nodes.data_ptr() != index.nodes.data_ptr()
        assert same(run(index, q, rq, prep, rule, period), ref)
        parts = [run(index, q[b:b + 700].contiguous(), rq[b:b + 700].contiguous(), prep, rule, period)
                 for b in range(0, q.shape[0], 700)]
        assert torch.equal(torch.cat([x[1] for x in parts]), ref[1])
        assert torch.equal(torch.cat([x[2] for x in parts]).view(torch.int32), ref[2].view(torch.int32))
        assert same(run(index, q, rq * rq, rp * rp, rule, period, squared=True), ref)
        per = {} if period is None else {"period": period}
        assert same(tuple(t.cpu() for t in E.reach_query_neighbors(p.to(DEV), q.to(DEV), rq.to(DEV), rp.to(DEV),
                                                                   rule=rule, **per)), ref)
    # the index's own arrays are untouched
    for t, k in zip((index.nodes, index.pts, index.perm), kept):
        assert t.dtype == k.dtype and torch.equal(t.view(torch.int32), k.view(torch.int32))
    assert "radius_reach" in E.kernels_used()


def test_open_period_and_self_neighbours():
    p, index = data("uniform", 1.0), index_of("uniform", 1.0)
    q = queries("uniform", "in_box")
    rq, rp = reach_radii(q.shape[0], 1e-3, 0.1, 75), reach_radii(p.shape[0], 1e-3, 0.1, 77)
    for rule in RULES:
        assert same(run(index, q, rq, rp, rule, (INF,) * 3), run(index, q, rq, rp, rule))
    sub = p[:6000].contiguous()
    h = reach_radii(6000, 1e-3, 0.2, 79)
    for period in (None, 1.0):
        per = {} if period is None else {"period": period}
        got = tuple(t.cpu() for t in E.reach_self_neighbors(sub.to(DEV), h.to(DEV), **per))
        assert same(got, oracle(sub, sub, h, h, "either", period))


def test_far_offset_and_odd_period():
    pname, n = "L205x75xinf", 8000
    period = S.PERIODS[pname]
    p = S.periodic_points("uniform", n, pname, "p1000")
    q = torch.cat([p[::10], S.periodic_points("uniform", 500, pname, "p1000", seed=3)]).contiguous()
    index = E.build_index(p.to(DEV), grid=True)
    top = S.period_radius(pname, 0.5)
    rq, rp = reach_radii(q.shape[0], top / 100, top / 3, 81, top=top), reach_radii(n, top / 100, top / 3, 83, top=top)
    for rule in RULES:
        _, c = check(index, p, q, rq, rp, rule, period, what=pname)
        conditions(p, q, rq, rp, rule, period, c)


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_identities_on_the_device(name):
    p, index, q = data(name, 1.0), index_of(name, 1.0), queries(name, "in_box")
    rq, rp = reach_radii(q.shape[0], 1e-3, 0.1, 85), reach_radii(p.shape[0], 1e-3, 0.1, 87)
    qd = q.to(DEV)
    # query_radii = 0.0 under `either`: the scatter search
    want = tuple(t.cpu() for t in E.point_radius_neighbors(index, qd, rp.to(DEV)))
    assert int(want[0][-1]) > 0 and same(run(index, q, 0.0, rp, "either"), want)
    assert torch.equal(run_counts(index, q, 0.0, rp, "either"), counts_of(want))
    # zero point radii: the gather search, open and periodic
    zero = torch.zeros(p.shape[0])
    for period in (None, 1.0):
        per = {} if period is None else {"period": period}
        want = tuple(t.cpu() for t in E.radius_neighbors(index, qd, rq.to(DEV), **per))
        assert int(want[0][-1]) > 0 and same(run(index, q, rq, zero, "either", period), want)
        assert bool((counts_of(run(index, q, rq, zero, "both", period)) == 0).all())


def test_nan_queries_inf_radii_and_empty_inputs():
    p, index = data("uniform"), index_of("uniform")
    q = queries("uniform", "in_box")[:300].clone()
    q[7, 2] = math.nan
    q[100] = math.nan
    q[201, 0] = -INF
    rq, rp = reach_radii(300, 1e-3, 0.1, 89), reach_radii(p.shape[0], 1e-3, 0.05, 97)
    rq[7] = rq[150] = INF
    rp[int(torch.randint(0, p.shape[0], (1,), generator=torch.Generator().manual_seed(98)))] = INF
    for rule in RULES:
        got, c = check(index, p, q, rq, rp, rule, what="nan")
        assert c[7] == 0 and c[100] == 0 and c[201] == 0 and c[150] >= 1
    assert c[150] < p.shape[0] == run_counts(index, q, rq, rp, "either")[150]
    fin_q, fin_p = rq.clamp(max=0.5), rp.clamp(max=0.5)
    for rule in RULES:
        _, c = check(index, p, q, fin_q, fin_p, rule, 1.0, what="nan/L1")
        assert c[7] == 0 and c[100] == 0 and c[201] == 0
    empty = E.build_index(torch.empty((0, 3), device=DEV), grid=True)
    none, no_r = torch.empty((0, 3)), torch.empty(0)
    for rule in RULES:
        assert torch.equal(run_counts(empty, q, rq, no_r, rule), torch.zeros(300, dtype=torch.int32))
        o, i, d = run(empty, q, rq, no_r, rule)
        assert torch.equal(o, torch.zeros(301, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0
        assert run_counts(index, none, no_r, rp, rule).shape == (0,)
        o, i, d = run(index, none, no_r, rp, rule)
        assert torch.equal(o, torch.zeros(1, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0


def test_errors():
    p, index = data("uniform"), index_of("uniform")
    qd = queries("uniform", "in_box").to(DEV)
    nq, n = qd.shape[0], p.shape[0]
    rq, rp = torch.full((nq,), 0.05, device=DEV), torch.full((n,), 0.05, device=DEV)
    over = S.float_above(0.5)
    big_q, big_p, neg = rq.clone(), rp.clone(), rp.clone()
    big_q[11] = big_p[11] = over
    neg[11] = -0.5
    for fn in (E.reach_counts, E.reach_neighbors):
        for a, b in ((rq.cpu(), rp), (rq, rp.cpu()), (rq.double(), rp), (rq, rp[:-1]), (rq, neg), (math.nan, rp)):
            with pytest.raises(ValueError):
                fn(index, qd, a, b)
        with pytest.raises(ValueError, match="rule"):
            fn(index, qd, rq, rp, rule="any")
        for a, b in ((big_q, rp), (rq, big_p), (over, rp), (rq, E.prepare_point_radii(index, big_p))):
            with pytest.raises(ValueError, match="period"):
                fn(index, qd, a, b, period=1.0)
        with pytest.raises(ValueError):
            fn(index, qd, rq, rp, period=(1.0, 0.0, 1.0))
        with pytest.raises(ValueError, match="another index"):
            fn(index_of("clustered"), qd, rq, E.prepare_point_radii(index, rp))
    total = int(E.reach_counts(index, qd, rq, rp).sum())
    with pytest.raises(ValueError, match=str(total)):
        E.reach_neighbors(index, qd, rq, rp, max_pairs=total - 1)
    assert E.reach_neighbors(index, qd, rq, rp, max_pairs=total)[1].numel() == total
    # an index built in a rotated frame serves its own points only
    tp = data("tilted_plane")
    rotated = E.build_index(tp.to(DEV), frame=torch.eye(3, device=DEV))
    assert rotated.qrot is not None
    for fn in (E.reach_counts, E.reach_neighbors):
        with pytest.raises(ValueError):
            fn(rotated, qd, rq, torch.full((tp.shape[0],), 0.05, device=DEV))
    # point_radius_* keeps its refusal of a period
    with pytest.raises(ValueError, match="not supported"):
        E.point_radius_neighbors(index, qd, rp, period=1.0)

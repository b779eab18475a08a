"""Variable-radius search on the GPU (radius_var.hip): per-query radii (gather) and per-point
radii (scatter) of radius_counts / radius_neighbors / point_radius_counts /
point_radius_neighbors bit for bit against the brute-force oracle K.radius_var_cpu, with the
device error word checked after every fill. Data, indexes and query sets are built once."""
import math

import numpy as np
import pytest
import torch

from datasets import GENERATORS, lattice, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 30_000
INF = math.inf
NAMES = sorted(GENERATORS) + ["lattice"]

_DATA: dict = {}
_INDEX: dict = {}
_QUERIES: dict = {}


def data(name, n=N):
    if (name, n) not in _DATA:
        if name == "lattice":
            _DATA[(name, n)] = lattice(32 if n == N else 21)  # 32768 / 9261 points
        else:
            _DATA[(name, n)] = GENERATORS[name](n, seed=21)
    return _DATA[(name, n)]


def index_of(name, n=N):
    if (name, n) not in _INDEX:
        _INDEX[(name, n)] = E.build_index(data(name, n).to(DEV), grid=True)
    return _INDEX[(name, n)]


def rand_in(lo, hi, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand((n, 3), generator=g)).contiguous()


def queries(name, kind, n=N):
    """in_box: 2000 queries in the data's box; scaled3: 3000 in the box scaled 3x about its centre."""
    if (name, kind, n) not in _QUERIES:
        p = data(name, n)
        lo, hi = p.min(0).values, p.max(0).values
        c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        q = rand_in(lo, hi, 2000, 1) if kind == "in_box" else rand_in(c - 3 * half, c + 3 * half, 3000, 2)
        _QUERIES[(name, kind, n)] = q
    return _QUERIES[(name, kind, n)]


def loguniform(m, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(m, generator=g)).float()


def gather_radii(profile, m):
    g = torch.Generator().manual_seed(90)
    if profile == "loguniform":
        return loguniform(m, 1e-4, 0.05, 91)
    if profile == "mixed":  # dead lanes, small and wide radii within one group
        u = torch.rand(m, generator=g)
        return torch.where(u < 0.70, torch.tensor(0.0), torch.where(u < 0.95, torch.tensor(0.02), torch.tensor(0.2)))
    if profile == "three_inf":
        r = torch.full((m,), 0.01)
        r[torch.randperm(m, generator=g)[:3]] = INF
        return r
    raise KeyError(profile)


def scatter_radii(profile, n):
    g = torch.Generator().manual_seed(92)
    if profile == "loguniform":
        return loguniform(n, 1e-4, 0.05, 93)
    if profile == "fifty":
        r = torch.zeros(n)
        r[torch.randperm(n, generator=g)[:50]] = 0.3
        return r
    if profile == "one_inf":
        r = torch.full((n,), 0.01)
        r[int(torch.randint(0, n, (1,), generator=g))] = INF
        return r
    raise KeyError(profile)


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def oracle(p, q, qr=None, pr=None, squared=False):
    """The oracle's lists with final distances; radii as distances unless `squared`."""
    c = lambda r: None if r is None else (r if squared else r * r)  # noqa: E731  (float32 product = cut2_of)
    offsets, idx, d2 = K.radius_var_cpu(p, q, qcut2=c(qr), pcut2=c(pr))
    return offsets, idx, final(d2)


def counts_of(lists):
    return (lists[0][1:] - lists[0][:-1]).int()


def check_lists(res, nq):
    offsets, idx, dist = res
    assert E.LAST_RADIUS_ERRORS[0] == 0  # the device error word of the fill pass
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert offsets.shape == (nq + 1,) and idx.shape == dist.shape == (int(offsets[-1]),)
    return offsets.cpu(), idx.cpu(), dist.cpu()


def run_gather(index, q, r, **kw):
    return check_lists(E.radius_neighbors(index, q.to(DEV), r.to(DEV), **kw), q.shape[0])


def run_scatter(index, q, r, **kw):
    return check_lists(E.point_radius_neighbors(index, q.to(DEV), r.to(DEV) if torch.is_tensor(r) else r, **kw),
                       q.shape[0])


def counts_gather(index, q, r, **kw):
    c = E.radius_counts(index, q.to(DEV), r.to(DEV), **kw)
    assert c.dtype == torch.int32 and c.shape == (q.shape[0],)
    return c.cpu()


def counts_scatter(index, q, r, **kw):
    c = E.point_radius_counts(index, q.to(DEV), r.to(DEV) if torch.is_tensor(r) else r, **kw)
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


@pytest.mark.parametrize("nq", [1, 63, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_shapes(n, nq):
    p = uniform(n, seed=40 + n)
    q = (uniform(nq, seed=50 + nq) * 1.4 - 0.2).contiguous()
    extent = float((p.max(0).values - p.min(0).values).max()) if n > 1 else 1.0
    g = torch.Generator().manual_seed(n * 100 + nq)
    index = E.build_index(p.to(DEV), grid=True)
    rq, rp = extent * torch.rand(nq, generator=g), extent * torch.rand(n, generator=g)
    ref = oracle(p, q, qr=rq)
    assert torch.equal(counts_gather(index, q, rq), counts_of(ref)), f"gather n={n} nq={nq}"
    got = run_gather(index, q, rq)
    assert same(got, ref), f"gather n={n} nq={nq}: {report(got, ref)}"
    ref = oracle(p, q, pr=rp)
    assert torch.equal(counts_scatter(index, q, rp), counts_of(ref)), f"scatter n={n} nq={nq}"
    got = run_scatter(index, q, rp)
    assert same(got, ref), f"scatter n={n} nq={nq}: {report(got, ref)}"


@pytest.mark.parametrize("kind", ["in_box", "scaled3"])
@pytest.mark.parametrize("name", NAMES)
def test_every_data_set_gather(name, kind):
    p, index, q = data(name), index_of(name), queries(name, kind)
    for profile in ("loguniform", "mixed", "three_inf"):
        r = gather_radii(profile, q.shape[0])
        ref = oracle(p, q, qr=r)
        c = counts_gather(index, q, r)
        assert torch.equal(c, counts_of(ref)), f"{name}/{kind}/{profile}: {int((c != counts_of(ref)).sum())} counts differ"
        got = run_gather(index, q, r)
        assert same(got, ref), f"{name}/{kind}/{profile}: {report(got, ref)}"
        if profile == "three_inf":  # rows beyond the LDS sort beside short ones
            assert int((c == p.shape[0]).sum()) == 3 and p.shape[0] > K.RADIUS_LDS_ROW
        if profile == "mixed":
            assert bool((c[r == 0] == 0).all())


@pytest.mark.parametrize("kind", ["in_box", "scaled3"])
@pytest.mark.parametrize("name", NAMES)
def test_every_data_set_scatter(name, kind):
    p, index, q = data(name), index_of(name), queries(name, kind)
    for profile in ("loguniform", "fifty", "one_inf"):
        r = scatter_radii(profile, p.shape[0])
        ref = oracle(p, q, pr=r)
        c = counts_scatter(index, q, r)
        assert torch.equal(c, counts_of(ref)), f"{name}/{kind}/{profile}: {int((c != counts_of(ref)).sum())} counts differ"
        got = run_scatter(index, q, r)
        assert same(got, ref), f"{name}/{kind}/{profile}: {report(got, ref)}"
        if profile == "one_inf":
            assert bool((c >= 1).all())


@pytest.mark.parametrize("kind", ["in_box", "scaled3"])
@pytest.mark.parametrize("name", NAMES)
def test_every_data_set_kth_distance_radii(name, kind):
    """Per-point squared radii = the points' own 16-th d² from the oracle, at about 10 000
    points: the reverse-neighbour search."""
    n = 10_000
    p, index, q = data(name, n), index_of(name, n), queries(name, kind, n)
    kth = K.knn_cpu(p, p, 16, INF)[1][:, 15].contiguous()
    ref = oracle(p, q, pr=kth, squared=True)
    c = counts_scatter(index, q, kth, squared=True)
    assert torch.equal(c, counts_of(ref)), f"{name}/{kind}: {int((c != counts_of(ref)).sum())} counts differ"
    got = run_scatter(index, q, kth, squared=True)
    assert same(got, ref), f"{name}/{kind}: {report(got, ref)}"


@pytest.mark.parametrize("name", ["uniform", "clustered", "mixed_scale"])
def test_whole_box_acceptance_per_lane(name):
    """Half the queries at twice the data's extent, the others at 0: the wide lanes take the
    root box whole, the dead ones nothing, and no distance is evaluated."""
    p, index, q = data(name), index_of(name), queries(name, "in_box")
    extent = float((p.max(0).values - p.min(0).values).max())
    r = torch.where(torch.arange(q.shape[0]) % 2 == 0, torch.tensor(2.0 * extent), torch.tensor(0.0))
    stats = E.KnnStats()
    c = counts_gather(index, q, r, stats=stats)
    assert torch.equal(c, torch.where(r > 0, p.shape[0], 0).int())
    assert torch.equal(c, K.radius_var_count_cpu(p, q, qcut2=r * r))
    assert stats.counters["radius_evals"] == 0 and stats.counters["radius_box_accepts"] > 0
    assert stats.counters["radius_nodes"] > 0
    # scatter reports the same counters and never accepts a box
    stats = E.KnnStats()
    counts_scatter(index, q, scatter_radii("fifty", p.shape[0]), stats=stats)
    assert stats.counters["radius_box_accepts"] == 0 and stats.counters["radius_nodes"] > 0
    assert set(stats.counters) == {"radius_evals", "radius_nodes", "radius_buckets", "radius_box_accepts"}


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_duality_on_the_device(name):
    """point_radius_neighbors(P-index, Q, rp) holds the pairs of radius_neighbors(Q-index, P,
    rp) transposed (dist2 is exactly symmetric); compared as sets, row by row."""
    p, q = data(name), queries(name, "in_box")
    rp = scatter_radii("loguniform", p.shape[0]) * 2.0
    got = by_id(run_scatter(index_of(name), q, rp))
    qindex = E.build_index(q.to(DEV), grid=True)
    o, i, d = run_gather(qindex, p, rp)
    row = torch.repeat_interleave(torch.arange(p.shape[0]), counts_of((o, i, d)).long())
    order = torch.argsort(i.long() * (1 << 31) + row)
    offsets = torch.zeros(q.shape[0] + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(i.long(), minlength=q.shape[0]), 0)
    want = (offsets, row[order].int(), d[order])
    assert int(offsets[-1]) > q.shape[0]
    assert same(got, want), report(got, want)


def test_tensor_against_scalar():
    p, index, q = data("uniform"), index_of("uniform"), queries("uniform", "scaled3")
    qd = q.to(DEV)
    for r in (0.0, 0.02, 0.05, INF):
        sq = q[:200].contiguous() if math.isinf(r) else q
        sqd = sq.to(DEV)
        sc = E.radius_counts(index, sqd, r).cpu()
        sl = check_lists(E.radius_neighbors(index, sqd, r), sq.shape[0])
        rq, rp = torch.full((sq.shape[0],), r), torch.full((p.shape[0],), r)
        assert torch.equal(counts_gather(index, sq, rq), sc) and same(run_gather(index, sq, rq), sl)
        assert torch.equal(counts_scatter(index, sq, rp), sc) and same(run_scatter(index, sq, rp), sl)
        c2 = torch.full((sq.shape[0],), E.cut2_of(r))
        assert same(run_gather(index, sq, c2, squared=True), sl)
        assert same(check_lists(E.radius_neighbors(index, sqd, E.cut2_of(r), squared=True), sq.shape[0]), sl)
    # the convenience forms
    r = gather_radii("loguniform", q.shape[0])
    ref = run_gather(index, q, r)
    assert same(check_lists(E.radius_query_neighbors(p.to(DEV), qd, r.to(DEV)), q.shape[0]), ref)
    assert torch.equal(E.radius_query_counts(p.to(DEV), qd, r.to(DEV)).cpu(), counts_of(ref))
    rp = scatter_radii("loguniform", p.shape[0])
    ref = run_scatter(index, q, rp)
    assert same(check_lists(E.point_radius_query_neighbors(p.to(DEV), qd, rp.to(DEV)), q.shape[0]), ref)
    assert torch.equal(E.point_radius_query_counts(p.to(DEV), qd, rp.to(DEV)).cpu(), counts_of(ref))
    sub = p[:5000].contiguous().to(DEV)
    assert same(check_lists(E.point_radius_self_neighbors(sub, rp[:5000].to(DEV)), 5000),
                check_lists(E.point_radius_query_neighbors(sub, sub, rp[:5000].to(DEV)), 5000))
    assert "radius_var" in E.kernels_used()


def test_prepared_point_radii_and_chunks():
    p, index, q = data("clustered"), index_of("clustered"), queries("clustered", "in_box")
    rp = scatter_radii("loguniform", p.shape[0])
    ref = run_scatter(index, q, rp)
    prep = E.prepare_point_radii(index, rp.to(DEV))
    assert same(run_scatter(index, q, prep), ref)
    assert torch.equal(counts_scatter(index, q, prep), counts_of(ref))
    parts = [run_scatter(index, q[b:b + 700].contiguous(), prep) for b in range(0, q.shape[0], 700)]
    assert torch.equal(torch.cat([x[1] for x in parts]), ref[1]) and torch.equal(torch.cat([x[2] for x in parts]), ref[2])
    with pytest.raises(ValueError):  # prepared for another index
        E.point_radius_counts(index_of("uniform"), q.to(DEV), prep)


def test_unsorted_rows_are_the_same_sets():
    p, index, q = data("clustered"), index_of("clustered"), queries("clustered", "in_box")
    rq, rp = gather_radii("mixed", q.shape[0]), scatter_radii("loguniform", p.shape[0])
    for got, ref in ((run_gather(index, q, rq, sort=False), oracle(p, q, qr=rq)),
                     (run_scatter(index, q, rp, sort=False), oracle(p, q, pr=rp))):
        assert int(ref[0][-1]) > 0 and same(by_id(got), by_id(ref))


def test_repeat_runs_are_bit_identical():
    p, index, q = data("duplicates"), index_of("duplicates"), queries("duplicates", "in_box")
    rq, rp = gather_radii("mixed", q.shape[0]), scatter_radii("loguniform", p.shape[0])
    assert same(run_gather(index, q, rq), run_gather(index, q, rq))
    assert same(run_scatter(index, q, rp), run_scatter(index, q, rp))
    assert torch.equal(counts_gather(index, q, rq), counts_gather(index, q, rq))
    assert torch.equal(counts_scatter(index, q, rp), counts_scatter(index, q, rp))


def test_the_index_is_untouched():
    p, q = data("uniform"), queries("uniform", "in_box")
    index = E.build_index(p.to(DEV), grid=True)
    qd = q.to(DEV)
    cfg = E.KnnConfig(k=16)
    before = E.query_points(index, qd, cfg).clone()
    kept = [t.clone() for t in (index.nodes, index.pts, index.perm)]
    rp = scatter_radii("fifty", p.shape[0])
    run_scatter(index, q, rp)
    counts_scatter(index, q, scatter_radii("one_inf", p.shape[0]))
    prep = E.prepare_point_radii(index, rp.to(DEV))
    assert prep.nodes.data_ptr() != index.nodes.data_ptr()
    for t, k in zip((index.nodes, index.pts, index.perm), kept):
        assert t.dtype == k.dtype and torch.equal(t.view(torch.int32), k.view(torch.int32))
    assert torch.equal(E.query_points(index, qd, cfg).view(torch.int32), before.view(torch.int32))


def test_nan_queries_and_empty_inputs():
    p, index = data("uniform"), index_of("uniform")
    q = queries("uniform", "in_box")[:300].clone()
    q[7, 2] = math.nan
    q[100] = math.nan
    q[201, 0] = -INF
    rq, rp = torch.full((300,), 0.08), scatter_radii("one_inf", p.shape[0])
    rq[7] = rq[150] = INF
    for got, ref in ((run_gather(index, q, rq), oracle(p, q, qr=rq)), (run_scatter(index, q, rp), oracle(p, q, pr=rp))):
        assert same(got, ref), report(got, ref)
        c = counts_of(got)
        assert c[7] == 0 and c[100] == 0 and c[201] == 0 and c[150] >= 1
    empty = E.build_index(torch.empty((0, 3), device=DEV), grid=True)
    none, no_r = torch.empty((0, 3)), torch.empty(0)
    assert torch.equal(counts_gather(empty, q, rq), torch.zeros(300, dtype=torch.int32))
    assert torch.equal(counts_scatter(empty, q, no_r), torch.zeros(300, dtype=torch.int32))
    for o, i, d in (run_gather(empty, q, rq), run_scatter(empty, q, no_r)):
        assert torch.equal(o, torch.zeros(301, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0
    assert counts_gather(index, none, no_r).shape == (0,) and counts_scatter(index, none, rp).shape == (0,)
    for o, i, d in (run_gather(index, none, no_r), run_scatter(index, none, rp)):
        assert torch.equal(o, torch.zeros(1, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0


def test_errors():
    p, index = data("uniform"), index_of("uniform")
    q = queries("uniform", "in_box")
    qd = q.to(DEV)
    nq, n = q.shape[0], p.shape[0]
    rq, rp = torch.full((nq,), 0.05, device=DEV), torch.full((n,), 0.05, device=DEV)

    def variants(r):
        neg, nan = r.clone(), r.clone()
        neg[11], nan[11] = -0.5, math.nan
        return [neg, nan, r.cpu(), r.double(), r[:-1], torch.cat([r, r[:1]])]

    for bad in variants(rq):
        with pytest.raises(ValueError):
            E.radius_counts(index, qd, bad)
        with pytest.raises(ValueError):
            E.radius_neighbors(index, qd, bad)
    for bad in variants(rp):
        with pytest.raises(ValueError):
            E.point_radius_counts(index, qd, bad)
        with pytest.raises(ValueError):
            E.point_radius_neighbors(index, qd, bad)
        with pytest.raises(ValueError):
            E.prepare_point_radii(index, bad)
    total = int(E.radius_counts(index, qd, rq).sum())
    for fn, r in ((E.radius_neighbors, rq), (E.point_radius_neighbors, rp)):
        with pytest.raises(ValueError, match=str(total)):
            fn(index, qd, r, max_pairs=total - 1)
        assert fn(index, qd, r, max_pairs=total)[1].numel() == total
    # an index built in a rotated frame serves its own points only
    tp = data("tilted_plane")
    rotated = E.build_index(tp.to(DEV), frame=torch.eye(3, device=DEV))
    assert rotated.qrot is not None
    for fn, r in ((E.radius_counts, rq), (E.radius_neighbors, rq),
                  (E.point_radius_counts, torch.full((tp.shape[0],), 0.05, device=DEV)),
                  (E.point_radius_neighbors, torch.full((tp.shape[0],), 0.05, device=DEV))):
        with pytest.raises(ValueError):
            fn(rotated, qd, r)

"""Neighbour lists on the GPU (knn_neighbors.hip on top of the foreign-query k-th pass): ids
and distances of query_neighbors bit for bit against the brute-force oracle K.knn_cpu.
Indexes and oracle lists are computed once per module (the oracle at the largest k: a
shorter list is its prefix whenever nothing is unfilled)."""
import math

import pytest
import torch

from datasets import GENERATORS, lattice, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 30_000
KS = (1, 16, 100, 128)

_DATA: dict = {}
_INDEX: dict = {}
_QUERIES: dict = {}
_ORACLE: dict = {}


def data(name):
    if name not in _DATA:
        _DATA[name] = lattice(32) if name == "lattice" else GENERATORS[name](N, seed=21)
    return _DATA[name]


def index_of(name, grid="auto"):
    """The index of a data set under E.GRID = `grid`, built once."""
    key = (name, grid)
    if key not in _INDEX:
        old = E.GRID
        E.GRID = grid
        try:
            _INDEX[key] = E.build_index(data(name).to(DEV), grid=True)
        finally:
            E.GRID = old
    return _INDEX[key]


def rand_in(lo, hi, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand((n, 3), generator=g)).contiguous()


def queries(name, kind):
    if (name, kind) in _QUERIES:
        return _QUERIES[(name, kind)]
    p = data(name)
    lo, hi = p.min(0).values, p.max(0).values
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    if kind == "in_box":
        q = rand_in(lo, hi, 3000, 1)
    elif kind == "scaled3":  # the box scaled 3x about its centre: about 26/27 of them outside
        q = rand_in(c - 3 * half, c + 3 * half, 3000, 2)
    elif kind == "dense":  # far denser than the data
        q = rand_in(c - 0.005, c + 0.005, 4000, 4)
    elif kind == "copies":  # 1000 copies of one query
        q = rand_in(lo, hi, 1, 6).repeat(1000, 1).contiguous()
    elif kind == "on_points":  # 500 exact copies of data points mixed with 500 random ones
        g = torch.Generator().manual_seed(7)
        q = torch.cat([p[torch.randint(0, p.shape[0], (500,), generator=g)], rand_in(lo, hi, 500, 8)])
        q = q[torch.randperm(1000, generator=g)].contiguous()
    else:
        raise KeyError(kind)
    _QUERIES[(name, kind)] = q
    return q


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def lists_cpu(p, q, k, r=math.inf):
    idx, d2 = K.knn_cpu(p, q, k, E.cut2_of(r))
    return idx, final(d2)


def oracle(name, kind, k):
    """Lists of a shared data set / query set without a cutoff: the k = 128 oracle's prefix
    (n >= 128, so no slot is unfilled and the first k of the first 128 are the first k)."""
    if (name, kind) not in _ORACLE:
        _ORACLE[(name, kind)] = lists_cpu(data(name), queries(name, kind), max(KS))
    idx, dist = _ORACLE[(name, kind)]
    return idx[:, :k].contiguous(), dist[:, :k].contiguous()


def run(index, q, k, r=math.inf, stats=None):
    idx, dist = E.query_neighbors(index, q.to(DEV), E.KnnConfig(k=k, max_radius=r), stats=stats)
    assert E.LAST_NEIGHBOR_ERRORS[0] == 0  # the device error word of the collect pass
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (q.shape[0], k)
    return idx.cpu(), dist.cpu()


def same(got, ref):
    return torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def report(got, ref):
    bad = ((got[0] != ref[0]) | (got[1] != ref[1])).any(dim=1)
    return f"{int(bad.sum())} of {bad.numel()} rows differ, first {bad.nonzero().flatten()[:5].tolist()}"


QUERY_KINDS = ["in_box", "scaled3", "dense", "on_points", "copies"]


@pytest.mark.parametrize("kind", QUERY_KINDS)
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_every_data_set_and_query_shape(name, kind):
    index = index_of(name)
    q = queries(name, kind)
    for k in KS:
        got, ref = run(index, q, k), oracle(name, kind, k)
        assert same(got, ref), f"{name}/{kind} k={k}: {report(got, ref)}"


# ------------------------------------------------------------------------------------ ties
def test_duplicates_lowest_rows_win():
    """50 sites with about 600 copies each, k = 100: every list is 100 of the nearest site's
    copies at one distance, and they must be its 100 lowest rows (the tie overflows the row:
    the wave-per-query path chooses)."""
    p = data("duplicates")
    sites = torch.unique(p, dim=0)
    assert sites.shape[0] == 50
    q = torch.cat([sites, sites + 1e-3]).contiguous()
    got = run(index_of("duplicates"), q, 100)
    assert same(got, lists_cpu(p, q, 100)), report(got, lists_cpu(p, q, 100))
    for i in range(50):
        rows = torch.nonzero((p == sites[i]).all(dim=1)).flatten()
        assert rows.numel() > 100
        assert torch.equal(got[0][i].long(), rows[:100]) and bool((got[1][i] == 0).all())
        assert torch.equal(got[0][50 + i].long(), rows[:100])


@pytest.mark.parametrize("k", [5, 7])
def test_lattice_sites(k):
    """Coordinates j / 32 (every d² exact): at a site, 1 point at 0 and 6 at 1/32; k = 5 cuts
    that tie in the middle, k = 7 fills it exactly."""
    p = data("lattice")
    g = torch.Generator().manual_seed(3)
    q = p[torch.randperm(p.shape[0], generator=g)[:3000]].contiguous()
    got, ref = run(index_of("lattice"), q, k), lists_cpu(p, q, k)
    assert same(got, ref), report(got, ref)
    inner = ((q > 0) & (q < 31 / 32)).all(dim=1)
    assert int(inner.sum()) > 2000
    assert bool((got[1][inner][:, 1:] == 1 / 32).all()) and bool((got[1][:, 0] == 0).all())


def test_seventy_thousand_copies():
    """70 000 copies of one point among 5000 others, rows shuffled, k = 100: queries on and
    near the copies tie 70 000 ways at their k-th distance (the tie-overflow path keeps the
    100 lowest rows)."""
    g = torch.Generator().manual_seed(9)
    base = torch.tensor([[0.25, 0.5, 0.75]])
    p = torch.cat([base.repeat(70_000, 1), uniform(5000, seed=10)])
    p = p[torch.randperm(p.shape[0], generator=g)].contiguous()
    q = torch.cat([base.repeat(40, 1), base + 0.01 * torch.randn((200, 3), generator=g), uniform(300, seed=11)])
    index = E.build_index(p.to(DEV), grid=True)
    got, ref = run(index, q, 100), lists_cpu(p, q, 100)
    assert same(got, ref), report(got, ref)
    rows = torch.nonzero((p == base).all(dim=1)).flatten()
    assert torch.equal(got[0][0].long(), rows[:100])


# ------------------------------------------------------------------------- cutoff and fill
@pytest.mark.parametrize("r", [0.0, 0.02, 0.05, 1.0])
def test_cutoff_leaves_lists_short(r):
    for name in ("uniform", "clustered"):
        p, index = data(name), index_of(name)
        for kind in ("in_box", "scaled3", "on_points"):
            q = queries(name, kind)[:1000].contiguous()
            for k in (1, 16, 100):
                got, ref = run(index, q, k, r=r), lists_cpu(p, q, k, r)
                assert same(got, ref), f"{name}/{kind} k={k} r={r}: {report(got, ref)}"
    if r == 0.05:  # some lists full, some short, and short ones carry -1 and the cutoff
        short = got[0][:, -1] < 0
        assert 0 < int(short.sum()) < 1000
        assert bool((got[1][got[0] < 0] == final(torch.tensor([E.cut2_of(r)]))[0]).all())


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_shapes(n):
    """The partial bucket, the partial query group and the row padding: k = 1, k = n (every
    point listed) and k = n + 1 (one unfilled slot), with and without a cutoff."""
    p = uniform(n, seed=n)
    index = E.build_index(p.to(DEV), grid=True)
    for nq in (1, 63, 65):
        q = uniform(nq, seed=100 + nq) * 1.4 - 0.2
        for k in sorted({1, n, n + 1}):
            got, ref = run(index, q, k), lists_cpu(p, q, k)
            assert same(got, ref), (n, nq, k, report(got, ref))
        got, ref = run(index, q, n + 1, r=0.5), lists_cpu(p, q, n + 1, 0.5)
        assert same(got, ref), (n, nq, report(got, ref))


def test_empty_sides_and_a_nan_query():
    p, index = data("uniform"), index_of("uniform")
    idx, dist = run(index, torch.empty((0, 3)), 4)
    assert idx.shape == dist.shape == (0, 4)
    z = torch.zeros((K.PAD_POINTS, 3), device=DEV)  # an index of no points: nothing of it is read
    empty = E.LocalIndex(0, z, z[:0, 0].to(torch.int32), z, z, 0, torch.zeros(8, device=DEV))
    q = uniform(70, seed=1)
    for r in (math.inf, 0.25):
        assert same(run(empty, q, 3, r=r), lists_cpu(p[:0], q, 3, r))
        got = E.knn_query_neighbors(z[:0], q.to(DEV), 3, max_radius=r)
        assert same((got[0].cpu(), got[1].cpu()), lists_cpu(p[:0], q, 3, r))
    q = queries("uniform", "in_box")[:300].clone()
    q[5, 0] = math.nan
    for k in (1, 100):
        got, ref = run(index, q, k), lists_cpu(p, q, k)
        assert same(got, ref), report(got, ref)
        assert bool((got[0][5] == -1).all()) and bool(torch.isinf(got[1][5]).all())


# ------------------------------------------------------------------------ limits and errors
def test_k_1024_and_limits():
    p = uniform(3000, seed=5)
    q = uniform(200, seed=6) * 1.2 - 0.1
    index = E.build_index(p.to(DEV), grid=True)
    got, ref = run(index, q, K.NEIGHBORS_MAX_K), lists_cpu(p, q, K.NEIGHBORS_MAX_K)
    assert same(got, ref), report(got, ref)
    with pytest.raises(ValueError, match="query_points"):
        E.query_neighbors(index, q.to(DEV), E.KnnConfig(k=K.NEIGHBORS_MAX_K + 1))
    with pytest.raises(ValueError):
        E.query_neighbors(index, q, E.KnnConfig(k=1))  # CPU queries, GPU index
    rot = E.build_index(data("tilted_plane").to(DEV), frame=torch.eye(3, device=DEV))
    assert rot.qrot is not None
    with pytest.raises(ValueError):
        E.query_neighbors(rot, q.to(DEV), E.KnnConfig(k=1))


# ------------------------------------------------------------------------------ invariants
def test_last_column_is_query_points():
    for name in ("uniform", "clustered", "duplicates"):
        index = index_of(name)
        q = queries(name, "scaled3").to(DEV)
        for k, r in ((1, math.inf), (16, math.inf), (100, math.inf), (100, 0.05)):
            cfg = E.KnnConfig(k=k, max_radius=r)
            dist = E.query_neighbors(index, q, cfg)[1]
            assert torch.equal(dist[:, k - 1], E.query_points(index, q, cfg)), (name, k, r)


def test_grid_on_and_off_give_identical_lists():
    q = queries("uniform", "scaled3")
    assert index_of("uniform", "off").grid is None and index_of("uniform", "on").grid.gate is None
    for k in (16, 100):
        E.reset_kernels_used()
        off = run(index_of("uniform", "off"), q, k)
        assert E.kernels_used() == ["rows"]
        E.reset_kernels_used()
        on = run(index_of("uniform", "on"), q, k)
        assert E.kernels_used() == ["grid"]
        assert same(on, off) and same(on, oracle("uniform", "scaled3", k))


@pytest.mark.parametrize("name", ["uniform", "duplicates"])
def test_lists_do_not_depend_on_the_kth_kernel(name, monkeypatch):
    """Every 7th query through the failure list, then every query through the exact kernel:
    the same lists as the production route."""
    index = index_of(name)
    q = queries(name, "in_box")
    ref = oracle(name, "in_box", 100)
    monkeypatch.setattr(E, "DEBUG_FAIL_MOD", 7)
    st = E.KnnStats()
    got = run(index, q, 100, stats=st)
    assert st.counters["fallback_queries"] >= (q.shape[0] + 6) // 7
    assert same(got, ref), report(got, ref)
    monkeypatch.setattr(E, "DEBUG_FAIL_MOD", 0)
    monkeypatch.setattr(E, "KNN_IMPL", "exact")
    E.reset_kernels_used()
    got = run(index, q, 100)
    assert E.kernels_used() == ["exact"]
    assert same(got, ref), report(got, ref)


def test_two_runs_are_bit_identical():
    for name in ("clustered", "duplicates"):
        index = index_of(name)
        q = queries(name, "on_points")
        assert same(run(index, q, 100), run(index, q, 100))


def test_self_form_equals_the_foreign_form():
    p = data("clustered")[:8000].contiguous().to(DEV)
    a = E.knn_neighbors(p, 16)
    b = E.knn_query_neighbors(p, p, 16)
    assert E.LAST_NEIGHBOR_ERRORS[0] == 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool((a[1][:, 0] == 0).all())
    ref = lists_cpu(p.cpu(), p.cpu(), 16)
    assert same((a[0].cpu(), a[1].cpu()), ref)

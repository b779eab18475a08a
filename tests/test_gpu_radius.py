"""Fixed-radius search on the GPU (radius.hip): counts and CSR neighbour lists of
radius_counts / radius_neighbors bit for bit against the brute-force oracle K.radius_cpu /
K.radius_count_cpu. Indexes, query sets and oracle results are computed once per module."""
import math

import numpy as np
import pytest
import torch

from datasets import GENERATORS, lattice, uniform
from mpi_cuda_largescaleknn_amd import _native
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 30_000
RADII = (0.0, 1e-4, 0.02, 0.05)

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
    """The query shapes of the neighbour-list tests, fewer of each (rows here can be long)."""
    if (name, kind) in _QUERIES:
        return _QUERIES[(name, kind)]
    p = data(name)
    lo, hi = p.min(0).values, p.max(0).values
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    if kind == "in_box":
        q = rand_in(lo, hi, 2000, 1)
    elif kind == "scaled3":  # the box scaled 3x about its centre: about 26/27 of them outside
        q = rand_in(c - 3 * half, c + 3 * half, 3000, 2)
    elif kind == "dense":  # far denser than the data
        q = rand_in(c - 0.005, c + 0.005, 600, 4)
    elif kind == "copies":  # 300 copies of one query
        q = rand_in(lo, hi, 1, 6).repeat(300, 1).contiguous()
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


def lists_cpu(p, q, r):
    offsets, idx, d2 = K.radius_cpu(p, q, E.cut2_of(r))
    return offsets, idx, final(d2)


def oracle(name, kind, r):
    if (name, kind, r) not in _ORACLE:
        _ORACLE[(name, kind, r)] = lists_cpu(data(name), queries(name, kind), r)
    return _ORACLE[(name, kind, r)]


def counts_of(lists):
    return (lists[0][1:] - lists[0][:-1]).int()


def run(index, q, r, **kw):
    offsets, idx, dist = E.radius_neighbors(index, q.to(DEV), r, **kw)
    assert E.LAST_RADIUS_ERRORS[0] == 0  # the device error word of the fill pass
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert offsets.shape == (q.shape[0] + 1,) and idx.shape == dist.shape == (int(offsets[-1]),)
    return offsets.cpu(), idx.cpu(), dist.cpu()


def run_counts(index, q, r, stats=None):
    c = E.radius_counts(index, q.to(DEV), r, stats=stats)
    assert c.dtype == torch.int32 and c.shape == (q.shape[0],)
    return c.cpu()


def same(got, ref):
    return all(torch.equal(g, w) for g, w in zip(got, ref))


def report(got, ref):
    if not torch.equal(got[0], ref[0]):
        bad = (counts_of(got) != counts_of(ref)).nonzero().flatten()
        return f"{bad.numel()} of {ref[0].numel() - 1} rows differ in length, first {bad[:5].tolist()}"
    bad = ((got[1] != ref[1]) | (got[2] != ref[2])).nonzero().flatten()
    rows_bad = torch.unique(torch.searchsorted(ref[0], bad, right=True) - 1)
    return f"{bad.numel()} of {ref[1].numel()} pairs differ, in {rows_bad.numel()} rows, first {rows_bad[:5].tolist()}"


def test_lds_row_constant_matches_the_kernels():
    assert _native.hip().lsk_hip_radius_lds_row() == K.RADIUS_LDS_ROW


QUERY_KINDS = ["in_box", "scaled3", "dense", "on_points", "copies"]


@pytest.mark.parametrize("kind", QUERY_KINDS)
@pytest.mark.parametrize("name", sorted(GENERATORS) + ["lattice"])
def test_every_data_set_and_query_shape(name, kind):
    index = index_of(name)
    q = queries(name, kind)
    for r in RADII:
        ref = oracle(name, kind, r)
        c = run_counts(index, q, r)
        assert torch.equal(c, counts_of(ref)), f"{name}/{kind} r={r}: {int((c != counts_of(ref)).sum())} counts differ"
        got = run(index, q, r)
        assert same(got, ref), f"{name}/{kind} r={r}: {report(got, ref)}"


def test_both_sort_paths():
    """Rows on both sides of K.RADIUS_LDS_ROW in one call: the LDS network and the
    global-memory one. At r = 0.33 a ball holds about 0.15 n = 4500 points in the middle of
    the cube and an eighth of that at a corner."""
    p = data("uniform")
    q = queries("uniform", "in_box")[:200].contiguous()
    ref = lists_cpu(p, q, 0.33)
    c = counts_of(ref)
    assert int((c > K.RADIUS_LDS_ROW).sum()) >= 20 and int(((c > 0) & (c <= K.RADIUS_LDS_ROW)).sum()) >= 20
    got = run(index_of("uniform"), q, 0.33)
    assert same(got, ref), report(got, ref)


def test_row_sort_of_hand_made_rows():
    """lsk_hip_radius_sort alone on hand-made CSR rows: lengths around every padding step of
    the LDS network and on both sides of K.RADIUS_LDS_ROW, keys with many repeats of one d²
    under different ids. Against torch.sort of the packed (d² bits << 32 | id) keys."""
    lens = [0, 1, 2, 3, 5, 64, 65, K.RADIUS_LDS_ROW - 1, K.RADIUS_LDS_ROW, K.RADIUS_LDS_ROW + 1]
    g = torch.Generator().manual_seed(77)
    bits, ids = [], []
    for m in lens:
        # d² bits of finite non-negative floats, about three ids per value; ids distinct within the row
        pool = torch.randint(0, 0x7F800000, (max(1, m // 3),), generator=g, dtype=torch.int64)
        bits.append(pool[torch.randint(0, pool.numel(), (m,), generator=g)])
        ids.append(torch.randperm(3 * m + 1, generator=g)[:m])
    bits, ids = torch.cat(bits), torch.cat(ids)
    offsets = torch.zeros(len(lens) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor(lens), 0)
    total = int(offsets[-1])
    d2 = bits.int().view(torch.float32)
    assert bool(torch.isfinite(d2).all()) and bool((d2 >= 0).all())
    packed = (bits << 32) | ids
    want = torch.cat([torch.sort(packed[a:b]).values for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())])
    assert int((want[1:] >> 32 == want[:-1] >> 32).sum()) > total // 2  # repeats of one d² survive the setup
    off_d = offsets.to(DEV)
    for sort, ref in ((1, want), (0, packed)):
        idx, dist = ids.int().to(DEV), d2.to(DEV)
        _native.check(_native.hip().lsk_hip_radius_sort(K._ptr(off_d), len(lens), total, max(lens), K._ptr(idx),
                                                       K._ptr(dist), sort, K._stream(idx)), "radius_sort")
        assert torch.equal(idx.cpu(), (ref & 0xFFFFFFFF).int()), f"sort={sort}: ids"
        assert torch.equal(dist.cpu(), final((ref >> 32).int().view(torch.float32))), f"sort={sort}: distances"


def test_seventy_thousand_copies():
    """Rows far beyond the LDS limit made of one distance: 70 000 copies of one point among
    5000 others; a query on the copies lists exactly their rows first, ascending."""
    g = torch.Generator().manual_seed(31)
    site = torch.tensor([[0.37, 0.52, 0.61]])
    p = torch.cat([site.repeat(70_000, 1), uniform(5000, seed=32)])
    p = p[torch.randperm(p.shape[0], generator=g)].contiguous()
    copies = (p == site).all(1).nonzero().flatten().int()
    assert copies.numel() == 70_000
    q = torch.cat([site.repeat(10, 1), site + 1e-4 * (torch.rand((10, 3), generator=g) - 0.5)]).contiguous()
    r = 0.01
    index = E.build_index(p.to(DEV), grid=True)
    ref = lists_cpu(p, q, r)
    assert int(counts_of(ref).min()) >= 70_000
    assert torch.equal(run_counts(index, q, r), counts_of(ref))
    got = run(index, q, r)
    assert same(got, ref), report(got, ref)
    for j in range(10):
        row = got[1][got[0][j]:got[0][j + 1]]
        assert torch.equal(row[:70_000], copies) and bool((got[2][got[0][j]:got[0][j] + 70_000] == 0).all())


@pytest.mark.parametrize("name", ["uniform", "clustered", "mixed_scale"])
def test_far_corner_acceptance(name):
    """Radii at which whole boxes lie inside the balls: r = 0.3 and r = 2.0, and for data of
    another extent (mixed_scale: 1000) also 0.3 and 2 extents."""
    p = data(name)
    index = index_of(name)
    q = queries(name, "scaled3")
    lo, hi = p.min(0).values, p.max(0).values
    extent = float((hi - lo).max())
    inside = ((q >= lo) & (q <= hi)).all(1)
    assert int(inside.sum()) >= 50
    radii = [0.3, 2.0] + ([0.3 * extent, 2.0 * extent] if extent > 1.2 else [])
    for r in radii:
        ref_c = K.radius_count_cpu(p, q, E.cut2_of(r))
        stats = E.KnnStats()
        c = run_counts(index, q, r, stats=stats)
        assert torch.equal(c, ref_c), f"{name} r={r}: {int((c != ref_c).sum())} counts differ"
        if r >= 0.25 * extent:
            # whole boxes were taken, and far fewer points tested than brute force would
            assert stats.counters["radius_box_accepts"] > 0
            assert stats.counters["radius_evals"] < 0.25 * q.shape[0] * p.shape[0]
        if r * r > 3.0 * extent * extent:
            # the ball around a query inside the data's box holds every point (the box's
            # diagonal is at most sqrt(3) extents); queries of the 3x box can be farther away
            assert bool((c[inside] == p.shape[0]).all())
        sub = q[:100].contiguous()
        got, ref = run(index, sub, r), lists_cpu(p, sub, r)
        assert same(got, ref), f"{name} r={r}: {report(got, ref)}"
    # every in-box query at 2 extents: the root box is accepted, no point is tested
    qi = queries(name, "in_box")
    stats = E.KnnStats()
    c = run_counts(index, qi, 2.0 * extent, stats=stats)
    assert bool((c == p.shape[0]).all()) and stats.counters["radius_evals"] == 0


@pytest.mark.parametrize("nq", [1, 63, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_shapes(n, nq):
    p = uniform(n, seed=40 + n)
    q = (uniform(nq, seed=50 + nq) * 1.4 - 0.2).contiguous()
    index = E.build_index(p.to(DEV), grid=True)
    for r in (0.1, 0.5, math.inf):
        ref = lists_cpu(p, q, r)
        assert torch.equal(run_counts(index, q, r), counts_of(ref)), f"n={n} nq={nq} r={r}"
        got = run(index, q, r)
        assert same(got, ref), f"n={n} nq={nq} r={r}: {report(got, ref)}"
        if math.isinf(r):
            assert bool((counts_of(got) == n).all())


def test_empty_and_nan_inputs():
    p = data("uniform")
    index = index_of("uniform")
    q = queries("uniform", "in_box")[:300].contiguous()
    empty = E.build_index(torch.empty((0, 3), device=DEV), grid=True)
    assert torch.equal(run_counts(empty, q, 0.1), torch.zeros(300, dtype=torch.int32))
    o, i, d = run(empty, q, 0.1)
    assert torch.equal(o, torch.zeros(301, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0
    for res in (E.radius_query_neighbors(torch.empty((0, 3), device=DEV), q.to(DEV), 0.1),):
        assert torch.equal(res[0].cpu(), torch.zeros(301, dtype=torch.int64)) and res[1].numel() == 0
    none = torch.empty((0, 3))
    assert run_counts(index, none, 0.1).shape == (0,)
    o, i, d = run(index, none, 0.1)
    assert torch.equal(o, torch.zeros(1, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0
    # NaN / infinite coordinates inside a batch: empty rows, every other row unchanged
    q2 = q.clone()
    q2[7, 2] = math.nan
    q2[100] = math.nan
    q2[201, 0] = -math.inf
    want = lists_cpu(p, q2, 0.08)
    got = run(index, q2, 0.08)
    assert same(got, want), report(got, want)
    c = counts_of(got)
    assert c[7] == 0 and c[100] == 0 and c[201] == 0
    plain = run(index, q, 0.08)
    for j in range(300):
        if j not in (7, 100, 201):
            a, b = plain[0][j], got[0][j]
            m = int(plain[0][j + 1] - a)
            assert m == int(c[j]) and torch.equal(plain[1][a:a + m], got[1][b:b + m]) \
                and torch.equal(plain[2][a:a + m], got[2][b:b + m])
    assert torch.equal(run_counts(index, q2, 0.08), c)


def test_lattice_strictness():
    """Spacing 1/32 and every d² exact: r = 1/32 excludes the six face neighbours (d² == cut2),
    the next float above it includes them."""
    p = data("lattice")
    j = torch.arange(32 ** 3)
    x, y, z = j // 1024, (j // 32) % 32, j % 32
    inner = ((x > 0) & (x < 31) & (y > 0) & (y < 31) & (z > 0) & (z < 31)).nonzero().flatten()
    q = p[inner[::11]].contiguous()
    index = index_of("lattice")
    step = np.float32(1.0 / 32.0)
    above = float(np.nextafter(step, np.float32(1.0)))
    assert bool((run_counts(index, q, float(step)) == 1).all())
    assert bool((run_counts(index, q, above) == 7).all())
    assert bool((run_counts(index, q, 0.0) == 0).all())
    assert bool((run_counts(index, q, math.inf) == p.shape[0]).all())
    o, i, d = run(index, q, above)
    assert torch.equal(o, 7 * torch.arange(q.shape[0] + 1))
    assert bool((d.view(-1, 7)[:, 0] == 0).all()) and bool((d.view(-1, 7)[:, 1:] == step).all())
    assert torch.equal(i.view(-1, 7)[:, 0], inner[::11].int())


@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates"])
def test_invariants_against_the_knn_api(name):
    index = index_of(name)
    q = queries(name, "in_box")
    qd = q.to(DEV)
    r = 0.05
    counts = run_counts(index, q, r)
    cutoff = float(K.finalize_distances(torch.tensor([E.cut2_of(r)]))[0])
    for k in (1, 16, 100):
        kth = E.query_points(index, qd, E.KnnConfig(k=k, max_radius=r)).cpu()
        assert torch.equal(counts >= k, kth < cutoff), f"{name} k={k}"
    offsets, idx, dist = run(index, q, r)
    assert torch.equal(offsets[1:], torch.cumsum(counts.long(), 0)) and offsets[0] == 0
    ni, nd = E.query_neighbors(index, qd, E.KnnConfig(k=128, max_radius=r))
    ni, nd = ni.cpu(), nd.cpu()
    checked = 0
    for j in ((counts >= 1) & (counts <= 128)).nonzero().flatten().tolist():
        m = int(counts[j])
        assert int((ni[j] != -1).sum()) == m
        assert torch.equal(ni[j, :m], idx[offsets[j]:offsets[j + 1]]), f"{name}: ids of row {j}"
        assert torch.equal(nd[j, :m], dist[offsets[j]:offsets[j + 1]]), f"{name}: distances of row {j}"
        checked += 1
    assert checked > 0 or name == "duplicates"  # (duplicates: every non-empty row holds about 600 copies)


def test_unsorted_rows_are_the_same_sets():
    index = index_of("clustered")
    q = queries("clustered", "in_box")
    ref = oracle("clustered", "in_box", 0.05)
    o, i, d = run(index, q, 0.05, sort=False)
    assert torch.equal(o, ref[0])
    # host sort of every row by (row, id): ids are distinct within a row
    row = torch.repeat_interleave(torch.arange(q.shape[0]), counts_of(ref).long())
    order = torch.argsort(row * (1 << 31) + i.long())
    want = torch.argsort(row * (1 << 31) + ref[1].long())
    assert torch.equal(i[order], ref[1][want]) and torch.equal(d[order], ref[2][want])


def test_repeat_runs_are_bit_identical():
    index = index_of("duplicates")
    q = queries("duplicates", "on_points")
    a, b = run(index, q, 0.05), run(index, q, 0.05)
    assert same(a, b)
    assert torch.equal(run_counts(index, q, 0.05), run_counts(index, q, 0.05))


def test_self_form():
    p = data("uniform")[:5000].contiguous()
    pd = p.to(DEV)
    for r in (0.02, 0.06):
        so, si, sd = (t.cpu() for t in E.radius_self_neighbors(pd, r))
        assert E.LAST_RADIUS_ERRORS[0] == 0
        fo, fi, fd = (t.cpu() for t in E.radius_query_neighbors(pd, pd, r))
        assert torch.equal(so, fo) and torch.equal(si, fi) and torch.equal(sd, fd)
        assert bool((sd[so[:-1]] == 0).all()) and torch.equal(si[so[:-1]], torch.arange(5000, dtype=torch.int32))
        assert same((so, si, sd), lists_cpu(p, p, r))
    assert torch.equal(E.radius_query_counts(pd, pd, 0.06).cpu(), (so[1:] - so[:-1]).int())


def test_grid_or_no_grid():
    q = queries("uniform", "scaled3")
    a = run(index_of("uniform", "on"), q, 0.05)
    b = run(index_of("uniform", "off"), q, 0.05)
    assert same(a, b) and same(a, oracle("uniform", "scaled3", 0.05))


def test_errors():
    index = index_of("uniform")
    q = queries("uniform", "in_box")
    total = int(counts_of(oracle("uniform", "in_box", 0.05)).sum())
    with pytest.raises(ValueError, match=str(total)):
        E.radius_neighbors(index, q.to(DEV), 0.05, max_pairs=total - 1)
    assert run(index, q, 0.05, max_pairs=total)[1].numel() == total
    with pytest.raises(ValueError):  # CPU queries on a GPU index
        E.radius_counts(index, q, 0.05)
    with pytest.raises(ValueError):
        E.radius_neighbors(index, q, 0.05)
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError):
            E.radius_counts(index, q.to(DEV), bad)
        with pytest.raises(ValueError):
            E.radius_neighbors(index, q.to(DEV), bad)
    # an index built in a rotated frame serves its own points only
    rotated = E.build_index(data("tilted_plane").to(DEV), frame=torch.eye(3, device=DEV))
    assert rotated.qrot is not None
    with pytest.raises(ValueError):
        E.radius_counts(rotated, q.to(DEV), 0.05)
    with pytest.raises(ValueError):
        E.radius_neighbors(rotated, q.to(DEV), 0.05)
    assert "radius" in E.kernels_used()

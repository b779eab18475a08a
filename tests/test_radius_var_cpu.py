"""Variable-radius search on the CPU path: the brute-force oracles K.radius_var_cpu /
radius_var_count_cpu against independent routes (gather: prefixes of the neighbour-list
oracle K.knn_cpu; scatter: the transpose of a gather search with the roles of points and
queries swapped), the scalar form bit for bit, the strict comparison per element on a
lattice, reverse nearest neighbours, the engine on a CPU index and the hipKNN_radius /
lsknn_tools rcheck round trip with --radii and --point-radii."""
import math
import os

import numpy as np
import pytest
import torch

import mpi_cuda_largescaleknn_amd as pkg
from mpi_cuda_largescaleknn_amd.apps import radius as radius_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import duplicates, lattice, uniform

N = 3000
INF = math.inf

DATA = {
    "uniform": lambda: (uniform(N, seed=3), uniform(200, seed=4) * 1.4 - 0.2),
    "duplicates": lambda: (duplicates(N, seed=5, ndistinct=40), duplicates(N, seed=5, ndistinct=40)[::15].clone()),
    "lattice": lambda: (lattice(15), lattice(15)[::13].clone()),
}


def radii(profile, m, seed):
    """float32 [m] radii: all zero, log-uniform 1e-3 .. 0.3, or a few inf among 0.05."""
    g = torch.Generator().manual_seed(seed)
    if profile == "zeros":
        return torch.zeros(m)
    if profile == "loguniform":
        return torch.exp(math.log(1e-3) + (math.log(0.3) - math.log(1e-3)) * torch.rand(m, generator=g)).float()
    if profile == "some_inf":
        r = torch.full((m,), 0.05)
        r[torch.randperm(m, generator=g)[:3]] = INF
        return r
    raise KeyError(profile)


PROFILES = ["zeros", "loguniform", "some_inf"]


def sq(r):
    """cut2 per element, the float32 product of cut2_of."""
    return (r.numpy().astype(np.float32) * r.numpy().astype(np.float32)).view(np.float32).copy()


def cut2_t(r):
    return torch.from_numpy(sq(r))


def rows(offsets, *arrays):
    return [tuple(a[offsets[i]:offsets[i + 1]] for a in arrays) for i in range(offsets.shape[0] - 1)]


def transpose(lists, ncols):
    """The CSR lists (offsets, idx, d2) of m rows over ids < ncols, transposed: ncols rows
    over ids < m, every row ascending by (d² bits, id)."""
    offsets, idx, d2 = (t.numpy() for t in lists)
    m = offsets.shape[0] - 1
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(offsets))
    bits = d2.view(np.int32).astype(np.int64)  # (non-negative floats order like their bits)
    order = np.lexsort((row, bits, idx.astype(np.int64)))
    out = np.zeros(ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx.astype(np.int64), minlength=ncols), out=out[1:])
    return torch.from_numpy(out), torch.from_numpy(row[order].astype(np.int32)), torch.from_numpy(d2[order].copy())


def same(got, ref):
    return all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, ref)) \
        and torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32))


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def test_exported():
    for name in ("point_radius_counts", "point_radius_neighbors", "point_radius_query_counts",
                 "point_radius_query_neighbors", "point_radius_self_neighbors", "prepare_point_radii"):
        assert getattr(pkg, name) is getattr(E, name)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("name", sorted(DATA))
def test_gather_oracle_against_the_neighbour_list_oracle(name, profile):
    p, q = DATA[name]()
    c2 = cut2_t(radii(profile, q.shape[0], 60))
    counts = K.radius_var_count_cpu(p, q, qcut2=c2)
    offsets, idx, d2 = K.radius_var_cpu(p, q, qcut2=c2)
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert offsets[0] == 0 and torch.equal(offsets[1:], torch.cumsum(counts.long(), 0))
    assert idx.shape[0] == d2.shape[0] == int(offsets[-1])
    # one slot more than the longest row, so that a row the oracle cut short would show
    kmax = min(p.shape[0], int(counts.max()) + 1)
    ki, kd = K.knn_cpu(p, q, kmax, INF)
    below = kd < c2[:, None]
    m = below.sum(1).int()
    assert bool((below[:, 1:] <= below[:, :-1]).all())  # a prefix
    assert torch.equal(m, counts)
    for i, (ri, rd) in enumerate(rows(offsets, idx, d2)):
        assert torch.equal(ki[i, :m[i]], ri), f"{name}/{profile}: ids of query {i}"
        assert torch.equal(kd[i, :m[i]].view(torch.int32), rd.view(torch.int32)), f"{name}/{profile}: d² of query {i}"
    if profile == "zeros":
        assert int(counts.sum()) == 0
    if profile == "some_inf":
        assert int((counts == p.shape[0]).sum()) == 3 and bool((counts[torch.isinf(c2)] == p.shape[0]).all())


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("name", sorted(DATA))
def test_scatter_oracle_is_the_transposed_gather(name, profile):
    """dist2 is exactly symmetric (the differences negate, the squares are equal), so the
    scatter rows over (P, Q, radii of P) are the transposed gather rows over (Q, P, the same
    radii as the queries' own)."""
    p, q = DATA[name]()
    c2 = cut2_t(radii(profile, p.shape[0], 61))
    got = K.radius_var_cpu(p, q, pcut2=c2)
    want = transpose(K.radius_var_cpu(q, p, qcut2=c2), q.shape[0])
    assert same(got, want)
    assert torch.equal(K.radius_var_count_cpu(p, q, pcut2=c2), (want[0][1:] - want[0][:-1]).int())
    if profile == "zeros":
        assert got[1].numel() == 0
    if profile == "some_inf":  # the three unbounded points are in every row
        big = torch.isinf(c2).nonzero().flatten().int()
        for ri, in rows(got[0], got[1]):
            assert bool(torch.isin(big, ri).all())


@pytest.mark.parametrize("r", [0.0, 0.01, 0.08, 0.3, INF])
def test_tensor_equals_scalar(r):
    p, q = DATA["uniform"]()
    cut2 = E.cut2_of(r)
    ref_c, ref = K.radius_count_cpu(p, q, cut2), K.radius_cpu(p, q, cut2)
    qc, pc = torch.full((q.shape[0],), cut2), torch.full((p.shape[0],), cut2)
    assert torch.equal(K.radius_var_count_cpu(p, q, qcut2=qc), ref_c) and same(K.radius_var_cpu(p, q, qcut2=qc), ref)
    assert torch.equal(K.radius_var_count_cpu(p, q, pcut2=pc), ref_c) and same(K.radius_var_cpu(p, q, pcut2=pc), ref)
    # the engine on a CPU index: a tensor filled with r, and squared=True with cut2_of(r)
    index = E.build_index(p)
    sc, sl = E.radius_counts(index, q, r), E.radius_neighbors(index, q, r)
    rq, rp = torch.full((q.shape[0],), r), torch.full((p.shape[0],), r)
    for c, lists in ((E.radius_counts(index, q, rq), E.radius_neighbors(index, q, rq)),
                     (E.radius_counts(index, q, qc, squared=True), E.radius_neighbors(index, q, qc, squared=True)),
                     (E.radius_counts(index, q, cut2, squared=True), E.radius_neighbors(index, q, cut2, squared=True)),
                     (E.point_radius_counts(index, q, rp), E.point_radius_neighbors(index, q, rp)),
                     (E.point_radius_counts(index, q, pc, squared=True),
                      E.point_radius_neighbors(index, q, pc, squared=True))):
        assert c.dtype == torch.int32 and torch.equal(c, sc)
        assert same(lists, sl)


def interior(m):
    j = torch.arange(m ** 3)
    x, y, z = j // (m * m), (j // m) % m, j % m
    return ((x > 0) & (x < m - 1) & (y > 0) & (y < m - 1) & (z > 0) & (z < m - 1)).nonzero().flatten()


def test_lattice_strictness_per_element():
    """Spacing 1/32, every d² exact: a radius of 1/32 excludes the six face neighbours (d² ==
    cut2), the next float above includes them; the two alternate from element to element."""
    p = lattice(32)
    inner = interior(32)
    step = np.float32(1.0 / 32.0)
    above = np.nextafter(step, np.float32(1.0))
    want = lambda m: torch.tensor([1, 7] * (m // 2) + [1] * (m % 2), dtype=torch.int32)  # noqa: E731
    alt = lambda m: torch.from_numpy(np.where(np.arange(m) % 2 == 0, step, above).astype(np.float32))  # noqa: E731
    q = p[inner[::29]].contiguous()
    nq = q.shape[0]
    index = E.build_index(p)
    assert torch.equal(K.radius_var_count_cpu(p, q, qcut2=cut2_t(alt(nq))), want(nq))
    assert torch.equal(E.radius_counts(index, q, alt(nq)), want(nq))
    # per point: every point is a query; an interior query is reached by itself (d² = 0 < any
    # cut2 > 0) and by those of its six face neighbours whose own radius is the larger one
    rp = alt(p.shape[0])
    c = E.point_radius_counts(index, p, rp)
    assert torch.equal(c, K.radius_var_count_cpu(p, p, pcut2=cut2_t(rp)))
    j = inner
    nb = torch.stack([j - 1024, j + 1024, j - 32, j + 32, j - 1, j + 1], 1)
    assert torch.equal(c[inner], (1 + (nb % 2 == 1).sum(1)).int())
    o, i, d = E.radius_neighbors(index, q, alt(nq))
    for k, (ri, rd) in enumerate(rows(o, i, d)):
        assert rd[0] == 0 and ri[0] == inner[::29][k] and bool((rd[1:] == step).all())


def test_reverse_neighbours():
    """Per-point squared radii = every point's own k-th d²: row q of the scatter search is
    the set of p with d²(q, p) strictly below p's k-th d², the transpose of the k-NN lists
    restricted to entries strictly below their row's k-th d²."""
    k = 16
    for name in ("uniform", "duplicates"):
        p = DATA[name]()[0]
        n = p.shape[0]
        ki, kd = K.knn_cpu(p, p, k, INF)
        kth = kd[:, k - 1].contiguous()
        keep = kd < kth[:, None]
        counts = keep.sum(1)
        offsets = torch.zeros(n + 1, dtype=torch.int64)
        torch.cumsum(counts, 0, out=offsets[1:])
        want = transpose((offsets, ki[keep], kd[keep]), n)
        index = E.build_index(p)
        got = E.point_radius_neighbors(index, p, kth, squared=True)
        assert same(got, (want[0], want[1], final(want[2]))), name
        assert same(E.point_radius_self_neighbors(p, kth, squared=True), got)
        assert torch.equal(E.point_radius_counts(index, p, kth, squared=True), (want[0][1:] - want[0][:-1]).int())


def test_engine_on_a_cpu_index():
    p, q = DATA["uniform"]()
    index = E.build_index(p)
    nq, n = q.shape[0], p.shape[0]
    rq, rp = radii("loguniform", nq, 70), radii("loguniform", n, 71)
    rq[3], rp[5], rp[6] = INF, INF, 0.0
    # gather
    ref = K.radius_var_cpu(p, q, qcut2=cut2_t(rq))
    assert torch.equal(E.radius_counts(index, q, rq), (ref[0][1:] - ref[0][:-1]).int())
    assert same(E.radius_neighbors(index, q, rq), (ref[0], ref[1], final(ref[2])))
    assert same(E.radius_query_neighbors(p, q, rq), (ref[0], ref[1], final(ref[2])))
    assert torch.equal(E.radius_query_counts(p, q, rq), (ref[0][1:] - ref[0][:-1]).int())
    assert same(E.radius_neighbors(index, q, cut2_t(rq), squared=True), (ref[0], ref[1], final(ref[2])))
    rs = radii("loguniform", n, 72) * 0.2
    assert same(E.radius_self_neighbors(p, rs), E.radius_query_neighbors(p, p, rs))
    # scatter, tensor and prepared object
    ref = K.radius_var_cpu(p, q, pcut2=cut2_t(rp))
    ref_f = (ref[0], ref[1], final(ref[2]))
    prep = E.prepare_point_radii(index, rp)
    assert torch.equal(prep.cut2.view(torch.int32), cut2_t(rp).view(torch.int32))
    for pr in (rp, prep):
        assert torch.equal(E.point_radius_counts(index, q, pr), (ref[0][1:] - ref[0][:-1]).int())
        assert same(E.point_radius_neighbors(index, q, pr), ref_f)
    assert same(E.point_radius_neighbors(index, q, cut2_t(rp), squared=True), ref_f)
    assert same(E.point_radius_neighbors(index, q, E.prepare_point_radii(index, cut2_t(rp), squared=True)), ref_f)
    assert same(E.point_radius_query_neighbors(p, q, rp), ref_f)
    assert torch.equal(E.point_radius_query_counts(p, q, rp), (ref[0][1:] - ref[0][:-1]).int())
    # sort=False: the same rows as sets
    uo, ui, ud = E.point_radius_neighbors(index, q, rp, sort=False)
    assert torch.equal(uo, ref[0])
    for (gi, gd), (wi, wd) in zip(rows(uo, ui, ud), rows(*ref_f)):
        o, w = torch.argsort(gi.long()), torch.argsort(wi.long())
        assert torch.equal(gi[o], wi[w]) and torch.equal(gd[o], wd[w])
    # a NaN or infinite query coordinate: an empty row in both forms, an inf radius included
    q2 = q.clone()
    q2[3, 1] = math.nan
    q2[9, 0] = INF
    for c in (E.radius_counts(index, q2, rq), E.point_radius_counts(index, q2, rp)):
        assert c[3] == 0 and c[9] == 0
    c1, c2 = E.point_radius_counts(index, q, rp), E.point_radius_counts(index, q2, rp)
    keep = torch.ones(nq, dtype=torch.bool)
    keep[[3, 9]] = False
    assert torch.equal(c1[keep], c2[keep]) and bool((c1 >= 1).all())  # (point 5 reaches every finite query)


def test_engine_limits_and_errors():
    p, q = DATA["uniform"]()
    index = E.build_index(p)
    nq, n = q.shape[0], p.shape[0]
    rq, rp = torch.full((nq,), 0.15), torch.full((n,), 0.15)
    total = int(K.radius_count_cpu(p, q, E.cut2_of(0.15)).sum())
    for fn, r in ((E.radius_neighbors, rq), (E.point_radius_neighbors, rp)):
        with pytest.raises(ValueError, match=str(total)) as exc:
            fn(index, q, r, max_pairs=total - 1)
        assert str(total - 1) in str(exc.value)
        assert fn(index, q, r, max_pairs=total)[1].shape[0] == total
    bad_q = {"negative": rq.clone(), "nan": rq.clone(), "dtype": rq.double(), "long": torch.full((nq + 1,), 0.1),
             "short": rq[:-1], "2d": rq[:, None], "list": [0.1] * nq}
    bad_q["negative"][7] = -1e-3
    bad_q["nan"][7] = math.nan
    for what, r in bad_q.items():
        if what != "list":  # (a list is not a tensor: the scalar path refuses it its own way)
            with pytest.raises(ValueError):
                E.radius_counts(index, q, r)
            with pytest.raises(ValueError):
                E.radius_neighbors(index, q, r)
            with pytest.raises(ValueError):
                E.radius_query_counts(torch.empty((0, 3)), q, r)
    bad_p = {"negative": rp.clone(), "nan": rp.clone(), "dtype": rp.double(), "long": torch.full((n + 1,), 0.1),
             "short": rp[:-1], "2d": rp[:, None], "list": [0.1] * n}
    bad_p["negative"][7] = -1e-3
    bad_p["nan"][7] = math.nan
    for what, r in bad_p.items():
        for fn in (E.point_radius_counts, E.point_radius_neighbors, E.prepare_point_radii):
            with pytest.raises(ValueError):
                fn(index, r) if fn is E.prepare_point_radii else fn(index, q, r)
    for sqd in (False, True):  # negative squared cutoffs are refused too
        with pytest.raises(ValueError):
            E.radius_counts(index, q, bad_q["negative"], squared=sqd)
    with pytest.raises(ValueError):  # prepared for another index
        E.point_radius_counts(E.build_index(p), q, E.prepare_point_radii(index, rp))
    with pytest.raises(ValueError):
        E.point_radius_counts(index, q.double(), rp)
    # empty points, empty queries
    none = torch.empty((0, 3))
    empty = E.build_index(none)
    no_r = torch.empty(0)
    assert torch.equal(E.radius_counts(empty, q, rq), torch.zeros(nq, dtype=torch.int32))
    assert torch.equal(E.point_radius_counts(empty, q, no_r), torch.zeros(nq, dtype=torch.int32))
    assert torch.equal(E.point_radius_query_counts(none, q, no_r), torch.zeros(nq, dtype=torch.int32))
    for res in (E.radius_neighbors(empty, q, rq), E.radius_query_neighbors(none, q, rq),
                E.point_radius_neighbors(empty, q, no_r), E.point_radius_query_neighbors(none, q, no_r)):
        assert torch.equal(res[0], torch.zeros(nq + 1, dtype=torch.int64))
        assert res[1].shape == (0,) and res[1].dtype == torch.int32 and res[2].shape == (0,)
    with pytest.raises(ValueError):
        E.point_radius_counts(empty, q, rp)
    c = E.radius_counts(index, none, no_r)
    assert c.shape == (0,) and c.dtype == torch.int32 and E.point_radius_counts(index, none, rp).shape == (0,)
    for res in (E.radius_neighbors(index, none, no_r), E.point_radius_neighbors(index, none, rp)):
        assert torch.equal(res[0], torch.zeros(1, dtype=torch.int64)) and res[1].shape == (0,) and res[2].shape == (0,)
    index.qrot = index.pts  # an index in a rotated frame serves its own points only
    for fn, r in ((E.radius_counts, rq), (E.radius_neighbors, rq), (E.point_radius_counts, rp),
                  (E.point_radius_neighbors, rp)):
        with pytest.raises(ValueError):
            fn(index, q, r)


# ------------------------------------------------------------------------------- CLI
def _read(path):
    with open(path, "rb") as f:
        return f.read()


SUFFIXES = (".count", ".offsets", ".ids", ".dist")


@pytest.mark.parametrize("mode", ["--radii", "--point-radii"])
def test_cli_round_trip(tmp_path, capsys, mode):
    p, q = uniform(2000, seed=11), uniform(500, seed=12) * 1.2 - 0.1
    fp, fq, fr = str(tmp_path / "p.float3"), str(tmp_path / "q.float3"), str(tmp_path / "r.float")
    io.write_points(fp, p)
    io.write_points(fq, q)
    gather = mode == "--radii"
    r = radii("loguniform", 500 if gather else 2000, 80)
    r[4] = 0.0
    io.write_array(fr, r)
    if gather:
        counts, lists = E.radius_query_counts(p, q, r), E.radius_query_neighbors(p, q, r)
    else:
        counts, lists = E.point_radius_query_counts(p, q, r), E.point_radius_query_neighbors(p, q, r)
    want = {".count": counts, ".offsets": lists[0], ".ids": lists[1], ".dist": lists[2]}
    pre = str(tmp_path / "rad")
    assert radius_app.main([fp, fq, mode, fr, "-o", pre, "--device", "cpu"]) == 0
    for suf in SUFFIXES:
        assert _read(pre + suf) == want[suf].numpy().tobytes(), suf
    # chunks, and chunks split along their prefix sums: byte-identical files
    largest = int(counts.max())
    assert sum(largest < int(counts[b:b + 64].sum()) for b in range(0, 500, 64)) >= 4  # chunks are split
    pre2 = str(tmp_path / "split")
    assert radius_app.main([fp, fq, mode, fr, "-o", pre2, "--device", "cpu", "--chunk", "64",
                            "--max-pairs", str(largest)]) == 0
    for suf in SUFFIXES:
        assert _read(pre2 + suf) == _read(pre + suf), suf
    # --squared with the squared values: the same files
    fr2, pre3 = str(tmp_path / "r2.float"), str(tmp_path / "squared")
    io.write_array(fr2, cut2_t(r))
    assert radius_app.main([fp, fq, mode, fr2, "--squared", "-o", pre3, "--device", "cpu", "--chunk", "128"]) == 0
    for suf in SUFFIXES:
        assert _read(pre3 + suf) == _read(pre + suf), suf
    capsys.readouterr()
    # rcheck passes, and fails after one id is altered
    assert tools.main(["rcheck", fp, fq, pre, mode, fr, "--samples", "500"]) == 0
    out = capsys.readouterr().out
    assert "sampled counts: 0 mismatches" in out and "sampled rows: 0 mismatches" in out
    assert tools.main(["rcheck", fp, fq, pre, mode, fr2, "--squared", "--samples", "500"]) == 0
    other = "--point-radii" if gather else "--radii"
    assert tools.main(["rcheck", fp, fq, pre, other, fr, "--samples", "500"]) == 1  # 500 values against 2000 rows
    capsys.readouterr()
    first = int((counts > 3).nonzero()[0])
    ids = io.read_array(pre + ".ids", torch.int32)
    ids[int(lists[0][first])] += 1
    io.write_array(pre + ".ids", ids)
    assert tools.main(["rcheck", fp, fq, pre, mode, fr, "--samples", "500"]) == 1
    assert "sampled rows: 1 mismatches" in capsys.readouterr().out


def test_cli_argument_errors(tmp_path, capsys):
    p, q = uniform(100, seed=13), uniform(10, seed=14)
    fp, fq, fr = str(tmp_path / "p.float3"), str(tmp_path / "q.float3"), str(tmp_path / "r.float")
    io.write_points(fp, p)
    io.write_points(fq, q)
    io.write_array(fr, torch.full((10,), 0.1))
    out = ["-o", str(tmp_path / "o"), "--device", "cpu"]
    for bad in ([], ["-r", "0.1", "--radii", fr], ["--radii", fr, "--point-radii", fr],
                ["-r", "0.1", "--point-radii", fr]):
        with pytest.raises(SystemExit):
            radius_app.main([fp, fq, *bad, *out])
        with pytest.raises(SystemExit):
            tools.main(["rcheck", fp, fq, str(tmp_path / "o"), *bad])
    capsys.readouterr()
    # a file of the wrong length: an error that names both lengths, before anything is written
    assert radius_app.main([fp, fq, "--point-radii", fr, *out]) == 1
    err = capsys.readouterr().err
    assert "10 values" in err and "100 rows" in err
    fr3 = str(tmp_path / "r3.float")
    io.write_array(fr3, torch.full((11,), 0.1))
    assert radius_app.main([fp, fq, "--radii", fr3, *out]) == 1
    err = capsys.readouterr().err
    assert "11 values" in err and "10 rows" in err
    assert not os.path.exists(str(tmp_path / "o.count"))
    bad = torch.full((10,), 0.1)
    bad[2] = -1.0
    io.write_array(fr3, bad)
    assert radius_app.main([fp, fq, "--radii", fr3, *out]) == 1
    assert radius_app.main([fp, fq, "--radii", fr, *out]) == 0

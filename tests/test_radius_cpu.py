"""Fixed-radius search on the CPU path: the brute-force oracle K.radius_cpu / radius_count_cpu
against an independent route (the filled prefix of the neighbour-list oracle K.knn_cpu), the
strict comparison on a lattice, radius_counts / radius_neighbors on a CPU index, and the
hipKNN_radius / lsknn_tools rcheck round trip."""
import math
import os
import subprocess

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000

DATA = {
    "uniform": lambda: (uniform(N, seed=3), uniform(200, seed=4) * 1.4 - 0.2),
    # 40 sites, about 75 copies each: rows are runs of equal distances, ordered by row
    "duplicates": lambda: (duplicates(N, seed=5, ndistinct=40), duplicates(N, seed=5, ndistinct=40)[::15].clone()),
    # coordinates j / 15: every d² exact, shells of 6, 12, 8 ... points
    "lattice": lambda: (lattice(15), lattice(15)[::13].clone()),
}


def test_exported():
    assert pkg.radius_counts is E.radius_counts and pkg.radius_neighbors is E.radius_neighbors
    assert pkg.radius_query_counts is E.radius_query_counts
    assert pkg.radius_query_neighbors is E.radius_query_neighbors
    assert pkg.radius_self_neighbors is E.radius_self_neighbors
    assert K.RADIUS_LDS_ROW & (K.RADIUS_LDS_ROW - 1) == 0  # a power of two


def rows(offsets, *arrays):
    return [tuple(a[offsets[i]:offsets[i + 1]] for a in arrays) for i in range(offsets.shape[0] - 1)]


@pytest.mark.parametrize("r", [0.0, 0.01, 0.08, 0.3, math.inf])
@pytest.mark.parametrize("name", sorted(DATA))
def test_oracle_against_the_neighbour_list_oracle(name, r):
    p, q = DATA[name]()
    cut2 = E.cut2_of(r)
    counts = K.radius_count_cpu(p, q, cut2)
    offsets, idx, d2 = K.radius_cpu(p, q, cut2)
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert offsets[0] == 0 and torch.equal(offsets[1:], torch.cumsum(counts.long(), 0))
    assert idx.shape[0] == d2.shape[0] == int(offsets[-1])
    kmax = max(1, int(counts.max()))
    ki, kd = K.knn_cpu(p, q, kmax, cut2)
    assert torch.equal((ki != -1).sum(1).int(), counts)
    for i, (ri, rd) in enumerate(rows(offsets, idx, d2)):
        m = int(counts[i])
        assert torch.equal(ki[i, :m], ri), f"{name} r={r}: ids of query {i}"
        assert torch.equal(kd[i, :m].view(torch.int32), rd.view(torch.int32)), f"{name} r={r}: d² of query {i}"
    if r == 0.0:
        assert int(counts.sum()) == 0
    if math.isinf(r):
        assert bool((counts == p.shape[0]).all())


def interior(m):
    """Rows of lattice(m) that are not on its surface."""
    j = torch.arange(m ** 3)
    x, y, z = j // (m * m), (j // m) % m, j % m
    return ((x > 0) & (x < m - 1) & (y > 0) & (y < m - 1) & (z > 0) & (z < m - 1)).nonzero().flatten()


def test_lattice_strictness():
    """Spacing 1/32 and every d² exact: r = 1/32 excludes the six face neighbours (d² == cut2),
    the next float above it includes them."""
    p = lattice(32)
    q = p[interior(32)[::29]].contiguous()
    step = np.float32(1.0 / 32.0)
    assert bool((K.radius_count_cpu(p, q, E.cut2_of(float(step))) == 1).all())
    above = float(np.nextafter(step, np.float32(1.0)))
    assert bool((K.radius_count_cpu(p, q, E.cut2_of(above)) == 7).all())
    assert bool((K.radius_count_cpu(p, q, E.cut2_of(0.0)) == 0).all())
    assert bool((K.radius_count_cpu(p, q, E.cut2_of(math.inf)) == p.shape[0]).all())
    index = E.build_index(p)
    assert bool((E.radius_counts(index, q, float(step)) == 1).all())
    assert bool((E.radius_counts(index, q, above) == 7).all())
    offsets, idx, dist = E.radius_neighbors(index, q, above)
    for ri, rd in rows(offsets, idx, dist):
        assert rd[0] == 0 and bool((rd[1:] == step).all()) and bool((ri[1:-1] < ri[2:]).all())


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def test_engine_on_a_cpu_index():
    p, q = DATA["uniform"]()
    index = E.build_index(p)
    r = 0.15
    ro, ri, rd2 = K.radius_cpu(p, q, E.cut2_of(r))
    counts = E.radius_counts(index, q, r)
    assert counts.dtype == torch.int32 and torch.equal(counts, K.radius_count_cpu(p, q, E.cut2_of(r)))
    offsets, idx, dist = E.radius_neighbors(index, q, r)
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert torch.equal(offsets, ro) and torch.equal(idx, ri) and torch.equal(dist, final(rd2))
    # sort=False: the same rows as sets
    uo, ui, ud = E.radius_neighbors(index, q, r, sort=False)
    assert torch.equal(uo, ro)
    for (gi, gd), (wi, wd) in zip(rows(uo, ui, ud), rows(ro, ri, final(rd2))):
        o, w = torch.argsort(gi.long()), torch.argsort(wi.long())
        assert torch.equal(gi[o], wi[w]) and torch.equal(gd[o], wd[w])
    # convenience forms
    assert torch.equal(E.radius_query_counts(p, q, r), counts)
    for got, ref in zip(E.radius_query_neighbors(p, q, r), (ro, ri, final(rd2))):
        assert torch.equal(got, ref)
    so, si, sd = E.radius_self_neighbors(p, 0.05)
    assert bool((sd[so[:-1]] == 0).all()) and torch.equal(si[so[:-1]], torch.arange(N, dtype=torch.int32))
    for got, ref in zip((so, si, sd), E.radius_query_neighbors(p, p, 0.05)):
        assert torch.equal(got, ref)


def test_engine_limits_and_errors():
    p, q = DATA["uniform"]()
    index = E.build_index(p)
    total = int(K.radius_count_cpu(p, q, E.cut2_of(0.15)).sum())
    with pytest.raises(ValueError, match=str(total)) as exc:
        E.radius_neighbors(index, q, 0.15, max_pairs=total - 1)
    assert str(total - 1) in str(exc.value)
    assert E.radius_neighbors(index, q, 0.15, max_pairs=total)[1].shape[0] == total
    for bad in (-1.0, -0.0001, math.nan):
        with pytest.raises(ValueError):
            E.radius_counts(index, q, bad)
        with pytest.raises(ValueError):
            E.radius_neighbors(index, q, bad)
        with pytest.raises(ValueError):
            E.radius_query_counts(torch.empty((0, 3)), q, bad)
    with pytest.raises(ValueError):
        E.radius_counts(index, q.double(), 0.1)
    with pytest.raises(ValueError):
        E.radius_neighbors(index, q[:, :2], 0.1)
    # a NaN or infinite coordinate: an empty row, the others unchanged
    q2 = q.clone()
    q2[5, 1] = math.nan
    q2[9, 0] = math.inf
    o1, i1, d1 = E.radius_neighbors(index, q, 0.15)
    o2, i2, d2 = E.radius_neighbors(index, q2, 0.15)
    c2 = E.radius_counts(index, q2, 0.15)
    assert c2[5] == 0 and c2[9] == 0 and torch.equal(c2, (o2[1:] - o2[:-1]).int())
    r1, r2 = rows(o1, i1, d1), rows(o2, i2, d2)
    for j in range(q.shape[0]):
        if j in (5, 9):
            assert r2[j][0].numel() == 0
        else:
            assert torch.equal(r1[j][0], r2[j][0]) and torch.equal(r1[j][1], r2[j][1])
    # empty points, empty queries
    empty = E.build_index(torch.empty((0, 3)))
    assert torch.equal(E.radius_counts(empty, q, 0.1), torch.zeros(q.shape[0], dtype=torch.int32))
    for res in (E.radius_neighbors(empty, q, 0.1), E.radius_query_neighbors(torch.empty((0, 3)), q, 0.1)):
        assert torch.equal(res[0], torch.zeros(q.shape[0] + 1, dtype=torch.int64))
        assert res[1].shape == (0,) and res[1].dtype == torch.int32 and res[2].shape == (0,)
    assert torch.equal(E.radius_query_counts(torch.empty((0, 3)), q, 0.1), torch.zeros(q.shape[0], dtype=torch.int32))
    none = torch.empty((0, 3))
    assert E.radius_counts(index, none, 0.1).shape == (0,) and E.radius_counts(index, none, 0.1).dtype == torch.int32
    o, i, d = E.radius_neighbors(index, none, 0.1)
    assert torch.equal(o, torch.zeros(1, dtype=torch.int64)) and i.shape == (0,) and d.shape == (0,)
    index.qrot = index.pts  # an index in a rotated frame serves its own points only
    with pytest.raises(ValueError):
        E.radius_counts(index, q, 0.1)
    with pytest.raises(ValueError):
        E.radius_neighbors(index, q, 0.1)


# ------------------------------------------------------------------------------- CLI
def _files(tmp_path, n=2000, nq=500):
    p, q = uniform(n, seed=11), uniform(nq, seed=12) * 1.2 - 0.1
    fp, fq = str(tmp_path / "p.float3"), str(tmp_path / "q.float3")
    io.write_points(fp, p)
    io.write_points(fq, q)
    return p, q, fp, fq


def _read(path):
    with open(path, "rb") as f:
        return f.read()


SUFFIXES = (".count", ".offsets", ".ids", ".dist")


def test_cli_round_trip(tmp_path, capsys):
    p, q, fp, fq = _files(tmp_path)
    r = 0.12
    pre = str(tmp_path / "rad")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK",
                                                             "PMI_SIZE", "OMPI_COMM_WORLD_RANK",
                                                             "OMPI_COMM_WORLD_SIZE", "PMIX_RANK")}
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_radius"), fp, fq, "-r", str(r), "-o", pre,
                           "--device", "cpu"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr
    offsets, idx, dist = E.radius_query_neighbors(p, q, r)
    counts = E.radius_query_counts(p, q, r)
    want = {".count": counts, ".offsets": offsets, ".ids": idx, ".dist": dist}
    for suf in SUFFIXES:
        assert _read(pre + suf) == want[suf].numpy().tobytes(), suf
    # chunks, and chunks split along their prefix sums: byte-identical files
    largest = int(counts.max())
    chunk_totals = [int(counts[b:b + 64].sum()) for b in range(0, q.shape[0], 64)]
    assert largest < min(chunk_totals)  # every chunk is split, no single query is refused
    pre2 = str(tmp_path / "split")
    assert radius_app.main([fp, fq, "-r", str(r), "-o", pre2, "--device", "cpu", "--chunk", "64",
                            "--max-pairs", str(largest)]) == 0
    for suf in SUFFIXES:
        assert _read(pre2 + suf) == _read(pre + suf), suf
    # --counts-only writes the counts and nothing else
    sub = tmp_path / "counts"
    sub.mkdir()
    assert radius_app.main([fp, fq, "-r", str(r), "-o", str(sub / "c"), "--device", "cpu", "--counts-only"]) == 0
    assert sorted(os.listdir(sub)) == ["c.count"]
    assert _read(str(sub / "c.count")) == _read(pre + ".count")
    # --unsorted: the same rows as sets (rcheck --unsorted)
    pre3 = str(tmp_path / "unsorted")
    assert radius_app.main([fp, fq, "-r", str(r), "-o", pre3, "--device", "cpu", "--unsorted"]) == 0
    assert tools.main(["rcheck", fp, fq, pre3, "-r", str(r), "--samples", "500", "--unsorted"]) == 0
    capsys.readouterr()
    # a single query above --max-pairs is an error that names it
    first = int((counts > 3).nonzero()[0])
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_radius"), fp, fq, "-r", str(r), "-o",
                           str(tmp_path / "small"), "--device", "cpu", "--max-pairs", "3"], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 1 and f"query {first} " in proc.stderr
    # rcheck passes, and fails after one id is altered
    assert tools.main(["rcheck", fp, fq, pre, "-r", str(r), "--samples", "500"]) == 0
    assert "sampled rows: 0 mismatches" in capsys.readouterr().out
    assert tools.main(["rcheck", fp, fq, str(sub / "c"), "-r", str(r), "--counts-only"]) == 0
    capsys.readouterr()
    ids = io.read_array(pre + ".ids", torch.int32)
    ids[int(offsets[first])] += 1
    io.write_array(pre + ".ids", ids)
    assert tools.main(["rcheck", fp, fq, pre, "-r", str(r), "--samples", "500"]) == 1
    assert "sampled rows: 1 mismatches" in capsys.readouterr().out
    # and after one count is altered
    cnt = io.read_array(pre + ".count", torch.int32)
    cnt[first] += 1
    io.write_array(pre + ".count", cnt)
    assert tools.main(["rcheck", fp, fq, pre, "-r", str(r), "--samples", "500", "--counts-only"]) == 1


def test_cli_refuses_a_bad_radius(tmp_path):
    _, _, fp, fq = _files(tmp_path, 100, 10)
    for bad in ("-1", "nan"):
        with pytest.raises(SystemExit):
            radius_app.main([fp, fq, "-r", bad, "-o", str(tmp_path / "o"), "--device", "cpu"])

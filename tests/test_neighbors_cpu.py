"""Neighbour lists on the CPU path: the brute-force oracle K.knn_cpu against an independent
torch computation (ids, order, tie rule, fill), query_neighbors on a CPU index, and the
hipKNN_query --neighbors / lsknn_tools check --neighbors round trip."""
import math
import os
import subprocess

import pytest
import torch

import mpi_cuda_largescaleknn_amd as pkg
from mpi_cuda_largescaleknn_amd.apps import query as query_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import duplicates, lattice, uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_lists(p, q, k, cut2=math.inf):
    """Independent lists in torch: the canonical d² = fma(dz, dz, fma(dy, dy, dx * dx)) of
    float32 differences, each step's exact value formed in float64 and rounded to float32
    (a product of two float32 is exact in float64), then one sort by (d² bits, row)."""
    d = (q[:, None, :] - p[None, :, :]).double()  # (the float32 differences, exactly)
    t = (d[..., 0] * d[..., 0]).float()
    t = (d[..., 1] * d[..., 1] + t.double()).float()
    d2 = (d[..., 2] * d[..., 2] + t.double()).float()
    n, nq = p.shape[0], q.shape[0]
    ok = d2 < cut2
    key = (d2.view(torch.int32).long() << 32) | torch.arange(n, dtype=torch.int64)[None, :]
    key = torch.where(ok, key, torch.full_like(key, torch.iinfo(torch.int64).max))
    key = torch.sort(key, dim=1).values[:, :k]
    idx = torch.full((nq, k), -1, dtype=torch.int32)
    out = torch.full((nq, k), cut2, dtype=torch.float32)
    m = key.shape[1]
    have = key != torch.iinfo(torch.int64).max
    idx[:, :m] = torch.where(have, (key & 0xFFFFFFFF).to(torch.int32), idx[:, :m])
    out[:, :m] = torch.where(have, (key >> 32).to(torch.int32).view(torch.float32), out[:, :m])
    return idx, out


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def test_exported():
    assert pkg.query_neighbors is E.query_neighbors and pkg.knn_neighbors is E.knn_neighbors
    assert pkg.knn_query_neighbors is E.knn_query_neighbors
    assert K.NEIGHBORS_MAX_K == 1024


DATA = {
    "uniform": lambda: (uniform(2000, seed=3), uniform(300, seed=4) * 1.4 - 0.2),
    # 40 sites, about 50 copies each: every list is cut inside a run of equal distances
    "duplicates": lambda: (duplicates(2000, seed=5, ndistinct=40), duplicates(2000, seed=5, ndistinct=40)[::7].clone()),
    # coordinates j / 8: every d² exact, ties of 6, 12, 8 ... at the lattice distances
    "lattice": lambda: (lattice(8), lattice(8)[::3].clone()),
}


@pytest.mark.parametrize("name", sorted(DATA))
def test_oracle_against_torch(name):
    p, q = DATA[name]()
    for k, r in ((1, math.inf), (5, math.inf), (7, math.inf), (16, math.inf), (100, math.inf), (16, 0.2),
                 (100, 0.13)):
        cut2 = E.cut2_of(r)
        idx, d2 = K.knn_cpu(p, q, k, cut2)
        ref_i, ref_d = torch_lists(p, q, k, cut2)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (q.shape[0], k)
        assert torch.equal(idx, ref_i), (name, k, r)
        assert torch.equal(d2, ref_d), (name, k, r)
        # ascending by (d², row); filled slots first
        key = (d2.view(torch.int32).long() << 32) | (idx.long() & 0xFFFFFFFF)
        assert bool((key[:, 1:] > key[:, :-1]).logical_or(idx[:, 1:] < 0).all())
        if r == 0.2 and name == "uniform":  # that cutoff leaves some lists short (queries off the box) and some not
            short = (idx[:, -1] < 0)
            assert 0 < int(short.sum()) < q.shape[0]
            assert bool((d2[idx < 0] == cut2).all())


def test_tie_rule_lowest_rows():
    """Lattice sites queried at a site: 1 point at 0, then 6 at 1/8 (k = 5 cuts that tie, k = 7
    fills it exactly); duplicates: the lowest rows of the nearest site's copies win."""
    p = lattice(8)
    centre = p[(p == 0.5).all(dim=1)]
    for k in (5, 7):
        idx, d2 = K.knn_cpu(p, centre, k, math.inf)
        at = torch.nonzero(((p - centre) ** 2).sum(1) == 1.0 / 64).flatten().to(torch.int32)
        assert at.numel() == 6 and int(idx[0, 0]) == int(torch.nonzero((p == 0.5).all(dim=1))[0])
        assert torch.equal(idx[0, 1:], at[:k - 1])  # (nonzero lists rows in ascending order)
        assert bool((d2[0, 1:] == 1.0 / 64).all())
    p = duplicates(2000, seed=5, ndistinct=40)
    idx, d2 = K.knn_cpu(p, p[:50], 10, math.inf)
    for i in range(50):
        same = torch.nonzero((p == p[i]).all(dim=1)).flatten()
        assert same.numel() >= 10 and torch.equal(idx[i].long(), same[:10]) and bool((d2[i] == 0).all())


@pytest.mark.parametrize("n", [1, 5, 64])
def test_fill_with_k_above_n(n):
    p, q = uniform(n, seed=n), uniform(9, seed=50 + n)
    for k in (n, n + 1, n + 30):
        idx, d2 = K.knn_cpu(p, q, k, math.inf)
        assert torch.equal(torch.sort(idx[:, :n].long(), dim=1).values, torch.arange(n).expand(9, n))
        assert bool((idx[:, n:] == -1).all()) and bool(torch.isinf(d2[:, n:]).all())
        ref_i, ref_d = torch_lists(p, q, k)
        assert torch.equal(idx, ref_i) and torch.equal(d2, ref_d)
    idx, d2 = K.knn_cpu(p[:0], q, 3, E.cut2_of(0.5))
    assert bool((idx == -1).all()) and bool((d2 == E.cut2_of(0.5)).all())
    assert K.knn_cpu(p, q[:0], 3, math.inf)[0].shape == (0, 3)


def test_nan_query_has_no_neighbours():
    p, q = uniform(100, seed=1), uniform(4, seed=2)
    q[2, 1] = math.nan
    idx, d2 = K.knn_cpu(p, q, 3, math.inf)
    assert bool((idx[2] == -1).all()) and bool(torch.isinf(d2[2]).all()) and bool((idx[[0, 1, 3]] >= 0).all())


@pytest.mark.parametrize("name", sorted(DATA))
def test_last_column_is_the_kth_distance(name):
    p, q = DATA[name]()
    for k, r in ((1, math.inf), (7, math.inf), (100, math.inf), (100, 0.13)):
        d2 = K.knn_cpu(p, q, k, E.cut2_of(r))[1]
        for method in ("brute", "kdtree"):
            assert torch.equal(d2[:, k - 1], K.kth_cpu(p, q, k, E.cut2_of(r), method=method)), (name, k, r, method)


# ------------------------------------------------------------------------ engine, CPU index
def test_query_neighbors_on_a_cpu_index():
    p = uniform(3000, seed=7)
    index = E.build_index(p, grid=True)
    assert not torch.equal(index.perm.long(), torch.arange(3000))  # ids are input rows, not sorted positions
    for k, r in ((1, math.inf), (16, math.inf), (100, 0.1)):
        cfg = E.KnnConfig(k=k, max_radius=r)
        q = uniform(400, seed=k) * 1.4 - 0.2
        idx, dist = E.query_neighbors(index, q, cfg)
        ref_i, ref_d2 = K.knn_cpu(p, q, k, cfg.cut2)
        assert torch.equal(idx, ref_i) and torch.equal(dist, final(ref_d2))
        assert torch.equal(dist[:, k - 1], E.query_points(index, q, cfg))
    oi, od = torch.empty((400, 100), dtype=torch.int32), torch.empty((400, 100))
    got = E.query_neighbors(index, q, cfg, out_idx=oi, out_dist=od)
    assert got[0] is oi and got[1] is od and torch.equal(oi, ref_i)
    idx, dist = E.query_neighbors(index, q[:0], cfg)
    assert idx.shape == dist.shape == (0, 100) and idx.dtype == torch.int32 and dist.dtype == torch.float32


def test_wrappers_limits_and_errors():
    p, q = uniform(500, seed=1), uniform(60, seed=2)
    idx, dist = E.knn_query_neighbors(p, q, 8, max_radius=0.3)
    ref_i, ref_d2 = K.knn_cpu(p, q, 8, E.cut2_of(0.3))
    assert torch.equal(idx, ref_i) and torch.equal(dist, final(ref_d2))
    si, sd = E.knn_neighbors(p, 8)
    qi, qd = E.knn_query_neighbors(p, p, 8)
    assert torch.equal(si, qi) and torch.equal(sd, qd)
    assert torch.equal(si[:, 0].long(), torch.arange(500)) and bool((sd[:, 0] == 0).all())
    # an empty point set: every slot unfilled
    idx, dist = E.knn_query_neighbors(p[:0], q, 3, max_radius=0.5)
    assert bool((idx == -1).all()) and bool((dist == final(torch.tensor([E.cut2_of(0.5)]))[0]).all())
    assert bool(torch.isinf(E.knn_query_neighbors(p[:0], q, 3)[1]).all())
    index = E.build_index(p, grid=True)
    with pytest.raises(ValueError, match="query_points"):
        E.query_neighbors(index, q, E.KnnConfig(k=K.NEIGHBORS_MAX_K + 1))
    with pytest.raises(ValueError, match="knn_query_distances"):
        E.knn_query_neighbors(p, q, K.NEIGHBORS_MAX_K + 1)
    with pytest.raises(ValueError):
        E.query_neighbors(index, q.double(), E.KnnConfig(k=1))
    with pytest.raises(ValueError):
        E.query_neighbors(index, q, E.KnnConfig(k=2), out_idx=torch.empty((60, 3), dtype=torch.int32))
    index.qrot = index.pts  # an index in a rotated frame serves its own points only
    with pytest.raises(ValueError):
        E.query_neighbors(index, q, E.KnnConfig(k=1))


# ------------------------------------------------------------------------------- CLI
def _files(tmp_path, n=3000, nq=2500):
    p, q = uniform(n, seed=11), uniform(nq, seed=12) * 1.2 - 0.1
    fp, fq = str(tmp_path / "p.float3"), str(tmp_path / "q.float3")
    io.write_points(fp, p)
    io.write_points(fq, q)
    return p, q, fp, fq


def test_cli_neighbors_round_trip(tmp_path, capsys):
    p, q, fp, fq = _files(tmp_path)
    out, pre = str(tmp_path / "d.float"), str(tmp_path / "nb")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK",
                                                             "PMI_SIZE", "OMPI_COMM_WORLD_RANK",
                                                             "OMPI_COMM_WORLD_SIZE", "PMIX_RANK")}
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_query"), fp, fq, "-o", out, "-k", "16", "-r", "0.3",
                           "--device", "cpu", "--chunk", "1000", "--neighbors", pre], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr
    ref_i, ref_d2 = K.knn_cpu(p, q, 16, E.cut2_of(0.3))
    with open(pre + ".ids", "rb") as f:
        assert f.read() == ref_i.numpy().tobytes()
    with open(pre + ".dist", "rb") as f:
        assert f.read() == final(ref_d2).numpy().tobytes()
    with open(out, "rb") as f:  # the -o file is unchanged by the flag: the k-th distances
        kth_bytes = f.read()
    assert kth_bytes == final(ref_d2)[:, 15].contiguous().numpy().tobytes()
    chk = ["check", fp, out, "-k", "16", "-r", "0.3", "--queries", fq, "--samples", "500"]
    assert tools.main(chk + ["--neighbors", pre]) == 0
    assert "sampled neighbour lists: 0 mismatches" in capsys.readouterr().out
    # one id altered (a row the check samples: all of them with --samples >= nq)
    ids = io.read_rows(pre + ".ids", 16, torch.int32)
    ids[1234, 3] = ids[1234, 3] + 1
    io.write_rows(pre + ".ids", ids)
    assert tools.main(["check", fp, out, "-k", "16", "-r", "0.3", "--queries", fq, "--samples", "2500",
                       "--neighbors", pre]) == 1
    assert "sampled neighbour lists: 1 mismatches" in capsys.readouterr().out
    assert tools.main(["check", fp, out, "-k", "16", "-r", "0.3", "--queries", fq, "--samples", "2500"]) == 0
    # without the flag (in process): the same -o bytes and no further file
    sub = tmp_path / "plain"
    sub.mkdir()
    assert query_app.main([fp, fq, "-o", str(sub / "d.float"), "-k", "16", "-r", "0.3", "--device", "cpu"]) == 0
    assert sorted(os.listdir(sub)) == ["d.float"]
    with open(sub / "d.float", "rb") as f:
        assert f.read() == kth_bytes


def test_cli_neighbors_refuses_large_k(tmp_path):
    _, _, fp, fq = _files(tmp_path, 100, 10)
    with pytest.raises(SystemExit):
        query_app.main([fp, fq, "-o", str(tmp_path / "o.float"), "-k", "1025", "--device", "cpu", "--neighbors",
                        str(tmp_path / "nb")])
    assert query_app.main([fp, fq, "-o", str(tmp_path / "o.float"), "-k", "1025", "--device", "cpu"]) == 0

"""Cross-set queries on the CPU path: k-th-neighbour distance from query points to a point
set (knn_query_distances / query_points, hipKNN_query, lsknn_tools check --queries), every
value bit for bit against the brute-force oracle."""
import math
import os
import subprocess
import sys

import pytest
import torch

import mpi_cuda_largescaleknn_amd as pkg
from mpi_cuda_largescaleknn_amd.apps import query as query_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(points, queries, k, r=math.inf):
    return K.finalize_distances(K.kth_cpu(points, queries, k, E.cut2_of(r), method="brute"))


def test_exported():
    assert pkg.knn_query_distances is E.knn_query_distances and pkg.query_points is E.query_points


@pytest.mark.parametrize("n", [1, 64, 130, 3000])
@pytest.mark.parametrize("nq", [0, 1, 65, 1000])
def test_matches_brute_force(n, nq):
    p = uniform(n, seed=n)
    q = uniform(nq, seed=1000 + nq) * 1.5 - 0.25  # some queries outside the points' box
    for k in (1, 16, 100):
        got = E.knn_query_distances(p, q, k)
        assert got.shape == (nq,) and got.dtype == torch.float32
        assert torch.equal(got, brute(p, q, k)), (n, nq, k)
    got = E.knn_query_distances(p, q, 16, max_radius=0.2)
    ref = brute(p, q, 16, 0.2)
    assert torch.equal(got, ref)
    if n >= 3000 and nq >= 1000:  # the cutoff decides some answers and not others
        cut = float(K.finalize_distances(torch.tensor([E.cut2_of(0.2)]))[0])
        assert 0 < int((ref == cut).sum()) < nq


def test_only_points_are_candidates():
    """A query on a point finds it at 0; other queries never count (Q concatenated to P
    would)."""
    p = uniform(500, seed=1)
    q = torch.cat([p[:10], p[:10], uniform(10, seed=2)])
    got = E.knn_query_distances(p, q, 1)
    assert bool((got[:20] == 0).all()) and bool((got[20:] > 0).all())
    assert torch.equal(E.knn_query_distances(p, q, 2), brute(p, q, 2))


def test_queries_equal_points_is_the_self_query():
    p = uniform(3000, seed=5)
    for k in (1, 16, 100):
        assert torch.equal(E.knn_query_distances(p, p.clone(), k), E.knn_distances(p, k))


def test_query_points_reuses_an_index_and_checks_its_input():
    p = uniform(2000, seed=7)
    index = E.build_index(p, grid=True)
    cfg = E.KnnConfig(k=8, max_radius=0.3)
    for seed in (1, 2, 3):
        q = uniform(300, seed=seed) * 2.0 - 0.5
        assert torch.equal(E.query_points(index, q, cfg), brute(p, q, 8, 0.3))
    out = torch.empty(300)
    assert E.query_points(index, q, cfg, out=out) is out and torch.equal(out, brute(p, q, 8, 0.3))
    with pytest.raises(ValueError):
        E.query_points(index, q.double(), cfg)
    with pytest.raises(ValueError):
        E.query_points(index, q[:, :2], cfg)
    index.qrot = index.pts  # an index in a rotated frame serves its own points only
    with pytest.raises(ValueError):
        E.query_points(index, q, cfg)


def test_k_above_n_and_non_finite_queries():
    p = uniform(50, seed=3)
    q = uniform(20, seed=4)
    assert bool(torch.isinf(E.knn_query_distances(p, q, 51)).all())
    assert torch.equal(E.knn_query_distances(p, q, 51, max_radius=0.5), brute(p, q, 51, 0.5))
    q[3, 1] = math.nan
    q[5, 0] = math.inf
    got, ref = E.knn_query_distances(p, q, 4), brute(p, q, 4)
    ok = torch.isfinite(q).all(dim=1)
    assert torch.equal(got[ok], ref[ok])
    assert E.knn_query_distances(torch.empty((0, 3)), uniform(5), 1).shape == (5,)


def test_locate_groups_cpu():
    """The CPU form of the group location: last bucket whose first key <= the median key."""
    bkeys = torch.tensor([0, 10, 10, 20, 50], dtype=torch.int32)
    qkeys = torch.sort(torch.randint(0, 60, (200,), generator=torch.Generator().manual_seed(0))).values.to(torch.int32)
    got = K.locate_groups(qkeys, 200, bkeys).tolist()
    for g, b in enumerate(got):
        med = int(qkeys[g * 64 + min(64, 200 - g * 64) // 2])
        want = max([i for i, v in enumerate(bkeys.tolist()) if v <= med], default=0)
        assert b == want
    assert K.locate_groups(qkeys[:0], 0, bkeys).shape == (0,)


# ------------------------------------------------------------------------------- CLI
def _files(tmp_path, n=3000, nq=2500):
    p, q = uniform(n, seed=11), uniform(nq, seed=12) * 1.2 - 0.1
    fp, fq = str(tmp_path / "p.float3"), str(tmp_path / "q.float3")
    io.write_points(fp, p)
    io.write_points(fq, q)
    return p, q, fp, fq


def _run_cli(args, env_extra=None):
    env = dict(os.environ)
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "OMPI_COMM_WORLD_RANK",
              "OMPI_COMM_WORLD_SIZE", "PMIX_RANK"):
        env.pop(v, None)
    env.update(env_extra or {})
    return subprocess.run([os.path.join(ROOT, "bin", "hipKNN_query"), *args], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)


def test_cli_bytes_equal_the_oracle_and_chunks_agree(tmp_path):
    p, q, fp, fq = _files(tmp_path)
    one, chunked = str(tmp_path / "one.float"), str(tmp_path / "chunked.float")
    proc = _run_cli([fp, fq, "-o", one, "-k", "16", "-r", "0.3", "--device", "cpu", "--stats",
                     str(tmp_path / "s.json"), "-v"])
    assert proc.returncode == 0, proc.stderr
    ref = brute(p, q, 16, 0.3)
    with open(one, "rb") as f:
        blob = f.read()
    assert blob == ref.numpy().tobytes()
    assert os.path.exists(tmp_path / "s.json")
    # in process (no second interpreter start): 2500 queries in chunks of 1000
    assert query_app.main([fp, fq, "-o", chunked, "-k", "16", "-r", "0.3", "--device", "cpu", "--chunk", "1000"]) == 0
    with open(chunked, "rb") as f:
        assert f.read() == blob


def test_cli_refuses_several_ranks(tmp_path):
    _, _, fp, fq = _files(tmp_path, 100, 10)
    proc = _run_cli([fp, fq, "-o", str(tmp_path / "o.float"), "-k", "1", "--device", "cpu"],
                    {"WORLD_SIZE": "2", "RANK": "0"})
    assert proc.returncode == 1
    assert len(proc.stderr.strip().splitlines()) == 1 and "one process" in proc.stderr
    assert not os.path.exists(tmp_path / "o.float")


def test_tools_check_queries(tmp_path, capsys):
    p, q, fp, fq = _files(tmp_path, 2000, 700)
    good, bad = str(tmp_path / "good.float"), str(tmp_path / "bad.float")
    d = brute(p, q, 8)
    io.write_floats(good, d)
    assert tools.main(["check", fp, good, "-k", "8", "--queries", fq]) == 0
    d[123] = d[123] * 1.0001
    io.write_floats(bad, d)
    assert tools.main(["check", fp, bad, "-k", "8", "--queries", fq]) == 1
    assert "1 mismatches" in capsys.readouterr().out
    # without --queries the file is taken for the points' own distances: wrong size here
    assert tools.main(["check", fp, good, "-k", "8"]) == 1

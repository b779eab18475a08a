"""Density clustering on the CPU path: the brute-force oracle K.cluster_cpu against an
independent transcription of the definition (a numpy union-find over the sorted rows of
K.radius_cpu), hand-made cases, the strict comparison, the edge inputs, compact_labels,
scikit-learn's DBSCAN where it is installed, and the hipKNN_cluster / lsknn_tools ccheck round
trip."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import mpi_cuda_largescaleknn_amd as pkg
from mpi_cuda_largescaleknn_amd.apps import cluster as cluster_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2000
EPS = 0.9 * N ** (-1.0 / 3.0)


def transcription(p, cut2, min_pts):
    """The definition, from the sorted fixed-radius rows: (labels, core) as numpy arrays."""
    off, idx, _ = (t.numpy() for t in K.radius_cpu(p, p, cut2))
    n = p.shape[0]
    core = np.diff(off) >= min_pts
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i in np.nonzero(core)[0]:
        for j in idx[off[i]:off[i + 1]]:
            if core[j]:
                a, b = find(i), find(j)
                parent[max(a, b)] = min(a, b)
    smallest = {}
    for i in np.nonzero(core)[0]:  # ascending: the first row seen is the smallest
        smallest.setdefault(find(i), i)
    labels = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if core[i]:
            labels[i] = smallest[find(i)]
    for i in np.nonzero(~core)[0]:
        first = [j for j in idx[off[i]:off[i + 1]] if core[j]][:1]  # rows ascend by (d² bits, row)
        labels[i] = labels[first[0]] if first else (i if min_pts == 1 else -1)
    return labels, core


def test_exported():
    assert pkg.cluster_labels is E.cluster_labels and pkg.cluster_points is E.cluster_points
    assert pkg.compact_labels is E.compact_labels


@pytest.mark.parametrize("min_pts", [1, 3, 5])
def test_oracle_against_transcription(min_pts):
    p = uniform(N, seed=21)
    cut2 = E.cut2_of(EPS)
    labels, core = K.cluster_cpu(p, cut2, min_pts)
    want_l, want_c = transcription(p, cut2, min_pts)
    assert labels.dtype == torch.int32 and core.dtype == torch.bool
    assert np.array_equal(core.numpy(), want_c)
    assert np.array_equal(labels.numpy(), want_l)
    # the regime is not trivial: clusters of several points, and for min_pts > 1 core, border and noise
    nclusters = E.compact_labels(labels)[1]
    assert 1 < nclusters < int(core.sum())
    if min_pts > 1:
        assert bool((~core & (labels >= 0)).any()) and bool((labels < 0).any())
    else:
        assert bool(core.all()) and bool((labels >= 0).all())
    # the engine on a CPU index, and from the points
    got = E.cluster_labels(E.build_index(p), EPS, min_pts)
    assert torch.equal(got[0], labels) and torch.equal(got[1], core)
    got = E.cluster_points(p, EPS, min_pts)
    assert torch.equal(got[0], labels) and torch.equal(got[1], core)


def test_two_triples_and_a_far_point():
    p = torch.tensor([[0.0, 0, 0], [10.0, 0, 0], [0.3, 0, 0], [10.0, 0.3, 0], [0, 0.3, 0], [10.0, 0, 0.3],
                      [50.0, 50.0, 50.0]])
    labels, core = E.cluster_points(p, 1.0, 3)
    assert labels.tolist() == [0, 1, 0, 1, 0, 1, -1]
    assert core.tolist() == [True] * 6 + [False]
    labels, core = E.cluster_points(p, 1.0, 1)  # friends-of-friends: the far point is its own group
    assert labels.tolist() == [0, 1, 0, 1, 0, 1, 6] and bool(core.all())


def test_border_tie_goes_to_the_lower_row():
    # rows 3 (cluster A, label 0) and 1 (cluster C, label 1) are both at d² = 1 exactly from
    # the border point, row 8: the lower row wins, not the lower label
    a = [[-1.5, 0, 0], [-1.0, 0, 0], [-1.5, 0.5, 0], [-1.5, -0.5, 0]]
    c = [[1.0, 0, 0], [1.5, 0, 0], [1.5, 0.5, 0], [1.5, -0.5, 0]]
    p = torch.tensor([a[0], c[0], a[2], a[1], a[3], c[1], c[2], c[3], [0.0, 0, 0]])
    labels, core = E.cluster_points(p, 1.2, 4)
    assert core.tolist() == [True] * 8 + [False]
    assert labels.tolist() == [0, 1, 0, 0, 0, 1, 1, 1, 1]
    q = p.clone()  # the two tied cores exchanged: now A's is the lower row
    q[[1, 3]] = p[[3, 1]]
    labels, core = E.cluster_points(q, 1.2, 4)
    assert labels.tolist() == [0, 0, 0, 3, 0, 3, 3, 3, 0]


def test_chain_with_one_core():
    p = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    labels, core = E.cluster_points(p, 1.5, 3)
    assert core.tolist() == [False, True, False] and labels.tolist() == [1, 1, 1]
    labels, core = E.cluster_points(p, 1.5, 4)
    assert core.tolist() == [False] * 3 and labels.tolist() == [-1] * 3


def pair_d2(p, i, j):
    """The oracle's own dist2 of rows i and j."""
    off, idx, d2 = K.radius_cpu(p, p[i:i + 1], math.inf)
    return float(d2[idx.tolist().index(j)])


def test_strict_comparison():
    p = torch.tensor([[0.1, 0.2, 0.3], [0.4, 0.6, 0.35]])
    d2 = pair_d2(p, 0, 1)
    assert d2 > 0
    labels, core = E.cluster_points(p, d2, 1, squared=True)  # d² < d² is false: not linked
    assert labels.tolist() == [0, 1]
    labels, core = E.cluster_points(p, d2, 2, squared=True)
    assert labels.tolist() == [-1, -1] and core.tolist() == [False, False]
    above = float(np.nextafter(np.float32(d2), np.float32(np.inf)))
    labels, core = E.cluster_points(p, above, 2, squared=True)
    assert labels.tolist() == [0, 0] and core.tolist() == [True, True]


def test_edge_inputs():
    p = uniform(300, seed=22)
    n = p.shape[0]
    rows = torch.arange(n, dtype=torch.int32)
    # eps = 0 links nothing, not even a point to itself
    labels, core = E.cluster_points(p, 0.0, 1)
    assert torch.equal(labels, rows) and not bool(core.any())
    labels, core = E.cluster_points(p, 0.0, 2)
    assert bool((labels == -1).all()) and not bool(core.any())
    # eps = inf: one cluster of all finite points
    q = p.clone()
    q[17, 1] = math.nan
    q[40, 0] = math.inf
    for min_pts in (1, 5):
        labels, core = E.cluster_points(q, math.inf, min_pts)
        want = torch.zeros(n, dtype=torch.int32)
        want[17], want[40] = (17, 40) if min_pts == 1 else (-1, -1)
        assert torch.equal(labels, want)
        assert core.tolist() == [i not in (17, 40) for i in range(n)]
    # a NaN point has no neighbours and is nobody's neighbour: the others are as without it
    eps = 0.9 * n ** (-1.0 / 3.0)
    keep = torch.tensor([i for i in range(n) if i not in (17, 40)])
    for min_pts in (1, 3):
        labels, core = E.cluster_points(q, eps, min_pts)
        sub_l, sub_c = E.cluster_points(q[keep].contiguous(), eps, min_pts)
        assert torch.equal(core[keep], sub_c) and not bool(core[17]) and not bool(core[40])
        assert torch.equal(E.compact_labels(labels[keep])[0], E.compact_labels(sub_l)[0])
        assert labels[17] == (17 if min_pts == 1 else -1) and labels[40] == (40 if min_pts == 1 else -1)
    # n = 0
    for got in (E.cluster_points(torch.empty((0, 3)), 0.1, 2), E.cluster_labels(E.build_index(torch.empty((0, 3))), 0.1)):
        assert got[0].shape == (0,) and got[0].dtype == torch.int32
        assert got[1].shape == (0,) and got[1].dtype == torch.bool


def test_value_errors():
    p = uniform(50, seed=23)
    index = E.build_index(p)
    for eps, min_pts in ((-1.0, 1), (math.nan, 1), (0.1, 0), (0.1, -3)):
        with pytest.raises(ValueError):
            E.cluster_points(p, eps, min_pts)
        with pytest.raises(ValueError):
            E.cluster_labels(index, eps, min_pts)
        with pytest.raises(ValueError):
            E.cluster_points(torch.empty((0, 3)), eps, min_pts)
    with pytest.raises(ValueError):
        K.cluster_cpu(p, 0.01, 0)


def test_compact_labels():
    labels = torch.tensor([7, -1, 2, 7, 2, 30, -1, 2], dtype=torch.int32)
    dense, nclusters = E.compact_labels(labels)
    assert dense.dtype == torch.int32 and nclusters == 3
    assert dense.tolist() == [1, -1, 0, 1, 0, 2, -1, 0]
    dense, nclusters = E.compact_labels(torch.tensor([-1, -1], dtype=torch.int32))
    assert dense.tolist() == [-1, -1] and nclusters == 0
    dense, nclusters = E.compact_labels(torch.empty(0, dtype=torch.int32))
    assert dense.shape == (0,) and nclusters == 0


def test_against_sklearn_dbscan():
    sk = pytest.importorskip("sklearn.cluster")
    p = uniform(N, seed=24)
    eps, min_pts = EPS, 4
    # no pair within 1e-5 relative of eps: float32 and float64 distances then agree on every link
    d = torch.cdist(p.double(), p.double())
    assert not bool(((d - eps).abs() < 1e-5 * eps).any())
    labels, core = E.cluster_points(p, eps, min_pts)
    ref = sk.DBSCAN(eps=eps, min_samples=min_pts).fit(p.double().numpy())
    ref_core = np.zeros(N, dtype=bool)
    ref_core[ref.core_sample_indices_] = True
    assert np.array_equal(core.numpy(), ref_core)
    # the partition of the core points: same label here <=> same label there
    mine, theirs = labels.numpy()[ref_core], ref.labels_[ref_core]
    pairs = set(zip(mine.tolist(), theirs.tolist()))
    assert len(pairs) == len(set(mine.tolist())) == len(set(theirs.tolist()))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_round_trip(tmp_path, capsys):
    p = uniform(N, seed=25)
    fp = str(tmp_path / "p.float3")
    io.write_points(fp, p)
    pre = str(tmp_path / "cl")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK",
                                                             "PMI_SIZE", "OMPI_COMM_WORLD_RANK",
                                                             "OMPI_COMM_WORLD_SIZE", "PMIX_RANK")}
    stats = str(tmp_path / "s.json")
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_cluster"), fp, "-r", str(EPS), "--min-pts", "3", "-o", pre,
                           "--device", "cpu", "--stats", stats], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr
    labels, core = E.cluster_points(p, EPS, 3)
    assert _read(pre + ".labels") == labels.numpy().tobytes()
    assert _read(pre + ".core") == core.to(torch.uint8).numpy().tobytes()
    nclusters, noise, largest = cluster_app.summary(labels)
    assert f"{N} points: {nclusters} clusters, {noise} noise points, largest cluster {largest}" in proc.stdout
    assert nclusters == E.compact_labels(labels)[1] and noise == int((labels < 0).sum())
    assert largest == int(torch.bincount(labels[labels >= 0].long()).max())
    assert os.path.getsize(stats) > 0
    # ccheck passes, and fails after one label is altered, then after one core flag is
    assert tools.main(["ccheck", fp, pre, "-r", str(EPS), "--min-pts", "3"]) == 0
    assert "0 core flag mismatches, 0 label mismatches" in capsys.readouterr().out
    assert tools.main(["ccheck", fp, pre, "-r", str(EPS), "--min-pts", "4"]) == 1
    capsys.readouterr()
    bad = labels.clone()
    bad[int((labels >= 0).nonzero()[0])] += 1
    io.write_array(pre + ".labels", bad)
    assert tools.main(["ccheck", fp, pre, "-r", str(EPS), "--min-pts", "3"]) == 1
    assert "0 core flag mismatches, 1 label mismatches" in capsys.readouterr().out
    io.write_array(pre + ".labels", labels)
    flags = core.to(torch.uint8).numpy().copy()
    flags[5] ^= 1
    flags.tofile(pre + ".core")
    assert tools.main(["ccheck", fp, pre, "-r", str(EPS), "--min-pts", "3"]) == 1
    assert "1 core flag mismatches, 0 label mismatches" in capsys.readouterr().out
    # --squared, in process
    pre2 = str(tmp_path / "sq")
    cut2 = E.cut2_of(EPS)
    assert cluster_app.main([fp, "-r", repr(cut2), "--squared", "--min-pts", "3", "-o", pre2, "--device", "cpu"]) == 0
    assert _read(pre2 + ".labels") == labels.numpy().tobytes()
    assert tools.main(["ccheck", fp, pre2, "-r", repr(cut2), "--squared", "--min-pts", "3"]) == 0
    capsys.readouterr()


def test_ccheck_refuses_large_sets(tmp_path, capsys):
    fp = str(tmp_path / "big.float3")
    io.write_points(fp, torch.zeros((tools.CCHECK_MAX + 1, 3)))
    assert tools.main(["ccheck", fp, str(tmp_path / "none"), "-r", "0.1"]) == 1
    assert "quadratic" in capsys.readouterr().out


def test_cli_refuses_bad_arguments(tmp_path):
    fp = str(tmp_path / "p.float3")
    io.write_points(fp, uniform(20, seed=1))
    for args in (["-r", "-1"], ["-r", "nan"], ["-r", "0.1", "--min-pts", "0"]):
        with pytest.raises(SystemExit):
            cluster_app.main([fp, *args, "-o", str(tmp_path / "x"), "--device", "cpu"])

"""hipKNN_mst and lsknn_tools mcheck: the launcher on the CPU device, in process on the GPU, with
--core-k and --cut, and mcheck's verdict on a corrupted edge file."""
import json
import math
import os
import subprocess

import pytest
import torch

from mpi_cuda_largescaleknn_amd.apps import mst as mst_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5000
EPS = 0.9 * N ** (-1.0 / 3.0)
_ORACLE: dict = {}


def points():
    return uniform(N, seed=41)


def oracle(core_k=0):
    if core_k not in _ORACLE:
        p = points()
        _ORACLE[core_k] = K.mst_cpu(p, K.kth_cpu(p, p, core_k, math.inf) if core_k else None)
    return _ORACLE[core_k]


def read_edges(pre):
    return io.read_array(pre + ".mst.rows", torch.int32).view(-1, 2), io.read_array(pre + ".mst.d2", torch.float32)


def round_trip(tmp_path, capsys, device):
    """The app in process on `device`: plain, --core-k 5 and --cut, each checked by mcheck."""
    fp = str(tmp_path / "p.float3")
    io.write_points(fp, points())
    pre = str(tmp_path / "t")
    stats = str(tmp_path / "s.json")
    assert mst_app.main([fp, "-o", pre, "--device", device, "--cut", repr(EPS), "--stats", stats]) == 0
    out = capsys.readouterr().out
    rows, d2 = read_edges(pre)
    want = oracle()
    assert torch.equal(rows, want[0]) and torch.equal(d2.view(torch.int32), want[1].view(torch.int32))
    assert f"{N} points: {N - 1} edges in " in out
    assert f"heaviest edge ({int(want[0][-1, 0])}, {int(want[0][-1, 1])}) d2 {want[1][-1].item()!r}" in out
    labels = io.read_array(pre + ".labels", torch.int32)
    assert torch.equal(labels, K.cluster_cpu(points(), E.cut2_of(EPS), 1)[0])
    assert f"{int(labels.unique().numel())} groups" in out
    with open(stats) as f:
        rec = json.load(f)
    assert rec["n"] == N and rec["edges"] == N - 1
    if device == "cuda":
        assert rec["mst"]["mst_rounds"] == len(rec["mst"]["mst_components"]) <= math.ceil(math.log2(N))
    assert tools.main(["mcheck", fp, pre]) == 0
    assert f"checked {N} points: {N - 1} edges, 0 edge mismatches" in capsys.readouterr().out
    # mutual reachability
    pre5 = str(tmp_path / "t5")
    assert mst_app.main([fp, "-o", pre5, "--device", device, "--core-k", "5"]) == 0
    capsys.readouterr()
    rows5, d25 = read_edges(pre5)
    want5 = oracle(5)
    assert torch.equal(rows5, want5[0]) and torch.equal(d25.view(torch.int32), want5[1].view(torch.int32))
    assert not os.path.exists(pre5 + ".labels")
    assert tools.main(["mcheck", fp, pre5, "--core-k", "5"]) == 0
    capsys.readouterr()
    assert tools.main(["mcheck", fp, pre5]) == 1  # (the plain tree is another one)
    capsys.readouterr()
    return fp, pre


def test_cli_cpu(tmp_path, capsys):
    fp, pre = round_trip(tmp_path, capsys, "cpu")
    rows, d2 = read_edges(pre)
    # the launcher itself, as a process
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK",
                                                             "PMI_SIZE", "OMPI_COMM_WORLD_RANK",
                                                             "OMPI_COMM_WORLD_SIZE", "PMIX_RANK")}
    pre2 = str(tmp_path / "proc")
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_mst"), fp, "-o", pre2, "--device", "cpu"], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr
    assert f"{N} points: {N - 1} edges" in proc.stdout
    got = read_edges(pre2)
    assert torch.equal(got[0], rows) and torch.equal(got[1], d2)
    # a corrupted edge file: one weight, then one row, then a missing edge
    bad = d2.clone()
    bad[100] = torch.nextafter(bad[100], torch.tensor(math.inf))
    io.write_array(pre + ".mst.d2", bad)
    assert tools.main(["mcheck", fp, pre]) == 1
    assert "1 edge mismatches" in capsys.readouterr().out
    io.write_array(pre + ".mst.d2", d2)
    swapped = rows.clone()
    swapped[7] = swapped[7].flip(0)
    io.write_array(pre + ".mst.rows", swapped.reshape(-1))
    assert tools.main(["mcheck", fp, pre]) == 1
    assert "1 edge mismatches" in capsys.readouterr().out
    io.write_array(pre + ".mst.rows", rows[:-1].reshape(-1))
    assert tools.main(["mcheck", fp, pre]) == 1
    capsys.readouterr()
    io.write_array(pre + ".mst.rows", rows.reshape(-1))
    assert tools.main(["mcheck", fp, pre]) == 0
    capsys.readouterr()


@pytest.mark.gpu
def test_cli_gpu(tmp_path, capsys):
    E.reset_kernels_used()
    round_trip(tmp_path, capsys, "cuda")
    assert "mst" in E.kernels_used()


def test_mcheck_refuses_large_sets(tmp_path, capsys):
    fp = str(tmp_path / "big.float3")
    io.write_points(fp, torch.zeros((tools.CCHECK_MAX + 1, 3)))
    assert tools.main(["mcheck", fp, str(tmp_path / "none")]) == 1
    assert "quadratic" in capsys.readouterr().out


def test_cli_refuses_bad_arguments(tmp_path):
    fp = str(tmp_path / "p.float3")
    io.write_points(fp, uniform(20, seed=1))
    for args in (["--cut", "-1"], ["--cut", "nan"], ["--core-k", "-2"]):
        with pytest.raises(SystemExit):
            mst_app.main([fp, *args, "-o", str(tmp_path / "x"), "--device", "cpu"])
    # more neighbours than points: the core distances are infinite
    assert mst_app.main([fp, "--core-k", "21", "-o", str(tmp_path / "x"), "--device", "cpu"]) == 1

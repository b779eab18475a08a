"""hipKNN_mst --period and lsknn_tools mcheck --period on the CPU device: the periodic tree passes
the periodic check and fails the open one, --cut gives hipKNN_cluster --period's groups, --core-k
the periodic core distances, and a bad --period is refused."""
import json

import pytest
import torch

from mpi_cuda_largescaleknn_amd.apps import cluster as cluster_app
from mpi_cuda_largescaleknn_amd.apps import mst as mst_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import uniform

N = 3000
EPS = 0.9 * N ** (-1.0 / 3.0)


def points_file(tmp_path):
    fp = str(tmp_path / "p.float3")
    io.write_points(fp, uniform(N, seed=41))
    return fp


def test_cli_period_cpu(tmp_path, capsys):
    fp = points_file(tmp_path)
    pre = str(tmp_path / "t")
    stats = str(tmp_path / "s.json")
    assert mst_app.main([fp, "-o", pre, "--device", "cpu", "--period", "1", "--cut", repr(EPS),
                         "--stats", stats]) == 0
    assert f"{N} points: {N - 1} edges in " in capsys.readouterr().out
    rows = io.read_array(pre + ".mst.rows", torch.int32).view(-1, 2)
    d2 = io.read_array(pre + ".mst.d2", torch.float32)
    want = K.mst_periodic_cpu(uniform(N, seed=41), 1.0)
    assert torch.equal(rows, want[0]) and torch.equal(d2.view(torch.int32), want[1].view(torch.int32))
    with open(stats) as f:
        rec = json.load(f)
    assert rec["period"] == [1.0, 1.0, 1.0] and rec["edges"] == N - 1
    assert tools.main(["mcheck", fp, pre, "--period", "1"]) == 0
    assert f"checked {N} points: {N - 1} edges, 0 edge mismatches" in capsys.readouterr().out
    assert tools.main(["mcheck", fp, pre]) == 1  # (the open tree is another one)
    capsys.readouterr()
    # the --cut groups are those of hipKNN_cluster --period
    cpre = str(tmp_path / "c")
    assert cluster_app.main([fp, "-o", cpre, "-r", repr(EPS), "--period", "1", "--device", "cpu"]) == 0
    capsys.readouterr()
    labels = io.read_array(pre + ".labels", torch.int32)
    assert torch.equal(labels, io.read_array(cpre + ".labels", torch.int32))
    assert 1 < int(labels.unique().numel()) < N
    # mutual reachability with the periodic core distances, on one open axis
    pre5 = str(tmp_path / "t5")
    assert mst_app.main([fp, "-o", pre5, "--device", "cpu", "--period", "1,inf,1", "--core-k", "5"]) == 0
    capsys.readouterr()
    assert tools.main(["mcheck", fp, pre5, "--core-k", "5", "--period", "1,inf,1"]) == 0
    capsys.readouterr()
    assert tools.main(["mcheck", fp, pre5, "--core-k", "5", "--period", "1"]) == 1
    capsys.readouterr()


# what the option's own validation says (an unknown option says none of it)
MESSAGE = {"0": "every period entry must be > 0", "-1": "every period entry must be > 0",
           "nan": "every period entry must be > 0", "1,2": "period must be one value or three",
           "x": "could not convert string to float"}


@pytest.mark.parametrize("bad", sorted(MESSAGE))
def test_cli_refuses_bad_period(tmp_path, capsys, bad):
    fp = points_file(tmp_path)
    with pytest.raises(SystemExit) as e:
        mst_app.main([fp, "-o", str(tmp_path / "x"), "--device", "cpu", "--period", bad])
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert "argument --period" in err and MESSAGE[bad] in err
    with pytest.raises(SystemExit):
        tools.main(["mcheck", fp, str(tmp_path / "x"), "--period", bad])
    err = capsys.readouterr().err
    assert "argument --period" in err and MESSAGE[bad] in err

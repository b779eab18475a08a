"""hipKNN_pairs and lsknn_tools pcheck on the CPU device: the file and its shape in both modes,
under a period, several chunks give the same bytes, the check passes and fails after one cell is
changed, and argument errors exit non-zero before anything is written."""
import json
import os
import subprocess

import pytest
import torch

from datasets import uniform
from mpi_cuda_largescaleknn_amd.apps import pairs as pairs_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.utils import io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NQ = 1500, 400
MODES = {"rppi": (["--rp", "0,0.03,0.08,0.08,0.2", "--pi", "0.02,0.1,0.25"], E.pair_counts_rppi),
         "smu": (["--s", "0.05,0.1,0.1,0.25", "--mu", "0,0.3,0.6,1,inf"], E.pair_counts_smu)}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs2d")
    p = uniform(N, seed=71)
    q = torch.cat([p[:NQ // 2], uniform(NQ - NQ // 2, seed=72)])
    io.write_points(str(d / "p.float3"), p)
    io.write_points(str(d / "q.float3"), q)
    return d, p, q


def raw(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("period", [None, "1", "1,inf,0.5"])
@pytest.mark.parametrize("mode", ["rppi", "smu"])
def test_pairs_cli_writes_the_file_and_passes_the_check(files, mode, period, capsys):
    d, p, q = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    pre = str(d / f"out_{mode}_{'open' if period is None else period.replace(',', '_')}")
    edges, fn = MODES[mode]
    first, second = ([float(v) for v in edges[i].split(",")] for i in (1, 3))
    opts = edges + ["--los", "x", "--device", "cpu"] + ([] if period is None else ["--period", period])
    assert pairs_app.main([fp, fq, "-o", pre, "--stats", pre + ".json"] + opts) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    per = None if period is None else (tuple(float(v) for v in period.split(",")) if "," in period else float(period))
    want = fn(E.build_index(p), q, first, second, los=0, period=per)
    got = io.read_array(pre + ".pairs2d", torch.int64)
    assert got.shape == (len(first) * len(second),)
    assert torch.equal(got.view(len(first), len(second)), want) and int(want[-1, -1]) > 0  # row-major [B1][B2]
    # one line per row of cells: the edge, then the binned counts
    cells = E.shell_counts_2d(want)
    assert len(lines) == len(first)
    for i, line in enumerate(lines):
        words = line.split()
        assert float(words[0]) == first[i] and [int(w) for w in words[1:]] == cells[i].tolist()
    with open(pre + ".json") as f:
        rec = json.load(f)
    assert rec["pairs"] == want.tolist() and rec["kernels"] == ["cpu"] and rec["mode"] == mode

    # a small chunk forces several passes, added on the host: the same bytes
    assert pairs_app.main([fp, fq, "-o", pre + "_chunked", "--chunk", "70"] + opts) == 0
    assert raw(pre + "_chunked.pairs2d") == raw(pre + ".pairs2d")
    capsys.readouterr()

    check = ["pcheck", fp, fq, pre] + edges + ["--los", "x"] + ([] if period is None else ["--period", period])
    assert tools.main(check) == 0
    assert f"checked {want.numel()} cells: 0 mismatches" in capsys.readouterr().out
    assert tools.main(["pcheck", fp, fq, pre] + edges + ["--los", "z"] + check[10:]) == 1  # another line of sight
    # one cell changed: the check fails and names it
    bad = got.clone()
    bad[len(second) + 1] += 1
    io.write_array(pre + ".pairs2d", bad, 0, truncate=True)
    capsys.readouterr()
    assert tools.main(check) == 1
    assert "PAIRS2D [1][1]" in capsys.readouterr().out
    io.write_array(pre + ".pairs2d", got[:-1], 0, truncate=True)
    assert tools.main(check) == 1
    assert "size mismatch" in capsys.readouterr().out


def test_the_launcher_and_squared_cutoffs(files):
    d, p, q = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    pre = str(d / "sq")
    edges = ["--rp", "0.0009,0.04", "--pi", "0.01,0.0625", "--squared"]
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_pairs"), fp, fq, "-o", pre, "--device", "cpu", "--period",
                           "1"] + edges, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    want = E.pair_counts_rppi(E.build_index(p), q, [0.0009, 0.04], [0.01, 0.0625], squared=True, period=1.0)
    assert torch.equal(io.read_array(pre + ".pairs2d", torch.int64).view(2, 2), want)
    assert tools.main(["pcheck", fp, fq, pre, "--period", "1"] + edges) == 0
    assert tools.main(["pcheck", fp, fq, pre, "--period", "1"] + edges[:-1]) == 1


@pytest.mark.parametrize("argv", [["--rp", "0.1"], ["--rp", "0.1", "--mu", "0.5"], ["--s", "0.1"], [],
                                  ["--rp", "0.1", "--pi", "0.1", "--s", "0.1", "--mu", "1"],
                                  ["--rp", "a,b", "--pi", "0.1"], ["--rp", "0.1", "--pi", "0.1", "--los", "w"],
                                  ["--rp", "0.1", "--pi", "0.1", "--chunk", "0"]])
def test_bad_options_are_usage_errors(files, argv):
    d, p, q = files
    with pytest.raises(SystemExit) as e:
        pairs_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", str(d / "u")] + argv)
    assert e.value.code == 2


@pytest.mark.parametrize("argv,text", [(["--rp", "0.2,0.1", "--pi", "0.1"], "ascend"),
                                       (["--rp", "0.1", "--pi", "-0.1"], ">= 0"),
                                       (["--s", "0.1", "--mu", "0.5,nan"], ">= 0"),
                                       (["--rp", "0.1", "--pi", "0.6", "--period", "1"], "line-of-sight"),
                                       (["--rp", "0.3", "--pi", "0.1", "--period", "1,0.5,1"], "perpendicular"),
                                       (["--s", "0.3", "--mu", "1", "--period", "1,1,0.5"], "line-of-sight")])
def test_bad_edges_exit_1_and_write_nothing(files, argv, text, capsys):
    d, p, q = files
    assert pairs_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", str(d / "bad"), "--device", "cpu"] + argv) == 1
    assert text in capsys.readouterr().err
    assert not (d / "bad.pairs2d").exists()
    assert tools.main(["pcheck", str(d / "p.float3"), str(d / "q.float3"), str(d / "bad")] + argv) == 1

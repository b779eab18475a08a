"""hipKNN_pairs --weights [--query-weights] and lsknn_tools pcheck --weights on the CPU device: the
file PREFIX.wpairs2d in both modes, several chunks give the same bytes, the check passes and fails
after one cell is changed, a bound violation exits non-zero with its message before anything is
written, and without --weights nothing changes."""
import json
import os
import subprocess

import pytest
import torch

from datasets import uniform
from mpi_cuda_largescaleknn_amd.apps import pairs as pairs_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NQ = 1200, 300
MODES = {"rppi": ["--rp", "0,0.03,0.08,0.08,0.2", "--pi", "0.02,0.1,0.25"],
         "smu": ["--s", "0.05,0.1,0.1,0.25", "--mu", "0,0.3,0.6,1,inf"]}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("wpairs2d")
    p = uniform(N, seed=91)
    q = torch.cat([p[:NQ // 2], uniform(NQ - NQ // 2, seed=92)])
    g = torch.Generator().manual_seed(93)
    w = torch.randint(-(1 << 34), (1 << 34) + 1, (N,), generator=g, dtype=torch.int64)
    wq = torch.randint(-16, 17, (NQ,), generator=g, dtype=torch.int64)
    io.write_points(str(d / "p.float3"), p)
    io.write_points(str(d / "q.float3"), q)
    io.write_array(str(d / "w.i64"), w, 0, truncate=True)
    io.write_array(str(d / "wq.i64"), wq, 0, truncate=True)
    return d, p, q, w, wq


def raw(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("with_wq", [False, True], ids=["w", "w_wq"])
@pytest.mark.parametrize("period", [None, "1,inf,0.8"])
@pytest.mark.parametrize("mode", ["rppi", "smu"])
def test_weights_write_the_file_and_pass_the_check(files, mode, period, with_wq, capsys):
    d, p, q, w, wq = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    pre = str(d / f"out_{mode}_{'open' if period is None else 'per'}_{int(with_wq)}")
    edges = MODES[mode]
    first, second = ([float(v) for v in edges[i].split(",")] for i in (1, 3))
    wopts = ["--weights", str(d / "w.i64")] + (["--query-weights", str(d / "wq.i64")] if with_wq else [])
    opts = edges + ["--los", "y", "--device", "cpu"] + ([] if period is None else ["--period", period]) + wopts
    assert pairs_app.main([fp, fq, "-o", pre, "--stats", pre + ".json"] + opts) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    per = None if period is None else tuple(float(v) for v in period.split(","))
    a2 = [E.cut2_of(r) for r in first]
    b2 = [E.cut2_of(r) for r in second]
    want = K.weighted_pair_sums_2d_cpu(p, q, a2, b2, w, mode, 1, per, query_weights=wq if with_wq else None)
    assert not os.path.exists(pre + ".pairs2d")
    got = io.read_array(pre + ".wpairs2d", torch.int64)
    assert got.shape == (len(first) * len(second),)
    assert torch.equal(got.view(len(first), len(second)), want) and int(want[-1, -1]) != 0  # row-major [B1][B2]
    cells = E.shell_counts_2d(want)
    assert len(lines) == len(first)
    for i, line in enumerate(lines):
        words = line.split()
        assert float(words[0]) == first[i] and [int(v) for v in words[1:]] == cells[i].tolist()
    with open(pre + ".json") as f:
        rec = json.load(f)
    assert rec["pairs"] == want.tolist() and rec["kernels"] == ["cpu"] and rec["weights"] == str(d / "w.i64")

    # a small chunk forces several passes, the query weights sliced with them: the same bytes
    assert pairs_app.main([fp, fq, "-o", pre + "_chunked", "--chunk", "70"] + opts) == 0
    assert raw(pre + "_chunked.wpairs2d") == raw(pre + ".wpairs2d")
    capsys.readouterr()

    check = ["pcheck", fp, fq, pre] + edges + ["--los", "y"] + ([] if period is None else ["--period", period]) + wopts
    assert tools.main(check) == 0
    assert f"checked {want.numel()} cells: 0 mismatches" in capsys.readouterr().out
    # other query weights: the check fails
    other = wopts[:2] + ([] if with_wq else ["--query-weights", str(d / "wq.i64")])
    assert tools.main(check[:len(check) - len(wopts)] + other) == 1
    # one cell changed: the check fails and names it
    bad = got.clone()
    bad[len(second) + 1] += 1
    io.write_array(pre + ".wpairs2d", bad, 0, truncate=True)
    capsys.readouterr()
    assert tools.main(check) == 1
    assert "WPAIRS2D [1][1]" in capsys.readouterr().out
    io.write_array(pre + ".wpairs2d", got[:-1], 0, truncate=True)
    assert tools.main(check) == 1
    assert "size mismatch" in capsys.readouterr().out


def test_the_launcher_with_weights(files):
    d, p, q, w, wq = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    pre = str(d / "launcher")
    edges = ["--s", "0.1,0.3", "--mu", "0.5,inf"]
    proc = subprocess.run([os.path.join(ROOT, "bin", "hipKNN_pairs"), fp, fq, "-o", pre, "--device", "cpu", "--period",
                           "1", "--weights", str(d / "w.i64"), "--query-weights", str(d / "wq.i64")] + edges,
                          capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    want = E.weighted_pair_sums_smu(E.build_index(p), q, [0.1, 0.3], [0.5, float("inf")], w, query_weights=wq,
                                    period=1.0)
    assert torch.equal(io.read_array(pre + ".wpairs2d", torch.int64).view(2, 2), want)


def test_without_weights_nothing_changes(files, capsys):
    d, p, q, w, wq = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    for mode, fn in (("rppi", E.pair_counts_rppi), ("smu", E.pair_counts_smu)):
        pre = str(d / ("plain_" + mode))
        edges = MODES[mode]
        first, second = ([float(v) for v in edges[i].split(",")] for i in (1, 3))
        assert pairs_app.main([fp, fq, "-o", pre, "--device", "cpu", "--period", "1"] + edges) == 0
        want = fn(E.build_index(p), q, first, second, period=1.0)
        assert raw(pre + ".pairs2d") == want.contiguous().numpy().tobytes()
        assert not os.path.exists(pre + ".wpairs2d")
        assert tools.main(["pcheck", fp, fq, pre, "--period", "1"] + edges) == 0
    capsys.readouterr()


def test_bound_violations_and_bad_files_exit_1_and_write_nothing(files, capsys):
    d, p, q, w, wq = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    base = [fp, fq, "-o", str(d / "bad"), "--device", "cpu", "--rp", "0.1", "--pi", "0.1"]
    # max|w| * n >= 2^62
    top = torch.ones(N, dtype=torch.int64)
    top[3] = -(1 << 60)
    io.write_array(str(d / "top.i64"), top, 0, truncate=True)
    assert pairs_app.main(base + ["--weights", str(d / "top.i64")]) == 1
    assert "2^62" in capsys.readouterr().err
    # (sum |w|) * (sum |wq|) >= 2^63 over the whole query file, though no chunk of 10 queries exceeds it
    big = torch.full((N,), 1 << 40, dtype=torch.int64)  # sum |w| ~ 2^50.2
    io.write_array(str(d / "big.i64"), big, 0, truncate=True)
    bigq = torch.full((NQ,), -(1 << 5), dtype=torch.int64)  # sum |wq| ~ 2^13.2: 2^63.4 in all, 2^58.5 per chunk
    io.write_array(str(d / "bigq.i64"), bigq, 0, truncate=True)
    assert pairs_app.main(base + ["--chunk", "10", "--weights", str(d / "big.i64"), "--query-weights",
                                  str(d / "bigq.i64")]) == 1
    assert "2^63" in capsys.readouterr().err
    # without query weights nq stands in their place: 2^50.2 * 300 < 2^63 passes, 2^55.2 * 300 does not
    assert pairs_app.main(base + ["--weights", str(d / "big.i64")]) == 0
    os.remove(str(d / "bad.wpairs2d"))
    io.write_array(str(d / "big2.i64"), torch.full((N,), 1 << 45, dtype=torch.int64), 0, truncate=True)
    capsys.readouterr()
    assert pairs_app.main(base + ["--weights", str(d / "big2.i64")]) == 1
    assert "2^63" in capsys.readouterr().err
    # files of the wrong length
    assert pairs_app.main(base + ["--weights", str(d / "wq.i64")]) == 1
    assert "--weights" in capsys.readouterr().err
    assert pairs_app.main(base + ["--weights", str(d / "w.i64"), "--query-weights", str(d / "w.i64")]) == 1
    assert "--query-weights" in capsys.readouterr().err
    assert not (d / "bad.wpairs2d").exists() and not (d / "bad.pairs2d").exists()
    assert tools.main(["pcheck", fp, fq, str(d / "bad"), "--rp", "0.1", "--pi", "0.1", "--weights",
                       str(d / "wq.i64")]) == 1
    with pytest.raises(SystemExit) as e:  # --query-weights alone is a usage error
        pairs_app.main(base + ["--query-weights", str(d / "wq.i64")])
    assert e.value.code == 2

"""hipKNN_radius --profile and lsknn_tools rcheck --profile on the CPU device: the two files and
their shapes, several chunks give the same bytes, --pairs-only the same pair counts, the check
passes and fails after one count is changed, and --profile beside -r is a usage error."""
import json

import pytest
import torch

from datasets import uniform
from mpi_cuda_largescaleknn_amd.apps import radius as radius_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.utils import io

N, NQ = 2000, 700
RADII = "0,0.03,0.08,0.08,0.2,0.5"
B = 6


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("profile")
    p, q = uniform(N, seed=71), uniform(NQ, seed=72)
    io.write_points(str(d / "p.float3"), p)
    io.write_points(str(d / "q.float3"), q)
    return d, p, q


def raw(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("period", [None, "1", "1,inf,2"])
def test_profile_cli_writes_both_files_and_passes_the_check(files, period, capsys):
    d, p, q = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    tag = "open" if period is None else period.replace(",", "_")
    pre = str(d / f"out_{tag}")
    opts = ["--profile", RADII, "--device", "cpu"] + ([] if period is None else ["--period", period])
    assert radius_app.main([fp, fq, "-o", pre, "--stats", pre + ".json"] + opts) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    radii = [float(v) for v in RADII.split(",")]
    per = None if period is None else (tuple(float(v) for v in period.split(",")) if "," in period else float(period))
    want = E.radius_profile(E.build_index(p), q, radii, period=per)
    prof = io.read_array(pre + ".profile", torch.int32)
    pairs = io.read_array(pre + ".pairs", torch.int64)
    assert prof.shape == (NQ * B,) and pairs.shape == (B,)
    assert torch.equal(prof.view(NQ, B), want)  # row-major [nq][B]
    assert torch.equal(pairs, want.sum(0, dtype=torch.int64))
    # one line per radius: radius, cumulative pairs, shell pairs
    assert len(lines) == B
    shells = [int(pairs[b]) - (int(pairs[b - 1]) if b else 0) for b in range(B)]
    for b, line in enumerate(lines):
        r, cum, shell = line.split()
        assert float(r) == radii[b] and int(cum) == int(pairs[b]) and int(shell) == shells[b]
    with open(pre + ".json") as f:
        rec = json.load(f)
    assert rec["pairs"] == pairs.tolist() and rec["kernels"] == ["cpu"]

    # a small chunk forces several passes: the same bytes
    pre2 = pre + "_chunked"
    assert radius_app.main([fp, fq, "-o", pre2, "--chunk", "97"] + opts) == 0
    assert raw(pre2 + ".profile") == raw(pre + ".profile") and raw(pre2 + ".pairs") == raw(pre + ".pairs")
    # --pairs-only: the same pair counts and no profile file
    pre3 = pre + "_pairs"
    assert radius_app.main([fp, fq, "-o", pre3, "--chunk", "300", "--pairs-only"] + opts) == 0
    assert raw(pre3 + ".pairs") == raw(pre + ".pairs")
    assert not (d / (f"out_{tag}_pairs.profile")).exists()
    capsys.readouterr()

    check = ["rcheck", fp, fq, pre, "--profile", RADII] + ([] if period is None else ["--period", period])
    assert tools.main(check) == 0
    assert f"checked {NQ} profile rows: 0 mismatches" in capsys.readouterr().out  # every row: nq <= 65536
    assert tools.main(check + ["--samples", "50"]) == 0
    assert "checked 50 profile rows" in capsys.readouterr().out
    assert tools.main(["rcheck", fp, fq, pre3, "--profile", RADII, "--pairs-only"] + check[6:]) == 0
    if period is not None:  # the open box differs: the set wraps
        assert tools.main(["rcheck", fp, fq, pre, "--profile", RADII]) == 1
    # one count changed: the rows fail; put back, one pair count changed: the sums fail
    bad = prof.clone()
    bad[NQ // 2 * B + 2] += 1
    io.write_array(pre + ".profile", bad, 0, truncate=True)
    assert tools.main(check) == 1
    io.write_array(pre + ".profile", prof, 0, truncate=True)
    assert tools.main(check) == 0
    off = pairs.clone()
    off[B - 1] -= 1
    io.write_array(pre + ".pairs", off, 0, truncate=True)
    assert tools.main(check) == 1
    io.write_array(pre3 + ".pairs", off, 0, truncate=True)
    assert tools.main(["rcheck", fp, fq, pre3, "--profile", RADII, "--pairs-only"] + check[6:]) == 1


def test_squared_cutoffs_and_a_radius_above_the_period_bound(files, capsys):
    d, p, q = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    pre = str(d / "sq")
    assert radius_app.main([fp, fq, "-o", pre, "--profile", "0.0009,0.04", "--squared", "--device", "cpu"]) == 0
    want = E.radius_profile(E.build_index(p), q, [0.0009, 0.04], squared=True)
    assert torch.equal(io.read_array(pre + ".profile", torch.int32).view(NQ, 2), want)
    assert tools.main(["rcheck", fp, fq, pre, "--profile", "0.0009,0.04", "--squared"]) == 0
    assert tools.main(["rcheck", fp, fq, pre, "--profile", "0.0009,0.04"]) == 1
    capsys.readouterr()
    assert radius_app.main([fp, fq, "-o", str(d / "big"), "--profile", "0.1,0.6", "--period", "1",
                            "--device", "cpu"]) == 1
    assert "half the period" in capsys.readouterr().err
    assert not (d / "big.profile").exists() and not (d / "big.pairs").exists()


@pytest.mark.parametrize("extra", [["-r", "0.1"], ["--radii", "x"], ["--point-radii", "x"]])
def test_profile_beside_another_radius_option_is_a_usage_error(files, extra):
    d, p, q = files
    with pytest.raises(SystemExit) as e:
        radius_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", str(d / "u"), "--profile", "0.1"] + extra)
    assert e.value.code == 2


@pytest.mark.parametrize("argv", [["--profile", "0.2,0.1"], ["--profile", "-1"], ["--profile", "a,b"],
                                  ["-r", "0.1", "--pairs-only"], ["--profile", "0.1", "--counts-only"]])
def test_bad_profile_arguments_are_usage_errors(files, argv):
    d, p, q = files
    with pytest.raises(SystemExit) as e:
        radius_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", str(d / "u")] + argv)
    assert e.value.code == 2

"""hipKNN_radius --profile --weights, lsknn_tools rcheck --profile --weights and lsknn_tools
fixweights on the CPU device: the two files equal the oracle, several chunks give the same
bytes, the check passes and fails after one value is changed, a weight file of the wrong length
exits 1, fixweights round-trips, and --profile without --weights writes what it always wrote."""
import json

import pytest
import torch

from datasets import uniform
from mpi_cuda_largescaleknn_amd.apps import radius as radius_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

N, NQ = 2000, 700
RADII = "0,0.03,0.08,0.08,0.2,0.5"
B = 6


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("wprofile")
    p, q = uniform(N, seed=71), uniform(NQ, seed=72)
    g = torch.Generator().manual_seed(73)
    w = torch.randint(-(1 << 30), (1 << 30) + 1, (N,), generator=g, dtype=torch.int64)
    wq = torch.randint(-100, 101, (NQ,), generator=g, dtype=torch.int64)
    io.write_points(str(d / "p.float3"), p)
    io.write_points(str(d / "q.float3"), q)
    io.write_array(str(d / "w.i64"), w)
    io.write_array(str(d / "wq.i64"), wq)
    return d, p, q, w, wq


def raw(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("with_wq", (False, True), ids=("unit-queries", "query-weights"))
@pytest.mark.parametrize("period", [None, "1", "1,inf,2"])
def test_weighted_cli_writes_both_files_and_passes_the_check(files, period, with_wq, capsys):
    d, p, q, w, wq = files
    fp, fq, fw = str(d / "p.float3"), str(d / "q.float3"), str(d / "w.i64")
    tag = ("open" if period is None else period.replace(",", "_")) + ("_wq" if with_wq else "")
    pre = str(d / f"out_{tag}")
    wopts = ["--weights", fw] + (["--query-weights", str(d / "wq.i64")] if with_wq else [])
    opts = ["--profile", RADII, "--device", "cpu"] + wopts + ([] if period is None else ["--period", period])
    assert radius_app.main([fp, fq, "-o", pre, "--stats", pre + ".json"] + opts) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    radii = [float(v) for v in RADII.split(",")]
    per = None if period is None else (tuple(float(v) for v in period.split(",")) if "," in period else float(period))
    cut2s = [E.cut2_of(r) for r in radii]
    want = K.weighted_profile_cpu(p, q, cut2s, w, per)  # the oracle
    want_pairs = K.weighted_pair_sums_cpu(p, q, cut2s, w, per, query_weights=wq if with_wq else None)
    prof = io.read_array(pre + ".wprofile", torch.int64)
    pairs = io.read_array(pre + ".wpairs", torch.int64)
    assert prof.shape == (NQ * B,) and pairs.shape == (B,)
    assert torch.equal(prof.view(NQ, B), want)  # row-major [nq][B]
    assert torch.equal(pairs, want_pairs)
    assert not (d / f"out_{tag}.profile").exists() and not (d / f"out_{tag}.pairs").exists()
    # one line per radius: radius, cumulative sum, shell sum
    assert len(lines) == B
    for b, line in enumerate(lines):
        r, cum, shell = line.split()
        assert float(r) == radii[b] and int(cum) == int(pairs[b])
        assert int(shell) == int(pairs[b]) - (int(pairs[b - 1]) if b else 0)
    with open(pre + ".json") as f:
        rec = json.load(f)
    assert rec["pairs"] == pairs.tolist() and rec["kernels"] == ["cpu"] and rec["weights"] == fw

    # a small chunk forces several passes: the same bytes
    pre2 = pre + "_chunked"
    assert radius_app.main([fp, fq, "-o", pre2, "--chunk", "97"] + opts) == 0
    assert raw(pre2 + ".wprofile") == raw(pre + ".wprofile") and raw(pre2 + ".wpairs") == raw(pre + ".wpairs")
    # --pairs-only: the same pair sums and no profile file
    pre3 = pre + "_pairs"
    assert radius_app.main([fp, fq, "-o", pre3, "--chunk", "300", "--pairs-only"] + opts) == 0
    assert raw(pre3 + ".wpairs") == raw(pre + ".wpairs")
    assert not (d / f"out_{tag}_pairs.wprofile").exists()
    capsys.readouterr()

    tail = wopts + ([] if period is None else ["--period", period])
    check = ["rcheck", fp, fq, pre, "--profile", RADII] + tail
    assert tools.main(check) == 0
    assert f"checked {NQ} weighted profile rows: 0 mismatches" in capsys.readouterr().out  # every row
    assert tools.main(check + ["--samples", "50"]) == 0
    assert "checked 50 weighted profile rows" in capsys.readouterr().out
    assert tools.main(["rcheck", fp, fq, pre3, "--profile", RADII, "--pairs-only"] + tail) == 0
    if with_wq:  # the sums without the query weights differ
        assert tools.main(["rcheck", fp, fq, pre, "--profile", RADII, "--weights", fw] + tail[4:]) == 1
    # one value changed: the rows fail; put back, one pair sum changed: the sums fail
    bad = prof.clone()
    bad[NQ // 2 * B + 2] += 1
    io.write_array(pre + ".wprofile", bad, 0, truncate=True)
    assert tools.main(check) == 1
    io.write_array(pre + ".wprofile", prof, 0, truncate=True)
    assert tools.main(check) == 0
    off = pairs.clone()
    off[B - 1] -= 1
    io.write_array(pre + ".wpairs", off, 0, truncate=True)
    assert tools.main(check) == 1
    io.write_array(pre3 + ".wpairs", off, 0, truncate=True)
    assert tools.main(["rcheck", fp, fq, pre3, "--profile", RADII, "--pairs-only"] + tail) == 1


def test_a_weight_file_of_the_wrong_length_exits_1(files, capsys):
    d, p, q, w, wq = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    io.write_array(str(d / "short.i64"), w[:-1])
    io.write_array(str(d / "longq.i64"), torch.cat([wq, wq[:1]]))
    pre = str(d / "wrong")
    assert radius_app.main([fp, fq, "-o", pre, "--profile", RADII, "--weights", str(d / "short.i64"),
                            "--device", "cpu"]) == 1
    assert f"holds {N - 1} values" in capsys.readouterr().err
    assert radius_app.main([fp, fq, "-o", pre, "--profile", RADII, "--weights", str(d / "w.i64"),
                            "--query-weights", str(d / "longq.i64"), "--device", "cpu"]) == 1
    assert f"holds {NQ + 1} values" in capsys.readouterr().err
    assert not (d / "wrong.wprofile").exists() and not (d / "wrong.wpairs").exists()
    assert tools.main(["rcheck", fp, fq, str(d / "out_open"), "--profile", RADII, "--weights",
                       str(d / "short.i64")]) == 1
    # weights beyond the bounds are refused with exit status 1 too
    io.write_array(str(d / "huge.i64"), torch.full((N,), 1 << 52, dtype=torch.int64))
    assert radius_app.main([fp, fq, "-o", pre, "--profile", RADII, "--weights", str(d / "huge.i64"),
                            "--device", "cpu"]) == 1
    assert "2^62" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["-r", "0.1", "--weights", "w"], ["--profile", "0.1", "--query-weights", "wq"]])
def test_weights_without_their_option_are_usage_errors(files, argv):
    d = files[0]
    with pytest.raises(SystemExit) as e:
        radius_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", str(d / "u")] + argv)
    assert e.value.code == 2


def test_fixweights_round_trips(files, capsys):
    d = files[0]
    g = torch.Generator().manual_seed(74)
    m = (torch.rand(N, generator=g) + 0.5) * 8.0  # float32 masses in [4, 12)
    io.write_array(str(d / "m.float"), m)
    assert tools.main(["fixweights", str(d / "m.float"), str(d / "m.i64")]) == 0
    out = capsys.readouterr().out
    fix = io.read_array(str(d / "m.i64"), torch.int64)
    want, s = E.fixed_point_weights(m)
    assert f"s = {s} " in out and torch.equal(fix, want)
    assert torch.equal(torch.ldexp(fix.double(), torch.tensor(s)), m.double())  # exact: the spread fits
    # --bits / --terms
    assert tools.main(["fixweights", str(d / "m.float"), str(d / "m31.i64"), "--bits", "31", "--terms",
                       str(1 << 20)]) == 0
    want, s31 = E.fixed_point_weights(m, n_terms=1 << 20, bits=31)
    assert f"s = {s31} " in capsys.readouterr().out
    assert torch.equal(io.read_array(str(d / "m31.i64"), torch.int64), want)
    # the file feeds --weights (31 bits leave room for the NQ queries): at r = inf the total mass per query
    pre = str(d / "mass")
    assert radius_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", pre, "--profile", "inf", "--weights",
                            str(d / "m31.i64"), "--pairs-only", "--device", "cpu"]) == 0
    assert int(io.read_array(pre + ".wpairs", torch.int64)[0]) == NQ * int(want.sum())
    capsys.readouterr()
    assert tools.main(["fixweights", str(d / "m.float"), str(d / "x.i64"), "--bits", "63"]) == 1
    io.write_array(str(d / "nan.float"), torch.tensor([1.0, float("nan")]))
    assert tools.main(["fixweights", str(d / "nan.float"), str(d / "x.i64")]) == 1


@pytest.mark.parametrize("period", [None, "1"])
def test_profile_without_weights_writes_what_it_always_wrote(files, period):
    """--profile alone: PREFIX.profile / PREFIX.pairs equal the unweighted oracle byte for byte and
    no weighted file appears."""
    d, p, q, w, wq = files
    pre = str(d / f"plain_{period}")
    opts = ["--profile", RADII, "--device", "cpu"] + ([] if period is None else ["--period", period])
    assert radius_app.main([str(d / "p.float3"), str(d / "q.float3"), "-o", pre] + opts) == 0
    cut2s = [E.cut2_of(float(v)) for v in RADII.split(",")]
    want = K.radius_profile_cpu(p, q, cut2s, None if period is None else float(period))
    assert want.dtype == torch.int32
    assert raw(pre + ".profile") == want.numpy().tobytes()
    assert raw(pre + ".pairs") == want.sum(0, dtype=torch.int64).numpy().tobytes()
    assert not (d / f"plain_{period}.wprofile").exists() and not (d / f"plain_{period}.wpairs").exists()
    assert tools.main(["rcheck", str(d / "p.float3"), str(d / "q.float3"), pre, "--profile", RADII] + opts[4:]) == 0

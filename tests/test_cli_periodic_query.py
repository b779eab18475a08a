"""hipKNN_query --period and lsknn_tools check --period: the files written in two chunks are
byte-identical to the Python API's results and pass the check against the periodic oracle; a
bad --period exits with status 1. On the CPU device, and (marked gpu) on the GPU."""
import math

import pytest
import torch

from datasets import uniform
from mpi_cuda_largescaleknn_amd.apps import query as query_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.utils import io

N, NQ, K_ = 3000, 500, 8
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pquery")
    p, q = uniform(N, seed=61), uniform(NQ, seed=62)
    io.write_points(str(d / "p.float3"), p)
    io.write_points(str(d / "q.float3"), q)
    return d, p, q


@pytest.mark.parametrize("period", ["1", "1,inf,0.999"])
@pytest.mark.parametrize("device", DEVICES)
def test_query_cli_equals_the_api_and_passes_the_check(files, device, period):
    d, p, q = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    per = tuple(float(v) for v in period.split(",")) if "," in period else float(period)
    out, pre = str(d / f"kth_{device}.float"), str(d / f"nb_{device}")
    common = ["-k", str(K_), "--period", period, "--chunk", str(NQ // 2 + 1), "--device", device]
    assert query_app.main([fp, fq, "-o", out] + common) == 0
    want = E.knn_query_distances(p.to(device), q.to(device), K_, period=per).cpu()
    assert torch.equal(io.read_floats(out).view(torch.int32), want.view(torch.int32))
    assert tools.main(["check", fp, out, "-k", str(K_), "--queries", fq, "--period", period]) == 0
    assert tools.main(["check", fp, out, "-k", str(K_), "--queries", fq]) == 1  # the open box differs: it wraps

    out2 = out + "2"
    assert query_app.main([fp, fq, "-o", out2, "--neighbors", pre] + common) == 0
    idx, dist = (t.cpu() for t in E.knn_query_neighbors(p.to(device), q.to(device), K_, period=per))
    assert torch.equal(io.read_rows(pre + ".ids", K_, torch.int32), idx)
    assert torch.equal(io.read_rows(pre + ".dist", K_, torch.float32).view(torch.int32), dist.view(torch.int32))
    assert torch.equal(io.read_floats(out2).view(torch.int32), want.view(torch.int32))
    assert tools.main(["check", fp, out2, "-k", str(K_), "--queries", fq, "--neighbors", pre, "--period", period]) == 0
    assert tools.main(["check", fp, out2, "-k", str(K_), "--queries", fq, "--neighbors", pre]) == 1


def test_an_open_period_writes_the_open_box_files(files):
    d, p, q = files
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    a, b = str(d / "open_a.float"), str(d / "open_b.float")
    assert query_app.main([fp, fq, "-o", a, "-k", str(K_), "--device", "cpu", "--period", "inf"]) == 0
    assert query_app.main([fp, fq, "-o", b, "-k", str(K_), "--device", "cpu"]) == 0
    assert torch.equal(io.read_floats(a).view(torch.int32), io.read_floats(b).view(torch.int32))
    assert not math.isinf(float(io.read_floats(a).max()))


@pytest.mark.parametrize("bad", ["0", "-1", "1,2", "nan", "x"])
def test_a_bad_period_exits_1(files, bad):
    d = files[0]
    fp, fq = str(d / "p.float3"), str(d / "q.float3")
    args = [fp, fq, "-o", str(d / "bad.float"), "-k", "4", "--device", "cpu", f"--period={bad}"]
    assert query_app.main(args) == 1
    assert query_app.main(args + ["--neighbors", str(d / "bad_nb")]) == 1


def test_check_needs_queries_for_a_period(files):
    d = files[0]
    fp = str(d / "p.float3")
    out = str(d / "self.float")
    io.write_floats(out, torch.zeros(N), 0, truncate=True, total_records=N)
    assert tools.main(["check", fp, out, "-k", "4", "--period", "1"]) == 1

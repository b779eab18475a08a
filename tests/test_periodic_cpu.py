"""Periodic boundaries on the CPU: the brute-force oracle of the minimum-image distance
(K.radius_periodic_cpu / radius_periodic_count_cpu / cluster_periodic_cpu), wrap_points, the
argument checks of the `period` keyword and the command-line tools on the CPU device. Data and
oracle results are computed once per module."""
import math

import numpy as np
import pytest
import torch

from mpi_cuda_largescaleknn_amd.apps import cluster as cluster_app
from mpi_cuda_largescaleknn_amd.apps import radius as radius_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

from datasets import uniform

INF = math.inf
OPEN = (INF, INF, INF)
N = 3000
R = 0.08  # about 26 points per ball at N = 12 000 (the bracket test)

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def pts_unit():
    return cached("unit", lambda: uniform(N, seed=3))


def counts_of(offsets):
    return (offsets[1:] - offsets[:-1]).int()


def n_clusters(labels):
    return E.compact_labels(labels)[1]


def same_partition(a, b):
    """Two label vectors describe the same partition (noise stays noise)."""
    a, b = a.tolist(), b.tolist()
    fwd, bwd = {}, {}
    for x, y in zip(a, b):
        if (x < 0) != (y < 0):
            return False
        if fwd.setdefault(x, y) != y or bwd.setdefault(y, x) != x:
            return False
    return True


# ---------------------------------------------------------------- 1. open period
def test_open_period_equals_the_open_box_oracle_bit_for_bit():
    p = pts_unit()
    q = uniform(500, seed=4)
    cut2 = E.cut2_of(R)
    a, b = K.radius_cpu(p, q, cut2), K.radius_periodic_cpu(p, q, cut2, OPEN)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(K.radius_count_cpu(p, q, cut2), K.radius_periodic_count_cpu(p, q, cut2, OPEN))
    assert torch.equal(K.radius_periodic_count_cpu(p, q, cut2, INF), counts_of(a[0]))
    for min_pts in (1, 4):
        want = K.cluster_cpu(p, E.cut2_of(0.04), min_pts)
        got = K.cluster_periodic_cpu(p, E.cut2_of(0.04), min_pts, OPEN)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # per-query cutoffs through the same entry
    g = torch.Generator().manual_seed(5)
    qc = (torch.rand(500, generator=g) * 0.1) ** 2
    a, b = K.radius_var_cpu(p, q, qc, None), K.radius_periodic_cpu(p, q, 0.0, OPEN, qc)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 2. symmetry
@pytest.mark.parametrize("shift", [0.0, 4096.0])
def test_pairs_are_symmetric_in_their_bits(shift):
    p = (pts_unit()[:2000] + shift).contiguous()
    offsets, idx, d2 = K.radius_periodic_cpu(p, p, E.cut2_of(R), 1.0)
    rows = torch.repeat_interleave(torch.arange(p.shape[0]), counts_of(offsets).long())
    bits = d2.view(torch.int32).long()
    fwd = set(zip(rows.tolist(), idx.tolist(), bits.tolist()))
    assert len(fwd) == idx.numel()
    assert fwd == set(zip(idx.tolist(), rows.tolist(), bits.tolist()))
    if shift == 0.0:  # the case really wraps
        assert idx.numel() > int(K.radius_count_cpu(p, p, E.cut2_of(R)).sum())


# ---------------------------------------------------------------- 3. exact translation invariance
def test_translation_by_grid_steps_is_exact():
    g = torch.Generator().manual_seed(6)
    p = (torch.randint(0, 1024, (2500, 3), generator=g).float() / 1024.0).contiguous()
    r, eps = 0.09, 0.05
    base = K.radius_periodic_cpu(p, p, E.cut2_of(r), 1.0)
    base_l = K.cluster_periodic_cpu(p, E.cut2_of(eps), 1, 1.0)[0]
    base_l3 = K.cluster_periodic_cpu(p, E.cut2_of(eps), 3, 1.0)[0]
    assert int(base[0][-1]) > int(K.radius_count_cpu(p, p, E.cut2_of(r)).sum())
    for t in ((311, 0, 1023), (512, 512, 512), (1, 700, 64)):
        moved = E.wrap_points(p + torch.tensor(t, dtype=torch.float32) / 1024.0, 1.0)
        assert float(moved.min()) >= 0.0 and float(moved.max()) < 1.0
        got = K.radius_periodic_cpu(moved, moved, E.cut2_of(r), 1.0)
        assert torch.equal(got[0], base[0])  # counts
        assert torch.equal(got[2], base[2])  # sorted distances, row by row
        assert same_partition(K.cluster_periodic_cpu(moved, E.cut2_of(eps), 1, 1.0)[0], base_l)
        assert same_partition(K.cluster_periodic_cpu(moved, E.cut2_of(eps), 3, 1.0)[0], base_l3)


# ---------------------------------------------------------------- 4. float64 bracket
def test_float64_bracket_of_the_minimum_image():
    n = 12_000
    p = uniform(n, seed=7)
    cut2 = E.cut2_of(R)
    offsets, idx, _ = K.radius_periodic_cpu(p, p, cut2, 1.0)
    got = torch.zeros((n, n), dtype=torch.bool)
    rows = torch.repeat_interleave(torch.arange(n), counts_of(offsets).long())
    got[rows, idx.long()] = True
    x = p.double()  # (an independent float64 evaluation: d -= L round(d / L))
    lo, hi = cut2 * (1.0 - 2.0 ** -14), cut2 * (1.0 + 2.0 ** -14)
    admitted = between = 0
    for b in range(0, n, 500):  # in slabs: the full float64 difference array would be 3.5 GB
        d = x[b:b + 500, None, :] - x[None, :, :]
        d -= 1.0 * torch.round(d / 1.0)
        d2 = (d * d).sum(-1)
        inside, outside = d2 < lo, d2 >= hi
        g = got[b:b + 500]
        assert not (inside & ~g).any(), "a pair clearly inside the ball is missing"
        assert not (outside & g).any(), "a pair clearly outside the ball was admitted"
        between += int((~inside & ~outside).sum())
        admitted += int(inside.sum())
    # the shell holds about 1.5 * 2^-13 = 0.02 % of a ball's volume: the reference's own
    # undecided pairs stay well inside the cap, and so do the ones the oracle admitted
    assert between <= 0.001 * admitted, (between, admitted)
    assert int(got.sum()) - admitted <= 0.001 * admitted
    assert 20 < admitted / n < 32  # about 26 per ball


# ---------------------------------------------------------------- 5. closed forms
def corner_blobs():
    g = torch.Generator().manual_seed(8)
    corners = torch.tensor([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    blobs = []
    for c in corners:
        off = torch.rand((50, 3), generator=g) * 0.01
        blobs.append(torch.where(c == 0.0, off, 1.0 - 0.01 + off * 0.999))
    p = torch.cat(blobs).float().contiguous()
    assert float(p.min()) >= 0.0 and float(p.max()) < 1.0
    return p


def cut_chain():
    x = 0.005 + 0.01 * torch.arange(100, dtype=torch.float64)
    x = x[(x <= 0.47) | (x >= 0.53)].float()
    return torch.stack([x, torch.full_like(x, 0.5), torch.full_like(x, 0.5)], dim=1).contiguous()


def closed_forms(cluster):
    """The three closed forms through `cluster(points, eps, period or None) -> labels`."""
    p = corner_blobs()
    assert n_clusters(cluster(p, 0.05, 1.0)) == 1
    assert n_clusters(cluster(p, 0.05, None)) == 8
    c = cut_chain()
    assert n_clusters(cluster(c, 0.015, 1.0)) == 1
    assert n_clusters(cluster(c, 0.015, None)) == 2


def test_closed_forms():
    def cluster(p, eps, period):
        if period is None:
            return K.cluster_cpu(p, E.cut2_of(eps), 1)[0]
        return K.cluster_periodic_cpu(p, E.cut2_of(eps), 1, period)[0]

    closed_forms(cluster)
    closed_forms(lambda p, eps, period: E.cluster_points(p, eps, 1, period=period)[0])
    one = torch.tensor([[0.3, 0.9, 0.0]])
    assert K.radius_periodic_count_cpu(one, one, E.cut2_of(0.5), 1.0).tolist() == [1]
    assert E.radius_query_counts(one, one, 0.5, period=1.0).tolist() == [1]


# ---------------------------------------------------------------- 6. wrap_points
def test_wrap_points_range_and_idempotence():
    g = torch.Generator().manual_seed(9)
    below1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    special = torch.tensor([[1.0, -1e-10, -0.0], [math.nan, 2.5, -0.25], [below1, -1e-7, 5.0],
                            [INF, -INF, 0.0], [-3.0, 1e-30, -1e-30]], dtype=torch.float32)
    p = torch.cat([special, (torch.rand((5000, 3), generator=g) - 0.5) * 7.0])
    w = E.wrap_points(p, 1.0)
    fin = torch.isfinite(p)
    assert bool(((w >= 0.0) & (w < 1.0))[fin].all())
    assert torch.equal(w[~fin].nan_to_num(7.0, 8.0, 9.0), p[~fin].nan_to_num(7.0, 8.0, 9.0))
    assert w[0].tolist() == [0.0, 0.0, 0.0] and w[1, 1:].tolist() == [0.5, 0.75] and w[2, 0].item() == below1
    again = E.wrap_points(w, 1.0)
    assert torch.equal(again.nan_to_num(7.0, 8.0, 9.0), w.nan_to_num(7.0, 8.0, 9.0))
    # anisotropic, an open axis and an origin; origin + L itself maps to the origin
    per, org = (2.0, INF, 0.75), (-1.0, 0.0, 10.0)
    q = torch.cat([torch.tensor([[1.0, 123.0, 10.75], [-1.0, -5.0, 10.0]]), p])
    w = E.wrap_points(q, per, org)
    fin = torch.isfinite(q)
    assert torch.equal(w[:, 1][fin[:, 1]], q[:, 1][fin[:, 1]])  # the open axis passes through
    assert bool(((w[:, 0] >= -1.0) & (w[:, 0] < 1.0))[fin[:, 0]].all())
    assert bool(((w[:, 2] >= 10.0) & (w[:, 2] < 10.75))[fin[:, 2]].all())
    assert w[0].tolist() == [-1.0, 123.0, 10.0] and w[1].tolist() == [-1.0, -5.0, 10.0]
    assert torch.equal(E.wrap_points(w, per, org).nan_to_num(7.0, 8.0, 9.0), w.nan_to_num(7.0, 8.0, 9.0))
    with pytest.raises(ValueError):
        E.wrap_points(p, 0.0)
    with pytest.raises(ValueError):
        E.wrap_points(p.double(), 1.0)


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors():
    p = pts_unit()
    index = E.build_index(p)
    q = p[:20].contiguous()
    above = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    above_sq = float(np.nextafter(np.float32(0.25), np.float32(1.0)))
    for fn in (lambda r, **kw: E.radius_counts(index, q, r, period=1.0, **kw),
               lambda r, **kw: E.radius_neighbors(index, q, r, period=1.0, **kw),
               lambda r, **kw: E.radius_query_counts(p, q, r, period=1.0, **kw),
               lambda r, **kw: E.radius_query_neighbors(p, q, r, period=1.0, **kw),
               lambda r, **kw: E.radius_self_neighbors(q, r, period=1.0, **kw),
               lambda r, **kw: E.cluster_labels(index, r, 2, period=1.0, **kw),
               lambda r, **kw: E.cluster_points(q, r, 2, period=1.0, **kw)):
        fn(0.5)  # r equal to L / 2 is accepted
        fn(0.25, squared=True)
        with pytest.raises(ValueError):
            fn(above)
        with pytest.raises(ValueError):
            fn(above_sq, squared=True)
    # the shortest finite axis decides; an open axis sets no bound
    E.radius_counts(index, q, 0.5, period=(1.0, INF, 2.0))
    E.radius_counts(index, q, 1e6, period=OPEN)
    with pytest.raises(ValueError):
        E.radius_counts(index, q, 0.5, period=(2.0, INF, 0.99))
    # a tensor of radii: the bound joins the entry check
    rad = torch.full((20,), 0.1)
    rad[7] = 0.5
    assert E.radius_counts(index, q, rad, period=1.0).shape == (20,)
    rad[7] = above
    with pytest.raises(ValueError):
        E.radius_counts(index, q, rad, period=1.0)
    with pytest.raises(ValueError):
        E.radius_neighbors(index, q, torch.full((20,), above_sq), squared=True, period=1.0)
    E.radius_neighbors(index, q, torch.full((20,), 0.25), squared=True, period=1.0)
    for bad in (0.0, -1.0, math.nan, (1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, math.nan, 1.0), (1.0, 0.0, INF), "x"):
        with pytest.raises(ValueError):
            E.radius_counts(index, q, 0.1, period=bad)
        with pytest.raises(ValueError):
            E.cluster_labels(index, 0.1, 1, period=bad)
        with pytest.raises(ValueError):
            K.radius_periodic_cpu(p, q, 0.01, bad)
    pr = torch.full((N,), 0.05)
    for fn in (lambda: E.point_radius_counts(index, q, pr, period=1.0),
               lambda: E.point_radius_neighbors(index, q, pr, period=1.0),
               lambda: E.point_radius_query_counts(p, q, pr, period=1.0),
               lambda: E.point_radius_query_neighbors(p, q, pr, period=1.0),
               lambda: E.point_radius_self_neighbors(p, pr, period=1.0)):
        with pytest.raises(ValueError, match="not supported"):
            fn()


# ---------------------------------------------------------------- 8. command-line tools, CPU device
def test_cli_round_trip_and_error_exits(tmp_path, capsys):
    g = torch.Generator().manual_seed(10)
    raw = ((torch.rand((4000, 3), generator=g) - 0.25) * 2.0).contiguous()  # [-0.5, 1.5)
    fr, fp, fq = (str(tmp_path / n) for n in ("raw.float3", "p.float3", "q.float3"))
    io.write_points(fr, raw)
    assert tools.main(["wrap", fr, fp, "--period", "1"]) == 0
    assert open(fp, "rb").read() == E.wrap_points(raw, 1.0).numpy().tobytes()
    f2 = str(tmp_path / "p2.float3")
    assert tools.main(["wrap", fr, f2, "--period", "1,inf,0.5", "--origin", "0.25,0,-1"]) == 0
    assert open(f2, "rb").read() == E.wrap_points(raw, (1.0, INF, 0.5), (0.25, 0.0, -1.0)).numpy().tobytes()
    p = io.read_points(fp)
    io.write_points(fq, p[:700].contiguous())
    pre = str(tmp_path / "rad")
    assert radius_app.main([fp, fq, "-r", "0.07", "--period", "1", "-o", pre, "--device", "cpu"]) == 0
    assert tools.main(["rcheck", fp, fq, pre, "-r", "0.07", "--period", "1"]) == 0
    assert tools.main(["rcheck", fp, fq, pre, "-r", "0.07"]) == 1  # the open box differs: it really wraps
    fr2 = str(tmp_path / "radii.float")
    io.write_array(fr2, torch.rand(700, generator=g) * 0.1, 0, truncate=True)
    pre_v = str(tmp_path / "radv")
    assert radius_app.main([fp, fq, "--radii", fr2, "--period", "1,1,inf", "-o", pre_v, "--device", "cpu"]) == 0
    assert tools.main(["rcheck", fp, fq, pre_v, "--radii", fr2, "--period", "1,1,inf"]) == 0
    pre_c = str(tmp_path / "clu")
    assert cluster_app.main([fp, "-r", "0.05", "--min-pts", "3", "--period", "1", "-o", pre_c, "--device", "cpu"]) == 0
    assert tools.main(["ccheck", fp, pre_c, "-r", "0.05", "--min-pts", "3", "--period", "1"]) == 0
    assert tools.main(["ccheck", fp, pre_c, "-r", "0.05", "--min-pts", "3"]) == 1
    capsys.readouterr()
    # --period with --point-radii: exit 1 and a message
    fpr = str(tmp_path / "prad.float")
    io.write_array(fpr, torch.full((4000,), 0.05), 0, truncate=True)
    assert radius_app.main([fp, fq, "--point-radii", fpr, "--period", "1", "-o", pre, "--device", "cpu"]) == 1
    assert "--period" in capsys.readouterr().err
    assert tools.main(["rcheck", fp, fq, pre, "--point-radii", fpr, "--period", "1"]) == 1
    # a radius above half the period: exit 1 and a message, nothing searched
    assert radius_app.main([fp, fq, "-r", "0.6", "--period", "1", "-o", pre, "--device", "cpu"]) == 1
    assert "period" in capsys.readouterr().err
    assert cluster_app.main([fp, "-r", "0.6", "--period", "1", "-o", pre_c, "--device", "cpu"]) == 1
    assert "period" in capsys.readouterr().err
    for bad in ("0", "1,2", "nan", "x"):
        with pytest.raises(SystemExit):
            radius_app.main([fp, fq, "-r", "0.05", "--period", bad, "-o", pre, "--device", "cpu"])

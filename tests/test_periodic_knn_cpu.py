"""Periodic k-NN on the CPU: the brute-force oracles K.kth_periodic_cpu / K.knn_periodic_cpu bit
for bit against a plain numpy reference of the contract (periodic_knn_ref), their consistency
with the periodic radius oracle and the open-box oracles, the CPU-index path of the public
functions and the argument checks of `period`. References are computed once per module."""
import math

import numpy as np
import pytest
import torch

import periodic_knn_ref as R
from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.parallel import pipelines as PL
from mpi_cuda_largescaleknn_amd.parallel.stream import SetStream

INF = math.inf
N, NQ = 2000, 300
KS = (1, 16, 100)

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def data(name):
    """(points, period): a generator's points wrapped into the unit box, or an edge case."""
    def make():
        if name == "far":
            return (uniform(N, seed=41) + 4096.0).contiguous(), 1.0
        if name == "aniso":
            return (uniform(N, seed=42) * torch.tensor([1.0, 2.0, 1.0])).contiguous(), (1.0, 2.0, 1.0)
        if name == "unwrapped":
            return (uniform(N, seed=43) * 2.0 - 0.5).contiguous(), 1.0
        if name == "mixed":
            return uniform(N, seed=44), (1.0, INF, 1.0)
        return E.wrap_points(GENERATORS[name](N, seed=40), 1.0).contiguous(), 1.0
    return cached(("data", name), make)


def queries(name):
    """Half data points, half random over the data's range."""
    def make():
        p = data(name)[0]
        g = torch.Generator().manual_seed(45)
        lo, hi = p.min(0).values, p.max(0).values
        return torch.cat([p[torch.randint(0, N, (NQ // 2,), generator=g)],
                          lo + (hi - lo) * torch.rand((NQ - NQ // 2, 3), generator=g)]).contiguous()
    return cached(("queries", name), make)


def reference(name, cut2=INF):
    """The numpy lists at k = max(KS): the lists at a smaller k are their first k columns."""
    p, per = data(name)
    return cached(("ref", name, cut2), lambda: R.knn_periodic(p, queries(name), max(KS), cut2, R.as_period(per)))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_oracles(p, q, k, cut2, per, ref_idx, ref_d2):
    idx, d2 = K.knn_periodic_cpu(p, q, k, cut2, per)
    assert np.array_equal(idx.numpy(), ref_idx)
    assert same_bits(d2.numpy(), ref_d2)
    assert same_bits(K.kth_periodic_cpu(p, q, k, cut2, per).numpy(), ref_d2[:, k - 1])


# ---------------------------------------------------------------- 1. the numpy reference
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(GENERATORS) + ["unwrapped", "far", "aniso", "mixed"])
def test_oracles_equal_the_numpy_reference(name, k):
    p, per = data(name)
    ref_idx, ref_d2 = reference(name)
    check_oracles(p, queries(name), k, INF, per, ref_idx[:, :k], ref_d2[:, :k])


def test_the_cases_wrap():
    """Otherwise the comparison above would say nothing about the period."""
    for name in ("uniform", "far", "aniso", "mixed", "unwrapped"):
        p, per = data(name)
        q = queries(name)
        assert (K.kth_periodic_cpu(p, q, 16, INF, per) != K.kth_cpu(p, q, 16, INF)).float().mean() > 0.1, name


@pytest.mark.parametrize("k", [N, N + 1])
def test_k_at_and_above_n(k):
    p, per = data("uniform")
    q = queries("uniform")[:20]
    ref_idx, ref_d2 = R.knn_periodic(p, q, k, INF, R.as_period(per))
    check_oracles(p, q, k, INF, per, ref_idx, ref_d2)
    assert (ref_idx[:, N:] == -1).all() and np.isinf(ref_d2[:, N:]).all() and (ref_idx[:, :N] >= 0).all()


def test_cutoff_leaves_rows_unfilled():
    p, per = data("uniform")
    cut2 = E.cut2_of(0.1)  # about 8 of 2000 points per ball: k = 16 is never reached, k = 1 mostly
    ref_idx, ref_d2 = reference("uniform", cut2)
    for k in (1, 16):
        check_oracles(p, queries("uniform"), k, cut2, per, ref_idx[:, :k], ref_d2[:, :k])
    filled = (ref_idx[:, :16] >= 0).sum(1)
    assert filled.min() < 16 and filled.max() > 1
    assert (ref_d2[:, :16][ref_idx[:, :16] < 0] == np.float32(cut2)).all()


def test_nan_and_inf_queries_have_no_neighbours():
    p, per = data("uniform")
    q = queries("uniform")[:4].clone()
    q[0, 1], q[1, 0], q[2, 2] = float("nan"), INF, -INF
    idx, d2 = K.knn_periodic_cpu(p, q, 3, INF, per)
    assert (idx[:3] == -1).all() and torch.isinf(d2[:3]).all() and (idx[3] >= 0).all()
    assert torch.isinf(K.kth_periodic_cpu(p, q, 3, INF, per)[:3]).all()
    ref_idx, ref_d2 = R.knn_periodic(p, q, 3, INF, R.as_period(per))
    assert np.array_equal(idx.numpy(), ref_idx) and same_bits(d2.numpy(), ref_d2)


# ---------------------------------------------------------------- 2. the other oracles
def test_first_k_of_the_periodic_radius_rows():
    p, per = data("uniform")
    q = queries("uniform")
    k = 16
    r = 0.3  # <= L/2; the ball holds about 226 of 2000 points
    offsets, ridx, rd2 = K.radius_periodic_cpu(p, q, E.cut2_of(r), per)
    assert int((offsets[1:] - offsets[:-1]).min()) >= k
    idx, d2 = K.knn_periodic_cpu(p, q, k, INF, per)
    rows = offsets[:-1, None] + torch.arange(k)[None, :]
    assert torch.equal(ridx[rows], idx)
    assert torch.equal(rd2[rows].view(torch.int32), d2.view(torch.int32))


@pytest.mark.parametrize("period", [INF, (INF, INF, INF)])
def test_open_period_equals_the_open_box_oracles(period):
    p = data("uniform")[0]
    q = queries("uniform")
    for k, cut2 in ((1, INF), (16, INF), (16, E.cut2_of(0.1))):
        assert torch.equal(K.kth_periodic_cpu(p, q, k, cut2, period).view(torch.int32),
                           K.kth_cpu(p, q, k, cut2).view(torch.int32))
        a, b = K.knn_periodic_cpu(p, q, k, cut2, period), K.knn_cpu(p, q, k, cut2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---------------------------------------------------------------- 3. the public functions, CPU index
def final(d2):
    return K.finalize_distances(torch.as_tensor(np.ascontiguousarray(d2)).reshape(-1)).view(d2.shape)


@pytest.mark.parametrize("name", ["uniform", "aniso", "mixed"])
def test_public_functions_on_a_cpu_index(name):
    p, per = data(name)
    q = queries(name)
    k = 16
    ref_idx, ref_d2 = reference(name)
    want_idx, want_dist = torch.as_tensor(ref_idx[:, :k].copy()), final(ref_d2[:, :k])
    index = E.build_index(p)
    cfg = E.KnnConfig(k=k)
    flagged = torch.ones(NQ, dtype=torch.bool)
    got = E.query_points(index, q, cfg, period=per, flagged=flagged)
    assert torch.equal(got.view(torch.int32), want_dist[:, k - 1].contiguous().view(torch.int32))
    assert not flagged.any()  # (the CPU path flags nothing)
    assert torch.equal(E.knn_query_distances(p, q, k, period=per), got)
    for idx, dist in (E.query_neighbors(index, q, cfg, period=per), E.knn_query_neighbors(p, q, k, period=per)):
        assert torch.equal(idx, want_idx) and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32))
    sidx, sdist = E.knn_neighbors(p, 4, period=per)
    assert torch.equal(sdist[:, 0], torch.zeros(N))
    oidx, od2 = K.knn_periodic_cpu(p, p, 4, INF, per)
    assert torch.equal(sidx, oidx) and torch.equal(sdist, K.finalize_distances(od2.view(-1)).view(N, 4))
    # an open period and no period are the same call
    a = E.query_neighbors(index, q, cfg, period=(INF, INF, INF))
    b = E.query_neighbors(index, q, cfg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_empty_inputs():
    p, per = data("uniform")
    none = torch.empty((0, 3))
    assert E.knn_query_distances(p, none, 4, period=per).shape == (0,)
    assert torch.isinf(E.knn_query_distances(none, p[:5], 4, period=per)).all()
    idx, dist = E.knn_query_neighbors(none, p[:5], 4, period=per)
    assert (idx == -1).all() and torch.isinf(dist).all()


# ---------------------------------------------------------------- 4. argument checks
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), (1.0, 2.0), (1.0, 0.0, 1.0), "x"])
def test_a_bad_period_is_a_value_error(bad):
    p = data("uniform")[0]
    q = queries("uniform")
    index = E.build_index(p)
    cfg = E.KnnConfig(k=4)
    for call in (lambda: E.query_points(index, q, cfg, period=bad),
                 lambda: E.query_neighbors(index, q, cfg, period=bad),
                 lambda: E.knn_query_distances(p, q, 4, period=bad),
                 lambda: E.knn_query_neighbors(p, q, 4, period=bad),
                 lambda: E.knn_neighbors(p, 4, period=bad),
                 lambda: E.knn_query_distances(torch.empty((0, 3)), q, 4, period=bad),
                 lambda: K.kth_periodic_cpu(p, q, 4, INF, bad),
                 lambda: K.knn_periodic_cpu(p, q, 4, INF, bad)):
        with pytest.raises(ValueError):
            call()


def test_unsupported_paths_say_so():
    p = data("uniform")[0]
    cfg = E.KnnConfig(k=4)
    index = E.build_index(p)
    rotated = E.build_index(p)
    rotated.qrot = rotated.pts  # (stands for an index built in a rotated frame)
    line = E.build_index(p)
    line.line = True
    for call in (lambda: E.knn_distances(p, 4, period=1.0),
                 lambda: SetStream(None, cfg, period=1.0),
                 lambda: PL.unordered_knn(p, None, cfg, period=1.0),
                 lambda: PL.prepartitioned_knn(p, None, cfg, period=1.0),
                 lambda: E.query_points(rotated, p, cfg, period=1.0),
                 lambda: E.query_neighbors(rotated, p, cfg, period=1.0),
                 lambda: E.query_points(line, p, cfg, period=1.0),
                 lambda: E.query_neighbors(line, p, cfg, period=1.0),
                 lambda: E.point_radius_counts(index, p, torch.full((N,), 0.01), period=1.0),
                 lambda: E.point_radius_neighbors(index, p, torch.full((N,), 0.01), period=1.0)):
        with pytest.raises(ValueError, match="not supported"):
            call()


def test_an_open_period_is_no_period_for_every_index():
    """(inf, inf, inf) equals None before the index is looked at: a line-keyed index answers as
    without the keyword, a rotated-frame one refuses foreign queries as it always does."""
    p = data("uniform")[0]
    q = queries("uniform")
    cfg = E.KnnConfig(k=4)
    line = E.build_index(p)
    line.line = True
    assert torch.equal(E.query_points(line, q, cfg, period=INF), E.query_points(line, q, cfg))
    a, b = E.query_neighbors(line, q, cfg, period=(INF, INF, INF)), E.query_neighbors(line, q, cfg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    rotated = E.build_index(p)
    rotated.qrot = rotated.pts
    for period in (None, INF):
        with pytest.raises(ValueError, match="serves its own points only"):
            E.query_points(rotated, q, cfg, period=period)

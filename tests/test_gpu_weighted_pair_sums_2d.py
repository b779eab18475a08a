"""Weighted anisotropic pair sums on the GPU (pair_counts_2d.hip, the weight policy):
weighted_pair_sums_rppi / weighted_pair_sums_smu, the whole [B1, B2] array bit for bit against the
brute-force oracle K.weighted_pair_sums_2d_cpu, against the unweighted walk with unit weights and
against weighted_pair_sums on the same GPU index where the two must agree. The shapes, data,
queries and indexes are those of test_gpu_pair_counts_2d.py (N = 12 000 points: 188 buckets, tree
depth 8; NQ = 1500 queries), shared with it; everything is an integer, so there is no tolerance.

Weights are uniform in +-2^34 (the high word and the second readlane matter), query weights in
+-2^4: (sum |w|) * (sum |wq|) <= 12 000 * 2^34 * 1500 * 2^4 ~ 2^62.1 < 2^63."""
import pytest
import torch

import test_gpu_pair_counts_2d as base
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF, N, NQ, ISO = base.INF, base.N, base.NQ, base.ISO
data, queries, index_of, grid, radii_of, r_for = (base.data, base.queries, base.index_of, base.grid, base.radii_of,
                                                  base.r_for)


def weights(n=N, bits=34, seed=61):
    def make():
        g = torch.Generator().manual_seed(seed)
        return torch.randint(-(1 << bits), (1 << bits) + 1, (n,), generator=g, dtype=torch.int64)
    return base.cached(("weights", n, bits, seed), make)


def query_weights(nq=NQ):
    return weights(nq, 4, 62)


def fn_of(mode):
    return E.weighted_pair_sums_rppi if mode == "rppi" else E.weighted_pair_sums_smu


def oracle(mode, p, q, first, second, w, wq, los, period):
    a2 = [E.cut2_of(r) for r in first]
    b2 = [E.cut2_of(r) for r in second]
    return K.weighted_pair_sums_2d_cpu(p, q, a2, b2, w, mode, los, period, query_weights=wq)


def same(got, want):
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} of {want.numel()} cells differ, first "
                               f"{[(tuple(c), int(got[tuple(c)]), int(want[tuple(c)])) for c in bad[:4].tolist()]}")


def check(mode, index, p, q, first, second, w, wq, los=2, period=None, stats=None):
    got = fn_of(mode)(index, q.to(DEV), first, second, w.to(DEV), query_weights=None if wq is None else wq.to(DEV),
                      los=los, period=period, stats=stats)
    assert got.dtype == torch.int64 and got.shape == (len(first), len(second)) and got.device.type == "cuda"
    got = got.cpu()
    same(got, oracle(mode, p, q, first, second, w, wq, los, period))
    return got


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "clustered", "duplicates"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_equals_the_oracle(mode, name, period):
    E.reset_kernels_used()
    first, second = grid(mode, 5, 7, period)
    w, wq = weights(), query_weights()
    assert int(w.abs().max()) > 1 << 32 and bool((w < 0).any()) and bool((wq < 0).any())
    stats = E.KnnStats()
    got = check(mode, index_of(name), data(name), queries(name), first, second, w, wq, period=period, stats=stats)
    assert "weighted_pair_sums_2d" in E.kernels_used()
    assert int(got[-1, -1]) != 0 and stats.counters["radius_evals"] > 0 and stats.counters["radius_nodes"] > 0
    if mode == "smu":
        assert stats.counters["radius_box_accepts"] == 0
    if name == "uniform":  # once without query weights
        check(mode, index_of(name), data(name), queries(name), first, second, w, None, period=period)


# ---------------------------------------------------------------- 2. unit weights: the unweighted walk
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_unit_weights_equal_the_counts_and_the_walks_are_the_same(mode, period):
    index, q = index_of("clustered"), queries("clustered").to(DEV)
    first, second = grid(mode, 5, 7, period)
    ones = torch.ones(N, dtype=torch.int64, device=DEV)
    sc, sw = E.KnnStats(), E.KnnStats()
    counts = (E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu)(index, q, first, second, period=period,
                                                                          stats=sc)
    sums = fn_of(mode)(index, q, first, second, ones, period=period, stats=sw)
    assert torch.equal(sums, counts) and int(counts[-1, -1]) > N
    assert sw.counters == sc.counters and sc.counters["radius_evals"] > 0
    sums = fn_of(mode)(index, q, first, second, ones, query_weights=torch.ones(NQ, dtype=torch.int64, device=DEV),
                       period=period)
    assert torch.equal(sums, counts)


# ---------------------------------------------------------------- 3. whole boxes: W[p1] - W[p0]
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
def test_coarse_grid_accepts_whole_boxes(period):
    top = 0.5 if period else r_for(N / 4.0)
    first, second = [0.5 * top, top], [0.6 * top, top]
    stats = E.KnnStats()
    check("rppi", index_of("uniform"), data("uniform"), queries("uniform"), first, second, weights(),
          query_weights(), period=period, stats=stats)
    assert stats.counters["radius_box_accepts"] > 0
    stats = E.KnnStats()
    check("smu", index_of("uniform"), data("uniform"), queries("uniform"), first, [0.6, INF], weights(),
          query_weights(), period=period, stats=stats)
    assert stats.counters["radius_box_accepts"] == 0


# ---------------------------------------------------------------- 4. slices
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("shape", ((1, 1), (40, 60), (2048, 1)), ids=str)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_grid_sizes_and_slices(mode, shape, period):
    """1 x 1; 40 x 60 = 2400 cells > 2048: two slices of whole rows; 2048 x 1: one slice of 2048 rows."""
    first, second = grid(mode, *shape, period)
    check(mode, index_of("uniform"), data("uniform"), queries("uniform"), first, second, weights(), query_weights(),
          period=period)


# ---------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("nq", (1, 64, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_query_counts_at_the_group_edge(mode, nq, period):
    first, second = grid(mode, 5, 7, period)
    check(mode, index_of("uniform"), data("uniform"), queries("uniform", nq), first, second, weights(),
          query_weights(nq), period=period)


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("n", (1, 64, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_point_counts_at_the_bucket_edge(mode, n, period):
    p = data("uniform", n)
    q = torch.cat([p, queries("uniform", 100)])
    first, second = grid(mode, 5, 7, period)
    if period is None:
        first[-1] = second[-1] = INF
    w, wq = weights(n), query_weights(n + 100)
    got = check(mode, index_of("uniform", n), p, q, first, second, w, wq, period=period)
    if period is None and mode == "rppi":  # every pair
        assert int(got[-1, -1]) == int(w.sum()) * int(wq.sum())


def test_non_finite_queries():
    p = data("uniform")
    q = queries("uniform").clone()
    q[3, 0] = float("nan")
    q[70, 2] = INF
    q[200, 1] = -INF
    for mode in ("rppi", "smu"):
        first, second = grid(mode, 5, 7, ISO)
        check(mode, index_of("uniform"), p, q, first, second, weights(), query_weights(), period=ISO)
    bad = ~torch.isfinite(q).all(1)
    first, second = grid("rppi", 5, 7, None)
    got = E.weighted_pair_sums_rppi(index_of("uniform"), q[bad].to(DEV), first, second, weights().to(DEV))
    assert int(got.abs().sum()) == 0


def test_duplicated_and_extreme_edges():
    p, q, index = data("duplicates"), queries("duplicates"), index_of("duplicates")
    w, wq = weights(), query_weights()
    check("rppi", index, p, q, [0.0, 0.0, 0.05, 0.05, 0.3, INF], [0.0, 0.01, 0.01, 0.2, INF, INF], w, wq)
    check("rppi", index, p, q, [0.3], [0.0], w, wq)
    check("smu", index, p, q, [0.0, 0.0, 0.05, 0.05, 0.3, INF], [0.0, 0.0, 0.5, 1.0, 1.0, INF, INF], w, wq)


@pytest.mark.parametrize("los", (1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_non_cubic_period_with_an_open_axis(mode, los):
    per = (1.0, INF, 0.8)  # bounds 0.5, none, 0.4
    first, second = grid(mode, 5, 7, None)
    first = [min(r, 0.4) for r in first]
    if mode == "rppi" and los == 2:
        second = [min(r, 0.4) for r in second]
    check(mode, index_of("uniform"), data("uniform"), queries("uniform"), first, second, weights(), query_weights(),
          los=los, period=per)


@pytest.mark.parametrize("los", (0, 1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_every_line_of_sight(mode, los):
    first, second = grid(mode, 5, 7, ISO)
    if mode == "rppi":
        second = [0.01, 0.03, 0.07, 0.07, 0.2, 0.35, 0.5]  # a grid that is not symmetric in the axes
    p, q, index = data("clustered"), queries("clustered"), index_of("clustered")
    got = check(mode, index, p, q, first, second, weights(), query_weights(), los=los, period=ISO)
    again = fn_of(mode)(index, q.to(DEV), first, second, weights().to(DEV), query_weights=query_weights().to(DEV),
                        los="xyz"[los], period=ISO)
    assert torch.equal(again.cpu(), got)


# ---------------------------------------------------------------- 6. against weighted_pair_sums on the same index
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("los", (0, 1, 2))
def test_a_plane_across_the_line_of_sight_gives_the_isotropic_sums(los, period):
    """Points and queries whose line-of-sight coordinate is one constant have par2 = 0 and, the fma
    of a zero being exact, d2 == perp2 bit for bit: the first column of (rp, pi) is the isotropic
    weighted pair sum."""
    p = data("clustered").clone()
    q = queries("clustered").clone()
    p[:, los] = 0.25
    q[:, los] = 0.25
    index = E.build_index(p.to(DEV))
    pw = E.prepare_point_weights(index, weights().to(DEV))
    wq = query_weights().to(DEV)
    R = radii_of(9, top=0.5 if period else None)
    got = E.weighted_pair_sums_rppi(index, q.to(DEV), R, [0.5 if period else 1.0], pw, query_weights=wq, los=los,
                                    period=period)
    want = E.weighted_pair_sums(index, q.to(DEV), R, pw, query_weights=wq, period=period)
    assert got.shape == (9, 1) and torch.equal(got[:, 0], want) and int(want[-1]) != 0


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "duplicates"))
def test_every_mu_gives_the_isotropic_sums_without_the_zero_distances(name, period):
    """par2 < inf * d2 holds for every pair with d2 > 0: column mu = inf is the isotropic weighted
    pair sum less the sums over the pairs at distance 0."""
    index, q = index_of(name), queries(name).to(DEV)
    pw = E.prepare_point_weights(index, weights().to(DEV))
    wq = query_weights().to(DEV)
    R = radii_of(9, top=0.5 if period else None)
    got = E.weighted_pair_sums_smu(index, q, R, [INF], pw, query_weights=wq, los=1, period=period)
    zero = E.weighted_pair_sums(index, q, [2.0 ** -149], pw, query_weights=wq, squared=True, period=period)[0]
    want = E.weighted_pair_sums(index, q, R, pw, query_weights=wq, period=period) - zero
    assert int(zero) != 0 and torch.equal(got[:, 0], want)


# ---------------------------------------------------------------- 7. prepared weights, the self form, repeatability
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_point_weights_prepared_once_serve_chunks(mode):
    index, q = index_of("clustered"), queries("clustered").to(DEV)
    pw = E.prepare_point_weights(index, weights().to(DEV))
    wq = query_weights().to(DEV)
    first, second = grid(mode, 5, 7, ISO)
    whole = fn_of(mode)(index, q, first, second, pw, query_weights=wq, period=ISO)
    parts = [fn_of(mode)(index, q[s].contiguous(), first, second, pw, query_weights=wq[s].contiguous(), period=ISO)
             for s in (slice(0, 700), slice(700, NQ))]
    assert torch.equal(parts[0] + parts[1], whole)
    assert torch.equal(whole, fn_of(mode)(index, q, first, second, weights().to(DEV), query_weights=wq, period=ISO))
    other = E.build_index(data("clustered").to(DEV))
    with pytest.raises(ValueError, match="another index"):
        fn_of(mode)(other, q, first, second, pw, period=ISO)


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_the_self_form_has_the_weights_on_both_sides(mode):
    p = data("uniform")
    w = weights(N, 16, 63)  # (sum |w|)^2 ~ (12 000 * 2^15)^2 ~ 2^57.1 < 2^63
    first, second = grid(mode, 3, 7 if mode == "smu" else 3, ISO)
    fs = E.weighted_pair_self_sums_rppi if mode == "rppi" else E.weighted_pair_self_sums_smu
    got = fs(p.to(DEV), first, second, w.to(DEV), period=ISO).cpu()
    same(got, oracle(mode, p, p, first, second, w, w, 2, ISO))
    fq = E.weighted_pair_query_sums_rppi if mode == "rppi" else E.weighted_pair_query_sums_smu
    assert torch.equal(fq(p.to(DEV), p.to(DEV), first, second, w.to(DEV), query_weights=w.to(DEV), period=ISO).cpu(),
                       got)


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_two_runs_give_the_same_bits(mode):
    first, second = grid(mode, 40, 60, ISO)
    q = queries("clustered").to(DEV)
    w, wq = weights().to(DEV), query_weights().to(DEV)
    a = fn_of(mode)(index_of("clustered"), q, first, second, w, query_weights=wq, period=ISO)
    b = fn_of(mode)(index_of("clustered"), q, first, second, w, query_weights=wq, period=ISO)
    assert torch.equal(a, b) and int(E.shell_counts_2d(a).sum()) == int(a[-1, -1])


def test_gpu_argument_errors_come_before_any_kernel():
    index, q = index_of("uniform"), queries("uniform").to(DEV)
    w = weights().to(DEV)
    ok = (0.1, 0.2)
    E.reset_kernels_used()
    for fn in (E.weighted_pair_sums_rppi, E.weighted_pair_sums_smu):
        with pytest.raises(ValueError, match=fn.__name__):
            fn(index, q, ok, ok, w.cpu())
        with pytest.raises(ValueError, match=fn.__name__):
            fn(index, q, ok, ok, w, query_weights=query_weights())
        with pytest.raises(ValueError, match=fn.__name__):
            fn(index, q, ok, ok, w.int())
        with pytest.raises(ValueError, match="2\\^63"):
            fn(index, q, ok, ok, w, query_weights=torch.full((NQ,), 1 << 20, dtype=torch.int64, device=DEV))
    assert E.kernels_used() == []

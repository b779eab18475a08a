"""Weighted radius profiles on the GPU (weighted_profile.hip): weighted_profile and
weighted_pair_sums bit for bit against the brute-force oracle K.weighted_profile_cpu /
K.weighted_pair_sums_cpu, against the neighbour lists and, with unit weights, against
radius_profile / pair_counts on the same GPU index. Every row is compared; everything is an
integer, so there is no tolerance. Data, indexes and weights are computed once per module."""
import math

import numpy as np
import pytest
import torch

import radius_profile_ref as R
from datasets import GENERATORS, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of the walk (as test_gpu_radius_profile.py)
NQ = 1500
M = 4097    # 65 buckets, the last one with a single point
ISO = (1.0, 1.0, 1.0)
PERIODS = pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def slice_width():
    return K.weighted_profile_bins()


# numbers of radii around the kernel's slice width W (known only with the library loaded)
N_RADII = {"1": lambda W: 1, "2": lambda W: 2, "W-1": lambda W: W - 1, "W": lambda W: W, "W+1": lambda W: W + 1,
           "2*W+1": lambda W: 2 * W + 1}


def n_radii(spec):
    return N_RADII[spec](slice_width())


def r_for(count, n=N, volume=1.0):
    """The radius whose ball holds `count` of n uniform points in `volume`."""
    return (3.0 * count * volume / (4.0 * math.pi * n)) ** (1.0 / 3.0)


def radii_of(B, n=N, top=None):
    """B ascending radii for expected counts from ~1 to ~n / 4 (log-spaced), the third one doubled."""
    top = r_for(n / 4.0, n) if top is None else top
    lo = min(r_for(1.0, n), top)
    r = [lo * (top / lo) ** (i / max(B - 1, 1)) for i in range(B)]
    r[-1] = top
    if B > 3:
        r[3] = r[2]
    return r


def data(name, n=N):
    def make():
        if name == "duplicates":
            return GENERATORS[name](n, seed=51, ndistinct=400).contiguous()
        return E.wrap_points(GENERATORS[name](n, seed=51), 1.0).contiguous()
    return cached(("data", name, n), make)


def queries(name, nq=NQ, n=N):
    """Half of them data points, half random over the data's range."""
    def make():
        p = data(name, n)
        g = torch.Generator().manual_seed(52)
        lo, hi = p.min(0).values, p.max(0).values
        q = torch.cat([p[torch.randint(0, p.shape[0], (nq // 2,), generator=g)],
                       lo + (hi - lo) * torch.rand((nq - nq // 2, 3), generator=g)])
        return q[torch.randperm(nq, generator=g)].contiguous()
    return cached(("queries", name, nq, n), make)


def index_of(name, n=N):
    return cached(("index", name, n), lambda: E.build_index(data(name, n).to(DEV)))


def weights(n, seed=70, bits=20):
    """int64 [n] drawn from +-2^bits."""
    def make():
        g = torch.Generator().manual_seed(seed + n)
        return torch.randint(-(1 << bits), (1 << bits) + 1, (n,), generator=g, dtype=torch.int64)
    return cached(("w", n, seed, bits), make)


def cut2s_of(radii):
    return [E.cut2_of(r) for r in radii]


def check(index, p, q, radii, w, period, squared=False, wq=None, stats=None, pairs=True):
    """weighted_profile against the oracle; weighted_pair_sums against its column sums and the
    oracle. w / wq on the CPU. Returns the profile (CPU)."""
    qd, wd = q.to(DEV), w.to(DEV) if isinstance(w, torch.Tensor) else w
    w_cpu = w if isinstance(w, torch.Tensor) else w.weights.cpu()
    got = E.weighted_profile(index, qd, radii, wd, squared=squared, period=period, stats=stats)
    assert got.dtype == torch.int64 and got.shape == (q.shape[0], len(radii)) and got.device.type == "cuda"
    got = got.cpu()
    cut2s = radii if squared else cut2s_of(radii)
    want = K.weighted_profile_cpu(p, q, cut2s, w_cpu, period)
    bad = (got != want).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {q.shape[0]} rows differ from the oracle, first {bad[:5].tolist()}"
    if pairs:
        for qw in (None, wq) if wq is not None else (None,):
            s = E.weighted_pair_sums(index, qd, radii, wd, query_weights=None if qw is None else qw.to(DEV),
                                     squared=squared, period=period)
            assert s.dtype == torch.int64 and s.shape == (len(radii),) and s.device.type == "cuda"
            rows = want if qw is None else want * qw[:, None]
            assert torch.equal(s.cpu(), rows.sum(0, dtype=torch.int64))
            assert torch.equal(s.cpu(), K.weighted_pair_sums_cpu(p, q, cut2s, w_cpu, period, query_weights=qw))
    return got


# ---------------------------------------------------------------- 1. oracle and neighbour lists
@PERIODS
@pytest.mark.parametrize("name", ("uniform", "clustered", "duplicates", "planar"))
def test_equals_the_oracle_and_the_neighbour_lists(name, period):
    E.reset_kernels_used()
    p, q, index, w = data(name, M), queries(name, M, M), index_of(name, M), weights(M)
    radii = radii_of(7, n=M, top=0.5 if period else None)
    got = check(index, p, q, radii, w, period)
    assert "weighted_profile" in E.kernels_used()
    assert torch.equal(got[:, 2], got[:, 3])
    b = 4
    offsets, idx, _ = E.radius_neighbors(index, q.to(DEV), radii[b], sort=False, period=period)
    rows = torch.repeat_interleave(torch.arange(M, device=DEV), offsets[1:] - offsets[:-1])
    seg = torch.zeros(M, dtype=torch.int64, device=DEV).index_add_(0, rows, w.to(DEV)[idx.long()])
    assert int(offsets[-1]) > M and torch.equal(seg.cpu(), got[:, b])


@PERIODS
def test_unit_weights_equal_radius_profile(period):
    index, q = index_of("clustered"), queries("clustered").to(DEV)
    radii = radii_of(slice_width() + 3, top=0.5 if period else None)
    ones = torch.ones(N, dtype=torch.int64, device=DEV)
    got = E.weighted_profile(index, q, radii, ones, period=period)
    ref = E.radius_profile(index, q, radii, period=period)
    assert torch.equal(got, ref.long())
    assert torch.equal(E.weighted_pair_sums(index, q, radii, ones, period=period),
                       E.pair_counts(index, q, radii, period=period))
    # one slice of each kernel: the two walks are the same walk
    sw, su = E.KnnStats(), E.KnnStats()
    E.weighted_profile(index, q, radii[:8], ones, period=period, stats=sw)
    E.radius_profile(index, q, radii[:8], period=period, stats=su)
    assert sw.counters == su.counters and sw.counters["radius_evals"] > 0


@PERIODS
@pytest.mark.parametrize("B", ("1", "2", "W-1", "W", "W+1", "2*W+1"))
def test_every_slice_edge(B, period):
    check(index_of("uniform"), data("uniform"), queries("uniform"), radii_of(n_radii(B), top=0.5 if period else None),
          weights(N), period, wq=weights(NQ, seed=71, bits=10))


# ---------------------------------------------------------------- 2. edge sizes
@PERIODS
@pytest.mark.parametrize("nq", (1, 63, 64, 65, 4097))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_edge_sizes(n, nq, period):
    """Partial buckets, partial query groups and node_span's clipping at n: the largest radii
    take whole nodes (the last, clipped one too) from the prefix sums."""
    p = cached(("edge", n), lambda: uniform(n, seed=53))
    q = cached(("edgeq", nq), lambda: uniform(nq, seed=54))
    index = cached(("edgei", n), lambda: E.build_index(p.to(DEV)))
    radii = radii_of(5, n=max(n, 8), top=0.5 if period else None) + ([] if period else [2.0, INF])
    check(index, p, q, radii, weights(n, bits=28), period, wq=weights(nq, seed=71, bits=10))


# ---------------------------------------------------------------- 3. whole-box acceptance
@PERIODS
def test_whole_boxes_are_accepted_and_the_sum_stays_exact(period):
    """The shape of test_gpu_radius_profile.py's whole-box test, on which the unweighted walk
    accepts boxes; the weights alternate in sign with magnitudes near 2^40, so that a wrong span
    of the prefix sums or a dropped high word cannot cancel by luck."""
    g = torch.Generator().manual_seed(72)
    w = ((1 << 40) + torch.randint(0, 1 << 20, (N,), generator=g, dtype=torch.int64))
    w[1::2] *= -1
    radii = [0.05, 0.2, 0.35, 0.5 if period else 0.8]
    index, q = index_of("uniform"), queries("uniform")
    stats, plain = E.KnnStats(), E.KnnStats()
    got = check(index, data("uniform"), q, radii, w, period, stats=stats, pairs=False)
    c = stats.counters
    print(period, c)
    assert c["radius_box_accepts"] > 0
    assert c["radius_nodes"] > 0 and c["radius_buckets"] > 0
    assert ("radius_images" in c) == (period is not None)
    E.radius_profile(index, q.to(DEV), radii, period=period, stats=plain)
    assert plain.counters == c  # the unweighted walk accepts the same boxes
    # pair sums over as many queries as the bound (sum |w|) * (sum |wq|) < 2^63 admits at 2^40 a weight
    wq = torch.ones(512, dtype=torch.int64)
    wq[::3] = -1
    s = E.weighted_pair_sums(index, q[:512].to(DEV), radii, w.to(DEV), query_weights=wq.to(DEV), period=period)
    assert torch.equal(s.cpu(), (got[:512] * wq[:, None]).sum(0, dtype=torch.int64))


@PERIODS
def test_negative_and_large_weights_use_all_64_bits(period):
    """max|w| * n just under 2^62: a 32-bit readlane mix-up or an int32 accumulator fails here."""
    top = ((1 << 62) - 1) // M
    g = torch.Generator().manual_seed(73)
    w = torch.randint(top // 2, top + 1, (M,), generator=g, dtype=torch.int64)
    w[torch.rand(M, generator=g) < 0.125] *= -1  # mostly positive: the sums themselves come near 2^62
    w[0], w[1] = top, -top
    assert int(w.abs().max()) * M < 1 << 62 <= (int(w.abs().max()) + 1) * M
    p, q, index = data("uniform", M), queries("uniform", M, M), index_of("uniform", M)
    radii = radii_of(6, n=M, top=0.5) + ([] if period else [INF])
    got = check(index, p, q, radii, w, period, pairs=False)
    assert int(got.abs().max()) > 1 << 58  # the sums themselves fill the high word
    if period is None:
        assert bool((got[:, -1] == int(w.sum())).all())
    # two queries with weights +1, -1: (sum |w|) * 2 < 2^63
    q2, wq = q[:2].contiguous(), torch.tensor([1, -1], dtype=torch.int64)
    s = E.weighted_pair_sums(index, q2.to(DEV), radii, w.to(DEV), query_weights=wq.to(DEV), period=period)
    assert torch.equal(s.cpu(), got[0] - got[1])


# ---------------------------------------------------------------- 4. cutoffs on existing values
@PERIODS
def test_cutoffs_on_and_one_ulp_around_a_distance(period):
    """Strictness per shell: a pair at d2 is out at the cutoff d2 itself and in one float above it."""
    p, q, w = data("clustered"), queries("clustered"), weights(N)
    v = R.dist2(p, q[:40], period)
    pick = np.sort(v.reshape(-1))[[50, 700, 5000, 20000]]
    assert np.all(pick > 0) and np.all(pick < 0.25)
    cuts = []
    for d2 in pick:
        cuts += [np.nextafter(d2, np.float32(0)), d2, np.nextafter(d2, np.float32(1))]
    cuts = np.unique(np.asarray(cuts, dtype=np.float32))
    cut2s = [float(c) for c in cuts]
    got = check(index_of("clustered"), p, q, cut2s, w, period, squared=True)
    for d2 in pick:
        b = int(np.searchsorted(cuts, d2))
        on = torch.from_numpy(v == d2)
        assert int(on.sum()) >= 1
        assert int((got[:40, b + 1] - got[:40, b]).sum()) == int((on * w[None, :]).sum())
    # adjacent cutoffs one ulp apart around a populated distance: [near, far] of a node straddles one
    mid = np.sort(R.dist2(data("uniform"), queries("uniform")[:8], period).reshape(-1))[3000]
    cuts = [mid]
    for _ in range(5):
        cuts.append(np.nextafter(cuts[-1], np.float32(1)))
        cuts.insert(0, np.nextafter(cuts[0], np.float32(0)))
    check(index_of("uniform"), data("uniform"), queries("uniform"), [float(c) for c in cuts], w, period, squared=True)


# ---------------------------------------------------------------- 5. pair sums
@PERIODS
@pytest.mark.parametrize("B", ("1", "W", "W+1"))
@pytest.mark.parametrize("nq", (4097, 20000))
def test_pair_sums_equal_weighted_column_sums_and_the_oracle(nq, B, period):
    p, q, w = data("uniform"), queries("uniform", nq), weights(N)
    index, qd, wd = index_of("uniform"), q.to(DEV), w.to(DEV)
    radii = radii_of(n_radii(B), top=r_for(200.0))
    cut2s = cut2s_of(radii)
    prof = E.weighted_profile(index, qd, radii, wd, period=period)
    for wq in (None, weights(nq, seed=71, bits=12), -torch.ones(nq, dtype=torch.int64)):
        wqd = None if wq is None else wq.to(DEV)
        a = E.weighted_pair_sums(index, qd, radii, wd, query_weights=wqd, period=period)
        assert a.dtype == torch.int64 and a.shape == (len(radii),)
        rows = prof if wqd is None else prof * wqd[:, None]
        assert torch.equal(a, rows.sum(0, dtype=torch.int64))
        assert torch.equal(a.cpu(), K.weighted_pair_sums_cpu(p, q, cut2s, w, period, query_weights=wq))


def test_pair_sums_never_allocate_the_profile():
    nq, B = 1 << 20, slice_width()
    index = cached("memi", lambda: E.build_index(uniform(20000, seed=57).to(DEV)))
    q = torch.rand((nq, 3), generator=torch.Generator().manual_seed(58)).to(DEV)
    radii = radii_of(B, n=20000, top=r_for(100.0, 20000))
    pw = E.prepare_point_weights(index, weights(20000).to(DEV))
    wq = weights(nq, seed=71, bits=8).to(DEV)
    E.weighted_pair_sums(index, q[:4096], radii, pw, query_weights=wq[:4096])  # (warm: first allocations)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pairs = E.weighted_pair_sums(index, q, radii, pw, query_weights=wq)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - base
    assert used < nq * B * 8, f"{used} bytes above the baseline, the profile array has {nq * B * 8}"
    part = (E.weighted_profile(index, q[:65536], radii, pw) * wq[:65536, None]).sum(0, dtype=torch.int64)
    assert torch.equal(E.weighted_pair_sums(index, q[:65536], radii, pw, query_weights=wq[:65536]), part)
    assert int(pairs.abs().sum()) > 0


def test_prepared_weights_serve_chunked_queries_and_reject_another_index():
    index, q, w = index_of("uniform"), queries("uniform").to(DEV), weights(N).to(DEV)
    radii = radii_of(5)
    before = [t.clone() for t in (index.pts, index.perm, index.nodes)]
    pw = E.prepare_point_weights(index, w)
    assert torch.equal(pw.sorted, w[index.perm[:N].long()])
    assert pw.prefix.shape == (N + 1,) and int(pw.prefix[0]) == 0
    assert torch.equal(pw.prefix[1:], torch.cumsum(pw.sorted, 0)) and pw.abs_sum == int(w.abs().sum())
    whole = E.weighted_profile(index, q, radii, w)
    chunks = [E.weighted_profile(index, q[a:a + 400], radii, pw) for a in range(0, NQ, 400)]
    assert torch.equal(torch.cat(chunks), whole)
    sums = sum(E.weighted_pair_sums(index, q[a:a + 400], radii, pw, period=ISO) for a in range(0, NQ, 400))
    assert torch.equal(sums, E.weighted_pair_sums(index, q, radii, w, period=ISO))
    for t, b in zip((index.pts, index.perm, index.nodes), before):
        assert torch.equal(t, b)  # the index is not written
    other = E.build_index(data("uniform").to(DEV))
    for fn in (E.weighted_profile, E.weighted_pair_sums):
        with pytest.raises(ValueError, match="another index"):
            fn(other, q, radii, pw)


# ---------------------------------------------------------------- 6. special values
@PERIODS
def test_bad_queries_zero_and_infinite_radii(period):
    p, index, w = data("uniform"), index_of("uniform"), weights(N)
    q = queries("uniform").clone()
    q[5, 0] = math.nan
    q[70, 2] = INF
    q[700] = -INF
    radii = [0.0, 0.0, 0.05, 0.05, 0.3] + ([] if period else [INF, INF])
    got = check(index, p, q, radii, w, period, wq=weights(NQ, seed=71, bits=10))
    finite = torch.isfinite(q).all(dim=1)
    assert int(got[~finite].abs().sum()) == 0
    assert int(got[:, :2].abs().sum()) == 0
    assert torch.equal(got[:, 2], got[:, 3])
    if period is None:
        assert bool((got[finite][:, 5:] == int(w.sum())).all())
    zeros = E.weighted_profile(index, q.to(DEV), [0.0], w.to(DEV))
    assert zeros.shape == (NQ, 1) and int(zeros.abs().sum()) == 0
    assert int(E.weighted_pair_sums(index, q.to(DEV), [0.0, 0.0], w.to(DEV))[1]) == 0


def test_an_open_period_equals_the_open_box():
    index, q, w = index_of("clustered"), queries("clustered").to(DEV), weights(N).to(DEV)
    radii = radii_of(9) + [INF]
    a = E.weighted_profile(index, q, radii, w)
    assert torch.equal(a, E.weighted_profile(index, q, radii, w, period=(INF, INF, INF)))
    assert torch.equal(E.weighted_pair_sums(index, q, radii, w), E.weighted_pair_sums(index, q, radii, w, period=INF))


def test_anisotropic_period_with_an_open_axis():
    p = cached("aniso", lambda: (uniform(N, seed=55) * torch.tensor([1.0, 2.0, 1.0])).contiguous())
    q = cached("anisoq", lambda: (uniform(NQ, seed=56) * torch.tensor([1.0, 2.0, 1.0])).contiguous())
    check(E.build_index(p.to(DEV)), p, q, radii_of(6, top=0.5), weights(N), (1.0, 2.0, INF),
          wq=weights(NQ, seed=71, bits=10))


@PERIODS
def test_two_runs_give_the_same_bits(period):
    index, q, w = index_of("clustered"), queries("clustered", 20000).to(DEV), weights(N, bits=25).to(DEV)
    wq = weights(20000, seed=71, bits=10).to(DEV)
    radii = radii_of(slice_width() + 1, top=0.5 if period else None)
    a = E.weighted_pair_sums(index, q, radii, w, query_weights=wq, period=period)
    b = E.weighted_pair_sums(index, q, radii, w, query_weights=wq, period=period)
    assert torch.equal(a, b)
    assert torch.equal(E.weighted_profile(index, q, radii, w, period=period),
                       E.weighted_profile(index, q, radii, w, period=period))


def test_self_forms_and_the_empty_cases():
    p, w = data("duplicates", M).to(DEV), weights(M, bits=16).to(DEV)
    radii = [0.0, 1e-6, 0.1]
    prof = E.weighted_self_profile(p, radii, w)
    assert torch.equal(prof.cpu(), K.weighted_profile_cpu(p.cpu(), p.cpu(), cut2s_of(radii), w.cpu()))
    assert torch.equal(E.weighted_pair_self_sums(p, radii, w), (prof * w[:, None]).sum(0, dtype=torch.int64))
    assert torch.equal(E.weighted_pair_self_sums(p, radii, w, query_weights=torch.ones_like(w), period=ISO),
                       E.weighted_self_profile(p, radii, w, period=ISO).sum(0, dtype=torch.int64))
    none = torch.empty((0, 3), dtype=torch.float32, device=DEV)
    index = E.build_index(p)
    assert E.weighted_profile(index, none, [0.1, 0.2], w).shape == (0, 2)
    assert E.weighted_pair_sums(index, none, [0.1, 0.2], w).tolist() == [0, 0]
    assert E.weighted_query_profile(none, p, [0.1], w[:0]).shape == (M, 1)


def test_errors_on_the_device():
    index, q, w = index_of("uniform"), queries("uniform").to(DEV), weights(N).to(DEV)
    line = E.build_index(GENERATORS["line"](2000, seed=59).to(DEV),
                         frame=E.LineAxis(torch.tensor([1.0, 0.2, -0.1], device=DEV)))
    assert line.line
    rot = E.build_index(GENERATORS["tilted_plane"](N, seed=59).to(DEV), frame=torch.eye(3, device=DEV))
    assert rot.qrot is not None
    wq = torch.ones(NQ, dtype=torch.int64, device=DEV)
    E.reset_kernels_used()
    for fn in (E.weighted_profile, E.weighted_pair_sums):
        for kw in (dict(radii=[]), dict(radii=[0.2, 0.1]), dict(radii=[-1.0]), dict(radii=[0.6], period=1.0),
                   dict(radii=torch.tensor([0.1], device=DEV))):
            with pytest.raises(ValueError):
                fn(index, q, weights=w, **kw)
        for bad in (w.int(), w.double(), w[:-1], w[:, None], w.cpu()):  # dtype, shape, device
            with pytest.raises(ValueError):
                fn(index, q, [0.1], bad)
        with pytest.raises(ValueError):
            fn(index, q.cpu(), [0.1], w)
        with pytest.raises(ValueError, match="not supported"):
            fn(line, q, [0.1], w[:2000])
        with pytest.raises(ValueError, match="not supported"):
            fn(rot, q, [0.1], w)
        big = torch.zeros(N, dtype=torch.int64, device=DEV)  # max|w| * n >= 2^62
        big[17] = -((1 << 62) // N + 1)
        with pytest.raises(ValueError, match="2\\^62"):
            fn(index, q, [0.1], big)
    for bad in (wq.int(), wq[:-1], wq.cpu()):
        with pytest.raises(ValueError, match="query_weights"):
            E.weighted_pair_sums(index, q, [0.1], w, query_weights=bad)
    heavy = torch.full((N,), 1 << 40, dtype=torch.int64, device=DEV)  # A_p = N * 2^40 > 2^53
    with pytest.raises(ValueError, match="2\\^63"):
        E.weighted_pair_sums(index, q, [0.1], heavy, query_weights=wq << 10)  # A_q = 1500 * 2^10 > 2^20
    with pytest.raises(ValueError, match="2\\^63"):
        E.weighted_pair_sums(index, q, [0.1], heavy)  # A_q = nq = 1500 > 2^10
    assert E.kernels_used() == []
    # the edges of both bounds, on a small index: 2^62 - 1 and 2^63 - 1 pass and are exact
    third = ((1 << 62) - 1) // 3
    p3 = uniform(3, seed=48)
    i3 = E.build_index(p3.to(DEV))
    w3 = torch.tensor([third, third, -third], dtype=torch.int64, device=DEV)
    assert E.weighted_profile(i3, p3.to(DEV), [INF], w3)[:, 0].tolist() == [third] * 3
    with pytest.raises(ValueError, match="2\\^62"):
        E.weighted_profile(i3, p3.to(DEV), [INF], w3 + torch.tensor([1, 0, 0], device=DEV))
    one = torch.tensor([0, 1, 0], dtype=torch.int64, device=DEV)
    ok = torch.tensor([1 << 62, 0, -((1 << 62) - 1)], dtype=torch.int64, device=DEV)  # A_q = 2^63 - 1
    assert E.weighted_pair_sums(i3, p3.to(DEV), [1e-3, INF], one, query_weights=ok).tolist() == [0, 1]
    with pytest.raises(ValueError, match="2\\^63"):
        E.weighted_pair_sums(i3, p3.to(DEV), [INF], one, query_weights=ok - torch.tensor([0, 0, 1], device=DEV))

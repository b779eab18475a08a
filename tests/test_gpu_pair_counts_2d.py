"""Anisotropic pair counts on the GPU (pair_counts_2d.hip): pair_counts_rppi / pair_counts_smu, the
whole [B1, B2] array bit for bit against the brute-force oracle K.pair_counts_2d_cpu, and against
pair_counts on the same GPU index where the two must agree. Data, indexes and queries are
computed once per module; everything is an integer, so there is no tolerance."""
import math

import pytest
import torch

from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
N = 12_000  # 188 buckets, tree depth 8: two expansion stages of the walk
NQ = 1500
ISO = (1.0, 1.0, 1.0)
MU = (0.1, 0.3, 0.5, 0.5, 0.8, 1.0, INF)

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


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
            return GENERATORS[name](n, seed=51, ndistinct=max(1, n // 30)).contiguous()
        return E.wrap_points(GENERATORS[name](n, seed=51), 1.0).contiguous()
    return cached(("data", name, n), make)


def queries(name, nq=NQ):
    """Half of them data points, half random over the data's range, six of those moved to within
    0.001 of a face of the unit box each."""
    def make():
        p = data(name)
        g = torch.Generator().manual_seed(52)
        lo, hi = p.min(0).values, p.max(0).values
        rnd = lo + (hi - lo) * torch.rand((nq - nq // 2, 3), generator=g)
        for f in range(min(6, rnd.shape[0])):
            rnd[f, f % 3] = 0.001 if f < 3 else 0.999
        q = torch.cat([p[torch.randint(0, p.shape[0], (nq // 2,), generator=g)], rnd])
        return q[torch.randperm(nq, generator=g)].contiguous()
    return cached(("queries", name, nq), make)


def index_of(name, n=N):
    return cached(("index", name, n), lambda: E.build_index(data(name, n).to(DEV)))


def grid(mode, B1, B2, period):
    top = 0.5 if period else None
    if mode == "rppi":
        return radii_of(B1, top=top), radii_of(B2, top=top)
    mu = list(MU) if B2 == len(MU) else [(j + 1) / B2 for j in range(B2 - 1)] + [INF]
    return radii_of(B1, top=top), mu


def oracle(mode, p, q, first, second, los, period):
    a2 = [E.cut2_of(r) for r in first]
    b2 = [E.cut2_of(r) for r in second]
    return K.pair_counts_2d_cpu(p, q, a2, b2, mode, los, period)


def check(mode, index, p, q, first, second, los=2, period=None, stats=None):
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    got = fn(index, q.to(DEV), first, second, los=los, period=period, stats=stats)
    assert got.dtype == torch.int64 and got.shape == (len(first), len(second)) and got.device.type == "cuda"
    got = got.cpu()
    want = oracle(mode, p, q, first, second, los, period)
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} of {want.numel()} cells differ from the oracle, first "
                               f"{[(tuple(c), int(got[tuple(c)]), int(want[tuple(c)])) for c in bad[:4].tolist()]}")
    return got


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "clustered", "duplicates"))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_equals_the_oracle(mode, name, period):
    E.reset_kernels_used()
    first, second = grid(mode, 5, 7, period)
    stats = E.KnnStats()
    got = check(mode, index_of(name), data(name), queries(name), first, second, period=period, stats=stats)
    assert "pair_counts_2d" in E.kernels_used()
    assert int(got[-1, -1]) > N and int(got[0, 0]) < int(got[-1, -1])
    assert stats.counters["radius_evals"] > 0 and stats.counters["radius_nodes"] > 0
    if period:
        assert stats.counters["radius_images"] > (NQ + 63) // 64  # queries near every face: more than one image
    if mode == "smu":
        assert stats.counters["radius_box_accepts"] == 0


@pytest.mark.parametrize("los", (0, 1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_every_line_of_sight(mode, los):
    first, second = grid(mode, 5, 7, ISO)
    if mode == "rppi":
        second = [0.01, 0.03, 0.07, 0.07, 0.2, 0.35, 0.5]  # a grid that is not symmetric in the axes
    p, q, index = data("clustered"), queries("clustered"), index_of("clustered")
    got = check(mode, index, p, q, first, second, los=los, period=ISO)
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    assert torch.equal(fn(index, q.to(DEV), first, second, los="xyz"[los], period=ISO).cpu(), got)


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("shape", ((1, 1), (40, 60), (60, 40), (2048, 1), (1, 2048)), ids=str)
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_grid_sizes_and_slices(mode, shape, period):
    """1 x 1; 40 x 60 = 2400 cells > 2048: two slices of whole rows; 2048 x 1: one slice of 2048
    rows; 1 x 2048: one row that fills the slice."""
    first, second = grid(mode, *shape, period)
    check(mode, index_of("uniform"), data("uniform"), queries("uniform"), first, second, period=period)


def test_duplicated_and_extreme_edges():
    p, q, index = data("duplicates"), queries("duplicates"), index_of("duplicates")
    check("rppi", index, p, q, [0.0, 0.0, 0.05, 0.05, 0.3, INF], [0.0, 0.01, 0.01, 0.2, INF, INF])
    check("rppi", index, p, q, [0.0], [0.3])
    check("rppi", index, p, q, [0.3], [0.0])
    check("smu", index, p, q, [0.0, 0.05, 0.05, INF], [0.0, 0.0, 0.5, 1.0, 1.0, INF, INF])
    check("smu", index, p, q, [0.3], [0.0])


# ---------------------------------------------------------------- 2. whole-box acceptance
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
def test_coarse_grid_accepts_whole_boxes(period):
    stats = E.KnnStats()
    top = 0.5 if period else r_for(N / 4.0)
    check("rppi", index_of("uniform"), data("uniform"), queries("uniform"), [0.5 * top, top], [0.6 * top, top],
          period=period, stats=stats)
    assert stats.counters["radius_box_accepts"] > 0


@pytest.mark.parametrize("los", (1, 2))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_non_cubic_period_with_an_open_axis(mode, los):
    per = (1.0, INF, 0.8)  # bounds 0.5, none, 0.4
    first, second = grid(mode, 5, 7, None)
    first = [min(r, 0.4) for r in first]
    if mode == "rppi" and los == 2:
        second = [min(r, 0.4) for r in second]
    stats = E.KnnStats()
    check(mode, index_of("uniform"), data("uniform"), queries("uniform"), first, second, los=los, period=per,
          stats=stats)
    assert stats.counters["radius_images"] > (NQ + 63) // 64


# ---------------------------------------------------------------- 3. edge sizes
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("nq", (1, 64, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_query_counts_at_the_group_edge(mode, nq, period):
    first, second = grid(mode, 5, 7, period)
    check(mode, index_of("uniform"), data("uniform"), queries("uniform", nq), first, second, period=period)


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("n", (1, 64, 65))
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_point_counts_at_the_bucket_edge(mode, n, period):
    p = data("uniform", n)
    q = torch.cat([p, queries("uniform", 100)])
    first, second = grid(mode, 5, 7, period)
    if period is None:
        first[-1] = second[-1] = INF
    got = check(mode, index_of("uniform", n), p, q, first, second, period=period)
    if period is None:  # every pair; (s, mu): but those at distance 0
        same = int((q[:, None, :] == p[None, :, :]).all(-1).sum())
        assert same >= n and int(got[-1, -1]) == (n * (n + 100) if mode == "rppi" else n * (n + 100) - same)


def test_non_finite_queries_and_the_self_form():
    p = data("uniform")
    q = queries("uniform").clone()
    q[3, 0] = float("nan")
    q[70, 2] = INF
    q[200, 1] = -INF
    for mode in ("rppi", "smu"):
        first, second = grid(mode, 5, 7, ISO)
        check(mode, index_of("uniform"), p, q, first, second, period=ISO)
    first, second = grid("rppi", 3, 3, ISO)
    got = E.pair_self_counts_rppi(p.to(DEV), first, second, period=ISO).cpu()
    assert torch.equal(got, oracle("rppi", p, p, first, second, 2, ISO))
    assert int(got[0, 0]) >= N  # every point with itself
    first, second = grid("smu", 3, 7, None)
    got = E.pair_query_counts_smu(p.to(DEV), p.to(DEV), first, second, los="x").cpu()
    assert torch.equal(got, oracle("smu", p, p, first, second, 0, None))
    assert torch.equal(got, E.pair_self_counts_smu(p.to(DEV), first, second, los=0).cpu())


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_two_runs_give_the_same_bits(mode):
    first, second = grid(mode, 40, 60, ISO)
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    q = queries("clustered").to(DEV)
    a = fn(index_of("clustered"), q, first, second, period=ISO)
    b = fn(index_of("clustered"), q, first, second, period=ISO)
    assert torch.equal(a, b)
    D = E.shell_counts_2d(a)
    assert bool((D >= 0).all()) and int(D.sum()) == int(a[-1, -1])


# ---------------------------------------------------------------- 4. against pair_counts on the same index
@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("los", (0, 1, 2))
def test_a_plane_across_the_line_of_sight_gives_pair_counts(los, period):
    """Points and queries whose line-of-sight coordinate is one constant have par2 = 0 and, the
    fma of a zero being exact, d2 == perp2 bit for bit: the first column of (rp, pi) is the
    isotropic pair count."""
    p = data("clustered").clone()
    q = queries("clustered").clone()
    p[:, los] = 0.25
    q[:, los] = 0.25
    index = E.build_index(p.to(DEV))
    R = radii_of(9, top=0.5 if period else None)
    got = E.pair_counts_rppi(index, q.to(DEV), R, [0.5 if period else 1.0], los=los, period=period)
    want = E.pair_counts(index, q.to(DEV), R, period=period)
    assert got.shape == (9, 1) and torch.equal(got[:, 0], want) and int(want[-1]) > 0


@pytest.mark.parametrize("period", (None, ISO), ids=("open", "iso"))
@pytest.mark.parametrize("name", ("uniform", "duplicates"))
def test_every_mu_gives_pair_counts_without_the_zero_distances(name, period):
    """par2 < inf * d2 holds for every pair with d2 > 0: column mu = inf is the isotropic pair count
    less the pairs at distance 0 (those below the smallest positive float32)."""
    index, q = index_of(name), queries(name).to(DEV)
    R = radii_of(9, top=0.5 if period else None)
    got = E.pair_counts_smu(index, q, R, [INF], los=1, period=period)
    zero = E.pair_counts(index, q, [2.0 ** -149], squared=True, period=period)[0]
    want = E.pair_counts(index, q, R, period=period) - zero
    assert int(zero) >= NQ // 2 and torch.equal(got[:, 0], want)


# ---------------------------------------------------------------- 5. the one entry point
def _entry_case():
    """200 uniform points (four buckets, a tree of depth 2), 70 queries (one full group and one
    partial), a 2 x 3 grid per mode; weights on both sides; everything the wrapper takes."""
    def make():
        g = torch.Generator().manual_seed(77)
        p, q = torch.rand((200, 3), generator=g), torch.rand((70, 3), generator=g)
        w = torch.randint(-9, 10, (200,), generator=g, dtype=torch.int64)
        wq = torch.randint(-3, 4, (70,), generator=g, dtype=torch.int64)
        index = E.build_index(p.to(DEV))
        assert index.depth == 2
        qsorted, qperm = E.prepare_queries(index, q.to(DEV), locate=False)[:2]
        pw = E.prepare_point_weights(index, w.to(DEV))
        edges = {"rppi": ([0.2, 0.4], [0.1, 0.25, 0.45]), "smu": ([0.2, 0.4], [0.3, 0.7, INF])}
        cuts = {m: tuple([E.cut2_of(r) for r in e] for e in fs) for m, fs in edges.items()}
        return p, q, w, wq, index, qsorted, qperm, pw, cuts
    return cached("entry", make)


OBSERVER = (0.5, 0.4, -2.0)


def _entry_oracle(mode, los, period, weighted, with_wq):
    p, q, w, wq, _, _, _, _, cuts = _entry_case()
    a2, b2 = cuts[mode]
    wq = wq if with_wq else None
    if isinstance(los, tuple):
        return K.weighted_pair_sums_2d_observer_cpu(p, q, a2, b2, w, mode, los, query_weights=wq) if weighted \
            else K.pair_counts_2d_observer_cpu(p, q, a2, b2, mode, los)
    return K.weighted_pair_sums_2d_cpu(p, q, a2, b2, w, mode, los, period, query_weights=wq) if weighted \
        else K.pair_counts_2d_cpu(p, q, a2, b2, mode, los, period)


def _entry_gpu(mode, los, period, weighted, with_wq):
    _, q, _, wq, index, qsorted, qperm, pw, cuts = _entry_case()
    return K.pair_sums_2d_gpu(index.tree(), qsorted, q.shape[0], *cuts[mode], mode, los, qperm, period,
                              (pw.sorted, pw.prefix) if weighted else None, wq.to(DEV) if with_wq else None).cpu()


_ENTRY_FORMS = ((False, False), (True, False), (True, True))  # (weights, query weights)
_ENTRY_LOS = ((0, None), (1, ISO), (2, None), (2, (1.0, INF, 0.9)), (OBSERVER, None))


@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_one_entry_serves_every_combination(mode):
    """K.pair_sums_2d_gpu once per valid combination of policy, line of sight and box: each result is
    the corresponding oracle's, bit for bit."""
    for weighted, with_wq in _ENTRY_FORMS:
        for los, period in _ENTRY_LOS:
            got = _entry_gpu(mode, los, period, weighted, with_wq)
            want = _entry_oracle(mode, los, period, weighted, with_wq)
            assert got.dtype == torch.int64 and torch.equal(got, want), (mode, weighted, with_wq, los, period)
    assert int(_entry_oracle(mode, 2, None, False, False)[-1, -1]) > 0


def test_one_entry_refuses_what_the_four_could_not_express():
    """Query weights without point weights, an observer with a period, an observer without the host
    copies of the cutoffs: each is refused in host code before anything is queued (the result
    buffer keeps its filling), and the next valid call equals the oracle."""
    from mpi_cuda_largescaleknn_amd import _native
    _, q, _, wq, index, qsorted, qperm, pw, cuts = _entry_case()
    nq, (a2, b2), tree = q.shape[0], cuts["rppi"], index.tree()
    wqd = wq.to(DEV)
    with pytest.raises(_native.NativeError, match="pair_counts_2d: .*wq"):
        K.pair_sums_2d_gpu(tree, qsorted, nq, a2, b2, "rppi", 2, qperm, query_weights=wqd)
    assert torch.equal(_entry_gpu("rppi", 2, None, False, False), _entry_oracle("rppi", 2, None, False, False))
    with pytest.raises(_native.NativeError, match="weighted_pair_sums_2d_observer: .*period"):
        K.pair_sums_2d_gpu(tree, qsorted, nq, a2, b2, "rppi", OBSERVER, qperm, ISO, (pw.sorted, pw.prefix), wqd)
    assert torch.equal(_entry_gpu("rppi", OBSERVER, None, True, True),
                       _entry_oracle("rppi", OBSERVER, None, True, True))

    # the library itself: the wrapper always sends the host copies with an observer
    import ctypes as C
    a, b = torch.tensor(a2), torch.tensor(b2)
    adev, bdev = a.to(DEV), b.to(DEV)
    tv = _native.TreeView(tree[0].data_ptr(), tree[1].data_ptr(), tree[2].data_ptr(), tree[3], tree[4], 0)
    obs, per = (C.c_float * 3)(*OBSERVER), (C.c_float * 3)(*ISO)
    out = torch.full((2, 3), -7, dtype=torch.int64, device=DEV)
    lib = _native.hip()

    def call(a_host, b_host, period, observer, wsorted, wpre, wq_):
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rc = lib.lsk_hip_pair_sums_2d(C.byref(tv), qsorted.data_ptr(), nq, adev.data_ptr(), ptr(a_host), 2,
                                      bdev.data_ptr(), ptr(b_host), 3, 0, 2, period, observer, qperm.data_ptr(),
                                      ptr(wsorted), ptr(wpre), ptr(wq_), out.data_ptr(), None,
                                      torch.cuda.current_stream().cuda_stream)
        return rc, lib.lsk_hip_last_error().decode()

    for args, text in (((None, None, None, None, None, None, wqd), "pair_counts_2d: "),
                       ((a, b, per, obs, None, None, None), "pair_counts_2d_observer: "),
                       ((None, None, None, obs, pw.sorted, pw.prefix, None), "weighted_pair_sums_2d_observer: "),
                       ((a, None, None, obs, None, None, None), "pair_counts_2d_observer: ")):
        rc, msg = call(*args)
        assert rc == 1 and msg.startswith(text), (rc, msg)
        assert bool((out == -7).all())  # not even the zero fill was queued
        assert torch.equal(_entry_gpu("rppi", 2, ISO, True, False), _entry_oracle("rppi", 2, ISO, True, False))
    rc, msg = call(a, b, None, obs, None, None, None)  # the same call, complete
    assert rc == 0, msg
    assert torch.equal(out.cpu(), _entry_oracle("rppi", OBSERVER, None, False, False))

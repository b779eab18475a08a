"""The ball walk (ball_walk.h) at every stage boundary of the bucket tree. The walk expands the
tree kWalkStep = 6 levels at a time, so its control flow depends on the tree's depth: `expand`
fills 2^min(6, depth - lvl) lanes and clips the slots past the last bucket, `node_span` shifts by
depth - lvl and clips at n, and the stack / Cover argument only bites with more than one
expansion stacked. The sizes below are the smallest that reach each case (kBucket = 64):

    n        buckets  depth
    129      3        2      one stage of 2 levels: 4 lanes, slot 3 empty
    2049     33       6      one full-width stage, 31 slots clipped, the last bucket holds 1 point
    4096     64       6      one full stage, every bucket full
    131073   2049     12     two full-width stages, half the slots empty
    262145   4097     13     three stages (6 + 6 + 1), the last bucket holds 1 point

1. At the three small sizes every walk kernel is compared bit for bit with its all-pairs oracle,
   in the open box and under period = 1 (the per-point radii have no periodic form).
2. At the two deep sizes the query-form kernels are compared with the same oracles over 321
   queries (five full groups and one lane of a sixth) that cover both ends of the curve order and
   the faces of the box; `clustered` joins at 262145.
3. At the two deep sizes the self-form kernels (cluster_labels, mst_edges, mst_labels), whose
   oracles are all-pairs, are compared with the sparse exact reference of sparse_ref.py, which
   test_sparse_ref_cpu.py holds to those oracles.

Every data set, index, query set and reference is computed once per module: the module-scoped
fixtures compute the references of one data set before its first test (CPU time, reported as that
test's setup), so a test's own time is the kernels and the comparison."""
import math
import time

import numpy as np
import pytest
import torch

import sparse_ref as S
from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
SHAPE = {129: (3, 2), 2049: (33, 6), 4096: (64, 6), 131_073: (2049, 12), 262_145: (4097, 13)}  # n: (buckets, depth)
SMALL = (129, 2049, 4096)
DEEP = (131_073, 262_145)
SMALL_SETS = [("uniform", n) for n in SMALL]
DEEP_SETS = [("uniform", n) for n in DEEP]
QUERY_SETS = SMALL_SETS + DEEP_SETS + [("clustered", 262_145)]
NQ = 321        # deep sizes: five full groups of 64 and one lane of a sixth
K_NN = 70       # more than one bucket
MU = (0.1, 0.3, 0.5, 0.5, 0.8, 1.0, INF)
# The graph of the pairs within MST_F mean spacings must be connected and hold the whole tree;
# sparse_ref.mst_weights asserts both. 2.5 does at both deep sizes with datasets.uniform(seed=61),
# open and periodic, with and without core distances: 4 053 689 / 4 289 292 pairs (open / period)
# at 131 073 points, 8 205 811 / 8 577 368 at 262 145.
MST_F = 2.5
PERIODS = pytest.mark.parametrize("period", (None, 1.0), ids=("open", "L1"))

_CACHE: dict = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def r_for(count, n):
    """The radius whose ball holds `count` of n uniform points in the unit box."""
    return (3.0 * count / (4.0 * math.pi * n)) ** (1.0 / 3.0)


def radii_of(B, n):
    """B ascending radii for expected counts from ~1 to ~n / 4 (log-spaced), the third one doubled
    (the radii of test_gpu_radius_profile.py). The largest is 0.39: admitted by period = 1."""
    top = r_for(n / 4.0, n)
    lo = min(r_for(1.0, n), top)
    r = [lo * (top / lo) ** (i / max(B - 1, 1)) for i in range(B)]
    r[-1] = top
    if B > 3:
        r[3] = r[2]
    return r


def cut2s_of(radii):
    return [E.cut2_of(r) for r in radii]


def final(d2):
    return K.finalize_distances(d2.reshape(-1)).view(d2.shape)


def bits(t):
    return t.contiguous().view(torch.int32)


def loguniform(m, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(m, generator=g)).float()


class Case:
    """One data set with its index, queries and references, each computed once."""

    def __init__(self, name, n):
        self.name, self.n = name, n
        self.deep = n in DEEP

    def c(self, key, fn):
        return cached((self.name, self.n) + key, fn)

    # ------------------------------------------------------------ data, index, queries
    @property
    def p(self):
        return self.c(("p",), lambda: E.wrap_points(GENERATORS[self.name](self.n, seed=61), 1.0).contiguous())

    @property
    def pd(self):
        return self.c(("pd",), lambda: self.p.to(DEV))

    @property
    def index(self):
        return self.c(("index",), lambda: E.build_index(self.pd, grid=True))

    @property
    def q(self):
        """Small sizes: the data points and 100 random positions. Deep sizes: NQ queries, half of
        them data points with the first and the last 64 positions of the curve order among them,
        half random positions. Six of the random ones lie within 0.001 of a face each."""
        def make():
            p, n = self.p, self.n
            g = torch.Generator().manual_seed(62)
            lo, hi = p.min(0).values, p.max(0).values
            nrnd = NQ - NQ // 2 if self.deep else 100
            rnd = lo + (hi - lo) * torch.rand((nrnd, 3), generator=g)
            for f in range(6):
                rnd[f, f % 3] = 0.001 if f < 3 else 0.999
            if self.deep:
                perm = self.index.perm[:n].cpu().long()
                rows = torch.cat([perm[:64], perm[-64:], torch.randint(0, n, (NQ // 2 - 128,), generator=g)])
                q = torch.cat([p[rows], rnd])
            else:
                q = torch.cat([p, rnd])
            return q[torch.randperm(q.shape[0], generator=g)].contiguous()
        return self.c(("q",), make)

    @property
    def qd(self):
        return self.c(("qd",), lambda: self.q.to(DEV))

    @property
    def groups(self):
        return (self.q.shape[0] + 63) // 64

    # ------------------------------------------------------------ radii
    def radii(self, period):
        """Expected counts from ~1 to ~n / 4, and every point in the open box."""
        return radii_of(7, self.n) + ([INF] if period is None else [])

    def list_radii(self):
        return [r_for(8.0, self.n), min(r_for(500.0, self.n), 0.5)]

    def query_radii(self, period):
        """One radius per query: log-uniform over expected counts 0.5 .. 1000, one 0, one that
        holds a quarter of the set and, in the open box, one infinite."""
        def make():
            n, nq = self.n, self.q.shape[0]
            r = loguniform(nq, r_for(0.5, n), min(r_for(1000.0, n), 0.39), 63)
            r[0] = 0.0
            r[1] = r_for(n / 4.0, n)
            if period is None:
                r[2] = INF
            return r
        return self.c(("qr", period), make)

    @property
    def point_radii(self):
        """One radius per point: log-uniform over expected counts 0.5 .. 50, three of 0.3, one 0,
        one infinite."""
        def make():
            n = self.n
            g = torch.Generator().manual_seed(64)
            r = loguniform(n, r_for(0.5, n), min(r_for(50.0, n), 0.39), 65)
            rows = torch.randperm(n, generator=g)[:5]
            r[rows[:3]] = 0.3
            r[rows[3]] = 0.0
            r[rows[4]] = INF
            return r
        return self.c(("pr",), make)

    @property
    def weights(self):
        def make():
            g = torch.Generator().manual_seed(66)
            return torch.randint(-(1 << 20), (1 << 20) + 1, (self.n,), generator=g, dtype=torch.int64)
        return self.c(("w",), make)

    def grid(self, mode, period, coarse=False):
        """(first, second) edges of a 5 x 7 grid, or a coarse 2 x 2 (rp, pi) grid whose cells hold
        whole boxes."""
        if coarse:
            top = 0.5 if period else r_for(self.n / 4.0, self.n)
            return [0.5 * top, top], [0.6 * top, top]
        first = radii_of(5, self.n)
        return (first, radii_of(7, self.n)) if mode == "rppi" else (first, list(MU))

    def eps(self):
        """0.9 mean spacings."""
        return 0.9 * self.n ** (-1.0 / 3.0)

    # ------------------------------------------------------------ references (brute force)
    def profile_ref(self, period):
        return self.c(("profile", period),
                      lambda: K.radius_profile_cpu(self.p, self.q, cut2s_of(self.radii(period)), period))

    def lists_ref(self, period, r):
        def make():
            cut2 = E.cut2_of(r)
            o, i, d2 = K.radius_cpu(self.p, self.q, cut2) if period is None else \
                K.radius_periodic_cpu(self.p, self.q, cut2, period)
            return o, i, final(d2)
        return self.c(("lists", period, r), make)

    def query_radii_ref(self, period):
        def make():
            qc = self.query_radii(period)
            qc = qc * qc  # (the float32 product: cut2_of)
            o, i, d2 = K.radius_var_cpu(self.p, self.q, qcut2=qc) if period is None else \
                K.radius_periodic_cpu(self.p, self.q, 0.0, period, qcut2=qc)
            return o, i, final(d2)
        return self.c(("qlists", period), make)

    def point_radii_ref(self):
        def make():
            pc = self.point_radii
            o, i, d2 = K.radius_var_cpu(self.p, self.q, pcut2=pc * pc)
            return o, i, final(d2)
        return self.c(("plists",), make)

    def knn_ref(self, period):
        def make():
            i, d2 = K.knn_cpu(self.p, self.q, K_NN, INF) if period is None else \
                K.knn_periodic_cpu(self.p, self.q, K_NN, INF, period)
            return i, final(d2)
        return self.c(("knn", period), make)

    def weighted_ref(self, period):
        return self.c(("weighted", period), lambda: K.weighted_profile_cpu(
            self.p, self.q, cut2s_of(self.radii(period)), self.weights, period))

    def pairs2d_ref(self, mode, period, coarse=False):
        def make():
            first, second = self.grid(mode, period, coarse)
            return K.pair_counts_2d_cpu(self.p, self.q, cut2s_of(first), cut2s_of(second), mode, 2, period)
        return self.c(("pairs2d", mode, period, coarse), make)

    def warm_queries(self):
        for period in (None, 1.0):
            self.profile_ref(period)
            for r in self.list_radii():
                self.lists_ref(period, r)
            self.query_radii_ref(period)
            self.knn_ref(period)
            self.weighted_ref(period)
            for mode in ("rppi", "smu"):
                self.pairs2d_ref(mode, period)
            self.pairs2d_ref("rppi", period, coarse=True)
        self.point_radii_ref()

    # ------------------------------------------------------------ references (self forms)
    def core_dev(self, period):
        """The device's squared 5th-neighbour distances (mst_core_d2), the core distances of the
        trees here; test_core_distances checks them against the oracle."""
        return self.c(("core_dev", period), lambda: E.mst_core_d2(self.index, 5, period=period))

    def cluster_ref(self, period, min_pts):
        """(labels, core) as CPU tensors: the all-pairs oracle at the small sizes, the sparse
        reference at the deep ones."""
        def make():
            cut2 = E.cut2_of(self.eps())
            if not self.deep:
                return K.cluster_cpu(self.p, cut2, min_pts) if period is None else \
                    K.cluster_periodic_cpu(self.p, cut2, min_pts, period)
            labels, core, count = S.dbscan_labels(self.p, cut2, min_pts, period)
            # (not a trivial answer: neither a few clusters nor every point its own)
            assert 1000 < count < self.n // 2, f"{count} clusters"
            return torch.from_numpy(labels), torch.from_numpy(core)
        return self.c(("cluster", period, min_pts), make)

    def mst_pairs(self, period):
        r = np.float32(MST_F * self.n ** (-1.0 / 3.0))
        return self.c(("mst_pairs", period), lambda: S.pairs_within(self.p, np.float32(r * r), period))

    def mst_ref(self, period, with_core):
        """Small sizes: the oracle's (rows, d2). Deep sizes: the ascending weights alone."""
        def make():
            core = self.core_dev(period).cpu() if with_core else None
            if not self.deep:
                return K.mst_cpu(self.p, core) if period is None else K.mst_periodic_cpu(self.p, period, core)
            return torch.from_numpy(S.mst_weights(self.p, MST_F * self.n ** (-1.0 / 3.0), core, period,
                                                  pairs=self.mst_pairs(period))[0])
        return self.c(("mst", period, with_core), make)

    def tree(self, period, with_core):
        """The device's tree: (rows, d2) on the device, and the counters of its rounds."""
        def make():
            E.reset_kernels_used()
            stats = E.KnnStats()
            rows, d2 = E.mst_edges(self.index, self.core_dev(period) if with_core else None, stats=stats,
                                   period=period)
            assert E.LAST_MST_ERRORS[0] == 0
            assert "mst" in E.kernels_used() and "cpu" not in E.kernels_used()
            assert rows.dtype == torch.int32 and d2.dtype == torch.float32 and rows.device.type == DEV
            return rows, d2, stats.counters
        return self.c(("tree", period, with_core), make)

    def warm_self(self):
        for period in (None, 1.0):
            for min_pts in (1, 5):
                self.cluster_ref(period, min_pts)
            for with_core in (False, True):
                self.mst_ref(period, with_core)


def _warm(case, what):
    t = time.perf_counter()
    getattr(case, what)()
    dt = time.perf_counter() - t
    print(f"[setup] {case.name}-{case.n}: {what} took {dt:.1f} s")
    return case


def set_id(s):
    return f"{s[0]}-{s[1]}"


@pytest.fixture(scope="module", params=QUERY_SETS, ids=set_id)
def qcase(request):
    """A data set with the references of the query-form kernels computed."""
    return _warm(Case(*request.param), "warm_queries")


@pytest.fixture(scope="module", params=SMALL_SETS + DEEP_SETS, ids=set_id)
def scase(request):
    """A data set with the references of the self-form kernels computed."""
    return _warm(Case(*request.param), "warm_self")


def same_lists(got, want):
    return all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want)) \
        and torch.equal(bits(got[2]), bits(want[2]))


def lists_of(res, nq):
    offsets, idx, dist = res
    assert E.LAST_RADIUS_ERRORS[0] == 0  # the device error word of the fill pass
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert offsets.shape == (nq + 1,) and idx.shape == dist.shape == (int(offsets[-1]),)
    return offsets.cpu(), idx.cpu(), dist.cpu()


def counts_of(lists):
    return (lists[0][1:] - lists[0][:-1]).int()


def rows_differ(got, want):
    bad = (got != want).reshape(got.shape[0], -1).any(dim=1).nonzero().flatten()
    return f"{bad.numel()} of {got.shape[0]} rows differ from the reference, first {bad[:5].tolist()}"


def check_walk_stats(case, stats, period, accepts):
    """A cull or an acceptance that silently never happens must not pass."""
    c = stats.counters
    print(case.name, case.n, period, c)
    assert c["radius_nodes"] > 0 and c["radius_evals"] > 0
    if case.deep:
        if accepts:
            assert c["radius_box_accepts"] > 0
        if period is not None:  # queries near every face: more than one image per group
            assert c["radius_images"] > case.groups


# ---------------------------------------------------------------- 0. the table
@pytest.mark.parametrize("n", SMALL + DEEP)
def test_the_sizes_reach_the_depths_of_the_table(n):
    buckets, depth = SHAPE[n]
    index = Case("uniform", n).index
    assert index.n == n and (n + 63) // 64 == buckets
    assert index.depth == depth == K.tree_depth(n)
    assert (1 << depth) >= buckets > (1 << depth) // 2  # no shallower tree holds the buckets
    assert index.nodes.shape[0] == 2 << depth
    stages = -(-depth // 6)
    assert stages == {2: 1, 6: 1, 12: 2, 13: 3}[depth]


def test_clustered_at_the_deepest_size():
    assert Case("clustered", 262_145).index.depth == 13


# ---------------------------------------------------------------- 1. + 2. the query-form kernels
@PERIODS
def test_radius_counts_and_neighbors_scalar_radius(qcase, period):
    E.reset_kernels_used()
    want = qcase.profile_ref(period)
    radii = qcase.radii(period)
    stats = E.KnnStats()  # (summed over the radii)
    for b, r in enumerate(radii):
        got = E.radius_counts(qcase.index, qcase.qd, r, period=period, stats=stats)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want[:, b]), f"radius {r}: " + rows_differ(got.cpu(), want[:, b])
    check_walk_stats(qcase, stats, period, accepts=True)
    for r in qcase.list_radii():
        got = lists_of(E.radius_neighbors(qcase.index, qcase.qd, r, period=period), qcase.q.shape[0])
        ref = qcase.lists_ref(period, r)
        assert same_lists(got, ref), f"radius {r}: " + rows_differ(counts_of(got), counts_of(ref))
    assert int(qcase.lists_ref(period, qcase.list_radii()[1])[0][-1]) > qcase.q.shape[0]
    assert ("radius_periodic" if period else "radius") in E.kernels_used() and "cpu" not in E.kernels_used()


@PERIODS
def test_radius_counts_and_neighbors_per_query_radii(qcase, period):
    E.reset_kernels_used()
    qr = qcase.query_radii(period).to(DEV)
    ref = qcase.query_radii_ref(period)
    stats = E.KnnStats()
    got = E.radius_counts(qcase.index, qcase.qd, qr, period=period, stats=stats)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), counts_of(ref)), rows_differ(got.cpu(), counts_of(ref))
    check_walk_stats(qcase, stats, period, accepts=True)
    got = lists_of(E.radius_neighbors(qcase.index, qcase.qd, qr, period=period), qcase.q.shape[0])
    assert same_lists(got, ref), rows_differ(counts_of(got), counts_of(ref))
    c = counts_of(ref)
    assert int(c[0]) == 0 and int(c[1]) > qcase.n // 16
    if period is None:
        assert int(c[2]) == qcase.n
    assert ("radius_periodic" if period else "radius_var") in E.kernels_used() and "cpu" not in E.kernels_used()


def test_point_radius_counts_and_neighbors(qcase):
    """(The per-point radii have no periodic form.)"""
    E.reset_kernels_used()
    pr = E.prepare_point_radii(qcase.index, qcase.point_radii.to(DEV))
    ref = qcase.point_radii_ref()
    stats = E.KnnStats()
    got = E.point_radius_counts(qcase.index, qcase.qd, pr, stats=stats)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), counts_of(ref)), rows_differ(got.cpu(), counts_of(ref))
    check_walk_stats(qcase, stats, None, accepts=False)
    got = lists_of(E.point_radius_neighbors(qcase.index, qcase.qd, pr), qcase.q.shape[0])
    assert same_lists(got, ref), rows_differ(counts_of(got), counts_of(ref))
    assert int(counts_of(ref).min()) >= 1  # the point of infinite radius reaches every query
    assert "radius_var" in E.kernels_used() and "cpu" not in E.kernels_used()


@PERIODS
def test_knn_query_neighbors(qcase, period):
    E.reset_kernels_used()
    idx, dist = E.knn_query_neighbors(qcase.pd, qcase.qd, K_NN, period=period)
    assert E.LAST_NEIGHBOR_ERRORS[0] == 0 and E.LAST_PERIODIC_KNN_ERRORS[0] == 0
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (qcase.q.shape[0], K_NN)
    want = qcase.knn_ref(period)
    assert torch.equal(idx.cpu(), want[0]), rows_differ(idx.cpu(), want[0])
    assert torch.equal(bits(dist.cpu()), bits(want[1])), rows_differ(bits(dist.cpu()), bits(want[1]))
    used = E.kernels_used()
    assert "cpu" not in used and ("grid" in used or "rows" in used)
    if period is not None:
        assert "knn_periodic" in used
        if qcase.name == "uniform":  # queries near every face: some list crosses one
            assert not torch.equal(want[0], qcase.knn_ref(None)[0])


@PERIODS
def test_radius_profile_and_pair_counts(qcase, period):
    E.reset_kernels_used()
    radii, want = qcase.radii(period), qcase.profile_ref(period)
    stats = E.KnnStats()
    got = E.radius_profile(qcase.index, qcase.qd, radii, period=period, stats=stats)
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), rows_differ(got.cpu(), want)
    check_walk_stats(qcase, stats, period, accepts=True)
    pairs = E.pair_counts(qcase.index, qcase.qd, radii, period=period)
    assert pairs.dtype == torch.int64 and torch.equal(pairs.cpu(), want.sum(0, dtype=torch.int64))
    if period is None:
        # radius inf: the root, or a stage-one node that holds the clipped last bucket, is taken
        # whole, and every (finite) query counts every point
        assert bool(torch.isfinite(qcase.q).all()) and bool((got[:, -1] == qcase.n).all())
        assert int(pairs[-1]) == qcase.n * qcase.q.shape[0]
    assert "radius_profile" in E.kernels_used() and "cpu" not in E.kernels_used()


@PERIODS
def test_weighted_profile(qcase, period):
    E.reset_kernels_used()
    radii, want = qcase.radii(period), qcase.weighted_ref(period)
    stats = E.KnnStats()
    got = E.weighted_profile(qcase.index, qcase.qd, radii, qcase.weights.to(DEV), period=period, stats=stats)
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), rows_differ(got.cpu(), want)
    check_walk_stats(qcase, stats, period, accepts=True)
    if period is None:
        assert bool((got[:, -1] == int(qcase.weights.sum())).all())
    assert "weighted_profile" in E.kernels_used() and "cpu" not in E.kernels_used()


@PERIODS
@pytest.mark.parametrize("mode", ("rppi", "smu"))
def test_pair_counts_2d(qcase, mode, period):
    E.reset_kernels_used()
    fn = E.pair_counts_rppi if mode == "rppi" else E.pair_counts_smu
    for coarse in (False, True) if mode == "rppi" else (False,):
        first, second = qcase.grid(mode, period, coarse)
        want = qcase.pairs2d_ref(mode, period, coarse)
        stats = E.KnnStats()
        got = fn(qcase.index, qcase.qd, first, second, period=period, stats=stats)
        assert got.dtype == torch.int64 and got.shape == want.shape
        bad = (got.cpu() != want).nonzero()
        assert bad.shape[0] == 0, f"{bad.shape[0]} of {want.numel()} cells differ, first {bad[:4].tolist()}"
        check_walk_stats(qcase, stats, period, accepts=coarse)
        assert int(want[-1, -1]) > 0
    assert "pair_counts_2d" in E.kernels_used() and "cpu" not in E.kernels_used()


# ---------------------------------------------------------------- 1. + 3. the self-form kernels
@PERIODS
@pytest.mark.parametrize("min_pts", (1, 5))
def test_cluster_labels(scase, min_pts, period):
    E.reset_kernels_used()
    want = scase.cluster_ref(period, min_pts)
    labels, core = E.cluster_labels(scase.index, scase.eps(), min_pts, period=period)
    assert E.LAST_CLUSTER_ERRORS[0] == 0
    assert labels.dtype == torch.int32 and core.dtype == torch.bool and labels.shape == core.shape == (scase.n,)
    assert torch.equal(core.cpu(), want[1]), rows_differ(core.cpu(), want[1])
    assert torch.equal(labels.cpu(), want[0]), rows_differ(labels.cpu(), want[0])
    assert ("cluster_periodic" if period else "cluster") in E.kernels_used() and "cpu" not in E.kernels_used()


@PERIODS
def test_core_distances(scase, period):
    """mst_core_d2 against the oracle: every row at the small sizes, NQ sampled rows (both ends of
    the curve order among them) at the deep ones."""
    n = scase.n
    got = scase.core_dev(period)
    assert got.dtype == torch.float32 and got.shape == (n,) and got.device.type == DEV
    if scase.deep:
        g = torch.Generator().manual_seed(67)
        perm = scase.index.perm[:n].cpu().long()
        rows = torch.cat([perm[:64], perm[-64:], torch.randint(0, n, (NQ - 128,), generator=g)])
    else:
        rows = torch.arange(n)
    p = scase.p
    want = K.kth_cpu(p, p[rows], 5, INF) if period is None else K.kth_periodic_cpu(p, p[rows], 5, INF, period)
    assert torch.equal(bits(got.cpu()[rows]), bits(want)), rows_differ(bits(got.cpu()[rows]), bits(want))
    assert float(want.min()) > 0.0


@PERIODS
@pytest.mark.parametrize("with_core", (False, True), ids=("plain", "core"))
def test_mst_edges(scase, with_core, period):
    """The small sizes: the oracle's tree bit for bit. The deep sizes: n - 1 edges that weigh
    what their rows say, span the set and carry the weights of a minimum spanning tree, in the
    order of the contract: a minimum spanning tree (and the order makes it the unique one)."""
    n, p = scase.n, scase.p
    rows, d2, c = scase.tree(period, with_core)
    rows, d2 = rows.cpu(), d2.cpu()
    want = scase.mst_ref(period, with_core)
    assert rows.shape == (n - 1, 2) and d2.shape == (n - 1,)
    lo, hi, w = rows[:, 0].numpy().astype(np.int64), rows[:, 1].numpy().astype(np.int64), d2.numpy()
    assert bool((lo < hi).all()) and int(lo.min()) >= 0 and int(hi.max()) < n
    core = scase.core_dev(period).cpu() if with_core else None
    assert np.array_equal(S.pair_weights(p, lo, hi, core, period).view(np.uint32), w.view(np.uint32))
    assert S.components_of_edges(rows, n) == 1
    b = w.view(np.int32).astype(np.int64)  # (weights are >= 0: their bits order as they do)
    up = (b[1:] > b[:-1]) | ((b[1:] == b[:-1]) & ((lo[1:] > lo[:-1]) | ((lo[1:] == lo[:-1]) & (hi[1:] > hi[:-1]))))
    assert bool(up.all()), f"{int((~up).sum())} rows do not ascend by (bits, lo, hi)"
    if scase.deep:
        assert torch.equal(bits(torch.sort(d2).values), bits(want)), "the weights are not those of a minimum spanning tree"
    else:
        assert torch.equal(rows, want[0]) and torch.equal(bits(d2), bits(want[1]))
    # the Boruvka rounds
    print(scase.n, period, with_core, c)
    comps = c["mst_components"]
    assert c["mst_rounds"] == len(comps) <= math.ceil(math.log2(n)) and comps[0] == n
    for before, after in zip(comps, comps[1:] + [1]):
        assert 2 * after <= before
    assert c["mst_evals"] > 0 and c["mst_nodes"] > 0 and c["mst_buckets"] > 0
    assert (c["mst_images"] > 0) == (period is not None)


@PERIODS
def test_mst_labels(scase, period):
    """The cut of the tree at 0.9 mean spacings is friends-of-friends: the tie-breaking along the cut."""
    rows, d2, _ = scase.tree(period, False)
    E.reset_kernels_used()
    got = E.mst_labels(rows, d2, scase.n, scase.eps())
    assert E.LAST_MST_ERRORS[0] == 0
    want = scase.cluster_ref(period, 1)[0]
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), rows_differ(got.cpu(), want)
    assert 1 < int(want.unique().numel()) < scase.n
    assert "mst" in E.kernels_used() and "cluster" in E.kernels_used()

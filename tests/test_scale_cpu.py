"""The host oracles at extreme scales, far offsets and periods that are no powers of two
(scale_cases.py), exactly against plain numpy written from the contract: the canonical chain
rounded to float32 after each fma (periodic_knn_ref.fma_sq), strict <, and the literal single
wrap per axis. test_gpu_scales.py compares every kernel with these oracles on the same
transforms, so this file is what makes them a reference there: squared distances that are
denormal, 0 between distinct points or inf, coordinates with six digits before the point, and
periods that round. It also runs the public functions on CPU tensors (the host-side Python:
radius hint, wrap_points, the period's radius bound) and checks the exact covariance under a
power of two that the GPU counter test leans on. Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

import mst_periodic_ref
import mst_ref
import pair_counts_2d_ref
import periodic_knn_ref
import radius_profile_ref
import scale_cases as S
import sparse_ref
import weighted_profile_ref
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

INF = math.inf
OPEN = (INF, INF, INF)
NA = 1500           # all-pairs forms
N, NQ = 3000, 500   # everything else
R4, R30 = S.r_for(4, N), S.r_for(30, N)
SELF_TRANSFORMS = [("scale", s) for s in (40, -40, -60, 62)] + [("offset", o) for o in S.OFFSETS]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tbits(t):
    return t.contiguous().view(torch.int32)


def same(t, a):
    """A float32 tensor and a numpy array: equal bit for bit."""
    return t.shape == tuple(a.shape) and np.array_equal(u32(t.numpy()), u32(a))


def final(a):
    return K.finalize_distances(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1)) \
        .view(tuple(a.shape)).numpy()


def ref_rows(D, cut2):
    """CSR (offsets, idx, d2) of {(d2, row) : d2 < cut2} per row of D, ascending by (bits, row)."""
    c2 = np.float32(cut2)
    offsets, idx, d2 = [0], [], []
    for r in range(D.shape[0]):
        with np.errstate(invalid="ignore"):
            ok = np.nonzero(D[r] < c2)[0]
        order = ok[np.argsort(u32(D[r, ok]), kind="stable")]
        idx.append(order)
        d2.append(D[r, order])
        offsets.append(offsets[-1] + order.size)
    return np.array(offsets, dtype=np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(d2)


def csr_same(got, ref):
    return np.array_equal(got[0].numpy(), ref[0]) and np.array_equal(got[1].numpy(), ref[1]) and same(got[2], ref[2])


def ref_clusters(W, cut2, min_pts):
    """(labels, core) of K.cluster_cpu's contract from the all-pairs weights W: sparse_ref's
    labelling, fed by all pairs (its k-d tree takes neither an origin nor denormal distances)."""
    return sparse_ref.dense_labels(W, cut2, min_pts)[:2]


# ------------------------------------------------------------------ 1. the open-box oracles
@pytest.mark.parametrize("name", S.BASES)
@pytest.mark.parametrize("t", S.TRANSFORMS, ids=S.tid)
def test_kth_and_lists(t, name):
    p, q = S.points(name, N, t), S.foreign(name, NQ, t, N)
    D = radius_profile_ref.dist2(p, q)
    index = E.build_index(p)
    for k in (1, 16):
        kth = np.partition(u32(D), k - 1, axis=1)[:, k - 1].view(np.float32)
        for method in ("kdtree", "brute"):
            assert same(K.kth_cpu(p, q, k, INF, method), kth), (S.tid(t), name, k, method)
        assert same(E.query_points(index, q, E.KnnConfig(k=k)), final(kth)), (S.tid(t), name, k)
    idx, d2 = periodic_knn_ref.knn_periodic(p, q, 16, INF, OPEN)
    got = K.knn_cpu(p, q, 16, INF)
    assert np.array_equal(got[0].numpy(), idx) and same(got[1], d2), (S.tid(t), name)
    got = E.query_neighbors(index, q, E.KnnConfig(k=16))
    assert np.array_equal(got[0].numpy(), idx) and same(got[1], final(d2)), (S.tid(t), name)
    # the set against itself, with the scaled cutoff
    r = S.radius(0.05, t)
    Dp = radius_profile_ref.dist2(p, p[:NQ])
    c2 = np.float32(E.cut2_of(r))
    live = np.where(Dp < c2, Dp, np.float32(INF))
    kth = np.partition(u32(live), 15, axis=1)[:, 15].view(np.float32)
    kth = np.where((Dp < c2).sum(1) >= 16, kth, c2).astype(np.float32)
    assert same(E.knn_distances(p, 16, r)[:NQ], final(kth)), (S.tid(t), name)


@pytest.mark.parametrize("t", S.TRANSFORMS, ids=S.tid)
def test_radius_family(t):
    p, q = S.points("uniform", N, t), S.foreign("uniform", NQ, t, N)
    D = radius_profile_ref.dist2(p, q)
    index = E.build_index(p)
    radii = [S.radius(r, t) for r in (R4, R30, R30, 0.5)]
    cut2s = [E.cut2_of(r) for r in radii]
    for r, cut2 in zip(radii[:2], cut2s[:2]):
        ref = ref_rows(D, cut2)
        assert csr_same(K.radius_cpu(p, q, cut2), ref), (S.tid(t), r)
        assert np.array_equal(K.radius_count_cpu(p, q, cut2).numpy(), np.diff(ref[0])), (S.tid(t), r)
        got = E.radius_neighbors(index, q, r)
        assert csr_same(got, (ref[0], ref[1], final(ref[2]))), (S.tid(t), r)
        assert np.array_equal(E.radius_counts(index, q, r).numpy(), np.diff(ref[0])), (S.tid(t), r)
    # one radius per query, one per indexed point: the predicate d2 < qcut2[q] and d2 < pcut2[p]
    g = torch.Generator().manual_seed(5)
    rq = S.radii((R30 / 8.0) * 16.0 ** torch.rand(NQ, generator=g), t)
    rp = S.radii((R30 / 8.0) * 16.0 ** torch.rand(N, generator=g), t)
    qc, pc = (rq * rq).numpy(), (rp * rp).numpy()
    with np.errstate(invalid="ignore"):
        ref = ref_rows(np.where(D < qc[:, None], D, np.float32(np.nan)), INF)
    assert csr_same(K.radius_var_cpu(p, q, rq * rq, None), ref), S.tid(t)
    assert np.array_equal(K.radius_var_count_cpu(p, q, rq * rq, None).numpy(), np.diff(ref[0])), S.tid(t)
    assert csr_same(E.radius_neighbors(index, q, rq), (ref[0], ref[1], final(ref[2]))), S.tid(t)
    assert np.array_equal(E.radius_counts(index, q, rq).numpy(), np.diff(ref[0])), S.tid(t)
    with np.errstate(invalid="ignore"):
        ref = ref_rows(np.where(D < pc[None, :], D, np.float32(np.nan)), INF)
    assert csr_same(K.radius_var_cpu(p, q, None, rp * rp), ref), S.tid(t)
    assert csr_same(E.point_radius_neighbors(index, q, rp), (ref[0], ref[1], final(ref[2]))), S.tid(t)
    assert np.array_equal(E.point_radius_counts(index, q, rp).numpy(), np.diff(ref[0])), S.tid(t)
    want = radius_profile_ref.radius_profile(p, q, cut2s)
    assert np.array_equal(K.radius_profile_cpu(p, q, cut2s).numpy(), want), S.tid(t)
    assert np.array_equal(E.radius_profile(index, q, radii).numpy(), want), S.tid(t)
    assert np.array_equal(E.pair_counts(index, q, radii).numpy(), want.sum(0, dtype=np.int64)), S.tid(t)
    w = torch.randint(-1000, 1000, (N,), generator=g, dtype=torch.int64)
    want = weighted_profile_ref.weighted_profile(p, q, cut2s, w)
    assert np.array_equal(K.weighted_profile_cpu(p, q, cut2s, w).numpy(), want), S.tid(t)
    assert np.array_equal(E.weighted_profile(index, q, radii, w).numpy(), want), S.tid(t)
    mu = [0.3, 1.0, INF]
    mu2 = [E.cut2_of(m) for m in mu]
    for los in (0, 2):
        want = pair_counts_2d_ref.pair_counts_2d(p, q, cut2s, cut2s, "rppi", los)
        assert np.array_equal(K.pair_counts_2d_cpu(p, q, cut2s, cut2s, "rppi", los).numpy(), want), (S.tid(t), los)
        assert np.array_equal(E.pair_counts_rppi(index, q, radii, radii, los=los).numpy(), want), (S.tid(t), los)
        want = pair_counts_2d_ref.pair_counts_2d(p, q, cut2s, mu2, "smu", los)
        assert np.array_equal(K.pair_counts_2d_cpu(p, q, cut2s, mu2, "smu", los).numpy(), want), (S.tid(t), los)
        assert np.array_equal(E.pair_counts_smu(index, q, radii, mu, los=los).numpy(), want), (S.tid(t), los)


@pytest.mark.parametrize("t", SELF_TRANSFORMS, ids=S.tid)
def test_clusters_and_trees(t):
    p = S.points("clustered", NA, t)
    W = mst_ref.pair_weights(p)
    index = E.build_index(p)
    for f in (0.5, 0.9):
        eps = S.radius(f * NA ** (-1.0 / 3.0), t)
        for min_pts in (1, 5):
            labels, core = ref_clusters(W, E.cut2_of(eps), min_pts)
            for got in (K.cluster_cpu(p, E.cut2_of(eps), min_pts), E.cluster_labels(index, eps, min_pts)):
                assert np.array_equal(got[0].numpy(), labels) and np.array_equal(got[1].numpy(), core), \
                    (S.tid(t), f, min_pts)
    core = K.kth_cpu(p, p, 5, INF)
    assert same(core, np.partition(u32(W), 4, axis=1)[:, 4].view(np.float32)), S.tid(t)
    assert same(E.mst_core_d2(index, 5), core.numpy()), S.tid(t)
    for c in (None, core):
        rows, d2 = mst_ref.mst(p, c)
        for got in (K.mst_cpu(p, c), E.mst_edges(index, c)):
            assert np.array_equal(got[0].numpy(), rows) and same(got[1], d2), (S.tid(t), c is not None)


# ----------------------------------------------------------------------------- 2. covariance
@pytest.mark.parametrize("s", S.COVARIANT)
@pytest.mark.parametrize("name", S.BASES)
def test_power_of_two_scaling_is_exact(name, s):
    """No squared distance leaves the normal range at s = +-40, so every float operation of the
    contract scales exactly: distances are ldexp(the unscaled ones, s) bit for bit, and with
    radii scaled alike the ids, counts, labels and tree rows are the unscaled ones."""
    t0, t = ("scale", 0), ("scale", s)
    p0, q0, p, q = S.points(name, N, t0), S.foreign(name, NQ, t0, N), S.points(name, N, t), S.foreign(name, NQ, t, N)
    a, b = K.knn_cpu(p0, q0, 16, INF), K.knn_cpu(p, q, 16, INF)
    assert torch.equal(a[0], b[0]) and same(b[1], np.ldexp(a[1].numpy(), 2 * s))
    assert same(K.finalize_distances(b[1].reshape(-1)), np.ldexp(K.finalize_distances(a[1].reshape(-1)).numpy(), s))
    for r in (R4, R30):
        a, b = K.radius_cpu(p0, q0, E.cut2_of(r)), K.radius_cpu(p, q, E.cut2_of(S.radius(r, t)))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and same(b[2], np.ldexp(a[2].numpy(), 2 * s))
    p0, p = p0[:NA].contiguous(), p[:NA].contiguous()
    eps = 0.9 * NA ** (-1.0 / 3.0)
    for min_pts in (1, 5):
        a, b = K.cluster_cpu(p0, E.cut2_of(eps), min_pts), K.cluster_cpu(p, E.cut2_of(S.radius(eps, t)), min_pts)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = K.mst_cpu(p0), K.mst_cpu(p)
    assert torch.equal(a[0], b[0]) and same(b[1], np.ldexp(a[1].numpy(), 2 * s))


# -------------------------------------------------------------- 3. periods, no powers of two
@pytest.mark.parametrize("pname,origin", S.PERIOD_CASES)
def test_periodic_oracles(pname, origin):
    per = S.PERIODS[pname]
    p = S.periodic_points("uniform", N, pname, origin)
    q = torch.cat([p[::12], S.periodic_points("uniform", NQ // 2, pname, origin, seed=3)]).contiguous()
    org = S.origin_of(per, origin)
    for ax in range(3):  # inside one period, also after rounding
        if math.isfinite(per[ax]):
            lo, hi = np.float32(org[ax]), np.float32(org[ax]) + np.float32(per[ax])
            assert float(p[:, ax].min()) >= lo and float(p[:, ax].max()) < hi
    assert torch.equal(E.wrap_points(p, per, org), p)
    D = radius_profile_ref.dist2(p, q, per)
    index = E.build_index(p)
    rmax = S.period_radius(pname, 0.5)
    radii = [S.period_radius(pname, 0.05), S.period_radius(pname, 0.12), rmax]
    cut2s = [E.cut2_of(r) for r in radii]
    for r, cut2 in zip(radii, cut2s):
        ref = ref_rows(D, cut2)
        assert int(ref[0][-1]) > int(K.radius_count_cpu(p, q, cut2).sum()), "the case does not wrap"
        assert csr_same(K.radius_periodic_cpu(p, q, cut2, per), ref), (pname, origin, r)
        assert np.array_equal(K.radius_periodic_count_cpu(p, q, cut2, per).numpy(), np.diff(ref[0]))
        assert csr_same(E.radius_neighbors(index, q, r, period=per), (ref[0], ref[1], final(ref[2])))
        assert np.array_equal(E.radius_counts(index, q, r, period=per).numpy(), np.diff(ref[0]))
    # one radius per query, up to the bound itself
    g = torch.Generator().manual_seed(8)
    rq = (radii[0] * (rmax / radii[0]) ** torch.rand(q.shape[0], generator=g)).clamp(max=rmax)
    rq[::7] = rmax
    with np.errstate(invalid="ignore"):
        ref = ref_rows(np.where(D < (rq * rq).numpy()[:, None], D, np.float32(np.nan)), INF)
    assert csr_same(K.radius_periodic_cpu(p, q, 0.0, per, rq * rq), ref), (pname, origin)
    assert csr_same(E.radius_neighbors(index, q, rq, period=per), (ref[0], ref[1], final(ref[2]))), (pname, origin)
    assert np.array_equal(E.radius_counts(index, q, rq, period=per).numpy(), np.diff(ref[0])), (pname, origin)
    # the bound is served, one float above it is refused (also as a tensor, a profile, an eps)
    above = S.float_above(rmax)
    assert E.check_period_radius("test", rmax, False, per) == K.check_period("test", per)
    for call in (lambda: E.radius_counts(index, q, above, period=per),
                 lambda: E.radius_counts(index, q, torch.full((q.shape[0],), above), period=per),
                 lambda: E.radius_profile(index, q, [above], period=per),
                 lambda: E.cluster_labels(index, above, 1, period=per)):
        with pytest.raises(ValueError):
            call()
    idx, d2 = periodic_knn_ref.knn_periodic(p, q, 16, INF, per)
    got = K.knn_periodic_cpu(p, q, 16, INF, per)
    assert np.array_equal(got[0].numpy(), idx) and same(got[1], d2), (pname, origin)
    assert same(K.kth_periodic_cpu(p, q, 16, INF, per), d2[:, 15]), (pname, origin)
    got = E.query_neighbors(index, q, E.KnnConfig(k=16), period=per)
    assert np.array_equal(got[0].numpy(), idx) and same(got[1], final(d2)), (pname, origin)
    assert same(E.query_points(index, q, E.KnnConfig(k=16), period=per), final(d2[:, 15])), (pname, origin)
    want = radius_profile_ref.radius_profile(p, q, cut2s, per)
    assert np.array_equal(K.radius_profile_cpu(p, q, cut2s, per).numpy(), want), (pname, origin)
    assert np.array_equal(E.radius_profile(index, q, radii, period=per).numpy(), want), (pname, origin)
    mu2 = [E.cut2_of(m) for m in (0.3, 1.0, INF)]
    for los in (0, 1):
        for mode, b2 in (("rppi", cut2s), ("smu", mu2)):
            want = pair_counts_2d_ref.pair_counts_2d(p, q, cut2s, b2, mode, los, per)
            assert np.array_equal(K.pair_counts_2d_cpu(p, q, cut2s, b2, mode, los, per).numpy(), want), \
                (pname, origin, mode, los)


@pytest.mark.parametrize("pname,origin", S.PERIOD_CASES)
def test_periodic_clusters_and_trees(pname, origin):
    per = S.PERIODS[pname]
    p = S.periodic_points("uniform", NA, pname, origin)
    W = mst_periodic_ref.pair_weights(p, per)
    index = E.build_index(p)
    vol = math.prod(v if math.isfinite(v) else max(S.finite_axes(per)) for v in per)
    eps = min(0.9 * (vol / NA) ** (1.0 / 3.0), S.period_radius(pname, 0.5))
    cut2 = E.cut2_of(eps)
    for min_pts in (1, 5):
        labels, core = ref_clusters(W, cut2, min_pts)
        for got in (K.cluster_periodic_cpu(p, cut2, min_pts, per), E.cluster_labels(index, eps, min_pts, period=per)):
            assert np.array_equal(got[0].numpy(), labels) and np.array_equal(got[1].numpy(), core), \
                (pname, origin, min_pts)
    assert not torch.equal(K.cluster_periodic_cpu(p, cut2, 1, per)[0], K.cluster_cpu(p, cut2, 1)[0]), \
        "the case does not wrap"
    rows, d2 = mst_periodic_ref.mst(p, per)
    for got in (K.mst_periodic_cpu(p, per), E.mst_edges(index, period=per)):
        assert np.array_equal(got[0].numpy(), rows) and same(got[1], d2), (pname, origin)
    assert not torch.equal(K.mst_cpu(p)[1], K.mst_periodic_cpu(p, per)[1]), "the case does not wrap"
    core = K.kth_periodic_cpu(p, p, 5, INF, per)
    assert same(core, np.partition(u32(W), 4, axis=1)[:, 4].view(np.float32)), (pname, origin)
    assert same(E.mst_core_d2(index, 5, period=per), core.numpy()), (pname, origin)


# ------------------------------------------------------------------- 4. host-side arithmetic
@pytest.mark.parametrize("t", S.TRANSFORMS, ids=S.tid)
def test_radius_hint_is_finite_and_covariant(t):
    """The density estimate of the k-th squared distance, float64 on the host: positive at every
    scale (it may leave float32's range: the kernels then start from their last resort), and
    exactly the unit value x 2^2s where float64 holds both."""
    box = K.bounds(S.points("uniform", N, t))
    h = E.radius_hint2(box, N, 16)
    assert h > 0.0 and not math.isnan(h)
    if t[0] == "scale":
        h0 = E.radius_hint2(K.bounds(S.points("uniform", N, ("scale", 0))), N, 16)
        assert abs(h / math.ldexp(h0, 2 * t[1]) - 1.0) < 1e-12


def probe_of(points, k):
    """A FrameProbe as its constructor leaves it for GPU points (the covariance sums of the
    strided sample and its largest coordinate), filled on the host: result() is what is tested."""
    fp = object.__new__(E.FrameProbe)
    n = points.shape[0]
    smp = points[::max(1, n // E.FRAME_SAMPLE)][:E.FRAME_SAMPLE].to(torch.float64)
    c = smp - smp.mean(0)
    fp.cov = torch.stack([(c[:, i] * c[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
                         + [smp.abs().max()])
    fp.k, fp.n, fp.m, fp.device = k, n, smp.shape[0], torch.device("cpu")
    return fp


@pytest.mark.parametrize("s,rotates", [(0, True), (40, True), (-40, True), (62, True), (-60, False), (-70, False),
                                       (-80, False)])
def test_a_frame_needs_a_normal_widening(s, rotates, monkeypatch):
    """FrameProbe gives a tilted plane its rotated frame only while the boxes' widening is a
    normal float32 when squared (FRAME_MIN_MARGIN2): below that the rounding of denormal squared
    distances outweighs the widening and a box that holds the k-th neighbour is culled. Without
    the rule the probe answers with a rotation at every one of these scales."""
    p = S.points("tilted_plane", 20_000, ("scale", s))
    frame = probe_of(p, 100).result()
    assert (isinstance(frame, torch.Tensor) and frame.shape == (3, 3)) == rotates, (s, frame)
    monkeypatch.setattr(E, "FRAME_MIN_MARGIN2", 0.0)
    assert isinstance(probe_of(p, 100).result(), torch.Tensor), s

#!/usr/bin/env python3
"""Fixed-radius search throughput on one GPU, beside the k-nearest lists of the same size.

    python scripts/radius_bench.py [--points 1e7] [--queries 1e6] [--mean 100] [--steps 5] [--warmup 2]
                                   [--radii scalar|query-equal|query-loguniform|query-kth|point-kth]
                                   [--period L | Lx,Ly,Lz]
    python scripts/radius_bench.py --profile B [-r R] [--self-queries] [--points ..] [--queries ..] [--mean ..]
                                   [--steps ..] [--warmup ..] [--period ..] [--weights]
    python scripts/radius_bench.py --pairs-2d BPxBL [--smu] [-r R] [--self-queries] [--points ..] [--queries ..]
                                   [--steps ..] [--warmup ..] [--period ..] [--skip-pair-list] [--weights]
                                   [--los midpoint [--observer ox,oy,oz]]
    python scripts/radius_bench.py --reach either|both [--period ..] [--dist uniform|clustered] [--kth K]
                                   [--points ..] [--steps ..] [--warmup ..]

Uniform points in the unit cube and uniform queries from another seed; the radius is the one
whose ball holds --mean points at the data's density (queries near the faces see fewer, so
the measured mean is a little lower; it is printed). On one index, device-synchronised host
clock, medians over the steps after the warm-up steps, the four timed alternately step by
step so that drift on a shared host hits them alike:
  * counts:    radius_counts;
  * sorted:    radius_neighbors (count + prefix sum + fill + row sort);
  * unsorted:  radius_neighbors(sort=False);
  * knn_lists: query_neighbors at k = --mean on the same index and queries — the yardstick:
               lists of the same size that need a selection pass first.
--radii selects what the three radius cases search with (default scalar: one radius r):
  * query-equal:      a per-query tensor filled with r (the gather kernels on the scalar's work);
  * query-loguniform: per-query radii log-uniform in [r / 8, 2 r];
  * query-kth:        per-query radii 1.3 x the query's k-th neighbour distance, k = --kth;
  * point-kth:        per-point radii = every point's own k-th neighbour distance (scatter:
                      the reverse-neighbour search), prepared once outside the timed region.
--period: the three radius cases search the periodic box (the unit cube holds the data, so 1 is
the extent; not with point-kth); the JSON then carries radius_images / groups, the image
walks per query group of the count pass, beside the times.
Prints one JSON line. Sampled rows are checked against brute force.

--reach either|both: the two-sided search with the points as their own queries and every
point's k-th neighbour distance (k = --kth) as its radius on both sides, prepared once outside
the timed region (--dist clustered: 100 Gaussian blobs, sigma 0.01, wrapped into the unit cube).
Timed alternately as above: reach_neighbors (sorted) and reach_counts; and, without --period,
the two walks the search replaces, radius_neighbors with the radius tensor (gather) and
point_radius_neighbors (scatter), whose sum `two_walks_s` holds no union of the two results: the
row-wise union a caller had to write comes on top of it. With --period no earlier path exists:
the open run of the same inputs is timed beside the periodic one. The JSON carries the medians
and the radius_* counters of every count walk; sampled rows are checked against brute force.

--profile B: the radius profile instead. B log-spaced radii from r / 8 up to r (-r, default the
radius of --mean), on one index and one set of queries (--self-queries: the points themselves),
timed alternately as above: one radius_profile call, one pair_counts call, and the B
radius_counts calls they replace. The JSON carries the three medians and the radius_* counters
of each (one extra, untimed call with stats); the profile's columns are compared with the B
counts, and its column sums with the pair counts, before anything is reported.

--profile B --weights: the weighted profile. int64 weights drawn from +-2^15 on the points, timed
alternately in one process: one weighted_profile call and one weighted_pair_sums call (weights
prepared once, outside the timed region); one radius_profile call, the same walk with 32-bit
counters and no weight traffic; and the route without the weighted kernels, at the largest radius
only: radius_neighbors(sort=False) in query chunks that respect max_pairs, a gather of the weights
by id and a segment sum in torch. The JSON carries the medians and the radius_* counters of the
weighted and the unweighted walk (equal when B fits one slice of both kernels: the walks are the
same); the weighted profile's last column is compared with the pair-list route, its column sums
with the pair sums, before anything is reported.

--pairs-2d BPxBL: the anisotropic pair counts. BP x BL linearly spaced edges up to R (-r, default
0.01) across and along the line of sight z (--smu: BP separations up to R and BL cosines up to 1),
timed alternately in one process: one pair_counts_rppi (pair_counts_smu) call; pair_counts with BP
radii up to the enclosing radius (sqrt(2) R; --smu: R), the floor of what one walk costs; and the
route without the kernel: radius_neighbors(sort=False) at the enclosing radius in query chunks that
respect max_pairs, the differences re-derived and binned in torch (its cells are compared with the
kernel's and the number that differ is reported: torch promises no fma). The JSON carries the
medians and the radius_* counters of the two walks.

--pairs-2d BPxBL --weights: the weighted anisotropic pair sums beside them. int64 weights drawn from
+-2^15 on the points and +-2^2 on the queries (prepared once, outside the timed region); one
weighted_pair_sums_rppi (_smu) call is timed alternately with the cases above, and the pair-list
route bins wq * w (an integer index_add) in the place of 1. The radius_* counters of the weighted
and the unweighted walk must be equal (asserted). Before anything is printed the weighted cells
are compared with one more, untimed pass of the pair-list route that forms perp2 and d2 as the
kernel does (the square exact in float64, one sum, rounded to float32: the fma but for a double
rounding that needs a 29-bit coincidence): every cell must be equal, or the run fails. The timed
route's own float32 cells are reported as before (the number that differ).

--pairs-2d BPxBL --los midpoint [--observer ox,oy,oz] (default 0.5,0.5,-3): the observer's line of
sight (open box). pairs2d / wpairs2d are then the observer walk; the axis walk (los z) of the same
grid is timed beside them as pairs2d_axis / wpairs2d_axis, the pair-list route forms par2 and perp2
of the observer contract in torch, and the JSON carries the ratios of the times and of the
radius_evals of the two walks.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpi_cuda_largescaleknn_amd.apps.radius import add_period_option  # noqa: E402
from mpi_cuda_largescaleknn_amd.models import knn_engine as E  # noqa: E402
from mpi_cuda_largescaleknn_amd.ops import kernels as K  # noqa: E402


def profile_bench(a, p: torch.Tensor, q: torch.Tensor, r: float, per: dict) -> int:
    """--profile B: one radius_profile call, one pair_counts call and B radius_counts calls."""
    B = a.profile
    radii = [r * 8.0 ** (-(B - 1 - b) / max(B - 1, 1)) for b in range(B)]
    radii[-1] = r
    index = E.build_index(p)
    out = {}
    cases = {
        "profile": lambda **kw: out.__setitem__("profile", E.radius_profile(index, q, radii, **per, **kw)),
        "pairs": lambda **kw: out.__setitem__("pairs", E.pair_counts(index, q, radii, **per, **kw)),
        "counts": lambda **kw: out.__setitem__("counts", [E.radius_counts(index, q, rb, **per, **kw) for rb in radii]),
    }
    times = {name: [] for name in cases}
    for step in range(a.warmup + a.steps):
        for name, fn in cases.items():
            out.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    counters = {}
    out.clear()
    for name, fn in cases.items():
        st = E.KnnStats()
        fn(stats=st)
        counters[name] = dict(st.counters)
    prof, pairs = out["profile"], out["pairs"]
    same_columns = all(bool(torch.equal(prof[:, b], c)) for b, c in enumerate(out["counts"]))
    same_sums = bool(torch.equal(prof.sum(0, dtype=torch.int64), pairs))
    rec = {
        "points": p.shape[0], "queries": q.shape[0], "self_queries": bool(a.self_queries), "profile": B,
        "radii": radii, "mean_count_at_r": float(pairs[-1]) / q.shape[0], "steps": a.steps, "warmup": a.warmup,
        "profile_s": med["profile"], "pairs_s": med["pairs"], "counts_s": med["counts"],
        "counts_over_profile": med["counts"] / med["profile"], "counts_over_pairs": med["counts"] / med["pairs"],
        "spread": {name: [min(ts), max(ts)] for name, ts in times.items()},
        "counters": counters, "pairs": pairs.tolist(),
        "columns_equal_counts": same_columns, "sums_equal_pairs": same_sums,
    }
    if a.period is not None:
        rec["period"] = list(a.period)
    print(json.dumps(rec), flush=True)
    return 0 if same_columns and same_sums else 1


def reach_bench(a, p: torch.Tensor, per: dict) -> int:
    """--reach either|both: reach_neighbors / reach_counts beside the gather and the scatter walk
    (open box) or beside their own open run (--period)."""
    rule, n = a.reach, p.shape[0]
    index = E.build_index(p)
    h = E.knn_distances(p, a.kth)
    prad = E.prepare_point_radii(index, h)
    big = {"max_pairs": (1 << 31) - 1}  # (k-th distance radii on 1e7 points select more than 2^28 pairs)
    out = {}
    cases = {
        "reach": lambda: out.__setitem__("reach", E.reach_neighbors(index, p, h, prad, rule=rule, **big, **per)),
        "reach_counts": lambda **kw: out.__setitem__("counts", E.reach_counts(index, p, h, prad, rule=rule, **per, **kw)),
    }
    if a.period is None:
        cases["gather"] = lambda: out.__setitem__("gather", E.radius_neighbors(index, p, h, **big))
        cases["scatter"] = lambda: out.__setitem__("scatter", E.point_radius_neighbors(index, p, prad, **big))
        cases["gather_counts"] = lambda **kw: out.__setitem__("gc", E.radius_counts(index, p, h, **kw))
        cases["scatter_counts"] = lambda **kw: out.__setitem__("sc", E.point_radius_counts(index, p, prad, **kw))
    else:
        cases["reach_open"] = lambda: out.__setitem__("open", E.reach_neighbors(index, p, h, prad, rule=rule, **big))
        cases["reach_open_counts"] = lambda **kw: out.__setitem__(
            "oc", E.reach_counts(index, p, h, prad, rule=rule, **kw))
    times = {name: [] for name in cases}
    for step in range(a.warmup + a.steps):
        for name, fn in cases.items():
            out.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    counters = {}
    for name, fn in cases.items():
        if name.endswith("counts"):
            st = E.KnnStats()
            fn(stats=st)
            counters[name] = dict(st.counters)
    offsets, idx, dist = E.reach_neighbors(index, p, h, prad, rule=rule, **big, **per)
    counts = E.reach_counts(index, p, h, prad, rule=rule, **per)
    smp = torch.randint(0, n, (64,), generator=torch.Generator().manual_seed(3))
    c2 = (h * h).cpu()
    ro, ri, rd2 = K.radius_reach_cpu(p.cpu(), p[smp.to(p.device)].cpu(), c2[smp], c2, rule, a.period)
    rd = K.finalize_distances(rd2)
    off = offsets.cpu()
    exact = 0
    for j, qi in enumerate(smp.tolist()):
        gi, gd = idx[off[qi]:off[qi + 1]].cpu(), dist[off[qi]:off[qi + 1]].cpu()
        exact += int(torch.equal(gi, ri[ro[j]:ro[j + 1]]) and torch.equal(gd, rd[ro[j]:ro[j + 1]]))
    consistent = bool(torch.equal(torch.cumsum(counts, 0, dtype=torch.int64), offsets[1:]))
    rec = {
        "points": n, "queries": n, "self_queries": True, "dist": a.dist, "reach": rule, "kth": a.kth,
        "pairs": int(offsets[-1]), "mean_count": int(offsets[-1]) / n, "max_count": int(counts.max()),
        "steps": a.steps, "warmup": a.warmup, **{f"{name}_s": t for name, t in med.items()},
        "spread": {name: [min(ts), max(ts)] for name, ts in times.items()}, "counters": counters,
        "sampled_exact": f"{exact}/64", "offsets_are_count_sums": consistent,
    }
    if a.period is None:
        rec["two_walks_s"] = med["gather"] + med["scatter"]
        rec["reach_over_two_walks"] = med["reach"] / rec["two_walks_s"]
        rec["union_included"] = False
    else:
        groups = (n + 63) // 64
        rec.update({"period": list(a.period), "periodic_over_open": med["reach"] / med["reach_open"],
                    "images_per_group": counters["reach_counts"]["radius_images"] / groups})
    print(json.dumps(rec), flush=True)
    return 0 if exact == 64 and consistent else 1


def clustered_points(n: int, dev: torch.device) -> torch.Tensor:
    """100 Gaussian blobs of sigma 0.01 with uniform centres, wrapped into the unit cube."""
    g = torch.Generator(device=dev).manual_seed(1)
    centres = torch.rand((100, 3), generator=g, device=dev)
    which = torch.randint(0, 100, (n,), generator=g, device=dev)
    p = centres[which] + 0.01 * torch.randn((n, 3), generator=g, device=dev)
    return E.wrap_points(p, 1.0)


def pair_list_sums(index, q: torch.Tensor, r: float, w: torch.Tensor, per: dict, chunk: int) -> torch.Tensor:
    """Sum of w over every query's neighbours within r by way of the pair lists: int64 [nq]."""
    out = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    for a in range(0, q.shape[0], chunk):
        offsets, idx, _ = E.radius_neighbors(index, q[a:a + chunk], r, sort=False, **per)
        run = torch.zeros(idx.shape[0] + 1, dtype=torch.int64, device=q.device)
        torch.cumsum(w[idx.long()], 0, out=run[1:])
        out[a:a + chunk] = run[offsets[1:]] - run[offsets[:-1]]
    return out


def weighted_bench(a, p: torch.Tensor, q: torch.Tensor, r: float, per: dict) -> int:
    """--profile B --weights: weighted_profile / weighted_pair_sums, radius_profile, the pair-list route."""
    B = a.profile
    radii = [r * 8.0 ** (-(B - 1 - b) / max(B - 1, 1)) for b in range(B)]
    radii[-1] = r
    index = E.build_index(p)
    w = torch.randint(-(1 << 15), (1 << 15) + 1, (p.shape[0],), dtype=torch.int64, device=p.device,
                      generator=torch.Generator(device=p.device).manual_seed(5))
    pw = E.prepare_point_weights(index, w)
    # query chunks of the pair-list route: at most 2^27 pairs expected in each (max_pairs is 2^28)
    chunk = max(1, int((1 << 27) / max(a.mean, 1)))
    out = {}
    cases = {
        "weighted_profile": lambda **kw: out.__setitem__(
            "wprofile", E.weighted_profile(index, q, radii, pw, **per, **kw)),
        "weighted_pairs": lambda **kw: out.__setitem__(
            "wpairs", E.weighted_pair_sums(index, q, radii, pw, **per, **kw)),
        "profile": lambda **kw: out.__setitem__("profile", E.radius_profile(index, q, radii, **per, **kw)),
        "pair_list": lambda: out.__setitem__("list", pair_list_sums(index, q, r, w, per, chunk)),
    }
    times = {name: [] for name in cases}
    for step in range(a.warmup + a.steps):
        for name, fn in cases.items():
            out.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    counters = {}
    out.clear()
    for name, fn in cases.items():
        if name == "pair_list":
            fn()
            continue
        st = E.KnnStats()
        fn(stats=st)
        counters[name] = dict(st.counters)
    wprof, wpairs = out["wprofile"], out["wpairs"]
    same_list = bool(torch.equal(wprof[:, -1], out["list"]))
    same_sums = bool(torch.equal(wprof.sum(0, dtype=torch.int64), wpairs))
    rec = {
        "points": p.shape[0], "queries": q.shape[0], "self_queries": bool(a.self_queries), "profile": B,
        "weights": "int64 +-2^15", "radii": radii, "steps": a.steps, "warmup": a.warmup,
        "mean_count_at_r": float(out["profile"][:, -1].sum(dtype=torch.int64)) / q.shape[0],
        "weighted_profile_s": med["weighted_profile"], "weighted_pairs_s": med["weighted_pairs"],
        "profile_s": med["profile"], "pair_list_s": med["pair_list"], "pair_list_chunk": chunk,
        "weighted_over_profile": med["weighted_profile"] / med["profile"],
        "pair_list_over_weighted": med["pair_list"] / med["weighted_profile"],
        "spread": {name: [min(ts), max(ts)] for name, ts in times.items()},
        "counters": counters, "counters_equal": counters["weighted_profile"] == counters["profile"],
        "wpairs": wpairs.tolist(),
        "last_column_equals_pair_list": same_list, "sums_equal_pairs": same_sums,
    }
    if a.period is not None:
        rec["period"] = list(a.period)
    print(json.dumps(rec), flush=True)
    return 0 if same_list and same_sums else 1


def pair_list_cells(index, p, q, R, first2, second2, smu: bool, per: dict, period, chunk: int,
                    weights: tuple | None = None, exact: bool = False, observer=None) -> torch.Tensor:
    """The differential [B1, B2] cells (int64) by way of the pair lists at the enclosing radius R;
    weights = (w, wq): every pair adds wq[q] * w[p] in the place of 1; exact: perp2 and d2 as the
    float32 fma of the kernel, by way of float64; observer: par2 and perp2 of the observer contract."""
    def fma(a, b, c):  # exact: the product exact in float64, one sum, rounded to float32
        return (a.double() * b.double() + c.double()).float() if exact else torch.addcmul(c, a, b)
    obs = None if observer is None else torch.tensor(observer, dtype=torch.float32, device=q.device)
    b1, b2 = first2.shape[0], second2.shape[0]
    cells = torch.zeros(b1 * b2, dtype=torch.int64, device=q.device)
    for a in range(0, q.shape[0], chunk):
        offsets, idx, _ = E.radius_neighbors(index, q[a:a + chunk], R, sort=False, **per)
        rows = torch.repeat_interleave(torch.arange(a, a + offsets.shape[0] - 1, device=q.device),
                                       offsets[1:] - offsets[:-1])
        d = q[rows] - p[idx.long()]
        if period is not None:
            for ax in range(3):
                L = period[ax]
                if math.isfinite(L):
                    x = d[:, ax]
                    d[:, ax] = torch.where(x > 0.5 * L, x - L, torch.where(x < -0.5 * L, x + L, x))
        par2 = d[:, 2] * d[:, 2]
        if exact:
            perp2 = (d[:, 1].double() * d[:, 1].double() + (d[:, 0] * d[:, 0]).double()).float()
        else:
            perp2 = torch.addcmul(d[:, 0] * d[:, 0], d[:, 1], d[:, 1])
        if obs is not None:
            l = (q[rows] - obs) + (p[idx.long()] - obs)
            sl = fma(d[:, 2], l[:, 2], fma(d[:, 1], l[:, 1], d[:, 0] * l[:, 0]))
            ll = fma(l[:, 2], l[:, 2], fma(l[:, 1], l[:, 1], l[:, 0] * l[:, 0]))
            d2 = fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
            par2 = (sl / ll) * sl
            perp2 = d2 - par2
            perp2 = torch.where(perp2 < 0, torch.zeros_like(perp2), perp2)
        if smu:
            if obs is None:
                d2 = (d[:, 2].double() * d[:, 2].double() + perp2.double()).float() if exact else perp2 + par2
            i0 = torch.bucketize(d2, first2, right=True)
            j0 = b2 - (par2[:, None] < second2[None, :] * d2[:, None]).sum(1)
        else:
            i0 = torch.bucketize(perp2, first2, right=True)
            j0 = torch.bucketize(par2, second2, right=True)
        ok = (i0 < b1) & (j0 < b2)
        if weights is None:
            cells += torch.bincount((i0 * b2 + j0)[ok], minlength=b1 * b2)
        else:
            cells.index_add_(0, (i0 * b2 + j0)[ok], (weights[1][rows] * weights[0][idx.long()])[ok])
    return cells.view(b1, b2)


def pairs2d_bench(a, p: torch.Tensor, q: torch.Tensor, per: dict) -> int:
    """--pairs-2d BPxBL [--smu]: the kernel, the isotropic pair counts as the floor, the pair-list route."""
    b1, b2 = (int(v) for v in a.pairs_2d.lower().split("x"))
    R = a.radius if a.radius is not None else 0.01
    first = [R * (i + 1) / b1 for i in range(b1)]
    second = [(1.0 if a.smu else R) * (j + 1) / b2 for j in range(b2)]
    Renc = R if a.smu else math.sqrt(2.0) * R * (1.0 + 1e-6)
    fn2d = E.pair_counts_smu if a.smu else E.pair_counts_rppi
    obs = a.observer if a.los == "midpoint" else None
    los = {} if obs is None else {"los": "midpoint", "observer": obs}
    index = E.build_index(p)
    first2 = torch.tensor([E.cut2_of(v) for v in first], device=p.device)
    second2 = torch.tensor([E.cut2_of(v) for v in second], device=p.device)
    mean = q.shape[0] and p.shape[0] * 4.0 / 3.0 * math.pi * Renc ** 3
    chunk = max(1, int((1 << (24 if a.smu else 26)) / max(mean, 1.0)))
    out = {}
    cases = {
        "pairs2d": lambda **kw: out.__setitem__("pairs2d", fn2d(index, q, first, second, **los, **per, **kw)),
        "pairs1d": lambda **kw: out.__setitem__(
            "pairs1d", E.pair_counts(index, q, [Renc * (i + 1) / b1 for i in range(b1)], **per, **kw)),
    }
    if obs is not None:
        cases["pairs2d_axis"] = lambda **kw: out.__setitem__("pairs2d_axis", fn2d(index, q, first, second, **kw))
    wts = None
    if a.weights:
        g = torch.Generator(device=p.device).manual_seed(5)
        w = torch.randint(-(1 << 15), (1 << 15) + 1, (p.shape[0],), dtype=torch.int64, device=p.device, generator=g)
        wq = torch.randint(-4, 5, (q.shape[0],), dtype=torch.int64, device=p.device, generator=g)
        wts = (w, wq)
        pw = E.prepare_point_weights(index, w)
        wfn2d = E.weighted_pair_sums_smu if a.smu else E.weighted_pair_sums_rppi
        cases["wpairs2d"] = lambda **kw: out.__setitem__(
            "wpairs2d", wfn2d(index, q, first, second, pw, query_weights=wq, **los, **per, **kw))
        if obs is not None:
            cases["wpairs2d_axis"] = lambda **kw: out.__setitem__(
                "wpairs2d_axis", wfn2d(index, q, first, second, pw, query_weights=wq, **kw))
    if not a.skip_pair_list:
        cases["pair_list"] = lambda: out.__setitem__(
            "list", pair_list_cells(index, p, q, Renc, first2, second2, a.smu, per, a.period, chunk, wts,
                                    observer=obs))
    times = {name: [] for name in cases}
    for step in range(a.warmup + a.steps):
        for name, fn in cases.items():
            out.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    counters = {}
    out.clear()
    for name, fn in cases.items():
        if name == "pair_list":
            fn()
            continue
        st = E.KnnStats()
        fn(stats=st)
        counters[name] = dict(st.counters)
    S = out["pairs2d"]
    rec = {
        "points": p.shape[0], "queries": q.shape[0], "self_queries": bool(a.self_queries),
        "mode": "smu" if a.smu else "rppi", "grid": [b1, b2], "R": R, "enclosing_radius": Renc,
        "pairs_in_grid": int(S[-1, -1]), "steps": a.steps, "warmup": a.warmup,
        "lib": os.environ.get("LSKNN_HIP_LIB", ""),
        "pairs2d_s": med["pairs2d"], "pairs1d_s": med["pairs1d"], "pair_list_s": med.get("pair_list"),
        "spread": {name: [min(ts), max(ts)] for name, ts in times.items()}, "counters": counters,
    }
    ok = True
    if obs is not None:
        rec.update({"los": "midpoint", "observer": list(obs), "pairs2d_axis_s": med["pairs2d_axis"],
                    "observer_over_axis": med["pairs2d"] / med["pairs2d_axis"],
                    "observer_over_axis_evals": counters["pairs2d"]["radius_evals"] /
                    max(counters["pairs2d_axis"]["radius_evals"], 1)})
        if a.weights:
            rec.update({"wpairs2d_axis_s": med["wpairs2d_axis"],
                        "weighted_observer_over_axis": med["wpairs2d"] / med["wpairs2d_axis"]})
    if a.weights:
        assert counters["wpairs2d"] == counters["pairs2d"], (counters["wpairs2d"], counters["pairs2d"])
        rec.update({"weights": "int64 +-2^15, query weights +-2^2", "wpairs2d_s": med["wpairs2d"],
                    "weighted_over_pairs2d": med["wpairs2d"] / med["pairs2d"], "counters_equal": True,
                    "weighted_total": int(out["wpairs2d"][-1, -1])})
        if "pair_list" in med:
            rec["pair_list_over_weighted"] = med["pair_list"] / med["wpairs2d"]
    if "list" in out:
        counted = out["list"] if wts is None else \
            pair_list_cells(index, p, q, Renc, first2, second2, a.smu, per, a.period, chunk, observer=obs)
        moved = E.shell_counts_2d(S) != counted
        rec["pair_list_chunk"] = chunk
        rec["pair_list_cells_differing"] = int(moved.sum())
        rec["pair_list_total"] = int(counted.sum())
        if wts is not None:
            rec["weighted_pair_list_cells_differing"] = int((E.shell_counts_2d(out["wpairs2d"]) != out["list"]).sum())
            fma = pair_list_cells(index, p, q, Renc, first2, second2, a.smu, per, a.period, chunk, wts, exact=True,
                                  observer=obs)
            ok = bool(torch.equal(E.shell_counts_2d(out["wpairs2d"]), fma))
            rec["weighted_equals_pair_list"] = ok
    if a.period is not None:
        rec["period"] = list(a.period)
    print(json.dumps(rec), flush=True)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=1e7)
    ap.add_argument("--queries", type=float, default=1e6)
    ap.add_argument("--mean", type=int, default=100, help="mean neighbours per query, and the yardstick's k")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radii", default="scalar",
                    choices=["scalar", "query-equal", "query-loguniform", "query-kth", "point-kth"])
    ap.add_argument("--kth", type=int, default=32, help="k of the k-th-distance radii (query-kth, point-kth)")
    ap.add_argument("--profile", type=int, default=0, metavar="B", help="time the radius profile at B radii instead")
    ap.add_argument("-r", dest="radius", type=float, default=None, help="--profile: the largest radius")
    ap.add_argument("--self-queries", action="store_true", help="--profile: the points are their own queries")
    ap.add_argument("--weights", action="store_true",
                    help="--profile: the weighted profile and its alternatives; --pairs-2d: the weighted sums too")
    ap.add_argument("--pairs-2d", default=None, metavar="BPxBL", help="time the anisotropic pair counts instead")
    ap.add_argument("--smu", action="store_true", help="--pairs-2d: the (s, mu) mode")
    ap.add_argument("--skip-pair-list", action="store_true", help="--pairs-2d: without the pair-list route")
    ap.add_argument("--los", type=str.lower, choices=["z", "midpoint"], default="z",
                    help="--pairs-2d: the line of sight, the z axis or from --observer to each pair's midpoint")
    ap.add_argument("--observer", type=lambda t: tuple(float(v) for v in t.split(",")), default=None,
                    metavar="ox,oy,oz", help="--los midpoint: the observer (default 0.5,0.5,-3)")
    ap.add_argument("--reach", choices=["either", "both"], default=None,
                    help="time the two-sided search under this rule instead (self queries, k-th distances as radii)")
    ap.add_argument("--dist", choices=["uniform", "clustered"], default="uniform", help="--reach: the point set")
    add_period_option(ap)
    a = ap.parse_args()
    if a.reach is None and a.dist != "uniform":
        ap.error("--dist belongs to --reach")
    if a.reach is not None and (a.profile or a.pairs_2d is not None or a.radii != "scalar"):
        ap.error("--reach is a mode of its own: not with --profile, --pairs-2d or --radii")
    if a.pairs_2d is None and (a.smu or a.skip_pair_list):
        ap.error("--smu and --skip-pair-list belong to --pairs-2d")
    if (a.los == "midpoint" and (a.pairs_2d is None or a.period is not None)) or \
            (a.observer is not None and a.los != "midpoint"):
        ap.error("--los midpoint belongs to --pairs-2d without --period, --observer to --los midpoint")
    if a.los == "midpoint" and a.observer is None:
        a.observer = (0.5, 0.5, -3.0)
    if a.profile < 0 or (a.profile == 0 and a.pairs_2d is None and
                         (a.radius is not None or a.self_queries or a.weights)):
        ap.error("--profile B needs B >= 1; -r, --self-queries and --weights belong to it")
    if a.period is not None and a.radii == "point-kth":
        ap.error("--period is not supported with --radii point-kth")
    per = {} if a.period is None else {"period": a.period}  # (none: the calls without the keyword)
    if not torch.cuda.is_available():
        sys.stderr.write("radius_bench: needs a GPU (a CPU timing says nothing about it)\n")
        return 2
    n, nq, k = int(a.points), int(a.queries), a.mean
    dev = torch.device("cuda", 0)
    p = torch.rand((n, 3), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    q = torch.rand((nq, 3), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    r = (k / (n * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)
    if a.reach is not None:
        return reach_bench(a, clustered_points(n, dev) if a.dist == "clustered" else p, per)
    if a.pairs_2d is not None:
        return pairs2d_bench(a, p, p if a.self_queries else q, per)
    if a.profile:
        bench = weighted_bench if a.weights else profile_bench
        return bench(a, p, p if a.self_queries else q, a.radius if a.radius is not None else r, per)
    index = E.build_index(p, grid=True)
    E.bucket_keys(index)
    cfg = E.KnnConfig(k=k)
    out = {}
    # what the radius cases search with: (counts, lists) functions and the oracle's cutoffs
    qc2 = pc2 = None
    if a.radii == "point-kth":
        pr = E.knn_distances(p, a.kth)
        prad = E.prepare_point_radii(index, pr)
        pc2 = pr * pr
        counts_fn = lambda: E.point_radius_counts(index, q, prad)  # noqa: E731
        lists_fn = lambda sort=True: E.point_radius_neighbors(index, q, prad, sort=sort)  # noqa: E731
    else:
        if a.radii == "scalar":
            rad = r
        elif a.radii == "query-equal":
            rad = torch.full((nq,), r, device=dev)
        elif a.radii == "query-loguniform":
            u = torch.rand(nq, generator=torch.Generator(device=dev).manual_seed(4), device=dev)
            rad = torch.exp(math.log(r / 8) + math.log(16.0) * u)
        else:
            rad = 1.3 * E.query_points(index, q, E.KnnConfig(k=a.kth))
        if a.radii != "scalar":
            qc2 = rad * rad
        counts_fn = lambda **kw: E.radius_counts(index, q, rad, **per, **kw)  # noqa: E731
        lists_fn = lambda sort=True: E.radius_neighbors(index, q, rad, sort=sort, **per)  # noqa: E731
    cases = {
        "counts": lambda: out.__setitem__("counts", counts_fn()),
        "sorted": lambda: out.__setitem__("sorted", lists_fn()),
        "unsorted": lambda: out.__setitem__("unsorted", lists_fn(sort=False)),
        "knn_lists": lambda: out.__setitem__("knn", E.query_neighbors(index, q, cfg)),
    }
    times = {name: [] for name in cases}
    for step in range(a.warmup + a.steps):
        for name, fn in cases.items():
            out.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(ts) for name, ts in times.items()}

    offsets, idx, dist = lists_fn()
    counts = counts_fn()
    total = int(offsets[-1])
    smp = torch.randint(0, nq, (64,), generator=torch.Generator().manual_seed(3))
    if a.period is not None:
        ro, ri, rd2 = K.radius_periodic_cpu(p.cpu(), q[smp.to(dev)].cpu(), E.cut2_of(r), a.period,
                                            None if qc2 is None else qc2[smp.to(dev)].cpu())
    elif a.radii == "scalar":
        ro, ri, rd2 = K.radius_cpu(p.cpu(), q[smp.to(dev)].cpu(), E.cut2_of(r))
    else:
        ro, ri, rd2 = K.radius_var_cpu(p.cpu(), q[smp.to(dev)].cpu(), None if qc2 is None else qc2[smp.to(dev)].cpu(),
                                       None if pc2 is None else pc2.cpu())
    rd = K.finalize_distances(rd2)
    off = offsets.cpu()
    exact = 0
    for j, qi in enumerate(smp.tolist()):
        gi, gd = idx[off[qi]:off[qi + 1]].cpu(), dist[off[qi]:off[qi + 1]].cpu()
        exact += int(torch.equal(gi, ri[ro[j]:ro[j + 1]]) and torch.equal(gd, rd[ro[j]:ro[j + 1]]))
    consistent = bool(torch.equal(torch.cumsum(counts, 0, dtype=torch.int64), offsets[1:]))
    rec = {
        "points": n, "queries": nq, "radii": a.radii, "radius": r, "mean_count": total / nq, "max_count": int(counts.max()),
        "pairs": total, "steps": a.steps, "warmup": a.warmup,
        "counts_s": med["counts"], "sorted_s": med["sorted"], "unsorted_s": med["unsorted"],
        "knn_lists_k": k, "knn_lists_s": med["knn_lists"],
        "spread": {name: [min(ts), max(ts)] for name, ts in times.items()},
        "sorted_over_knn_lists": med["sorted"] / med["knn_lists"],
        "sorted_Mpairs_per_s": total / med["sorted"] / 1e6, "counts_Mqueries_per_s": nq / med["counts"] / 1e6,
        "sampled_exact": f"{exact}/64", "offsets_are_count_sums": consistent,
    }
    if a.period is not None:
        st = E.KnnStats()
        counts_fn(stats=st)
        groups = (nq + 63) // 64
        rec.update({"period": list(a.period), "radius_images": st.counters["radius_images"], "groups": groups,
                    "images_per_group": st.counters["radius_images"] / groups})
    print(json.dumps(rec), flush=True)
    return 0 if exact == 64 and consistent else 1


if __name__ == "__main__":
    sys.exit(main())

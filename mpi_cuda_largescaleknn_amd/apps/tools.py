"""Data tools (SURVEY §7.1 lsknn_gen / lsknn_split / lsknn_check):

    python -m mpi_cuda_largescaleknn_amd.apps.tools gen   out.float3 -n N [--dist uniform|clustered] [--seed S]
    python -m mpi_cuda_largescaleknn_amd.apps.tools split in.float3 -p P -o prefix [--spatial]
           -> prefix_%06d.float3 + prefix.list (contiguous blocks, or spatial x-slabs)
    python -m mpi_cuda_largescaleknn_amd.apps.tools check in.float3 dist.float -k K [-r R] [--samples S]
           [--queries q.float3]  (dist.float then holds hipKNN_query's output for q.float3)
           [--neighbors PREFIX]  (also PREFIX.ids / PREFIX.dist of hipKNN_query --neighbors)
           [--period L | Lx,Ly,Lz]  (with --queries: hipKNN_query --period, the periodic oracle)
           -> exact CPU oracle on sampled points, bitwise compare (replaces the reference's
              disabled '#if 0' RES dump, unorderedDataVariant.cu:215-227)
    python -m mpi_cuda_largescaleknn_amd.apps.tools rcheck in.float3 q.float3 PREFIX [--samples S]
           (-r R | --radii FILE | --point-radii FILE | --reach QRADII PRADII [--rule either|both])
           [--squared] [--counts-only] [--unsorted] [--period L | Lx,Ly,Lz]
           -> hipKNN_radius' PREFIX.count (and .offsets / .ids / .dist) for q.float3 against the
              brute-force oracle: every count's consistency with the offsets, sampled rows bitwise
    python -m mpi_cuda_largescaleknn_amd.apps.tools rcheck in.float3 q.float3 PREFIX --profile R1,R2,... [--squared]
           [--pairs-only] [--samples S] [--period L | Lx,Ly,Lz]
           -> hipKNN_radius --profile's PREFIX.profile rows against the brute-force oracle (all rows
              without --samples when there are at most 65536) and PREFIX.pairs against the column sums
    python -m mpi_cuda_largescaleknn_amd.apps.tools rcheck in.float3 q.float3 PREFIX --profile R1,R2,... --weights W.i64
           [--query-weights WQ.i64] [--pairs-only] ...
           -> hipKNN_radius --profile --weights' PREFIX.wprofile and PREFIX.wpairs against the oracle, on
              the same sampling rules
    python -m mpi_cuda_largescaleknn_amd.apps.tools pcheck in.float3 q.float3 PREFIX (--rp .. --pi .. | --s .. --mu ..)
           [--los x|y|z|midpoint [--observer ox,oy,oz]] [--squared] [--period L | Lx,Ly,Lz]
           [--weights W.i64 [--query-weights WQ.i64]]
           -> hipKNN_pairs' PREFIX.pairs2d (--weights: PREFIX.wpairs2d) against the brute-force oracle,
              every cell (at most 65536 queries: the oracle visits every pair)
    python -m mpi_cuda_largescaleknn_amd.apps.tools fixweights in.float out.i64 [--bits N] [--terms T]
           -> float32 masses as exact fixed-point int64 weights
              (knn_engine.fixed_point_weights); prints the exponent s: physical sum = result * 2^s
    python -m mpi_cuda_largescaleknn_amd.apps.tools ccheck in.float3 PREFIX -r EPS [--min-pts M] [--squared]
           [--period L | Lx,Ly,Lz]
           -> hipKNN_cluster's PREFIX.labels and PREFIX.core against the brute-force oracle, every
              point (at most 65536: the oracle visits every pair)
    python -m mpi_cuda_largescaleknn_amd.apps.tools mcheck in.float3 PREFIX [--core-k K] [--period L | Lx,Ly,Lz]
           -> hipKNN_mst's PREFIX.mst.rows and PREFIX.mst.d2 against the brute-force oracle, every
              edge (at most 65536 points: the oracle visits every pair)
    python -m mpi_cuda_largescaleknn_amd.apps.tools wrap in.float3 out.float3 --period L | Lx,Ly,Lz [--origin O | Ox,Oy,Oz]
           -> the points brought into one period [O, O + L) per finite axis (knn_engine.wrap_points)
    python -m mpi_cuda_largescaleknn_amd.apps.tools cat prefix P out.float  (concatenate per-rank outputs)
    python -m mpi_cuda_largescaleknn_amd.apps.tools cmp a.float b.float
"""
from __future__ import annotations

import argparse
import math
import sys

import numpy as np
import torch

from ..models.knn_engine import cut2_of, fixed_point_weights, wrap_points
from ..ops import kernels as K
from ..utils import io


def gen(a) -> int:
    g = torch.Generator().manual_seed(a.seed)
    n = int(a.n)
    chunk = 1 << 24
    out = torch.empty((n, 3), dtype=torch.float32)
    if a.dist == "uniform":
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            out[s:s + m] = torch.rand((m, 3), generator=g)
    else:
        centers = torch.rand((max(1, a.clusters), 3), generator=g)
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            w = torch.randint(0, centers.shape[0], (m,), generator=g)
            out[s:s + m] = centers[w] + a.sigma * torch.randn((m, 3), generator=g)
    io.write_points(a.out, out)
    print(f"wrote {n} points to {a.out}")
    return 0


def split(a) -> int:
    pts = io.read_points(a.inp)
    n = pts.shape[0]
    names = []
    if a.spatial:
        order = torch.argsort(pts[:, 0], stable=True)
    for r in range(a.p):
        b, e = n * r // a.p, n * (r + 1) // a.p
        part = pts[order[b:e]] if a.spatial else pts[b:e]
        name = f"{a.out}_{r:06d}.float3"
        io.write_points(name, part)
        names.append(name)
    with open(a.out + ".list", "w") as f:
        f.write("\n".join(names) + "\n")
    if a.spatial:
        torch.save(order.to(torch.int64), a.out + ".order.pt")
    print(f"wrote {a.p} files and {a.out}.list")
    return 0


def check(a) -> int:
    pts = io.read_points(a.inp)
    dist = io.read_floats(a.dist_file)
    # --queries: the distances belong to the rows of that file (hipKNN_query), checked by
    # brute force over all points
    qry = io.read_points(a.queries) if a.queries else pts
    n = qry.shape[0]
    if dist.shape[0] != n:
        print(f"size mismatch: {dist.shape[0]} distances for {n} {'queries' if a.queries else 'points'}")
        return 1
    if a.period is not None and not a.queries:
        print("check: --period needs --queries (the periodic k-NN serves hipKNN_query only)")
        return 1
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, n, (min(a.samples, n),), generator=g) if a.samples < n else torch.arange(n)
    if a.period is not None:
        ref = K.finalize_distances(K.kth_periodic_cpu(pts, qry[idx], a.k, cut2_of(a.r), a.period))
    else:
        ref = K.finalize_distances(K.kth_cpu(pts, qry[idx], a.k, cut2_of(a.r), "brute" if a.queries else "kdtree"))
    got = dist[idx]
    bad = int((got != ref).sum())
    print(f"checked {idx.numel()} sampled points: {bad} mismatches")
    for i in (got != ref).nonzero().flatten()[:10].tolist():
        print(f"RES {int(idx[i]):012d} = {got[i].item()!r} (oracle {ref[i].item()!r})")
    if a.neighbors:
        bad += _check_neighbors(a, pts, qry, idx)
    return 0 if bad == 0 else 1


def _check_neighbors(a, pts, qry, idx) -> int:
    """The sampled rows of PREFIX.ids / PREFIX.dist against the brute-force lists, bitwise."""
    ids = io.read_rows(a.neighbors + ".ids", a.k, torch.int32)
    nd = io.read_rows(a.neighbors + ".dist", a.k, torch.float32)
    n = qry.shape[0]
    if ids.shape[0] != n or nd.shape[0] != n:
        print(f"size mismatch: {ids.shape[0]} id rows, {nd.shape[0]} distance rows for {n} queries")
        return 1
    if a.period is not None:
        ref_i, ref_d2 = K.knn_periodic_cpu(pts, qry[idx], a.k, cut2_of(a.r), a.period)
    else:
        ref_i, ref_d2 = K.knn_cpu(pts, qry[idx], a.k, cut2_of(a.r))
    ref_d = K.finalize_distances(ref_d2.view(-1)).view(-1, a.k)
    wrong = ((ids[idx] != ref_i) | (nd[idx] != ref_d)).any(dim=1)
    bad = int(wrong.sum())
    print(f"checked {idx.numel()} sampled neighbour lists: {bad} mismatches")
    for i in wrong.nonzero().flatten()[:10].tolist():
        j = int(((ids[idx][i] != ref_i[i]) | (nd[idx][i] != ref_d[i])).nonzero()[0])
        print(f"ROW {int(idx[i]):012d} slot {j}: id {int(ids[idx][i][j])} dist {nd[idx][i][j].item()!r} "
              f"(oracle id {int(ref_i[i][j])} dist {ref_d[i][j].item()!r})")
    return bad


CCHECK_MAX = 65536  # points ccheck (and rows rcheck --profile) takes whole: the oracle visits every pair


def _rcheck_profile(a, pts, qry) -> int:
    """PREFIX.profile / PREFIX.pairs of hipKNN_radius --profile against the oracle."""
    nq, nb = qry.shape[0], len(a.profile)
    cut2s = [float(np.float32(r)) if a.squared else cut2_of(r) for r in a.profile]
    pairs = io.read_array(a.prefix + ".pairs", torch.int64)
    if pairs.shape[0] != nb:
        print(f"size mismatch: {pairs.shape[0]} pair counts for {nb} radii")
        return 1
    if a.pairs_only:  # no rows to sample: the sums themselves, which visits every pair
        if nq > CCHECK_MAX:
            print(f"rcheck: --pairs-only with {nq} queries, more than {CCHECK_MAX}: the oracle visits every pair; "
                  "check a smaller set, or the profile file")
            return 1
        ref = K.pair_counts_cpu(pts, qry, cut2s, a.period)
        bad = int((pairs != ref).sum())
        print(f"checked {nb} pair counts: {bad} mismatches")
        for b in (pairs != ref).nonzero().flatten()[:10].tolist():
            print(f"PAIRS {b} = {int(pairs[b])} (oracle {int(ref[b])})")
        return 0 if bad == 0 else 1
    prof = io.read_array(a.prefix + ".profile", torch.int32)
    if prof.shape[0] != nq * nb:
        print(f"size mismatch: {prof.shape[0]} profile entries for {nq} queries x {nb} radii")
        return 1
    prof = prof.view(nq, nb)
    if a.samples is None and nq <= CCHECK_MAX:
        idx = torch.arange(nq)
    else:
        g = torch.Generator().manual_seed(0)
        samples = 1000 if a.samples is None else a.samples
        idx = torch.randint(0, nq, (min(samples, nq),), generator=g) if samples < nq else torch.arange(nq)
    ref = K.radius_profile_cpu(pts, qry[idx], cut2s, a.period)
    wrong = (prof[idx] != ref).any(dim=1)
    bad = int(wrong.sum())
    print(f"checked {idx.numel()} profile rows: {bad} mismatches")
    for i in wrong.nonzero().flatten()[:10].tolist():
        b = int((prof[idx[i]] != ref[i]).nonzero()[0])
        print(f"PROFILE {int(idx[i]):012d} column {b} = {int(prof[idx[i]][b])} (oracle {int(ref[i][b])})")
    sums = prof.sum(0, dtype=torch.int64)
    off = (pairs != sums).nonzero().flatten()
    print(f"checked {nb} pair counts against the column sums: {off.numel()} mismatches")
    for b in off[:10].tolist():
        print(f"PAIRS {b} = {int(pairs[b])} (column sum {int(sums[b])})")
    return 0 if bad + off.numel() == 0 else 1


def pcheck(a) -> int:
    """PREFIX.pairs2d (--weights: PREFIX.wpairs2d) of hipKNN_pairs against the oracle, every cell."""
    from ..models.knn_engine import _pairs2d_cutoffs
    try:
        a2, b2, los, per = _pairs2d_cutoffs("pcheck", a.mode, a.first, a.second, a.los, a.squared, a.period,
                                            a.observer)
    except ValueError as e:
        print(e)
        return 1
    pts, qry = io.read_points(a.inp), io.read_points(a.queries)
    if qry.shape[0] > CCHECK_MAX:
        print(f"pcheck: {qry.shape[0]} queries, more than {CCHECK_MAX}: the oracle visits every pair; check a "
              "smaller set")
        return 1
    weighted = a.weights is not None
    if weighted:
        from .radius import read_weights
        try:
            w = read_weights(a.weights, "--weights", pts.shape[0], a.inp)
            wq = None if a.query_weights is None else \
                read_weights(a.query_weights, "--query-weights", qry.shape[0], a.queries)
        except ValueError as e:
            print(f"pcheck: {e}")
            return 1
    name = "WPAIRS2D" if weighted else "PAIRS2D"
    got = io.read_array(a.prefix + ("." + name.lower()), torch.int64)
    if got.shape[0] != a2.shape[0] * b2.shape[0]:
        print(f"size mismatch: {got.shape[0]} cells for {a2.shape[0]} x {b2.shape[0]} edges")
        return 1
    got = got.view(a2.shape[0], b2.shape[0])
    ref = K._pairs2d_cpu("pcheck", pts, qry, a2, b2, a.mode, los, per, (w, wq) if weighted else None,
                         observer=isinstance(los, tuple))  # (a tuple: the observer of --los midpoint)
    wrong = (got != ref).nonzero()
    print(f"checked {ref.numel()} cells: {wrong.shape[0]} mismatches")
    for i, j in wrong[:10].tolist():
        print(f"{name} [{i}][{j}] = {int(got[i, j])} (oracle {int(ref[i, j])})")
    return 0 if wrong.shape[0] == 0 else 1


def _rcheck_weighted(a, pts, qry) -> int:
    """PREFIX.wprofile / PREFIX.wpairs of hipKNN_radius --profile --weights against the oracle,
    on the sampling rules of _rcheck_profile."""
    from .radius import read_weights
    nq, nb = qry.shape[0], len(a.profile)
    cut2s = [float(np.float32(r)) if a.squared else cut2_of(r) for r in a.profile]
    try:
        w = read_weights(a.weights, "--weights", pts.shape[0], a.inp)
        wq = None if a.query_weights is None else read_weights(a.query_weights, "--query-weights", nq, a.queries)
    except ValueError as e:
        print(f"rcheck: {e}")
        return 1
    pairs = io.read_array(a.prefix + ".wpairs", torch.int64)
    if pairs.shape[0] != nb:
        print(f"size mismatch: {pairs.shape[0]} pair sums for {nb} radii")
        return 1
    if a.pairs_only:  # no rows to sample: the sums themselves, which visits every pair
        if nq > CCHECK_MAX:
            print(f"rcheck: --pairs-only with {nq} queries, more than {CCHECK_MAX}: the oracle visits every pair; "
                  "check a smaller set, or the profile file")
            return 1
        ref = K.weighted_pair_sums_cpu(pts, qry, cut2s, w, a.period, query_weights=wq)
        bad = int((pairs != ref).sum())
        print(f"checked {nb} weighted pair sums: {bad} mismatches")
        for b in (pairs != ref).nonzero().flatten()[:10].tolist():
            print(f"WPAIRS {b} = {int(pairs[b])} (oracle {int(ref[b])})")
        return 0 if bad == 0 else 1
    prof = io.read_array(a.prefix + ".wprofile", torch.int64)
    if prof.shape[0] != nq * nb:
        print(f"size mismatch: {prof.shape[0]} profile entries for {nq} queries x {nb} radii")
        return 1
    prof = prof.view(nq, nb)
    if a.samples is None and nq <= CCHECK_MAX:
        idx = torch.arange(nq)
    else:
        g = torch.Generator().manual_seed(0)
        samples = 1000 if a.samples is None else a.samples
        idx = torch.randint(0, nq, (min(samples, nq),), generator=g) if samples < nq else torch.arange(nq)
    ref = K.weighted_profile_cpu(pts, qry[idx], cut2s, w, a.period)
    wrong = (prof[idx] != ref).any(dim=1)
    bad = int(wrong.sum())
    print(f"checked {idx.numel()} weighted profile rows: {bad} mismatches")
    for i in wrong.nonzero().flatten()[:10].tolist():
        b = int((prof[idx[i]] != ref[i]).nonzero()[0])
        print(f"WPROFILE {int(idx[i]):012d} column {b} = {int(prof[idx[i]][b])} (oracle {int(ref[i][b])})")
    sums = (prof if wq is None else prof * wq[:, None]).sum(0, dtype=torch.int64)
    off = (pairs != sums).nonzero().flatten()
    print(f"checked {nb} weighted pair sums against the weighted column sums: {off.numel()} mismatches")
    for b in off[:10].tolist():
        print(f"WPAIRS {b} = {int(pairs[b])} (column sum {int(sums[b])})")
    return 0 if bad + off.numel() == 0 else 1


def fixweights(a) -> int:
    w = io.read_array(a.inp, torch.float32)
    try:
        fix, s = fixed_point_weights(w, n_terms=a.terms, bits=a.bits)
    except ValueError as e:
        print(f"fixweights: {e}")
        return 1
    io.write_array(a.out, fix, 0, truncate=True, total=fix.shape[0])
    print(f"wrote {fix.shape[0]} int64 weights to {a.out}: s = {s} (physical value = weight * 2^{s})")
    return 0


def rcheck(a) -> int:
    pts = io.read_points(a.inp)
    qry = io.read_points(a.queries)
    nq = qry.shape[0]
    if a.pairs_only and a.profile is None:
        print("rcheck: --pairs-only needs --profile")
        return 1
    if (a.weights is not None and a.profile is None) or (a.query_weights is not None and a.weights is None):
        print("rcheck: --weights needs --profile, --query-weights needs --weights")
        return 1
    if a.profile is not None and a.weights is not None:
        return _rcheck_weighted(a, pts, qry)
    if a.profile is not None:
        return _rcheck_profile(a, pts, qry)
    if a.rule is not None and a.reach is None:
        print("rcheck: --rule needs --reach")
        return 1
    if a.samples is None:
        a.samples = 1000
    if a.period is not None and a.point_radii is not None:
        print("rcheck: --period is not supported with --point-radii")
        return 1
    # the oracle of the sampled queries idx: (counts, lists) under the option given
    if a.radius is not None:
        cut2 = float(np.float32(a.radius)) if a.squared else cut2_of(a.radius)

        def oracle(idx):
            if a.period is not None:
                return (K.radius_periodic_count_cpu(pts, qry[idx], cut2, a.period),
                        lambda: K.radius_periodic_cpu(pts, qry[idx], cut2, a.period))
            return K.radius_count_cpu(pts, qry[idx], cut2), lambda: K.radius_cpu(pts, qry[idx], cut2)
    elif a.reach is not None:
        from .radius import read_radii
        try:
            qrad = read_radii(a.reach[0], "--reach", nq, a.queries)
            prad = read_radii(a.reach[1], "--reach", pts.shape[0], a.inp)
        except ValueError as e:
            print(e)
            return 1
        qc2, pc2 = (qrad, prad) if a.squared else (qrad * qrad, prad * prad)
        rule = a.rule or "either"

        def oracle(idx):
            return (K.radius_reach_count_cpu(pts, qry[idx], qc2[idx], pc2, rule, a.period),
                    lambda: K.radius_reach_cpu(pts, qry[idx], qc2[idx], pc2, rule, a.period))
    else:
        from .radius import read_radii
        try:
            if a.radii is not None:
                rad = read_radii(a.radii, "--radii", nq, a.queries)
            else:
                rad = read_radii(a.point_radii, "--point-radii", pts.shape[0], a.inp)
        except ValueError as e:
            print(e)
            return 1
        c2 = rad if a.squared else rad * rad

        def oracle(idx):
            qc, pc = (c2[idx], None) if a.radii is not None else (None, c2)
            if a.period is not None:
                return (K.radius_periodic_count_cpu(pts, qry[idx], 0.0, a.period, qc),
                        lambda: K.radius_periodic_cpu(pts, qry[idx], 0.0, a.period, qc))
            return K.radius_var_count_cpu(pts, qry[idx], qc, pc), lambda: K.radius_var_cpu(pts, qry[idx], qc, pc)
    counts = io.read_array(a.prefix + ".count", torch.int32)
    if counts.shape[0] != nq:
        print(f"size mismatch: {counts.shape[0]} counts for {nq} queries")
        return 1
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, nq, (min(a.samples, nq),), generator=g) if a.samples < nq else torch.arange(nq)
    ref_c, ref_lists = oracle(idx)
    wrong = counts[idx] != ref_c
    bad = int(wrong.sum())
    print(f"checked {idx.numel()} sampled counts: {bad} mismatches")
    for i in wrong.nonzero().flatten()[:10].tolist():
        print(f"COUNT {int(idx[i]):012d} = {int(counts[idx[i]])} (oracle {int(ref_c[i])})")
    if a.counts_only:
        return 0 if bad == 0 else 1
    offsets = io.read_array(a.prefix + ".offsets", torch.int64)
    ids = io.read_array(a.prefix + ".ids", torch.int32)
    dist = io.read_array(a.prefix + ".dist", torch.float32)
    want = torch.zeros(nq + 1, dtype=torch.int64)
    torch.cumsum(counts, 0, dtype=torch.int64, out=want[1:])
    if offsets.shape != want.shape or not torch.equal(offsets, want) or ids.shape[0] != int(want[nq]) \
            or dist.shape[0] != int(want[nq]):
        print(f"offsets are not the prefix sums of the counts, or ids ({ids.shape[0]}) / dist ({dist.shape[0]}) "
              f"do not hold their total of {int(want[nq])} pairs")
        return 1
    ro, ri, rd2 = ref_lists()
    rd = K.finalize_distances(rd2)
    rows_bad = 0
    for i, qi in enumerate(idx.tolist()):
        if wrong[i]:
            continue  # (reported above)
        gi, gd = ids[offsets[qi]:offsets[qi + 1]], dist[offsets[qi]:offsets[qi + 1]]
        wi, wd = ri[ro[i]:ro[i + 1]], rd[ro[i]:ro[i + 1]]
        if a.unsorted:  # compared as sets: ids are distinct within a row
            o, w = torch.argsort(gi.long()), torch.argsort(wi.long())
            gi, gd, wi, wd = gi[o], gd[o], wi[w], wd[w]
        diff = ((gi != wi) | (gd != wd)).nonzero().flatten()
        if diff.numel():
            rows_bad += 1
            if rows_bad <= 10:
                j = int(diff[0])
                print(f"ROW {qi:012d} slot {j}: id {int(gi[j])} dist {gd[j].item()!r} "
                      f"(oracle id {int(wi[j])} dist {wd[j].item()!r})")
    print(f"checked {idx.numel()} sampled rows: {rows_bad} mismatches")
    return 0 if bad + rows_bad == 0 else 1


def ccheck(a) -> int:
    pts = io.read_points(a.inp)
    n = pts.shape[0]
    if n > CCHECK_MAX:
        print(f"ccheck: {n} points, more than {CCHECK_MAX}: the oracle is quadratic (it visits every pair of "
              "points); check a smaller set")
        return 1
    if math.isnan(a.eps) or a.eps < 0 or a.min_pts < 1:
        print("ccheck: -r must be >= 0 and --min-pts at least 1")
        return 1
    labels = io.read_array(a.prefix + ".labels", torch.int32)
    core = torch.from_numpy(np.fromfile(a.prefix + ".core", dtype=np.uint8))
    if labels.shape[0] != n or core.shape[0] != n:
        print(f"size mismatch: {labels.shape[0]} labels, {core.shape[0]} core flags for {n} points")
        return 1
    cut2 = float(np.float32(a.eps)) if a.squared else cut2_of(a.eps)
    if a.period is not None:
        ref_l, ref_c = K.cluster_periodic_cpu(pts, cut2, a.min_pts, a.period)
    else:
        ref_l, ref_c = K.cluster_cpu(pts, cut2, a.min_pts)
    bad_c = (core != ref_c.to(torch.uint8)).nonzero().flatten()
    bad_l = (labels != ref_l).nonzero().flatten()
    print(f"checked {n} points: {bad_c.numel()} core flag mismatches, {bad_l.numel()} label mismatches")
    for i in bad_c[:10].tolist():
        print(f"CORE {i:012d} = {int(core[i])} (oracle {int(ref_c[i])})")
    for i in bad_l[:10].tolist():
        print(f"LABEL {i:012d} = {int(labels[i])} (oracle {int(ref_l[i])})")
    return 0 if bad_c.numel() + bad_l.numel() == 0 else 1


def mcheck(a) -> int:
    pts = io.read_points(a.inp)
    n = pts.shape[0]
    if n > CCHECK_MAX:
        print(f"mcheck: {n} points, more than {CCHECK_MAX}: the oracle is quadratic (it visits every pair of "
              "points); check a smaller set")
        return 1
    if a.core_k < 0:
        print("mcheck: --core-k must be at least 1")
        return 1
    rows = io.read_array(a.prefix + ".mst.rows", torch.int32)
    d2 = io.read_array(a.prefix + ".mst.d2", torch.float32)
    if rows.shape[0] != 2 * d2.shape[0]:
        print(f"size mismatch: {rows.shape[0]} row entries for {d2.shape[0]} weights")
        return 1
    rows = rows.view(-1, 2)
    core = None
    if a.core_k:  # the oracle's squared K-th distances, 0 for a point that is no vertex
        core = K.kth_cpu(pts, pts, a.core_k, math.inf) if a.period is None else \
            K.kth_periodic_cpu(pts, pts, a.core_k, math.inf, a.period)
        core[~torch.isfinite(pts).all(dim=1)] = 0.0
        if not bool(torch.isfinite(core).all()):
            print(f"mcheck: --core-k {a.core_k} exceeds the number of finite points")
            return 1
    ref_r, ref_d = K.mst_cpu(pts, core) if a.period is None else K.mst_periodic_cpu(pts, a.period, core)
    if ref_d.shape[0] != d2.shape[0]:
        print(f"checked {n} points: {d2.shape[0]} edges, the oracle has {ref_d.shape[0]}")
        return 1
    bad = ((rows != ref_r).any(dim=1) | (d2.view(torch.int32) != ref_d.view(torch.int32))).nonzero().flatten()
    print(f"checked {n} points: {ref_d.shape[0]} edges, {bad.numel()} edge mismatches")
    for i in bad[:10].tolist():
        print(f"EDGE {i:012d} = ({int(rows[i, 0])}, {int(rows[i, 1])}) d2 {d2[i].item()!r} "
              f"(oracle ({int(ref_r[i, 0])}, {int(ref_r[i, 1])}) d2 {ref_d[i].item()!r})")
    return 0 if bad.numel() == 0 else 1


def wrap(a) -> int:
    pts = io.read_points(a.inp)
    try:
        origin = [float(v) for v in a.origin.split(",")]
        out = wrap_points(pts, a.period, origin[0] if len(origin) == 1 else origin)
    except ValueError as e:
        print(f"wrap: {e}")
        return 1
    io.write_points(a.out, out)
    print(f"wrote {out.shape[0]} points to {a.out}")
    return 0


def cat(a) -> int:
    parts = [io.read_floats(f"{a.prefix}_{r:06d}.float") for r in range(a.p)]
    out = torch.cat(parts)
    if a.order:
        order = torch.load(a.order, weights_only=True)
        full = torch.empty_like(out)
        full[order] = out
        out = full
    io.write_floats(a.out, out)
    print(f"wrote {out.shape[0]} distances to {a.out}")
    return 0


def cmp(a) -> int:
    x, y = io.read_floats(a.a), io.read_floats(a.b)
    if x.shape != y.shape:
        print(f"different sizes {x.shape[0]} vs {y.shape[0]}")
        return 1
    same = (x == y) | (torch.isnan(x) & torch.isnan(y))
    nbad = int((~same).sum())
    print("identical" if nbad == 0 else f"{nbad} differing values")
    return 0 if nbad == 0 else 1


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="lsknn-tools")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("gen")
    p.add_argument("out")
    p.add_argument("-n", type=float, required=True)
    p.add_argument("--dist", choices=["uniform", "clustered"], default="uniform")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--clusters", type=int, default=100)
    p.add_argument("--sigma", type=float, default=0.01)
    p = sub.add_parser("split")
    p.add_argument("inp")
    p.add_argument("-p", type=int, required=True)
    p.add_argument("-o", dest="out", required=True)
    p.add_argument("--spatial", action="store_true")
    p = sub.add_parser("check")
    p.add_argument("inp")
    p.add_argument("dist_file")
    p.add_argument("-k", type=int, required=True)
    p.add_argument("-r", type=float, default=math.inf)
    p.add_argument("--samples", type=int, default=10000)
    p.add_argument("--queries", default=None, help="float3 file whose rows the distances belong to (hipKNN_query)")
    p.add_argument("--neighbors", default=None, metavar="PREFIX",
                   help="also check PREFIX.ids / PREFIX.dist (hipKNN_query --neighbors)")
    from .radius import add_period_option, add_radius_options
    add_period_option(p)
    p = sub.add_parser("rcheck")
    p.add_argument("inp")
    p.add_argument("queries")
    p.add_argument("prefix", help="the -o PREFIX of hipKNN_radius")
    add_radius_options(p)
    p.add_argument("--samples", type=int, default=None,
                   help="rows compared (default 1000; --profile: every row of up to 65536)")
    p.add_argument("--counts-only", action="store_true")
    p.add_argument("--unsorted", action="store_true", help="rows written with --unsorted: compared as sets")
    p = sub.add_parser("pcheck")
    p.add_argument("inp")
    p.add_argument("queries")
    p.add_argument("prefix", help="the -o PREFIX of hipKNN_pairs")
    from .pairs import add_pairs_options, pairs_mode
    add_pairs_options(p)
    pcheck_parser = p
    p = sub.add_parser("fixweights")
    p.add_argument("inp", help="headerless float32 file of weights (masses)")
    p.add_argument("out", help="headerless int64 file")
    p.add_argument("--bits", type=int, default=62, help="sum |w_fix| <= 2^bits (default 62; pair sums: split them)")
    p.add_argument("--terms", type=int, default=None, help="weights that can meet in one sum (default: the file's)")
    p = sub.add_parser("ccheck")
    p.add_argument("inp")
    p.add_argument("prefix", help="the -o PREFIX of hipKNN_cluster")
    p.add_argument("-r", dest="eps", type=float, required=True)
    p.add_argument("--min-pts", type=int, default=1)
    p.add_argument("--squared", action="store_true", help="-r is the squared cutoff")
    add_period_option(p)
    p = sub.add_parser("mcheck")
    p.add_argument("inp")
    p.add_argument("prefix", help="the -o PREFIX of hipKNN_mst")
    p.add_argument("--core-k", type=int, default=0, metavar="K", help="the --core-k of the run")
    add_period_option(p)
    p = sub.add_parser("wrap")
    p.add_argument("inp")
    p.add_argument("out")
    add_period_option(p)
    p.add_argument("--origin", default="0", metavar="O | Ox,Oy,Oz", help="lower corner of the period (default 0)")
    p = sub.add_parser("cat")
    p.add_argument("prefix")
    p.add_argument("p", type=int)
    p.add_argument("out")
    p.add_argument("--order", default=None, help="order file written by split --spatial")
    p = sub.add_parser("cmp")
    p.add_argument("a")
    p.add_argument("b")
    a = ap.parse_args(argv)
    if a.cmd == "wrap" and a.period is None:
        ap.error("wrap: --period is required")
    if a.cmd == "pcheck":
        pairs_mode(pcheck_parser, a)
    return {"pcheck": pcheck, "gen": gen, "split": split, "check": check, "rcheck": rcheck, "ccheck": ccheck, "mcheck": mcheck, "wrap": wrap,
            "cat": cat,
            "cmp": cmp, "fixweights": fixweights}[a.cmd](a)


if __name__ == "__main__":
    sys.exit(main())

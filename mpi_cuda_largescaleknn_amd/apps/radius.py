"""hipKNN_radius — fixed-radius search: every point within a distance of each query.

    hipKNN_radius <points.float3> <queries.float3> (-r <radius> | --radii FILE | --point-radii FILE) [--squared]
                  -o <PREFIX> [--counts-only] [--unsorted] [--chunk N] [--max-pairs M]
                  [--period L | Lx,Ly,Lz] [--device auto|cuda|cpu] [--stats f.json] [-v]
    hipKNN_radius <points.float3> <queries.float3> --reach QRADII.float PRADII.float [--rule either|both] [--squared]
                  -o <PREFIX> [--counts-only] [--unsorted] [--chunk N] [--max-pairs M]
                  [--period L | Lx,Ly,Lz] [--device auto|cuda|cpu] [--stats f.json] [-v]
    hipKNN_radius <points.float3> <queries.float3> --profile R1,R2,... [--squared] -o <PREFIX> [--pairs-only]
                  [--weights W.i64 [--query-weights WQ.i64]]
                  [--chunk N] [--period L | Lx,Ly,Lz] [--device auto|cuda|cpu] [--stats f.json] [-v]

For every row of the query file, the points of the point file with dist2 < radius² (float32
product, strict: the comparison of the -r cutoff of the k-NN tools), however many there
are. Exactly one of: -r, one radius for all; --radii, a headerless float32 file with one
radius per query row (gather: dist2 < the query's radius²); --point-radii, one radius per
point row (scatter: dist2 < the point's radius², the points whose own ball holds the query).
--squared: the values are the squared cutoffs themselves. PREFIX.count holds one int32 per query. Unless --counts-only is given the lists follow
in CSR form: PREFIX.offsets (int64 [nq + 1], row q = [offsets[q], offsets[q + 1])),
PREFIX.ids (int32 [total], rows of the point file) and PREFIX.dist (float32 [total]); each
row ascending by (distance, row) unless --unsorted. All files are headerless.

--period L or Lx,Ly,Lz (inf: an open axis): the box is periodic, distances are those of the
minimum image of the coordinate difference (lsknn_tools wrap brings coordinates into one
period); a radius may not exceed half the period of a finite axis. Not with --point-radii (--reach with an all-zero QRADII file is that
search under a period).

--reach QRADII.float PRADII.float: a radius on both sides, one float32 per query row and one per
point row. --rule either (default): dist2 < max(query's, point's)², the symmetric
neighbourhood; --rule both: dist2 < min(...)², the mutual one. Under "either" a query with
radius 0 is still reached by points. The point radii are prepared once for all chunks. With
--period every value of both files may not exceed half the period of a finite axis.

--profile R1,R2,...: ascending radii (inf allowed); in place of the lists, the counts at every
radius from one walk: PREFIX.profile (int32 [nq][B], row-major; column b = the counts of -r
Rb) and PREFIX.pairs (int64 [B], the column sums: the cumulative pair counts of a two-point
histogram). --pairs-only writes PREFIX.pairs alone and never holds an [nq][B] array. One line per
radius is printed: radius, cumulative pairs, pairs in the shell below it.

--profile with --weights W.i64 (a headerless little-endian int64 file, one weight per point row,
negative allowed): in place of the counts, the exact sums of the weights within every radius,
PREFIX.wprofile (int64 [nq][B]) and PREFIX.wpairs (int64 [B], the sums over the queries, each row
times its weight of --query-weights WQ.i64, one int64 per query row; without it 1). The weights are
prepared once for all chunks; max|w| * n must be below 2^62 and (sum |w|) * (sum |wq|) below 2^63
(lsknn_tools fixweights turns float masses into such weights). One line per radius: radius,
cumulative sum, sum of the shell below it. Without --weights nothing about --profile changes.

The index over the points is built once; the queries go through it in chunks of --chunk
rows. A chunk with more than --max-pairs pairs is split along its counts' prefix sums into
runs of queries that fit, so device memory bounds --max-pairs, not the output. One process,
one device.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time

import torch

from ..models import knn_engine as E
from ..ops import kernels as K
from ..parallel import launch as L
from ..utils import io
from .query import _device


def period_arg(text: str) -> tuple[float, float, float]:
    """--period L | Lx,Ly,Lz: three values > 0, inf = open axis (also hipKNN_cluster, lsknn_tools)."""
    try:
        vals = [float(v) for v in text.split(",")]
        if len(vals) == 1:
            vals = vals * 3
        return K.check_period("--period", vals)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def add_period_option(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--period", type=period_arg, default=None, metavar="L | Lx,Ly,Lz",
                    help="periodic box: minimum-image distances (inf: an open axis)")


def profile_arg(text: str) -> list[float]:
    """--profile R1,R2,...: at least one radius, each >= 0, ascending (inf allowed)."""
    try:
        vals = [float(v) for v in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--profile: not a list of numbers: {text!r}") from None
    if any(math.isnan(v) or v < 0 for v in vals) or any(b < a for a, b in zip(vals, vals[1:])):
        raise argparse.ArgumentTypeError("--profile: radii must be >= 0, not NaN and ascending")
    return vals


def add_radius_options(ap: argparse.ArgumentParser) -> None:
    """Exactly one of -r / --radii / --point-radii / --profile / --reach, --rule, --squared and
    --period (also lsknn_tools rcheck)."""
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("-r", dest="radius", type=float, default=None, help="one radius for every query")
    g.add_argument("--radii", default=None, metavar="FILE",
                   help="headerless float32 file, one radius per query row: points with dist2 < its square")
    g.add_argument("--point-radii", default=None, metavar="FILE",
                   help="headerless float32 file, one radius per point row: points whose own ball holds the query")
    g.add_argument("--profile", type=profile_arg, default=None, metavar="R1,R2,...",
                   help="ascending radii: the counts at every radius (PREFIX.profile) and their sums (PREFIX.pairs)")
    g.add_argument("--reach", nargs=2, default=None, metavar=("QRADII", "PRADII"),
                   help="two headerless float32 files, one radius per query row and one per point row: points "
                        "with dist2 < max (--rule both: min) of the two squares")
    ap.add_argument("--rule", choices=["either", "both"], default=None,
                    help="with --reach: either ball reaches the other's centre (default), or both do")
    ap.add_argument("--pairs-only", action="store_true", help="with --profile: PREFIX.pairs (.wpairs) only")
    ap.add_argument("--weights", default=None, metavar="W.i64",
                    help="with --profile: headerless int64 file, one weight per point row: the sums of the weights "
                         "within every radius (PREFIX.wprofile, PREFIX.wpairs)")
    ap.add_argument("--query-weights", default=None, metavar="WQ.i64",
                    help="with --weights: headerless int64 file, one weight per query row, for PREFIX.wpairs")
    ap.add_argument("--squared", action="store_true", help="the given values are squared cutoffs")
    add_period_option(ap)


def read_radii(path: str, what: str, rows: int, of: str) -> torch.Tensor:
    """A radius file of `rows` float32 values; ValueError names both lengths otherwise."""
    r = io.read_array(path, torch.float32)
    if r.shape[0] != rows:
        raise ValueError(f"{what} {path} holds {r.shape[0]} values, {of} has {rows} rows")
    return r


def read_weights(path: str, what: str, rows: int, of: str) -> torch.Tensor:
    """A weight file of `rows` int64 values; ValueError names both lengths otherwise."""
    w = io.read_array(path, torch.int64)
    if w.shape[0] != rows:
        raise ValueError(f"{what} {path} holds {w.shape[0]} values, {of} has {rows} rows")
    return w


def check_reach_options(ap: argparse.ArgumentParser, a: argparse.Namespace) -> None:
    if a.rule is not None and a.reach is None:
        ap.error("--rule needs --reach")
    if a.reach is not None and a.rule is None:
        a.rule = "either"


def read_reach(a: argparse.Namespace, nq: int, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The two radius files of --reach (host tensors), every value checked: >= 0, not NaN and,
    under --period, within its bound. ValueError otherwise."""
    qrad = read_radii(a.reach[0], "--reach", nq, a.queries)
    prad = read_radii(a.reach[1], "--reach", n, a.points)
    upper = math.inf if a.period is None else E.period_radius_bound(a.period, a.squared)
    for path, r in zip(a.reach, (qrad, prad)):
        if not bool((r >= 0).all()):
            raise ValueError(f"--reach {path}: every value must be >= 0 and not NaN")
        if not bool((r <= upper).all()):
            raise ValueError(f"--reach {path}: a value exceeds half the period of a finite axis "
                             f"({'squared ' if a.squared else ''}bound {upper})")
    return qrad, prad


def check_weight_options(ap: argparse.ArgumentParser, a: argparse.Namespace) -> None:
    if a.weights is not None and a.profile is None:
        ap.error("--weights needs --profile")
    if a.query_weights is not None and a.weights is None:
        ap.error("--query-weights needs --weights")


def parse(argv: list[str]) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="hipKNN_radius")
    ap.add_argument("points", help="float3 file: the point set")
    ap.add_argument("queries", help="float3 file: the query positions")
    add_radius_options(ap)
    ap.add_argument("-o", dest="out", required=True, metavar="PREFIX",
                    help="writes PREFIX.count and, unless --counts-only, PREFIX.offsets / .ids / .dist")
    ap.add_argument("--counts-only", action="store_true")
    ap.add_argument("--unsorted", action="store_true", help="rows in no particular order (cheaper)")
    ap.add_argument("--chunk", type=int, default=1 << 24, help="queries per pass (default 2^24)")
    ap.add_argument("--max-pairs", type=int, default=1 << 28, help="pairs held on the device at once (default 2^28)")
    ap.add_argument("--device", choices=["auto", "cuda", "cpu"], default="auto")
    ap.add_argument("--stats", default="", help="write run statistics to this JSON file")
    ap.add_argument("-v", dest="verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.radius is not None and (math.isnan(a.radius) or a.radius < 0):
        ap.error("-r must be >= 0")
    if a.chunk < 1:
        ap.error("--chunk must be at least 1")
    if a.max_pairs < 1:
        ap.error("--max-pairs must be at least 1")
    if a.pairs_only and a.profile is None:
        ap.error("--pairs-only needs --profile")
    check_weight_options(ap, a)
    check_reach_options(ap, a)
    if a.profile is not None and (a.counts_only or a.unsorted):
        ap.error("--profile writes no lists: not with --counts-only / --unsorted")
    return a


def run_profile(a: argparse.Namespace, index, nq: int, dev: torch.device, stats) -> list[int] | None:
    """--profile: PREFIX.profile (unless --pairs-only) and PREFIX.pairs, the queries in chunks;
    the cumulative pair counts, or None after an error message."""
    per = {} if a.period is None else {"period": a.period}
    nb = len(a.profile)
    gpu = dev.type == "cuda"
    pairs = [0] * nb  # Python ints: no overflow however many chunks
    try:
        E._profile_cutoffs("--profile", a.profile, a.squared, a.period)  # before anything is written
        if not a.pairs_only:
            io.write_array(a.out + ".profile", torch.empty(0, dtype=torch.int32), 0, truncate=True, total=nq * nb)
        for begin in range(0, nq, a.chunk):
            q = io.read_range(a.queries, begin, min(a.chunk, nq - begin), pin_memory=gpu).to(dev)
            if a.pairs_only:
                part = E.pair_counts(index, q, a.profile, squared=a.squared, stats=stats, **per)
            else:
                prof = E.radius_profile(index, q, a.profile, squared=a.squared, stats=stats, **per)
                io.write_array(a.out + ".profile", prof.cpu().reshape(-1), begin * nb, truncate=False)
                part = prof.sum(0, dtype=torch.int64)
            pairs = [s + int(v) for s, v in zip(pairs, part.cpu().tolist())]
    except ValueError as e:
        sys.stderr.write(f"hipKNN_radius: {e}\n")
        return None
    io.write_array(a.out + ".pairs", torch.tensor(pairs, dtype=torch.int64), 0, truncate=True, total=nb)
    for b, r in enumerate(a.profile):
        print(f"{r!r} {pairs[b]} {pairs[b] - (pairs[b - 1] if b else 0)}", flush=True)
    return pairs


def run_weighted_profile(a: argparse.Namespace, index, nq: int, dev: torch.device, stats) -> list[int] | None:
    """--profile --weights: PREFIX.wprofile (unless --pairs-only) and PREFIX.wpairs, the weights
    prepared once and the queries in chunks; the cumulative weighted pair sums, or None after an
    error message."""
    per = {} if a.period is None else {"period": a.period}
    nb = len(a.profile)
    gpu = dev.type == "cuda"
    sums = [0] * nb
    try:
        E._profile_cutoffs("--profile", a.profile, a.squared, a.period)  # before anything is written
        pw = E.prepare_point_weights(index, read_weights(a.weights, "--weights", index.n, a.points).to(dev))
        wq = None if a.query_weights is None else read_weights(a.query_weights, "--query-weights", nq, a.queries)
        E.check_pair_sum_bound("--weights", pw, wq, nq)  # the whole file's bound: PREFIX.wpairs holds int64
        if not a.pairs_only:
            io.write_array(a.out + ".wprofile", torch.empty(0, dtype=torch.int64), 0, truncate=True, total=nq * nb)
        for begin in range(0, nq, a.chunk):
            q = io.read_range(a.queries, begin, min(a.chunk, nq - begin), pin_memory=gpu).to(dev)
            wqc = None if wq is None else wq[begin:begin + q.shape[0]].to(dev)
            if a.pairs_only:
                part = E.weighted_pair_sums(index, q, a.profile, pw, query_weights=wqc, squared=a.squared,
                                            stats=stats, **per)
            else:
                prof = E.weighted_profile(index, q, a.profile, pw, squared=a.squared, stats=stats, **per)
                io.write_array(a.out + ".wprofile", prof.cpu().reshape(-1), begin * nb, truncate=False)
                part = (prof if wqc is None else prof * wqc[:, None]).sum(0, dtype=torch.int64)
            sums = [s + int(v) for s, v in zip(sums, part.cpu().tolist())]
    except ValueError as e:
        sys.stderr.write(f"hipKNN_radius: {e}\n")
        return None
    io.write_array(a.out + ".wpairs", torch.tensor(sums, dtype=torch.int64), 0, truncate=True, total=nb)
    for b, r in enumerate(a.profile):
        print(f"{r!r} {sums[b]} {sums[b] - (sums[b - 1] if b else 0)}", flush=True)
    return sums


def split_runs(counts: torch.Tensor, max_pairs: int) -> list[tuple[int, int]]:
    """Maximal runs [s, e) of consecutive queries whose counts (CPU tensor) sum to at most
    max_pairs. Raises ValueError(position) for a single query above max_pairs."""
    csum = torch.cumsum(counts.long(), 0)
    runs, s, base, m = [], 0, 0, counts.shape[0]
    while s < m:
        # the last e with csum[e - 1] - base <= max_pairs
        e = int(torch.searchsorted(csum, torch.tensor(base + max_pairs), right=True))
        if e <= s:
            raise ValueError(s)
        runs.append((s, e))
        s, base = e, int(csum[e - 1])
    return runs


def main(argv: list[str] | None = None) -> int:
    a = parse(list(sys.argv[1:] if argv is None else argv))
    if L.rank_info("auto")[1] > 1:
        sys.stderr.write("hipKNN_radius: runs as one process on one device (radius queries over several ranks "
                         "are not supported)\n")
        return 1
    if a.period is not None and a.point_radii is not None:
        sys.stderr.write("hipKNN_radius: --period is not supported with --point-radii\n")
        return 1
    try:
        if a.period is not None and a.radius is not None:
            E.check_period_radius("-r", a.radius, a.squared, a.period)
    except ValueError as e:
        sys.stderr.write(f"hipKNN_radius: {e}\n")
        return 1
    # (None: the calls below are the ones without the keyword)
    per = {} if a.period is None else {"period": a.period}
    dev = _device(a.device)
    gpu = dev.type == "cuda"
    stats = E.KnnStats() if a.stats else None
    sync = (lambda: torch.cuda.synchronize(dev)) if gpu else (lambda: None)
    t0 = time.perf_counter()
    points = io.read_points(a.points, pin_memory=gpu).to(dev)
    index = E.build_index(points)
    sync()
    t1 = time.perf_counter()
    nq = io.portion(a.queries, 0, 1)[2]
    if a.profile is not None:
        sums = (run_profile if a.weights is None else run_weighted_profile)(a, index, nq, dev, stats)
        if sums is None:
            return 1
        sync()
        t2 = time.perf_counter()
        if a.verbose:
            print(f"index of {index.n} points: {t1 - t0:.3f}s; {nq} queries, {len(a.profile)} radii: {t2 - t1:.3f}s  "
                  f"kernels {E.kernels_used()}", flush=True)
        if a.stats:
            rec = {"n": index.n, "nq": nq, "profile": a.profile, "pairs": sums, "chunk": a.chunk,
                   "device": str(dev), "index_s": t1 - t0, "query_s": t2 - t1, "kernels": E.kernels_used(),
                   "radius_search": stats.counters}
            if a.weights is not None:
                rec.update({"weights": a.weights, "query_weights": a.query_weights})
            if a.squared:
                rec["squared"] = True
            if a.period is not None:
                rec["period"] = list(a.period)
            with open(a.stats, "w") as f:
                json.dump(rec, f, indent=1)
        return 0
    # the search of queries [b, e) of the file: one radius, one per query (sliced with the
    # queries), one per point (prepared once), or both
    try:
        if a.radii is not None:
            qrad = read_radii(a.radii, "--radii", nq, a.queries)
            if not bool((qrad >= 0).all()):
                raise ValueError(f"--radii {a.radii}: every value must be >= 0 and not NaN")

            def count_fn(q, b, e):
                return E.radius_counts(index, q, qrad[b:e].to(dev), stats=stats, squared=a.squared, **per)

            def lists_fn(q, b, e):
                return E.radius_neighbors(index, q, qrad[b:e].to(dev), sort=not a.unsorted, max_pairs=a.max_pairs,
                                          squared=a.squared, **per)
        elif a.reach is not None:
            qrad, prow = read_reach(a, nq, index.n)
            prad = E.prepare_point_radii(index, prow.to(dev), squared=a.squared)

            def count_fn(q, b, e):
                return E.reach_counts(index, q, qrad[b:e].to(dev), prad, rule=a.rule, squared=a.squared, stats=stats,
                                      **per)

            def lists_fn(q, b, e):
                return E.reach_neighbors(index, q, qrad[b:e].to(dev), prad, rule=a.rule, squared=a.squared,
                                         sort=not a.unsorted, max_pairs=a.max_pairs, **per)
        elif a.point_radii is not None:
            prad = E.prepare_point_radii(index, read_radii(a.point_radii, "--point-radii", index.n, a.points).to(dev),
                                         squared=a.squared)

            def count_fn(q, b, e):
                return E.point_radius_counts(index, q, prad, stats=stats)

            def lists_fn(q, b, e):
                return E.point_radius_neighbors(index, q, prad, sort=not a.unsorted, max_pairs=a.max_pairs)
        else:
            def count_fn(q, b, e):
                return E.radius_counts(index, q, a.radius, stats=stats, squared=a.squared, **per)

            def lists_fn(q, b, e):
                return E.radius_neighbors(index, q, a.radius, sort=not a.unsorted, max_pairs=a.max_pairs,
                                          squared=a.squared, **per)
    except ValueError as e:
        sys.stderr.write(f"hipKNN_radius: {e}\n")
        return 1
    lists = not a.counts_only
    io.write_array(a.out + ".count", torch.empty(0, dtype=torch.int32), 0, truncate=True, total=nq)
    if lists:
        io.write_array(a.out + ".offsets", torch.empty(0, dtype=torch.int64), 0, truncate=True, total=nq + 1)
        io.write_array(a.out + ".ids", torch.empty(0, dtype=torch.int32), 0, truncate=True)
        io.write_array(a.out + ".dist", torch.empty(0, dtype=torch.float32), 0, truncate=True)
    pairs = 0  # pairs written so far = the global offset of the next row
    for begin in range(0, nq, a.chunk):
        q = io.read_range(a.queries, begin, min(a.chunk, nq - begin), pin_memory=gpu).to(dev)
        try:
            counts = count_fn(q, begin, begin + q.shape[0]).cpu()
        except ValueError as e:  # (a --radii entry above half the period)
            if a.period is None:
                raise
            sys.stderr.write(f"hipKNN_radius: {e}\n")
            return 1
        io.write_array(a.out + ".count", counts, begin, truncate=False)
        if not lists:
            pairs += int(counts.sum())
            continue
        try:
            runs = split_runs(counts, a.max_pairs)
        except ValueError as e:
            s = int(e.args[0])
            sys.stderr.write(f"hipKNN_radius: query {begin + s} alone has {int(counts[s])} points within the radius, "
                             f"more than --max-pairs {a.max_pairs}\n")
            return 1
        for s, e in runs:
            offsets, idx, dist = lists_fn(q[s:e], begin + s, begin + e)
            io.write_array(a.out + ".offsets", offsets[:-1].cpu() + pairs, begin + s, truncate=False)
            io.write_array(a.out + ".ids", idx, pairs, truncate=False)
            io.write_array(a.out + ".dist", dist, pairs, truncate=False)
            pairs += idx.shape[0]
    if lists:
        io.write_array(a.out + ".offsets", torch.tensor([pairs], dtype=torch.int64), nq, truncate=False)
    sync()
    t2 = time.perf_counter()
    if a.verbose:
        print(f"index of {index.n} points: {t1 - t0:.3f}s; {nq} queries, {pairs} pairs: {t2 - t1:.3f}s  "
              f"{nq / max(t2 - t1, 1e-9) / 1e6:.1f} Mqueries/s  kernels {E.kernels_used()}", flush=True)
    if a.stats:
        rec = {"n": index.n, "nq": nq, "radius": a.radius, "pairs": pairs, "chunk": a.chunk,
               "max_pairs": a.max_pairs, "device": str(dev), "index_s": t1 - t0, "query_s": t2 - t1,
               "kernels": E.kernels_used(), "radius_search": stats.counters}
        if a.radius is None:
            rec.update({"radii": a.radii, "point_radii": a.point_radii})
            if a.reach is not None:
                rec.update({"reach": list(a.reach), "rule": a.rule})
        if a.squared:
            rec["squared"] = True
        if a.period is not None:
            rec["period"] = list(a.period)
        with open(a.stats, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

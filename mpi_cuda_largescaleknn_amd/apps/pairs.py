"""hipKNN_pairs — anisotropic pair counts along a line of sight: DD(rp, pi) and DD(s, mu).

    hipKNN_pairs <points.float3> <queries.float3> (--rp R1,R2,... --pi P1,P2,... | --s S1,S2,... --mu M1,M2,...)
                 [--los x|y|z|midpoint [--observer ox,oy,oz]] [--squared] [--period L | Lx,Ly,Lz]
                 [--weights W.i64 [--query-weights WQ.i64]] [--chunk N] [--device auto|cuda|cpu] [--stats f.json]
                 [-v] -o <PREFIX>

For every pair (row of the query file, row of the point file) the float32 differences q - p, with
--period their minimum image, are split along the line of sight --los (a box axis, default z):
par2 = dl * dl and perp2 = fmaf(db, db, da * da) of the other two axes. --rp / --pi: ascending
radii across and along the line of sight (inf allowed); cell [i][j] of the result counts the
pairs with perp2 < rp[i]² and par2 < pi[j]², strict and cumulative on both axes. --s / --mu:
ascending separations and cosines to the line of sight (inf allowed); cell [i][j] counts the pairs
with d2 < s[i]² and par2 < mu[j]² * d2, so a pair at distance 0 counts nowhere and mu = 1 leaves
out the pairs exactly along the line of sight, which mu = inf takes in. --squared: --rp, --pi and
--s hold the squared cutoffs themselves (--mu is always plain mu). With --period a radius along
the line of sight may not exceed half the period of that axis, one across it not half the period
of a finite perpendicular axis.

--los midpoint: every pair has its own line of sight, the direction from --observer (three finite
numbers, default 0,0,0) to the pair's midpoint, as for survey catalogues, light cones and mocks
with randoms. With l = (q - o) + (p - o) per axis and sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx)):
par2 = (sl / dist2(l)) * sl and perp2 = d2 - par2 (a negative one becomes 0), all float32; the
cells are the same. A pair whose midpoint is the observer counts nowhere. Open box only: --period
is refused, and so is --observer with an axis --los.

PREFIX.pairs2d holds the counts, headerless int64 [B1][B2], row-major. One line per row of cells
is printed: the first-axis edge, then the row's binned (not cumulative) counts. The index over the
points is built once; the queries go through it in chunks of --chunk rows whose counts are added
on the host. One process, one device.

--weights W.i64: a headerless little-endian int64 file, one weight per row of the point file,
negative allowed; --query-weights WQ.i64: the same per row of the query file (without it every
query weighs 1). Every pair then adds wq * w in the place of 1 and the result goes to
PREFIX.wpairs2d (int64 [B1][B2], cumulative; PREFIX.pairs2d is not written), the printed rows hold
the binned sums. The sums are exact: max|w| * n must be below 2^62 and (sum |w|) * (sum |wq|) (the
number of queries without --query-weights) below 2^63, checked over the whole query file before the
first chunk. lsknn_tools fixweights turns float masses into such weights.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch

from ..models import knn_engine as E
from ..parallel import launch as L
from ..utils import io
from .query import _device
from .radius import add_period_option, read_weights


def edges_arg(name: str):
    def parse(text: str) -> list[float]:
        try:
            return [float(v) for v in text.split(",")]
        except ValueError:
            raise argparse.ArgumentTypeError(f"{name}: not a list of numbers: {text!r}") from None
    return parse


def add_pairs_options(ap: argparse.ArgumentParser) -> None:
    """--rp --pi | --s --mu, --los, --observer, --squared and --period (also lsknn_tools pcheck)."""
    ap.add_argument("--rp", type=edges_arg("--rp"), default=None, metavar="R1,R2,...",
                    help="ascending radii across the line of sight (with --pi)")
    ap.add_argument("--pi", type=edges_arg("--pi"), default=None, metavar="P1,P2,...",
                    help="ascending radii along the line of sight (with --rp)")
    ap.add_argument("--s", type=edges_arg("--s"), default=None, metavar="S1,S2,...",
                    help="ascending separations (with --mu)")
    ap.add_argument("--mu", type=edges_arg("--mu"), default=None, metavar="M1,M2,...",
                    help="ascending cosines to the line of sight, inf allowed (with --s)")
    ap.add_argument("--los", type=str.lower, choices=["x", "y", "z", "midpoint"], default="z",
                    help="the line-of-sight axis (default z), or midpoint: from --observer to each pair's midpoint")
    ap.add_argument("--observer", type=edges_arg("--observer"), default=None, metavar="ox,oy,oz",
                    help="with --los midpoint: the observer, default 0,0,0 (a negative first value: --observer=-1,0,0)")
    ap.add_argument("--squared", action="store_true", help="--rp / --pi / --s are squared cutoffs")
    add_period_option(ap)
    ap.add_argument("--weights", default=None, metavar="W.i64",
                    help="headerless int64 file, one weight per point row: the sums of wq * w (PREFIX.wpairs2d)")
    ap.add_argument("--query-weights", default=None, metavar="WQ.i64",
                    help="with --weights: headerless int64 file, one weight per query row")


def pairs_mode(ap: argparse.ArgumentParser, a: argparse.Namespace) -> None:
    """Sets a.mode ('rppi' | 'smu'), a.first, a.second; exactly one complete pair of lists."""
    rppi = a.rp is not None or a.pi is not None
    smu = a.s is not None or a.mu is not None
    if rppi == smu or (rppi and (a.rp is None or a.pi is None)) or (smu and (a.s is None or a.mu is None)):
        ap.error("exactly one of: --rp with --pi, --s with --mu")
    a.mode = "rppi" if rppi else "smu"
    a.first, a.second = (a.rp, a.pi) if rppi else (a.s, a.mu)
    if a.query_weights is not None and a.weights is None:
        ap.error("--query-weights needs --weights")


def parse(argv: list[str]) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="hipKNN_pairs")
    ap.add_argument("points", help="float3 file: the point set")
    ap.add_argument("queries", help="float3 file: the query positions")
    add_pairs_options(ap)
    ap.add_argument("-o", dest="out", required=True, metavar="PREFIX", help="writes PREFIX.pairs2d (--weights: PREFIX.wpairs2d)")
    ap.add_argument("--chunk", type=int, default=1 << 24, help="queries per pass (default 2^24)")
    ap.add_argument("--device", choices=["auto", "cuda", "cpu"], default="auto")
    ap.add_argument("--stats", default="", help="write run statistics to this JSON file")
    ap.add_argument("-v", dest="verbose", action="store_true")
    a = ap.parse_args(argv)
    pairs_mode(ap, a)
    if a.chunk < 1:
        ap.error("--chunk must be at least 1")
    return a


def main(argv: list[str] | None = None) -> int:
    a = parse(list(sys.argv[1:] if argv is None else argv))
    if L.rank_info("auto")[1] > 1:
        sys.stderr.write("hipKNN_pairs: runs as one process on one device\n")
        return 1
    try:  # before anything is read or written
        E._pairs2d_cutoffs("hipKNN_pairs", a.mode, a.first, a.second, a.los, a.squared, a.period, a.observer)
    except ValueError as e:
        sys.stderr.write(f"hipKNN_pairs: {e}\n")
        return 1
    per = {} if a.period is None else {"period": a.period}
    if a.observer is not None:
        per["observer"] = a.observer
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
    weighted = a.weights is not None
    if weighted:
        fn = E.weighted_pair_sums_rppi if a.mode == "rppi" else E.weighted_pair_sums_smu
    else:
        fn = E.pair_counts_rppi if a.mode == "rppi" else E.pair_counts_smu
    b1, b2 = len(a.first), len(a.second)
    total = [[0] * b2 for _ in range(b1)]  # Python ints: no overflow however many chunks
    try:
        if weighted:  # the weights once, and the whole file's bound: PREFIX.wpairs2d holds int64
            pw = E.prepare_point_weights(index, read_weights(a.weights, "--weights", index.n, a.points).to(dev))
            wq = None if a.query_weights is None else read_weights(a.query_weights, "--query-weights", nq, a.queries)
            E.check_pair_sum_bound("--weights", pw, wq, nq)
        for begin in range(0, nq, a.chunk):
            q = io.read_range(a.queries, begin, min(a.chunk, nq - begin), pin_memory=gpu).to(dev)
            if weighted:
                wqc = None if wq is None else wq[begin:begin + q.shape[0]].to(dev)
                part = fn(index, q, a.first, a.second, pw, query_weights=wqc, los=a.los, squared=a.squared,
                          stats=stats, **per)
            else:
                part = fn(index, q, a.first, a.second, los=a.los, squared=a.squared, stats=stats, **per)
            total = [[s + int(v) for s, v in zip(row, prow)] for row, prow in zip(total, part.cpu().tolist())]
    except ValueError as e:
        sys.stderr.write(f"hipKNN_pairs: {e}\n")
        return 1
    S = torch.tensor(total, dtype=torch.int64).reshape(b1, b2)
    io.write_array(a.out + (".wpairs2d" if weighted else ".pairs2d"), S.reshape(-1), 0, truncate=True, total=b1 * b2)
    for edge, row in zip(a.first, E.shell_counts_2d(S).tolist()):
        print(f"{edge!r} " + " ".join(str(v) for v in row), flush=True)
    sync()
    t2 = time.perf_counter()
    if a.verbose:
        print(f"index of {index.n} points: {t1 - t0:.3f}s; {nq} queries, {b1} x {b2} cells: {t2 - t1:.3f}s  "
              f"kernels {E.kernels_used()}", flush=True)
    if a.stats:
        rec = {"n": index.n, "nq": nq, "mode": a.mode, "first": a.first, "second": a.second, "los": a.los,
               "pairs": total, "chunk": a.chunk, "device": str(dev), "index_s": t1 - t0, "query_s": t2 - t1,
               "kernels": E.kernels_used(), "radius_search": stats.counters}
        if weighted:
            rec["weights"] = a.weights
            if a.query_weights is not None:
                rec["query_weights"] = a.query_weights
        if a.squared:
            rec["squared"] = True
        if a.period is not None:
            rec["period"] = list(a.period)
        if a.observer is not None:
            rec["observer"] = list(a.observer)
        with open(a.stats, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""hipKNN_query — k-th-NN distances from query points to a point set.

    hipKNN_query <points.float3> <queries.float3> -o <dist.float> -k <k> [-r <maxRadius>]
                 [--device auto|cuda|cpu] [--chunk N] [--neighbors PREFIX] [--period L | Lx,Ly,Lz]
                 [--max-pairs N] [--stats f.json] [-v]

For every row of the query file, the distance to its k-th nearest point of the point file
(only the points are candidates: a query that coincides with a point finds it at distance
0). The output holds one float32 per query, in the query file's order. The index over the
points is built once; the queries go through it in chunks of --chunk rows (read, uploaded,
brought into the index's curve order, answered, written at their record offset), so a
query file larger than device memory works. One process, one device: cross queries over
several ranks are not supported.

--neighbors PREFIX additionally writes the neighbour lists, chunk by chunk: PREFIX.ids
(headerless int32 [nq][k], rows of the point file, -1 in unfilled slots) and PREFIX.dist
(headerless float32 [nq][k]), each row ascending by (distance, row); k <= 1024. The -o file
is then the lists' last column.

--period L or Lx,Ly,Lz (inf: an open axis): the box is periodic, distances and lists are those of
the minimum image (knn_engine.query_points; for coordinates inside one period, lsknn_tools wrap,
the physical periodic distance). Unlike hipKNN_radius there is no bound on the radius. Queries
near a face run a periodic radius search of at most --max-pairs pairs at a time. A bad period
exits with status 1.
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


def parse(argv: list[str]) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="hipKNN_query")
    ap.add_argument("points", help="float3 file: the point set")
    ap.add_argument("queries", help="float3 file: the query positions")
    ap.add_argument("-o", dest="out", required=True, help="output: one float32 distance per query")
    ap.add_argument("-k", type=int, required=True)
    ap.add_argument("-r", dest="max_radius", type=float, default=math.inf)
    ap.add_argument("--device", choices=["auto", "cuda", "cpu"], default="auto")
    ap.add_argument("--chunk", type=int, default=1 << 26, help="queries per pass (default 2^26)")
    ap.add_argument("--neighbors", default="", metavar="PREFIX",
                    help="also write PREFIX.ids (int32 [nq][k]) and PREFIX.dist (float32 [nq][k])")
    ap.add_argument("--period", default=None, metavar="L | Lx,Ly,Lz",
                    help="periodic box: minimum-image distances (inf: an open axis)")
    ap.add_argument("--max-pairs", type=int, default=1 << 28,
                    help="with --period: pairs held on the device at once (default 2^28)")
    ap.add_argument("--stats", default="", help="write run statistics to this JSON file")
    ap.add_argument("-v", dest="verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.k < 1:
        ap.error("-k must be at least 1")
    if a.chunk < 1:
        ap.error("--chunk must be at least 1")
    if a.max_pairs < 1:
        ap.error("--max-pairs must be at least 1")
    if a.neighbors and a.k > K.NEIGHBORS_MAX_K:
        ap.error(f"--neighbors lists at most {K.NEIGHBORS_MAX_K} neighbours per query (without it, -k is unlimited)")
    return a


def _device(pref: str) -> torch.device:
    if pref == "cpu" or (pref == "auto" and not torch.cuda.is_available()):
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise RuntimeError("--device cuda: no GPU available")
    return torch.device("cuda", torch.cuda.current_device())


def main(argv: list[str] | None = None) -> int:
    a = parse(list(sys.argv[1:] if argv is None else argv))
    if L.rank_info("auto")[1] > 1:
        sys.stderr.write("hipKNN_query: runs as one process on one device (cross queries over several ranks "
                         "are not supported)\n")
        return 1
    per = {}  # (no --period: the calls below are the ones without the keyword)
    if a.period is not None:
        from .radius import period_arg  # (hipKNN_radius' parser of the same option)
        try:
            per = {"period": period_arg(a.period), "max_pairs": a.max_pairs}
        except argparse.ArgumentTypeError as e:
            sys.stderr.write(f"hipKNN_query: {e}\n")
            return 1
    dev = _device(a.device)
    gpu = dev.type == "cuda"
    cfg = E.KnnConfig(k=a.k, max_radius=a.max_radius)
    stats = E.KnnStats() if a.stats else None
    sync = (lambda: torch.cuda.synchronize(dev)) if gpu else (lambda: None)
    t0 = time.perf_counter()
    points = io.read_points(a.points, pin_memory=gpu).to(dev)
    index = E.build_index(points, grid=True)
    sync()
    t1 = time.perf_counter()
    nq = io.portion(a.queries, 0, 1)[2]
    io.write_floats(a.out, torch.empty(0, dtype=torch.float32), 0, truncate=True, total_records=nq)
    if a.neighbors:
        io.write_rows(a.neighbors + ".ids", torch.empty((0, a.k), dtype=torch.int32), 0, truncate=True, total_rows=nq)
        io.write_rows(a.neighbors + ".dist", torch.empty((0, a.k), dtype=torch.float32), 0, truncate=True,
                      total_rows=nq)
    for begin in range(0, nq, a.chunk):
        q = io.read_range(a.queries, begin, min(a.chunk, nq - begin), pin_memory=gpu).to(dev)
        if a.neighbors:
            idx, dist = E.query_neighbors(index, q, cfg, stats=stats, **per)
            io.write_rows(a.neighbors + ".ids", idx, begin, truncate=False)
            io.write_rows(a.neighbors + ".dist", dist, begin, truncate=False)
            io.write_floats(a.out, dist[:, a.k - 1], begin, truncate=False)
        else:
            io.write_floats(a.out, E.query_points(index, q, cfg, stats=stats, **per), begin, truncate=False)
    sync()
    t2 = time.perf_counter()
    if a.verbose:
        print(f"index of {index.n} points: {t1 - t0:.3f}s; {nq} queries: {t2 - t1:.3f}s  "
              f"{nq / max(t2 - t1, 1e-9) / 1e6:.1f} Mqueries/s  kernels {E.kernels_used()}", flush=True)
    if a.stats:
        with open(a.stats, "w") as f:
            rec = {"n": index.n, "nq": nq, "k": a.k, "chunk": a.chunk, "device": str(dev),
                   "index_s": t1 - t0, "query_s": t2 - t1, "kernels": E.kernels_used(), "knn": stats.counters}
            if per:
                rec["period"] = list(per["period"])
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

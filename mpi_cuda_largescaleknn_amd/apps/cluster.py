"""hipKNN_cluster — density clustering: friends-of-friends groups and DBSCAN labels.

    hipKNN_cluster <points.float3> -r <EPS> [--min-pts M] [--squared] -o <PREFIX>
                   [--period L | Lx,Ly,Lz] [--device auto|cuda|cpu] [--stats f.json] [-v]

Two points are linked when dist2 < EPS² (float32 product, strict: the comparison of
hipKNN_radius; --squared: EPS is the squared cutoff itself). A point is a core point when at
least M points (itself and exact copies included; default 1: friends-of-friends) are linked
to it. Clusters are the connected components of the core points; a cluster's label is the
smallest row among its core points. A non-core point takes the label of its nearest core
point within the cutoff (ties: the lowest row), and is noise (-1) without one; with M = 1 a
point without any neighbour is a cluster of its own. PREFIX.labels holds one int32 per point
row, PREFIX.core one byte (1 = core point). Both files are headerless.

--period L or Lx,Ly,Lz (inf: an open axis): the box is periodic and dist2 is that of the
minimum image of the coordinate difference, so a group across a face is one group; EPS may
not exceed half the period of a finite axis.

No pair is stored, so memory stays proportional to the number of points however dense the
set is. One process, one device.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time

import torch

from ..models import knn_engine as E
from ..parallel import launch as L
from ..utils import io
from .query import _device
from .radius import add_period_option


def parse(argv: list[str]) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="hipKNN_cluster")
    ap.add_argument("points", help="float3 file: the point set")
    ap.add_argument("-r", dest="eps", type=float, required=True, help="linking length")
    ap.add_argument("--min-pts", type=int, default=1, help="points within EPS that make a core point (default 1)")
    ap.add_argument("--squared", action="store_true", help="EPS is the squared cutoff")
    ap.add_argument("-o", dest="out", required=True, metavar="PREFIX", help="writes PREFIX.labels and PREFIX.core")
    add_period_option(ap)
    ap.add_argument("--device", choices=["auto", "cuda", "cpu"], default="auto")
    ap.add_argument("--stats", default="", help="write run statistics to this JSON file")
    ap.add_argument("-v", dest="verbose", action="store_true")
    a = ap.parse_args(argv)
    if math.isnan(a.eps) or a.eps < 0:
        ap.error("-r must be >= 0")
    if a.min_pts < 1:
        ap.error("--min-pts must be at least 1")
    return a


def summary(labels: torch.Tensor) -> tuple[int, int, int]:
    """(clusters, noise points, size of the largest cluster) of a label vector."""
    dense, nclusters = E.compact_labels(labels)
    noise = int((dense < 0).sum())
    largest = int(torch.bincount(dense[dense >= 0].long()).max()) if nclusters else 0
    return nclusters, noise, largest


def main(argv: list[str] | None = None) -> int:
    a = parse(list(sys.argv[1:] if argv is None else argv))
    if L.rank_info("auto")[1] > 1:
        sys.stderr.write("hipKNN_cluster: runs as one process on one device (clustering over several ranks "
                         "is not supported)\n")
        return 1
    dev = _device(a.device)
    gpu = dev.type == "cuda"
    stats = E.KnnStats() if a.stats else None
    sync = (lambda: torch.cuda.synchronize(dev)) if gpu else (lambda: None)
    t0 = time.perf_counter()
    points = io.read_points(a.points, pin_memory=gpu).to(dev)
    index = E.build_index(points)
    sync()
    t1 = time.perf_counter()
    try:
        if a.period is None:
            labels, core = E.cluster_labels(index, a.eps, a.min_pts, squared=a.squared, stats=stats)
        else:
            labels, core = E.cluster_labels(index, a.eps, a.min_pts, squared=a.squared, stats=stats, period=a.period)
    except ValueError as e:
        sys.stderr.write(f"hipKNN_cluster: {e}\n")
        return 1
    labels, core = labels.cpu(), core.cpu()
    t2 = time.perf_counter()
    io.write_array(a.out + ".labels", labels, 0, truncate=True)
    core.to(torch.uint8).numpy().tofile(a.out + ".core")
    nclusters, noise, largest = summary(labels)
    print(f"{index.n} points: {nclusters} clusters, {noise} noise points, largest cluster {largest}", flush=True)
    if a.verbose:
        print(f"index: {t1 - t0:.3f}s; clustering: {t2 - t1:.3f}s  "
              f"{index.n / max(t2 - t1, 1e-9) / 1e6:.1f} Mpoints/s  kernels {E.kernels_used()}", flush=True)
    if a.stats:
        rec = {"n": index.n, "eps": a.eps, "min_pts": a.min_pts, "squared": a.squared, "clusters": nclusters,
               "noise": noise, "largest": largest, "core": int(core.sum()), "device": str(dev),
               "index_s": t1 - t0, "cluster_s": t2 - t1, "kernels": E.kernels_used(), "cluster": stats.counters}
        if a.period is not None:
            rec["period"] = list(a.period)
        with open(a.stats, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

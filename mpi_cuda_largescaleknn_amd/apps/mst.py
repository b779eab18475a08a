"""hipKNN_mst — Euclidean minimum spanning tree: single linkage at every linking length.

    hipKNN_mst <points.float3> -o <PREFIX> [--core-k K] [--cut EPS [--squared]]
               [--period L | Lx,Ly,Lz] [--device auto|cuda|cpu] [--stats f.json] [-v]

The vertices are the points with finite coordinates; the weight of a pair is its squared
distance dist2 (float32, the value hipKNN_radius compares), and edges are ordered by (bits of
the weight, lower row, higher row), so the tree is unique. PREFIX.mst.rows holds the edges as
int32 pairs (lower row, higher row), PREFIX.mst.d2 their float32 weights, both ascending by that
key and headerless. The edges below a cutoff are the friends-of-friends groups at that cutoff
(hipKNN_cluster at the same EPS, --min-pts 1); in ascending order they are the single-linkage
dendrogram. Weights stay squared: a cut compares them with EPS² exactly as hipKNN_radius does.

--core-k K: mutual-reachability weights max(dist2, core(a), core(b)) with core(p) the squared
distance from p to its K-th nearest neighbour (itself counted): the tree HDBSCAN starts from.
--cut EPS (--squared: EPS is the squared cutoff) also writes PREFIX.labels, one int32 per point
row: the smallest row of the point's component under the edges with weight < EPS².

--period L or Lx,Ly,Lz (inf: an open axis): the box is periodic and dist2 is that of the
minimum image of the difference (hipKNN_radius --period), with no bound on an edge's length;
the --core-k distances are the periodic ones and the --cut groups those of hipKNN_cluster
--period at the same EPS. Bring the points into one period first (lsknn_tools wrap).

One process, one device.
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
    ap = argparse.ArgumentParser(prog="hipKNN_mst")
    ap.add_argument("points", help="float3 file: the point set")
    ap.add_argument("-o", dest="out", required=True, metavar="PREFIX",
                    help="writes PREFIX.mst.rows and PREFIX.mst.d2")
    ap.add_argument("--core-k", type=int, default=0, metavar="K",
                    help="mutual-reachability weights from the squared K-th neighbour distances")
    ap.add_argument("--cut", type=float, default=None, metavar="EPS", help="also write PREFIX.labels at this cutoff")
    ap.add_argument("--squared", action="store_true", help="--cut is the squared cutoff")
    add_period_option(ap)
    ap.add_argument("--device", choices=["auto", "cuda", "cpu"], default="auto")
    ap.add_argument("--stats", default="", help="write run statistics to this JSON file")
    ap.add_argument("-v", dest="verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.core_k < 0:
        ap.error("--core-k must be at least 1")
    if a.cut is not None and (math.isnan(a.cut) or a.cut < 0):
        ap.error("--cut must be >= 0")
    return a


def main(argv: list[str] | None = None) -> int:
    a = parse(list(sys.argv[1:] if argv is None else argv))
    if L.rank_info("auto")[1] > 1:
        sys.stderr.write("hipKNN_mst: runs as one process on one device (a spanning tree over several ranks "
                         "is not supported)\n")
        return 1
    dev = _device(a.device)
    gpu = dev.type == "cuda"
    stats = E.KnnStats()
    sync = (lambda: torch.cuda.synchronize(dev)) if gpu else (lambda: None)
    t0 = time.perf_counter()
    points = io.read_points(a.points, pin_memory=gpu).to(dev)
    index = E.build_index(points, grid=gpu and a.core_k > 0)
    sync()
    t1 = time.perf_counter()
    try:
        core = E.mst_core_d2(index, a.core_k, period=a.period) if a.core_k else None
        rows, d2 = E.mst_edges(index, core, stats=stats, period=a.period)
        labels = E.mst_labels(rows, d2, index.n, a.cut, squared=a.squared) if a.cut is not None else None
    except ValueError as e:
        sys.stderr.write(f"hipKNN_mst: {e}\n")
        return 1
    rows, d2 = rows.cpu(), d2.cpu()
    t2 = time.perf_counter()
    io.write_array(a.out + ".mst.rows", rows.reshape(-1), 0, truncate=True)
    io.write_array(a.out + ".mst.d2", d2, 0, truncate=True)
    rounds = stats.counters.get("mst_rounds", 0)
    heaviest = f"heaviest edge ({int(rows[-1, 0])}, {int(rows[-1, 1])}) d2 {d2[-1].item()!r}" if d2.numel() else \
        "no edge"
    print(f"{index.n} points: {d2.numel()} edges in {rounds} rounds, {heaviest}", flush=True)
    if labels is not None:
        labels = labels.cpu()
        io.write_array(a.out + ".labels", labels, 0, truncate=True)
        print(f"cut {a.cut!r}: {int(torch.unique(labels).numel())} groups", flush=True)
    if a.verbose:
        print(f"index: {t1 - t0:.3f}s; spanning tree: {t2 - t1:.3f}s  "
              f"{index.n / max(t2 - t1, 1e-9) / 1e6:.1f} Mpoints/s  kernels {E.kernels_used()}", flush=True)
    if a.stats:
        rec = {"n": index.n, "edges": int(d2.numel()), "core_k": a.core_k, "cut": a.cut, "squared": a.squared,
               "device": str(dev), "index_s": t1 - t0, "mst_s": t2 - t1, "kernels": E.kernels_used(),
               "mst": stats.counters}
        if a.period is not None:
            rec["period"] = list(a.period)
        with open(a.stats, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

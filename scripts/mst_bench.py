#!/usr/bin/env python3
"""Minimum-spanning-tree time on one GPU, beside what a caller pays today for one linking length
and for the first Boruvka round alone.

    python scripts/mst_bench.py [--data uniform|clustered] [--points N] [--steps 5] [--warmup 2]
                                [--f 0.9] [--core-k K] [--period L]

On one index, device-synchronised host clock, medians over the steps after the warm-up steps,
the cases timed alternately step by step:
  * mst:     mst_edges (with --core-k K: mutual-reachability weights; the core distances are
             computed before the clock starts);
  * cluster: cluster_labels(min_pts = 1) at eps = f x extent x n^(-1/3) (f = 0.9 is near
             percolation for uniform points): one linking length, no merge order;
  * knn2:    knn_neighbors(k = 2), index build included as for any caller: every point's nearest
             other point, which is round one of the tree and nothing more.
Defaults: 1e7 uniform points, 2e7 clustered (100 Gaussian blobs, sigma 0.01). Prints one JSON line
with the times, the rounds, the component counts and the distance evaluations per point and
round. The tree is checked on the spot: n - 1 edges, and mst_labels at eps equal to the labels of
cluster_labels. --period L: the tree, the core distances and the labels under the period L on every
axis (the generated points lie in the unit box: --period 1 wraps every face); the record then
also holds the period and the image walks beyond image 0 per wave and round.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(data: str, n: int, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(1)
    if data == "uniform":
        return torch.rand((n, 3), generator=g, device=dev)
    centers = torch.rand((100, 3), generator=g, device=dev)  # clustered: 100 Gaussian blobs, sigma 0.01
    which = torch.randint(0, 100, (n,), generator=g, device=dev)
    return (centers[which] + 0.01 * torch.randn((n, 3), generator=g, device=dev)).contiguous()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="uniform", choices=["uniform", "clustered"])
    ap.add_argument("--points", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--f", type=float, default=0.9)
    ap.add_argument("--core-k", type=int, default=0)
    ap.add_argument("--period", type=float, default=None, help="periodic box of this period on every axis")
    ap.add_argument("--mst-only", action="store_true", help="time nothing but the tree")
    a = ap.parse_args()
    import torch
    from mpi_cuda_largescaleknn_amd.models import knn_engine as E
    if not torch.cuda.is_available():
        sys.stderr.write("mst_bench: needs a GPU (a CPU timing says nothing about it)\n")
        return 2
    n = int(a.points) or (10_000_000 if a.data == "uniform" else 20_000_000)
    dev = torch.device("cuda", 0)
    p = make(a.data, n, dev)
    extent = float((p.max(0).values - p.min(0).values).max())
    eps = a.f * extent * n ** (-1.0 / 3.0)
    index = E.build_index(p, grid=a.core_k > 0)
    per = {} if a.period is None else {"period": a.period}  # (open box: the calls of the open path, unchanged)
    core = E.mst_core_d2(index, a.core_k, **per) if a.core_k else None
    out = {}
    cases = {"mst": lambda: out.__setitem__("m", E.mst_edges(index, core, **per))}
    if not a.mst_only:
        cases["cluster"] = lambda: out.__setitem__("l", E.cluster_labels(index, eps, 1, **per))
        cases["knn2"] = lambda: out.__setitem__("k", E.knn_neighbors(p, 2))
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
    stats = E.KnnStats()
    rows, d2 = E.mst_edges(index, core, stats=stats, **per)
    c = stats.counters
    ok = rows.shape[0] == n - 1
    if core is None:
        ok = ok and torch.equal(E.mst_labels(rows, d2, n, eps), E.cluster_labels(index, eps, 1, **per)[0])
    rec = {"data": a.data, "points": n, "core_k": a.core_k, "steps": a.steps, "warmup": a.warmup,
           "mst_s": med["mst"], "mst_Mpoints_per_s": n / med["mst"] / 1e6,
           "rounds": c["mst_rounds"], "components": c["mst_components"],
           "evals_per_point_per_round": c["mst_evals"] / n / max(c["mst_rounds"], 1),
           "evals_per_point": c["mst_evals"] / n, "cas_retries_per_point": c["mst_cas_retries"] / n,
           "heaviest_d2": float(d2[-1]) if d2.numel() else None,
           "f": a.f, "eps": eps, "cluster_s": med.get("cluster"), "knn2_s": med.get("knn2"),
           "mst_over_cluster": med["mst"] / med["cluster"] if "cluster" in med else None,
           "mst_over_knn2": med["mst"] / med["knn2"] if "knn2" in med else None,
           "spread": {name: [min(ts), max(ts)] for name, ts in times.items()},
           "checked": bool(ok)}
    if a.period is not None:
        waves = (n + 63) // 64
        rec.update(period=a.period, mst_images=c["mst_images"],
                   images_per_wave_per_round=c["mst_images"] / waves / max(c["mst_rounds"], 1))
    print(json.dumps(rec), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Density clustering throughput on one GPU, beside the fixed-radius passes over the same
points at the same eps.

    python scripts/cluster_bench.py [--data uniform|clustered|duplicates] [--points N]
                                    [--f 0.2,0.9,2.0] [--min-pts 1,5] [--steps 5] [--warmup 2]
                                    [--no-half] [--counts-only] [--package-root DIR]
                                    [--period L | Lx,Ly,Lz]

eps = f x extent x n^(-1/3) (f = 0.9 is near percolation for uniform points, 2.0 one giant
component). For every (f, min_pts), on one index, device-synchronised host clock, medians
over the steps after the warm-up steps, the cases timed alternately step by step:
  * counts:  radius_counts of the points on themselves, the same traversal without unions
             (and the first pass of cluster_labels itself);
  * cluster: cluster_labels;
  * lists:   radius_neighbors(sort=False) of the points on themselves, what a caller pays
             before any union-find of their own, where the pairs fit --max-pairs.
Defaults: 1e7 uniform points; 2e7 for clustered and duplicates (f = 0.5). Prints one JSON line
per configuration with the times, the ratios, clusters / core / noise counts and the walk's
counters (CAS retries per point, clique acceptances). 64 sampled core flags are checked against
radius_count_cpu. --counts-only times nothing but `counts` and imports nothing newer than
radius_counts, so that with --package-root it measures another checkout of the package (the
parent commit) on the same data. --no-half: see knn_engine.CLUSTER_HALF. --period: the data is
wrapped into [0, L) (wrap_points) and every case searches the periodic box; the JSON then also
carries radius_images / groups of the count pass.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(data: str, n: int, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(1)
    if data == "uniform":
        return torch.rand((n, 3), generator=g, device=dev)
    if data == "clustered":  # 100 Gaussian blobs, sigma 0.01
        centers = torch.rand((100, 3), generator=g, device=dev)
        which = torch.randint(0, 100, (n,), generator=g, device=dev)
        return (centers[which] + 0.01 * torch.randn((n, 3), generator=g, device=dev)).contiguous()
    base = torch.rand((1000, 3), generator=g, device=dev)  # duplicates: 1000 sites of exact copies
    return base[torch.randint(0, 1000, (n,), generator=g, device=dev)].contiguous()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="uniform", choices=["uniform", "clustered", "duplicates"])
    ap.add_argument("--points", type=float, default=0.0)
    ap.add_argument("--f", default="")
    ap.add_argument("--min-pts", default="1,5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-pairs", type=int, default=1 << 28)
    ap.add_argument("--no-half", action="store_true")
    ap.add_argument("--counts-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--period", default="", metavar="L | Lx,Ly,Lz")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from mpi_cuda_largescaleknn_amd.models import knn_engine as E
    from mpi_cuda_largescaleknn_amd.ops import kernels as K
    if not torch.cuda.is_available():
        sys.stderr.write("cluster_bench: needs a GPU (a CPU timing says nothing about it)\n")
        return 2
    n = int(a.points) or (10_000_000 if a.data == "uniform" else 20_000_000)
    fs = [float(v) for v in (a.f or ("0.2,0.9,2.0" if a.data == "uniform" else "0.5")).split(",")]
    dev = torch.device("cuda", 0)
    p = make(a.data, n, dev)
    per = {}  # (no --period: the calls without the keyword)
    if a.period:
        vals = [float(v) for v in a.period.split(",")]
        per = {"period": K.check_period("--period", vals * 3 if len(vals) == 1 else vals)}
        p = E.wrap_points(p, per["period"]).contiguous()
    extent = float((p.max(0).values - p.min(0).values).max())
    index = E.build_index(p)
    if a.no_half:
        E.CLUSTER_HALF = False
    ok = True
    for f in fs:
        eps = f * extent * n ** (-1.0 / 3.0)
        counts = E.radius_counts(index, p, eps, **per)
        pairs = int(counts.sum(dtype=torch.int64))
        for min_pts in ([0] if a.counts_only else [int(v) for v in a.min_pts.split(",")]):
            out = {}
            cases = {"counts": lambda: out.__setitem__("c", E.radius_counts(index, p, eps, **per))}
            if not a.counts_only:
                cases["cluster"] = lambda: out.__setitem__("l", E.cluster_labels(index, eps, min_pts, **per))
                if pairs <= a.max_pairs:
                    cases["lists"] = lambda: out.__setitem__("n", E.radius_neighbors(index, p, eps, sort=False,
                                                                                      max_pairs=a.max_pairs, **per))
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
            rec = {"data": a.data, "points": n, "f": f, "eps": eps, "pairs": pairs, "mean_count": pairs / n,
                   "steps": a.steps, "warmup": a.warmup, "counts_s": med["counts"],
                   "spread": {name: [min(ts), max(ts)] for name, ts in times.items()}}
            if not a.counts_only:
                stats = E.KnnStats()
                labels, core = E.cluster_labels(index, eps, min_pts, stats=stats, **per)
                smp = torch.randint(0, n, (64,), generator=torch.Generator().manual_seed(3))
                if per:
                    ref = K.radius_periodic_count_cpu(p.cpu(), p[smp.to(dev)].cpu(), E.cut2_of(eps),
                                                      per["period"]) >= min_pts
                else:
                    ref = K.radius_count_cpu(p.cpu(), p[smp.to(dev)].cpu(), E.cut2_of(eps)) >= min_pts
                exact = int((core[smp.to(dev)].cpu() == ref).sum())
                ok = ok and exact == 64
                dense, nclusters = E.compact_labels(labels)
                c = stats.counters
                rec.update({
                    "min_pts": min_pts, "half": bool(E.CLUSTER_HALF), "cluster_s": med["cluster"],
                    "cluster_over_counts": med["cluster"] / med["counts"],
                    "cluster_Mpoints_per_s": n / med["cluster"] / 1e6,
                    "lists_s": med.get("lists"),
                    "cluster_over_lists": med["cluster"] / med["lists"] if "lists" in med else None,
                    "clusters": nclusters, "core": int(core.sum()), "noise": int((labels < 0).sum()),
                    "largest": int(torch.bincount(dense[dense >= 0].long()).max()) if nclusters else 0,
                    "cas_retries_per_point": c["cluster_cas_retries"] / n, "clique_accepts": c["cluster_clique_accepts"],
                    "cluster_evals_per_point": c["cluster_evals"] / n, "count_evals_per_point": c["radius_evals"] / n,
                    "sampled_core_exact": f"{exact}/64",
                })
                if per:
                    groups = (n + 63) // 64
                    rec.update({"period": list(per["period"]), "radius_images": c["radius_images"], "groups": groups,
                                "images_per_group": c["radius_images"] / groups})
            print(json.dumps(rec), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

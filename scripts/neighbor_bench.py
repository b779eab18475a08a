#!/usr/bin/env python3
"""Neighbour-list throughput on one GPU, beside the k-th-only query of the same shape.

    python scripts/neighbor_bench.py [--shapes 2e7:2e7:16,2e7:4e6:100] [--steps 3] [--warmup 1]

Uniform points and uniform queries from another seed; each shape is points:queries:k. Per
shape (device-synchronised host clock, medians over the steps after the warm-up steps):
  * kth:     query_points — the yardstick: prepare + the foreign-query k-th pass;
  * lists:   query_neighbors into preallocated [nq, k] outputs — the same pass, then the
             collect + tie + sort kernels of knn_neighbors.hip;
  * collect: the collect + sort launch alone, on prepared queries and their k-th d².
Prints one JSON line per shape. Sampled rows are checked against brute force.
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

import torch  # noqa: E402

from mpi_cuda_largescaleknn_amd.apps.radius import add_period_option  # noqa: E402
from mpi_cuda_largescaleknn_amd.models import knn_engine as E  # noqa: E402
from mpi_cuda_largescaleknn_amd.ops import kernels as K  # noqa: E402


def timed(fn, steps: int, warmup: int) -> float:
    ts = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def one(n: int, nq: int, k: int, steps: int, warmup: int, per: dict) -> bool:
    dev = torch.device("cuda", 0)
    p = torch.rand((n, 3), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    q = torch.rand((nq, 3), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    cfg = E.KnnConfig(k=k)
    index = E.build_index(p, grid=True)
    E.bucket_keys(index)
    kth = torch.empty(nq, dtype=torch.float32, device=dev)
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=torch.float32, device=dev)

    t_kth = timed(lambda: E.query_points(index, q, cfg, out=kth, **per), steps, warmup)
    t_lists = timed(lambda: E.query_neighbors(index, q, cfg, out_idx=idx, out_dist=dist, **per), steps, warmup)
    # what was timed, before the open-box collect pass below overwrites it
    smp = torch.randint(0, nq, (128,), generator=torch.Generator().manual_seed(3))
    got_i, got_d = idx[smp.to(dev)].cpu(), dist[smp.to(dev)].cpu()
    same_kth = bool(torch.equal(dist[:, k - 1], kth))
    qsorted, qperm, d2 = E._foreign_kth(index, q, cfg, None, kth, want_d2=True)

    def collect():
        err = K.knn_neighbors_gpu(index.tree(), index.perm, qsorted, nq, d2, k, cfg.cut2, qperm, idx, dist)
        return int(err.item())

    assert collect() == 0
    t_collect = timed(collect, steps, warmup)

    if per:
        ref_i, ref_d2 = K.knn_periodic_cpu(p.cpu(), q[smp.to(dev)].cpu(), k, cfg.cut2, per["period"])
    else:
        ref_i, ref_d2 = K.knn_cpu(p.cpu(), q[smp.to(dev)].cpu(), k, cfg.cut2)
    ref_d = K.finalize_distances(ref_d2.view(-1)).view(-1, k)
    exact = int(((got_i == ref_i) & (got_d == ref_d)).all(dim=1).sum())
    rec = {
        "points": n, "queries": nq, "k": k, "steps": steps, "warmup": warmup,
        "output_GB": nq * k * 8 / 1e9, "kth_s": t_kth, "lists_s": t_lists, "collect_sort_s": t_collect,
        "lists_over_kth": t_lists / t_kth, "lists_Mqueries_per_s": nq / t_lists / 1e6,
        "kth_Mqueries_per_s": nq / t_kth / 1e6, "sampled_exact": f"{exact}/128", "last_column_is_kth": same_kth,
    }
    if per:
        stats = E.KnnStats()
        E.query_points(index, q, cfg, out=kth, stats=stats, **per)
        c = stats.counters
        rec.update(period=list(per["period"]), periodic_flagged=c["periodic_flagged"], periodic_pairs=c["periodic_pairs"],
                   radius_images=c["radius_images"], flagged_share=c["periodic_flagged"] / nq,
                   pairs_per_flagged=c["periodic_pairs"] / max(c["periodic_flagged"], 1))
    print(json.dumps(rec), flush=True)
    return exact == 128 and same_kth


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2e7:2e7:16,2e7:4e6:100", help="points:queries:k, comma separated")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    add_period_option(ap)  # kth_s and lists_s under the period, checked against the periodic oracle
    a = ap.parse_args()
    per = {} if a.period is None else {"period": a.period}  # (none: the calls without the keyword)
    ok = True
    for shape in a.shapes.split(","):
        n, nq, k = shape.split(":")
        ok = one(int(float(n)), int(float(nq)), int(k), a.steps, a.warmup, per) and ok
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

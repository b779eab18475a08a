#!/usr/bin/env python3
"""Cross-set query throughput on one GPU, beside the self-query of the same data.

    python scripts/cross_query_bench.py [--points 2e7] [--queries 2e7] [--k 100] [--steps 5] [--warmup 2]

Uniform points and uniform queries from another seed. Per step (device-synchronised host
clock, medians over the steps after the warm-up steps):
  * prepare: keys of the queries in the index's cube, sort, gather, group location;
  * query:   the k-NN launch over prepared queries — with the grid kernel (the index's gate
             picks it for uniform data) and with knn_rows (the same index without its grid);
  * self:    knn_distances on the same points (index build + query), and the query alone of
             a built index: the yardsticks.
Prints one JSON line. A sample of the cross-query output is checked against brute force.
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=2e7)
    ap.add_argument("--queries", type=float, default=2e7)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    add_period_option(ap)  # the cross query (cross_total_s) under the period, checked against the periodic oracle
    a = ap.parse_args()
    per = {} if a.period is None else {"period": a.period}  # (none: the calls without the keyword)
    n, nq, k = int(a.points), int(a.queries), a.k
    dev = torch.device("cuda", 0)
    p = torch.rand((n, 3), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    q = torch.rand((nq, 3), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    cfg = E.KnnConfig(k=k)

    index = E.build_index(p, grid=True)
    E.reset_kernels_used()
    out = torch.empty(nq, dtype=torch.float32, device=dev)

    def launch(idx, prepared):
        qsorted, qperm, qbucket = prepared
        use_grid = idx.grid is not None
        fw = K.knn_gpu(qsorted, nq, [idx.tree()], k, cfg.cut2, E.radius_hint(idx.box, idx.n, k), None,
                       seed=E.SEED_BUCKETS, impl="grid" if use_grid else "rows",
                       grid=idx.grid.view() if use_grid else None, out_perm=qperm, out_final=out, qbucket=qbucket)
        return fw.value()

    E.bucket_keys(index)
    t_prep = timed(lambda: E.prepare_queries(index, q), a.steps, a.warmup)
    prepared = E.prepare_queries(index, q)
    fails = {}
    t_query = {}
    rows_index = E.LocalIndex(index.n, index.pts, index.perm, index.nodes, index.qnodes, index.depth, index.box,
                              bkeys=index.bkeys)
    for name, idx in (("grid", index), ("rows", rows_index)):
        fails[name] = launch(idx, prepared)
        t_query[name] = timed(lambda idx=idx: launch(idx, prepared), a.steps, a.warmup)
    t_cross = timed(lambda: E.query_points(index, q, cfg, out=out, **per), a.steps, a.warmup)
    used = E.kernels_used()

    # correctness of what was timed: sampled queries against brute force over all points
    stats = E.KnnStats()
    got = E.query_points(index, q, cfg, stats=stats, **per).cpu()
    smp = torch.randint(0, nq, (256,), generator=torch.Generator().manual_seed(3))
    if per:
        ref = K.finalize_distances(K.kth_periodic_cpu(p.cpu(), q[smp.to(dev)].cpu(), k, cfg.cut2, per["period"]))
    else:
        ref = K.finalize_distances(K.kth_cpu(p.cpu(), q[smp.to(dev)].cpu(), k, cfg.cut2, method="brute"))
    exact = int((got[smp] == ref).sum())

    t_self = timed(lambda: E.knn_distances(p, k), a.steps, a.warmup)
    self_out = torch.empty(n, dtype=torch.float32, device=dev)
    hint2 = E.radius_hint(index.box, n, k)
    t_self_query = timed(lambda: E.query(index, cfg, hint2, final_out=self_out), a.steps, a.warmup)

    rec = {
        "points": n, "queries": nq, "k": k, "steps": a.steps, "warmup": a.warmup,
        "prepare_s": t_prep, "query_grid_s": t_query["grid"], "query_rows_s": t_query["rows"],
        "cross_total_s": t_cross, "cross_Mqueries_per_s": nq / t_cross / 1e6,
        "self_total_s": t_self, "self_Mpts_per_s": n / t_self / 1e6, "self_query_only_s": t_self_query,
        "fallback_queries": fails, "kernels_used": used, "sampled_exact": f"{exact}/256",
    }
    if per:
        c = stats.counters
        rec.update(period=list(per["period"]), periodic_flagged=c.get("periodic_flagged", 0),
                   periodic_pairs=c.get("periodic_pairs", 0), radius_images=c.get("radius_images", 0),
                   flagged_share=c.get("periodic_flagged", 0) / nq,
                   pairs_per_flagged=c.get("periodic_pairs", 0) / max(c.get("periodic_flagged", 0), 1))
    print(json.dumps(rec), flush=True)
    return 0 if exact == 256 else 1


if __name__ == "__main__":
    sys.exit(main())

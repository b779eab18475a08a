#!/usr/bin/env python3
"""One radius_profile and one weighted_profile call on the same input (open box, then period 1),
the workload of an LDS counter run that compares the two walk kernels:

    rocprofv3 --pmc SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVES -d OUT -o run \
        --output-format csv -- python scripts/weighted_profile_lds.py [--points 2e6]

OUT/run_counter_collection.csv then holds one row per kernel and counter (radius_profile_walk_kernel,
CountPolicy and WeightPolicy, <false, false> and <true, false>). 16 log-spaced radii from r/8 to
r, r for ~100 neighbours, the points as their own queries; figures in docs/ARCHITECTURE.md.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpi_cuda_largescaleknn_amd.models import knn_engine as E  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=2e6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.stderr.write("weighted_profile_lds: needs a GPU\n")
        return 2
    n = int(a.points)
    dev = torch.device("cuda", 0)
    p = torch.rand((n, 3), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    r = (100 / (n * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)
    radii = [r * 8.0 ** (-(15 - b) / 15) for b in range(16)]
    index = E.build_index(p)
    w = torch.randint(-(1 << 15), (1 << 15) + 1, (n,), dtype=torch.int64, device=dev,
                      generator=torch.Generator(device=dev).manual_seed(5))
    pw = E.prepare_point_weights(index, w)
    for per in (None, 1.0):
        counts = E.radius_profile(index, p, radii, period=per)
        sums = E.weighted_profile(index, p, radii, pw, period=per)
        torch.cuda.synchronize()
        print(f"period {per}: {int(counts[:, -1].sum())} pairs, weight sum {int(sums[:, -1].sum())}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

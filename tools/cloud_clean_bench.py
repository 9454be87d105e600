#!/usr/bin/env python3
"""Times of the outlier removal (itermvs_amd.cloud_filter) on a synthetic fused cloud: a wavy surface with 1 % floaters, at 1 M,
10 M and 30 M points by default.

    python tools/cloud_clean_bench.py [--points 1000000 10000000 30000000] [--k 20] [--repeats 2] [--cpu_points 1000000] [--json FILE]

Per size: the cell edge the default rule picks, seconds of sort and of search (the best of ``--repeats`` runs after one warm-up),
the share of queries that needed the coarse pass, what the statistical mask removes, and the same for the radius mask at a radius of
the default cap / 4.  With scipy importable, ``cKDTree.query`` (k + 1 neighbours, up to 16 threads) is timed on clouds of at most
``--cpu_points`` points; larger ones are reported as not measured."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_cloud(n: int, seed: int = 0, floaters: float = 0.01, device="cuda") -> torch.Tensor:
    """float32 [n,3] on the device: a noisy wavy surface over the unit square and ``floaters`` of the points uniform in its box"""
    g = torch.Generator(device=device).manual_seed(seed)
    u = torch.rand((n, 2), generator=g, device=device)
    z = 0.08 * torch.sin(6.0 * u[:, 0]) * torch.cos(5.0 * u[:, 1]) + 0.0005 * torch.randn((n,), generator=g, device=device)
    pts = torch.cat([u, z[:, None]], 1)
    nf = int(n * floaters)
    pts[:nf] = torch.rand((nf, 3), generator=g, device=device) * torch.tensor([1.2, 1.2, 0.8], device=device) - \
        torch.tensor([0.1, 0.1, 0.4], device=device)
    return pts[torch.randperm(n, generator=g, device=device)].contiguous()


def main(argv=None) -> list:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--points", type=int, nargs="+", default=[1_000_000, 10_000_000, 30_000_000])
    p.add_argument("--k", type=int, default=20)
    p.add_argument("--std_ratio", type=float, default=2.0)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--cpu_points", type=int, default=1_000_000)
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    from itermvs_amd import cloud_filter as CF
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    rows = []
    for n in args.points:
        pts = make_cloud(n)
        cap = CF.default_cap(pts)
        row = {"points": n, "k": args.k, "cap": cap}
        best = None
        for it in range(args.repeats + 1):
            info = {}
            t0 = time.perf_counter()
            keep = CF.statistical_outlier_mask(pts, args.k, args.std_ratio, cap, info=info)
            torch.cuda.synchronize()
            info["seconds_total"] = time.perf_counter() - t0
            if it and (best is None or info["seconds_total"] < best["seconds_total"]):
                best = info
        row["statistical"] = {key: best[key] for key in ("edge", "coarse_edge", "second_pass", "isolated", "removed", "threshold",
                                                         "seconds_sort", "seconds_search", "seconds_total")}
        row["statistical"]["coarse_share"] = best["second_pass"] / n
        best = None
        for it in range(args.repeats + 1):
            info = {}
            t0 = time.perf_counter()
            CF.radius_outlier_mask(pts, cap / 4, 8, info=info)
            torch.cuda.synchronize()
            info["seconds_total"] = time.perf_counter() - t0
            if it and (best is None or info["seconds_total"] < best["seconds_total"]):
                best = info
        row["radius"] = dict(radius=cap / 4, min_neighbours=8, **{key: best[key] for key in ("edge", "removed", "seconds_sort",
                                                                                               "seconds_search", "seconds_total")})
        if cKDTree is None:
            row["ckdtree"] = "not measured: scipy is not importable"
        elif n > args.cpu_points:
            row["ckdtree"] = f"not measured: above --cpu_points {args.cpu_points}"
        else:
            x = pts.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(x)
            t1 = time.perf_counter()
            d, _ = tree.query(x, k=args.k + 1, distance_upper_bound=cap, workers=min(16, os.cpu_count() or 1))
            t2 = time.perf_counter()
            m = d[:, 1:].mean(1)
            row["ckdtree"] = {"seconds_build": t1 - t0, "seconds_query": t2 - t1, "isolated": int(np.isinf(m).sum()),
                              "isolated_gpu": row["statistical"]["isolated"]}
        del pts, keep
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()

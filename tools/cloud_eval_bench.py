#!/usr/bin/env python3
"""Stage times of the DTU evaluator (itermvs_amd.cloud_eval) on synthetic scenes of DTU-like size, against the same protocol
on the CPU with a KD-tree (scipy.spatial.cKDTree, 16 workers).

    python tools/cloud_eval_bench.py --sizes 2000000 10000000 --gt 3000000 --repeats 3 --out profiles/cloud_eval/bench.json
    python tools/cloud_eval_bench.py --sizes 2000000 --cpu            # also time the CPU restatement at these sizes
    python tools/cloud_eval_bench.py --sizes 2000000 --driver         # also the wall time of dtu_eval.py for one scan (files -> JSON)

Scene: a wavy surface of 300 x 300 mm in a bb of DTU's extent; the ground truth is ``--gt`` samples of it, the prediction
``size`` samples of 70 % of it with 0.1 mm noise plus 1 % outliers in the bb.  Every stage is timed between device
synchronisations (the stages of cloud_eval report their own seconds); one warm-up run, then the median over ``--repeats``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BB = np.array([[-30.0, -30.0, 0.0], [330.0, 330.0, 110.0]])
RES = 2.0


def surface(n, gen, part=1.0):
    xy = gen.random((n, 2)) * np.array([300.0 * part, 300.0])
    z = 40.0 + 6.0 * np.sin(xy[:, 0] / 30.0) + 6.0 * np.cos(xy[:, 1] / 40.0)
    return np.concatenate([xy, z[:, None]], 1)


def scene(n_pred, n_gt, seed=0):
    gen = np.random.default_rng(seed)
    gt = surface(n_gt, gen).astype(np.float32)
    n_out = n_pred // 100
    pred = surface(n_pred - n_out, gen, 0.7) + gen.normal(0, 0.1, (n_pred - n_out, 3))
    out = gen.uniform(BB[0], BB[1], (n_out, 3))
    pred = np.concatenate([pred, out]).astype(np.float32)
    pred = pred[gen.permutation(n_pred)]
    size = np.floor((BB[1] - BB[0]) / RES).astype(int) + 1
    mask = np.ones(tuple(size), np.uint8)
    mask[:20] = 0
    return pred, gt, mask, np.array([0.0, 0.0, 1.0, -36.0])


def gpu_run(pred, gt, mask, plane, seed):
    from itermvs_amd import cloud_eval as CE
    dev = "cuda"
    t0 = time.perf_counter()
    p, g, m = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    c = CE.compare_points(p, g, m, BB, RES, plane, seed=seed)
    st = CE.scan_statistics(c["Ddata"], c["Dstl"], c["DataInMask"], c["StlAbovePlane"])
    torch.cuda.synchronize()
    sec = dict(c["seconds"], upload=t1 - t0, total=time.perf_counter() - t0)
    return sec, st, {"n_reduced": c["n_reduced"], "rounds": c["rounds"]}


def cpu_run(pred, gt, mask, plane, seed, workers=16):
    """the same protocol on the CPU: rangesearch + the sequential loop, two capped KD-tree passes, the mask lookup"""
    from scipy.spatial import cKDTree
    sec = {}
    t0 = time.perf_counter()
    p64 = pred.astype(np.float64)
    tree = cKDTree(p64)
    order = torch.randperm(pred.shape[0], generator=torch.Generator().manual_seed(seed)).numpy()
    keep = np.ones(pred.shape[0], bool)
    chunk = 1_000_000                                      # neighbour lists of a chunk of the order at a time (memory)
    for a in range(0, order.size, chunk):
        ids = order[a:a + chunk]
        nbrs = tree.query_ball_point(p64[ids], 0.2, workers=workers)
        for i, nb in zip(ids, nbrs):
            if keep[i]:
                keep[nb] = False
                keep[i] = True
    sec["reduce"] = time.perf_counter() - t0
    t1 = time.perf_counter()
    q = p64[keep]
    g64 = gt.astype(np.float64)
    ddata = cKDTree(g64).query(q, distance_upper_bound=60.0, workers=workers)[0]
    sec["data_to_stl"] = time.perf_counter() - t1
    t2 = time.perf_counter()
    dstl = cKDTree(q).query(g64, distance_upper_bound=60.0, workers=workers)[0]
    sec["stl_to_data"] = time.perf_counter() - t2
    t3 = time.perf_counter()
    v = (q - BB[0]) / RES + 1
    v = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    inside = ((v > 0) & (v <= np.array(mask.shape))).all(1)
    in_mask = np.zeros(q.shape[0], bool)
    in_mask[inside] = mask[v[inside, 0] - 1, v[inside, 1] - 1, v[inside, 2] - 1] != 0
    above = (g64 @ plane[:3] + plane[3]) > 0
    d = ddata[in_mask]
    s = dstl[above]
    st = {"MeanData": float(d[d < 20].mean()), "MeanStl": float(s[s < 20].mean()), "n_reduced": int(keep.sum())}
    sec["mask_plane"] = time.perf_counter() - t3
    sec["total"] = time.perf_counter() - t0
    return sec, st


def driver_run(pred, gt, mask, plane, seed):
    from itermvs_amd import fusion
    with tempfile.TemporaryDirectory() as root:
        data, ply = os.path.join(root, "MVS Data"), os.path.join(root, "outputs")
        os.makedirs(os.path.join(data, "Points", "stl"))
        os.makedirs(os.path.join(data, "ObsMask"))
        os.makedirs(ply)
        fusion.write_ply(os.path.join(data, "Points", "stl", "stl001_total.ply"), gt, np.zeros((gt.shape[0], 3), np.uint8))
        fusion.write_ply(os.path.join(ply, "scan1.ply"), pred, np.zeros((pred.shape[0], 3), np.uint8))
        np.savez(os.path.join(data, "ObsMask", "ObsMask1_10.npz"), ObsMask=mask, BB=BB, Res=RES)
        np.savez(os.path.join(data, "ObsMask", "Plane1.npz"), P=plane)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "dtu_eval.py"), "--data_path", data, "--ply_path", ply, "--scans", "1",
                            "--seed", str(seed), "--out", os.path.join(root, "r.json")], capture_output=True, text=True)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        with open(os.path.join(root, "r.json")) as f:
            return {"wall_seconds": wall, "stage_seconds": json.load(f)["scans"][0]["seconds"], "last_line": r.stdout.strip().splitlines()[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[2_000_000, 10_000_000, 30_000_000])
    ap.add_argument("--gt", type=int, default=3_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu", action="store_true", help="also run the KD-tree restatement on the CPU (16 workers)")
    ap.add_argument("--driver", action="store_true", help="also time dtu_eval.py for one scan, files to JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_eval_bench needs an MI355X: a CPU run cannot give these times")
    rows = []
    for n in a.sizes:
        pred, gt, mask, plane = scene(n, a.gt, a.seed)
        gpu_run(pred, gt, mask, plane, a.seed)                                  # warm-up: code objects, allocator
        runs = [gpu_run(pred, gt, mask, plane, a.seed) for _ in range(a.repeats)]
        row = {"n_pred": n, "n_gt": a.gt, "repeats": a.repeats, "stats": runs[0][1], **runs[0][2],
               "gpu_seconds_median": {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]},
               "gpu_total_all": [r[0]["total"] for r in runs]}
        if a.cpu:
            sec, st = cpu_run(pred, gt, mask, plane, a.seed)
            row["cpu_seconds"], row["cpu_stats"] = sec, st
            row["cpu_over_gpu_total"] = sec["total"] / row["gpu_seconds_median"]["total"]
        if a.driver:
            row["driver"] = driver_run(pred, gt, mask, plane, a.seed)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"argv": sys.argv[1:], "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()

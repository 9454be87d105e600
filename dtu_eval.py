#!/usr/bin/env python3
"""DTU evaluation driver -- counterpart of the reference's ``evaluations/dtu/BaseEvalMain_web.m`` (with the statistics of
``ComputeStat_web.m``) for the MI355X engine: accuracy, completeness and overall of fused point clouds, in mm.

    python dtu_eval.py --data_path "<SampleSet>/MVS Data" --ply_path ./outputs [--scans 1 4 9 | --testlist lists/dtu/test.txt]
                       [--method itermvs --light l3] [--dst 0.2 --max_dist 20 --seed 0] [--out results.json]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 dtu_eval.py ...

``--data_path`` holds ``Points/stl/stl<scan:03d>_total.ply``, ``ObsMask/ObsMask<scan>_10.mat`` and ``ObsMask/Plane<scan>.mat``
(or ``.npz`` files with the same keys: no scipy needed then); ``--ply_path`` holds ``<method><scan:03d>_<light>.ply`` like
BaseEvalMain_web.m:34, or this project's ``scan<N>.ply``.  Scans are sharded over the ranks like eval.py's fusion stage.
The searches run on the GPU (itermvs_amd.cloud_eval); ``--seed`` fixes the visiting order of the 0.2 mm reduction, which
MATLAB draws with an unseeded randperm."""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="DTU accuracy / completeness of fused point clouds (MI355X engine)")
    p.add_argument("--data_path", required=True, help="the dataset's 'MVS Data' folder: Points/stl, ObsMask")
    p.add_argument("--ply_path", required=True, help="folder of the point clouds to score")
    p.add_argument("--scans", nargs="+", type=int, default=None, help="scan numbers (default: the 22 evaluation scans, UsedSets)")
    p.add_argument("--testlist", default=None, help="file with one scan<N> per line (lists/dtu/test.txt of the reference)")
    p.add_argument("--method", default="itermvs")
    p.add_argument("--light", default="l3")
    p.add_argument("--dst", type=float, default=0.2, help="min distance between points when reducing (mm)")
    p.add_argument("--max_dist", type=float, default=20.0, help="outlier threshold (mm)")
    p.add_argument("--seed", type=int, default=0, help="seed of the reduction's visiting order")
    p.add_argument("--out", default=None, help="write per-scan statistics, sizes, seconds and the summary as JSON")
    return p


def scan_numbers(args) -> list:
    from itermvs_amd.cloud_eval import USED_SETS
    if args.scans:
        return [int(s) for s in args.scans]
    if args.testlist:
        with open(args.testlist) as f:
            return [int(re.sub(r"\D", "", line)) for line in f if re.search(r"\d", line)]
    return list(USED_SETS)


def scan_lines(stat: dict) -> list:
    """BaseEvalMain_web.m:71-72"""
    return ["mean/median Data (acc.) %f/%f" % (stat["MeanData"], stat["MedData"]),
            "mean/median Stl (comp.) %f/%f" % (stat["MeanStl"], stat["MedStl"])]


def final_line(summ: dict) -> str:
    """BaseEvalMain_web.m:100"""
    return "final evaluation result on all scans: acc.: %f, comp.: %f, overall: %f" % (summ["acc"], summ["comp"], summ["overall"])


def parse_final_line(line: str) -> dict:
    m = re.search(r"acc\.: (\S+), comp\.: (\S+), overall: (\S+)", line)
    return {"acc": float(m.group(1)), "comp": float(m.group(2)), "overall": float(m.group(3))}


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    import torch
    import torch.distributed as dist
    from itermvs_amd import cloud_eval, shard
    rank, local_rank, world = shard.init_distributed()
    torch.cuda.set_device(local_rank)
    dev = "cuda:%d" % local_rank
    scans = scan_numbers(args)
    mine = []
    for i in shard.shard_indices(len(scans), rank, world):
        t0 = time.time()
        res = cloud_eval.evaluate_scan(args.data_path, args.ply_path, scans[i], args.method, args.light, args.dst, args.max_dist,
                                       args.seed, dev)
        print("scan {}: {} -> {} points, downsample factor: {:.4f}, {} rounds, {:.2f} s".format(
            scans[i], res["n_pred"], res["n_reduced"], res["downsample_factor"], res["rounds"], time.time() - t0))
        for line in scan_lines(res):
            print(line)
        mine.append(res)
    per_scan = mine
    if dist.is_available() and dist.is_initialized():
        parts = [None] * world
        dist.all_gather_object(parts, mine)
        per_scan = [r for part in parts for r in part]
    shard.barrier()
    per_scan = sorted(per_scan, key=lambda r: scans.index(r["scan"]))
    summ = cloud_eval.summary(per_scan)
    result = {"scans": per_scan, "summary": summ, "seed": args.seed, "dst": args.dst, "max_dist": args.max_dist,
              "method": args.method, "light": args.light}
    if rank == 0:
        print(final_line(summ))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()

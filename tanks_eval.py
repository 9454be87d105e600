#!/usr/bin/env python3
"""Tanks and Temples evaluation driver for the MI355X engine: precision, recall and F-score of fused point clouds against the
laser scans of the training scenes (Barn, Caterpillar, Church, Courthouse, Ignatius, Meetingroom, Truck), in the order of the
benchmark's scoring script and without Open3D.

    python tanks_eval.py --scene Barn --gt_dir <dir with Barn.ply, Barn.json, Barn_trans.txt, Barn_COLMAP_SfM.log>
                         --ply_path <cloud or outdir holding Barn.ply>
                         [--traj_path user.log] [--tau X] [--no_refine] [--device cuda:0] [--out results.json]

Without ``--traj_path`` the cloud is taken to be in the frame of the provided COLMAP cameras (``<Scene>_trans.txt`` alone
aligns it).  With it, the user's camera centres are fitted to the reference log's (equal camera counts; the official script's
RANSAC and mapping file are not implemented).  The tau table in itermvs_amd/cloud_register.py was written from memory of the
official toolbox: check it, or pass ``--tau``.  Several ``--scene`` values are scored one after the other and averaged."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Tanks and Temples precision / recall / F-score of fused point clouds (MI355X engine)")
    p.add_argument("--scene", nargs="+", required=True, help="scene name(s), e.g. Barn")
    p.add_argument("--gt_dir", required=True, help="folder with <Scene>.ply, <Scene>.json, <Scene>_trans.txt, <Scene>_COLMAP_SfM.log")
    p.add_argument("--ply_path", required=True, help="the cloud to score, or a folder holding <Scene>.ply")
    p.add_argument("--traj_path", default=None, help="the user's camera trajectory (.log, camera-to-world)")
    p.add_argument("--tau", type=float, default=None, help="distance threshold (default: the scene's)")
    p.add_argument("--no_refine", action="store_true", help="skip the three ICP rounds")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default=None, help="write per-scene results (curves included) and the mean as JSON")
    return p


def scene_line(res: dict) -> str:
    return "{}: precision {:.6f} recall {:.6f} f-score {:.6f} (tau {:g}; {} pred / {} gt points after crop and down-sampling)".format(
        res["scene"], res["precision"], res["recall"], res["fscore"], res["tau"], res["n_pred"], res["n_gt"])


def mean_line(mean: dict) -> str:
    return "mean over {} scenes: precision {:.6f} recall {:.6f} f-score {:.6f}".format(
        mean["scenes"], mean["precision"], mean["recall"], mean["fscore"])


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    import torch
    from itermvs_amd import cloud_register
    torch.cuda.set_device(torch.device(args.device))
    scenes = []
    for scene in args.scene:
        t0 = time.time()
        res = cloud_register.evaluate_scene_files(args.gt_dir, args.ply_path, scene, args.traj_path, args.tau, not args.no_refine,
                                                  args.device)
        res["seconds"] = time.time() - t0
        print(scene_line(res))
        scenes.append(res)
    mean = {"scenes": len(scenes)}
    for k in ("precision", "recall", "fscore"):
        mean[k] = sum(s[k] for s in scenes) / len(scenes)
    if len(scenes) > 1:
        print(mean_line(mean))
    result = {"scenes": scenes, "mean": mean, "refine": not args.no_refine}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()

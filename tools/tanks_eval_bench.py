#!/usr/bin/env python3
"""Stage times of the Tanks and Temples evaluator at a Barn-like size on one GPU: crop, voxel down-sampling, one ICP iteration
(neighbour index + sums + read-back) and the two capped distance passes, on a synthetic closed surface.

    python tools/tanks_eval_bench.py [--pred 10000000] [--gt 8000000] [--tau 0.01] [--repeats 3] [--out profiles/tanks_eval/bench.json]

Prints one JSON line: the median seconds per stage after one warm-up, and the sizes after crop and down-sampling."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def surface(n: int, seed: int, noise: float, device: str):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    d = torch.randn((n, 3), generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    r = 5.0 * (1 + 0.08 * torch.sin(5 * torch.atan2(d[:, 1], d[:, 0])) * torch.cos(4 * torch.acos(d[:, 2].clamp(-1, 1))))
    return (d * r[:, None] + noise * torch.randn((n, 3), generator=gen)).float().to(device)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred", type=int, default=10_000_000)
    ap.add_argument("--gt", type=int, default=8_000_000)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from itermvs_amd import cloud_eval, cloud_register as CR
    dev, tau = args.device, args.tau
    pred, gt = surface(args.pred, 0, 0.3 * tau, dev), surface(args.gt, 1, 0.0, dev)
    poly = np.array([[-6, -6, 0], [6, -6, 0], [6, 6, 0], [0, 5.5, 0], [-6, 6, 0]], dtype=np.float64)
    vol = CR.SelectionVolume(2, -4.0, 4.0, poly)
    stages = {k: [] for k in ("crop", "voxel_tau", "voxel_half_tau", "icp_iteration", "distances")}
    sizes = {}

    def timed(name, fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        stages[name].append(time.perf_counter() - t0)
        return out

    for rep in range(args.repeats + 1):
        keep = timed("crop", lambda: (CR.crop(pred, vol), CR.crop(gt, vol)))
        s, t = pred[keep[0]].contiguous(), gt[keep[1]].contiguous()
        s1, t1 = timed("voxel_tau", lambda: (CR.voxel_down_sample(s, tau), CR.voxel_down_sample(t, tau)))
        s2, t2 = timed("voxel_half_tau", lambda: (CR.voxel_down_sample(s, tau / 2), CR.voxel_down_sample(t, tau / 2)))
        tg = CR.build_target_grid(t1, 10 * tau)
        timed("icp_iteration", lambda: CR.icp(s1, tg, None, 80 * tau, max_iter=0))
        both = torch.cat([s2, t2])
        bb = np.stack([both.min(0).values.double().cpu().numpy() - 5 * tau, both.max(0).values.double().cpu().numpy() + 5 * tau])
        timed("distances", lambda: (cloud_eval.capped_nn_distance(s2, t2, bb, 5 * tau, 2.5 * tau),
                                    cloud_eval.capped_nn_distance(t2, s2, bb, 5 * tau, 2.5 * tau)))
        sizes = {"cropped": [int(s.shape[0]), int(t.shape[0])], "voxel_tau": [int(s1.shape[0]), int(t1.shape[0])],
                 "voxel_half_tau": [int(s2.shape[0]), int(t2.shape[0])]}
    result = {"pred": args.pred, "gt": args.gt, "tau": tau, "repeats": args.repeats, "sizes": sizes,
              "seconds": {k: statistics.median(v[1:]) for k, v in stages.items()}}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()

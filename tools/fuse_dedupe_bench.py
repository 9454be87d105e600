#!/usr/bin/env python3
"""``--fuse_dedupe`` on one MI355X, on the synthetic scan folder ``tools/fusion_bench.py --scan`` builds (49 views, 10 source
views each): vertices and PLY bytes with and without it, files-to-PLY wall time per scan of ``fusion.filter_depth(points=
"device")`` both ways (alternating, ``--repeats`` each after a warm-up of both, wall clock around calls that end in a
synchronise), and the per-view time of ``itermvs_fuse_depth`` against ``itermvs_fuse_depth_claim`` over the scan's reference
views in ``pair.txt`` order (HIP events around the 49 launches, so the claim maps fill up as they do in a scan).  One JSON line.
usage: fuse_dedupe_bench.py [--height 1152 --width 1600 --views 49 --src 10 --repeats 3]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fusion_bench import build_scan_folder, scan_views  # noqa: E402
from itermvs_amd import fusion, ops  # noqa: E402


def kernel_times(views, pairs, photo_thres, repeats):
    """ms per reference view, [plain, claim] alternating -> {name: [ms per view of each repeat]}"""
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                # noqa: E731
    depth = [t(v[2]) for v in views]
    conf = [t(v[3]) for v in views]
    mats = [t(np.stack([fusion.pair_matrices(views[r][0], views[r][1], views[s][0], views[s][1]) for s in srcs]))
            for r, srcs in pairs]
    h, w = views[0][2].shape
    claimed = [torch.zeros((h, w), device=dev, dtype=torch.uint8) for _ in views]

    def scan(claim):
        for c in claimed:
            c.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for (r, srcs), m in zip(pairs, mats):
            if claim:
                ops.fuse_depth_claim(depth[r], conf[r], [depth[s] for s in srcs], m, claimed[r], [claimed[s] for s in srcs],
                                     1.0, 0.01, photo_thres, 3)
            else:
                ops.fuse_depth(depth[r], conf[r], [depth[s] for s in srcs], m, 1.0, 0.01, photo_thres, 3)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(pairs)

    for claim in (False, True):
        scan(claim)
    out = {"fuse_depth": [], "fuse_depth_claim": []}
    for _ in range(repeats):
        out["fuse_depth"].append(scan(False))
        out["fuse_depth_claim"].append(scan(True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--src", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--photo_thres", type=float, default=0.55)
    ap.add_argument("--height", type=int, default=1152)
    ap.add_argument("--width", type=int, default=1600)
    a = ap.parse_args()
    h, w = a.height, a.width
    root = tempfile.mkdtemp(prefix="fuse_dedupe_bench_")
    views = scan_views(a.views, h, w)
    scan, out = build_scan_folder(root, views, a.src, h, w)
    pairs = fusion.read_pair_file(os.path.join(scan, "pair.txt"))

    def once(dedupe):
        info = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fusion.filter_depth(scan, out, os.path.join(root, f"dedupe_{int(dedupe)}.ply"), 1.0, 0.01, a.photo_thres, device="cuda",
                            img_wh=(w, h), points="device", info=info, dedupe=dedupe)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, info

    for dedupe in (False, True):
        once(dedupe)
    runs = {False: [], True: []}
    for _ in range(a.repeats):
        for dedupe in (False, True):
            runs[dedupe].append(once(dedupe))
    result = {"metric": "filter_depth(points='device') end to end, seconds per scan (files on disk -> PLY), without / with dedupe",
              "unit": "s/scan",
              "config": {"workload": f"{a.views} views, {a.src} source views each, {w}x{h}, synthetic plane scene, photo_thres "
                                     f"{a.photo_thres}", "repeats": a.repeats}}
    for dedupe, name in ((False, "plain"), (True, "dedupe")):
        tot = sorted(r[0] for r in runs[dedupe])
        result[name] = {"seconds_per_scan": [r[0] for r in runs[dedupe]], "median": tot[len(tot) // 2], "spread": tot[-1] - tot[0],
                        "vertices": runs[dedupe][0][1]["vertices"],
                        "ply_bytes": os.path.getsize(os.path.join(root, f"dedupe_{int(dedupe)}.ply")),
                        "gpu_wait_median_s": sorted(r[1]["seconds"]["gpu_wait"] for r in runs[dedupe])[len(tot) // 2]}
    result["vertex_ratio"] = result["dedupe"]["vertices"] / max(1, result["plain"]["vertices"])
    result["kernel_ms_per_view"] = kernel_times(views, pairs, a.photo_thres, a.repeats)
    result["value"] = result["dedupe"]["median"]
    print(json.dumps(result))
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()

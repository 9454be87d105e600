#!/usr/bin/env python3
"""eval.py --filter end to end on one MI355X, images on disk -> PLY: today's two passes (save_depth, then fuse_scans with
--fuse_points device) against --fuse_source memory, on the synthetic scan folder tools/fusion_bench.py --scan builds
(``--views`` views with ``--src`` source views each, JPEGs; random weights -- the clouds are not meaningful, the work is).
Modes alternate inside one process, ``--repeats`` times each after one warm-up of every mode; wall clock around calls that
end in a synchronise.  One JSON line.

    fuse_memory_bench.py [--height 1152 --width 1600 --views 49 --src 10 --n_views 5 --repeats 3] [--store_height 1200]
    fuse_memory_bench.py --kernels      itermvs_resize_rgb8 beside itermvs_image_pyramid on the same image (HIP events);
                                        under rocprofv3 --kernel-trace --stats the same launches are the trace's subject
"""
import argparse
import contextlib
import io
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval as E  # noqa: E402
from fusion_bench import build_scan_folder, scan_views  # noqa: E402
from itermvs_amd import ops  # noqa: E402

MODES = {
    "two_pass": ["--fuse_points", "device"],
    "two_pass_cached": ["--fuse_points", "device", "--feature_cache", "{views}"],
    "memory": ["--fuse_source", "memory"],
    "memory_cached": ["--fuse_source", "memory", "--feature_cache", "{views}"],
    "memory_no_pfm": ["--fuse_source", "memory", "--no_pfm"],
    "memory_cached_no_pfm": ["--fuse_source", "memory", "--feature_cache", "{views}", "--no_pfm"],
}


def run_modes(a):
    h, w = a.height, a.width
    sh, sw = a.store_height or h, a.store_width or w
    root = tempfile.mkdtemp(prefix="fuse_memory_bench_")
    views = scan_views(a.views, sh, sw)               # cameras of the stored size; eval.py rescales them to the inference size
    scan, _ = build_scan_folder(root, views, a.src, sh, sw)
    shutil.rmtree(os.path.join(root, "out"))          # the PFMs come from the runs themselves
    for name in os.listdir(os.path.join(scan, "cams_1")):             # a depth range the network can search: the plane lies at ~700
        path = os.path.join(scan, "cams_1", name)
        with open(path) as f:
            text = f.read()
        with open(path, "w") as f:
            f.write(text.replace("\n425 2.5\n", "\n425.0 2.5 192 935.0\n"))
    data = os.path.dirname(scan)

    def once(mode):
        out = os.path.join(root, "out_" + mode)
        shutil.rmtree(out, ignore_errors=True)
        extra = [x.format(views=a.views) for x in MODES[mode]]
        args = E.build_parser().parse_args(["--dataset", "folder", "--testpath", data, "--n_views", str(a.n_views), "--img_wh", str(w),
                                            str(h), "--iteration", str(a.iteration), "--outdir", out, "--filter", "--photo_thres",
                                            str(a.photo_thres), "--feature_dtype", a.feature_dtype] + extra)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            if mode.startswith("memory"):
                E.fuse_memory(args)
                t1 = time.perf_counter()
            else:
                E.save_depth(args)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                E.fuse_scans(args)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        with open(os.path.join(out, "scan.ply"), "rb") as f:
            ply = f.read()
        return {"total": t2 - t0, "first_pass": t1 - t0, "second_pass": t2 - t1}, ply

    modes = [m for m in MODES if m in a.modes.split(",")] if a.modes else list(MODES)
    plys = {m: once(m)[1] for m in modes}             # warm-up: code objects, pinned staging, the allocator's blocks
    runs = {m: [] for m in modes}
    for _ in range(a.repeats):
        for m in modes:
            runs[m].append(once(m)[0])
    out = {"metric": "eval.py --filter end to end, seconds per scan (images on disk -> PLY), model load and graph capture included",
           "unit": "s/scan",
           "config": {"workload": f"{a.views} views, {a.src} source views each in pair.txt, n_views {a.n_views}, {w}x{h} from "
                                  f"{sw}x{sh} JPEGs, iteration {a.iteration}, feature storage {a.feature_dtype}, random weights",
                      "repeats": a.repeats},
           "vertices": int(plys[modes[0]].split(b"element vertex ", 1)[1].split(b"\n", 1)[0]),
           "ply_identical_across_modes": all(p == plys[modes[0]] for p in plys.values())}
    for m, rs in runs.items():
        tot = sorted(r["total"] for r in rs)
        out[m] = {"seconds_per_scan": [r["total"] for r in rs], "median": tot[len(tot) // 2], "spread": tot[-1] - tot[0],
                  "first_pass_median": sorted(r["first_pass"] for r in rs)[len(rs) // 2],
                  "second_pass_median": sorted(r["second_pass"] for r in rs)[len(rs) // 2]}
    out["value"] = out[modes[-1]]["median"]
    print(json.dumps(out))
    shutil.rmtree(root, ignore_errors=True)


def run_kernels(a):
    h, w = a.height, a.width
    sh, sw = a.store_height or h, a.store_width or w
    raw = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1, sh, sw, 3), dtype=np.uint8)).to("cuda")
    subjects = {"itermvs_resize_rgb8": lambda: ops.resize_rgb8(raw, h, w),
                "itermvs_image_pyramid (level 0 only)": lambda: ops.image_pyramid(raw, h, w, all_levels=False)}
    ms = {}
    for name, fn in subjects.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms[name] = e0.elapsed_time(e1) / a.steps
    print(json.dumps({"metric": "back-to-back launches on one image, HIP events (allocation of the output included)", "unit": "ms",
                      "config": {"image": f"{sw}x{sh} -> {w}x{h}", "steps": a.steps}, "ms_per_image": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--height", type=int, default=1152)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--store_height", type=int, default=0, help="rows of the JPEGs on disk (default: --height)")
    ap.add_argument("--store_width", type=int, default=0)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--src", type=int, default=10)
    ap.add_argument("--n_views", type=int, default=5)
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--feature_dtype", default="fp32")
    ap.add_argument("--photo_thres", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--modes", default="", help="comma separated subset of " + ",".join(MODES))
    a = ap.parse_args()
    return run_kernels(a) if a.kernels else run_modes(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""colmap_input.py --undistort on one MI355X.  One JSON line per mode.

    undistort_bench.py --kernels [--steps 2000]
        itermvs_undistort_rgb8 at 1600x1200 and 4000x3000, SIMPLE_RADIAL and OPENCV_FISHEYE, output camera by the rule of
        undistort.undistorted_camera: back-to-back launches into one preallocated output between HIP events (the C entry point,
        no allocation in the window).  Bytes = the source read once + the destination written; the roof is the HBM bandwidth a
        copy kernel reaches (MEASURED_HBM_TBS).  Under ``rocprofv3 --kernel-trace --stats`` the same launches are the trace's
        subject; ``--read_trace DIR --steps N`` then prints each case's kernel time from the trace.
    undistort_bench.py --convert [--views 49 --width 1600 --height 1200 --num_workers 4 --repeats 3]
        colmap.convert(..., undistort=True) on a synthetic scan of ``--views`` JPEGs of one SIMPLE_RADIAL camera: wall clock
        and its stages.  decode and encode are summed over the pool's threads, so they may exceed the wall time.
"""
import argparse
import ctypes as C
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
from itermvs_amd import _lib, colmap, undistort  # noqa: E402

MEASURED_HBM_TBS = 6.3      # what a float4 copy reaches on the MI355X (spec: 8.0)
KERNEL_CASES = {"SIMPLE_RADIAL": lambda f, w, h: [f, w / 2, h / 2, -0.08],
                "OPENCV_FISHEYE": lambda f, w, h: [f, f, w / 2, h / 2, 0.05, -0.01, 0.002, 0.0]}


def photo(h, w, seed=0):
    """a smooth pattern with fine noise: compresses like a photograph, unlike white noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(x / 97 + seed) * np.cos(y / 61), 127 + 90 * np.sin((x + y) / 143), 127 + 90 * np.cos(x / 211 - y / 47)], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def run_kernels(a):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for w, h in ((1600, 1200), (4000, 3000)):
        raw = torch.from_numpy(photo(h, w)).to("cuda")
        for model, make in KERNEL_CASES.items():
            cam = colmap.Camera(1, model, w, h, np.array(make(0.8 * w, w, h)))
            out = undistort.undistorted_camera(cam)
            for path in ("1 pixel per lane", "4 pixels per lane"):
                run_case(a, lib, stream, raw, cam, out, out.width if path[0] == "1" else out.width // 4 * 4, path, rows)
    print(json.dumps({"metric": "itermvs_undistort_rgb8, back-to-back launches between HIP events (launch gaps included)",
                      "unit": "us", "config": {"steps": a.steps, "roof_TB_per_s": MEASURED_HBM_TBS}, "cases": rows}))


def run_case(a, lib, stream, raw, cam, out, width, path, rows):
    """``width``: the rule's width (odd in the cases above: byte stores) or the multiple of 4 below it (dword stores)"""
    h, w, model = cam.height, cam.width, cam.model
    assert (width % 4 == 0) == (path[0] == "4")
    dst = torch.empty((out.height, width, 3), dtype=torch.uint8, device="cuda")
    params = (C.c_double * len(cam.params))(*cam.params)
    fx, fy, cx, cy = (float(x) for x in out.params)

    def launch():
        status = lib.itermvs_undistort_rgb8(raw.data_ptr(), h, w, colmap.CAMERA_MODEL_NAMES[model][0], params, len(cam.params),
                                            fx, fy, cx, cy, out.height, width, dst.data_ptr(), None, stream)
        assert status == 0, status

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.steps
    moved = h * w * 3 + out.height * width * 3
    rows.append({"source": f"{w}x{h}", "model": model, "output": f"{width}x{out.height}", "path": path,
                 "filled_share": float((dst != 0).any(-1).float().mean()), "us_per_launch": us, "bytes": moved,
                 "GB_per_s": moved / us * 1e-3, "share_of_measured_hbm_roof": moved / us * 1e-6 / MEASURED_HBM_TBS})


def read_trace(a):
    """kernel durations from the kernel trace of a ``rocprofv3 --kernel-trace`` run of ``--kernels --steps N``: the dispatches of
    the kernel in time order are the cases of run_kernels in its order, 10 warm-up launches and N timed ones each"""
    import csv
    import glob
    import sqlite3
    found = lambda pattern: glob.glob(os.path.join(a.read_trace, "**", pattern), recursive=True)      # noqa: E731
    if found("*kernel_trace.csv"):                                       # --output-format csv
        with open(found("*kernel_trace.csv")[0], newline="") as f:
            rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    else:                                                                # rocprofv3's default: a rocpd database
        rows = list(sqlite3.connect(found("*_results.db")[0]).execute("select name, start, end from kernels"))
    rows = sorted((r for r in rows if "undistort_rgb8_kernel" in r[0]), key=lambda r: r[1])
    group = 10 + a.steps
    assert len(rows) == 8 * group, (len(rows), group)
    cases = [(f"{w}x{h}", model, path) for w, h in ((1600, 1200), (4000, 3000)) for model in KERNEL_CASES
             for path in ("1 pixel per lane", "4 pixels per lane")]
    out = []
    for i, (size, model, path) in enumerate(cases):
        part = rows[i * group + 10:(i + 1) * group]
        ns = sorted(end - start for _, start, end in part)
        px4 = "ILi4E" in part[0][0] or "<4>" in part[0][0]
        assert px4 == (path[0] == "4"), part[0][0]
        out.append({"source": size, "model": model, "path": path, "kernel_us_median": ns[len(ns) // 2] / 1e3, "kernel_us_min": ns[0] / 1e3,
                    "kernel_us_max": ns[-1] / 1e3})
    print(json.dumps({"metric": "itermvs_undistort_rgb8 kernel time, rocprofv3 --kernel-trace", "unit": "us", "cases": out}))


def run_convert(a):
    from colmap_bench import make_model
    from PIL import Image as PILImage
    w, h = a.width, a.height
    root = tempfile.mkdtemp(prefix="undistort_bench_")
    model = make_model(a.views, 1000)
    model.cameras = {1: colmap.Camera(1, "SIMPLE_RADIAL", w, h, np.array([0.8 * w, w / 2, h / 2, -0.08]))}
    os.makedirs(os.path.join(root, "images"))
    colmap.write_model(os.path.join(root, "sparse"), model, ".bin")
    for i, im in enumerate(model.images):
        PILImage.fromarray(photo(h, w, seed=i % 7)).save(os.path.join(root, "images", im.name), format="JPEG", quality=95)
    runs = {"copy": [], "undistort": []}
    for rep in range(a.repeats + 1):                                   # the first round is the warm-up
        for mode in runs:
            out = os.path.join(root, "out_" + mode)
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            colmap.convert(root, out, info=info, undistort=mode == "undistort", num_workers=a.num_workers)
            info["wall_s"] = time.perf_counter() - t0
            if rep:
                runs[mode].append(info)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]          # noqa: E731
    keys = ["wall_s", "undistort_s", "undistort_decode_s", "undistort_device_s", "undistort_encode_s"]
    result = {"metric": "colmap.convert end to end on a synthetic scan, wall clock; decode / encode summed over the pool's threads",
              "unit": "s", "config": {"views": a.views, "image": f"{w}x{h}", "num_workers": a.num_workers, "repeats": a.repeats},
              "copy_wall_s": [r["wall_s"] for r in runs["copy"]], "undistort_wall_s": [r["wall_s"] for r in runs["undistort"]],
              "undistort_median": {k: med(runs["undistort"], k) for k in keys}}
    print(json.dumps(result))
    shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--convert", action="store_true")
    ap.add_argument("--read_trace", type=str, default="", help="directory a rocprofv3 --kernel-trace run of --kernels wrote")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.read_trace:
        return read_trace(a)
    assert torch.cuda.is_available(), "undistort_bench.py needs an MI355X"
    if a.kernels:
        run_kernels(a)
    if a.convert:
        run_convert(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""itermvs_fuse_depth (eval.py:154-269) on one MI355X: reference views per second at the DTU
evaluation size, HBM roofline of the kernel, and the numpy restatement (oracle/fusion_oracle.py) on the host beside it.
One JSON line.  usage: fusion_bench.py [--height 1152 --width 1600 --src 10 --steps 50]

``--scan``: the whole filter stage of one scan instead -- a synthetic scan folder (``--views`` views, ``--src`` source views each,
PFMs, cameras and JPEGs in a temporary folder), then ``fusion.filter_depth`` end to end with ``points="host"`` and
``points="device"`` alternating, ``--repeats`` times each after one warm-up of both; wall clock around calls that end in a
synchronise.  Per mode: seconds per scan (each repeat, median, spread) and where the time goes.  ``--trace-views N``: no
timing, N reference views through fuse_depth + fuse_points for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...).
``--dynamic``: per-view kernel time of ``itermvs_fuse_depth_dynamic`` (default steps and levels, no claim maps) against
``itermvs_fuse_depth`` on the same inputs, ``--repeats`` blocks of ``--steps`` launches each, the two kernels alternating;
per CALL (Python, the outputs' allocation and the launch included: enqueue-bound at small sizes) every block's mean, their median
and spread, and the ratio of the medians.  ``--dynamic --trace-views N``: N untimed launches of each after the warm-up, for the
kernels' own durations from ``rocprofv3 --kernel-trace --stats -- python ...`` (profiles/fuse_dynamic/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from itermvs_amd import fusion, ops  # noqa: E402


def build_scan_folder(root, views, n_src, h, w):
    """pair.txt (the n_src nearest views by index), cams_1/, images/*.jpg, depth_est/ + confidence/ PFMs of the plane scene"""
    from PIL import Image
    from itermvs_amd.data_io import save_pfm
    scan, out = os.path.join(root, "scan"), os.path.join(root, "out")
    for d in (os.path.join(scan, "cams_1"), os.path.join(scan, "images"), os.path.join(out, "depth_est"), os.path.join(out, "confidence")):
        os.makedirs(d)
    rng = np.random.default_rng(0)
    lines = [str(len(views))]
    rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)      # noqa: E731
    for v, (k, e, d, conf) in enumerate(views):
        with open(os.path.join(scan, "cams_1", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write(f"extrinsic\n{rows(e)}\n\nintrinsic\n{rows(k)}\n\n425 2.5\n")
        small = rng.integers(0, 256, (h // 8, w // 8, 3), dtype=np.uint8)          # texture with some detail: a realistic JPEG to decode
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(os.path.join(scan, "images", "{:0>8}.jpg".format(v)), quality=92)
        save_pfm(os.path.join(out, "depth_est", "{:0>8}.pfm".format(v)), d)
        save_pfm(os.path.join(out, "confidence", "{:0>8}.pfm".format(v)), conf)
        near = sorted((u for u in range(len(views)) if u != v), key=lambda u: (abs(u - v), u))[:n_src]
        lines += [str(v), f"{len(near)} " + " ".join(f"{u} 1.0" for u in near)]
    with open(os.path.join(scan, "pair.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return scan, out


def scan_views(n_views, h, w):
    """the tilted plane of tests/test_fusion.py:_scene seen from ``n_views`` cameras one degree apart (10 neighbours stay consistent);
    confidence uniform in 0..1 with photo_thres 0.55 keeps about 45 % of the pixels"""
    rng = np.random.default_rng(0)
    k = np.array([[1.2 * w, 0, w / 2 + 1.3], [0, 1.2 * w, h / 2 - 0.7], [0, 0, 1]], np.float32)
    out = []
    for v in range(n_views):
        conf = rng.uniform(0, 1, (h, w)).astype(np.float32)
        ang = np.deg2rad(1.0 * (v - n_views // 2))
        r = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        c = np.array([120.0 * np.sin(ang), 0.5 * v, 0.0])
        e = np.eye(4)
        e[:3, :3], e[:3, 3] = r, -r @ c
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        rays = np.linalg.inv(k.astype(np.float64)) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
        t = (700.0 - np.array([0.1, -0.05, 1.0]) @ c) / (np.array([0.1, -0.05, 1.0]) @ (r.T @ rays))
        out.append((k.copy(), e.astype(np.float32), t.reshape(h, w).astype(np.float32), conf))
    return out


class Stopwatch:
    """seconds spent inside wrapped functions of itermvs_amd.fusion, by name"""

    def __init__(self):
        self.seconds = {}

    def wrap(self, name, fn, sync=False):
        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                r = fn(*a, **kw)
                if sync:
                    torch.cuda.synchronize()
                return r
            finally:
                self.seconds[name] = self.seconds.get(name, 0.0) + time.perf_counter() - t0
        return timed


def run_scan(a):
    import tempfile
    h, w = a.height, a.width
    root = tempfile.mkdtemp(prefix="fusion_bench_")
    t0 = time.perf_counter()
    scan, out = build_scan_folder(root, scan_views(a.views, h, w), a.src, h, w)
    built = time.perf_counter() - t0
    plain = {n: getattr(fusion, n) for n in ("read_scan_image", "read_pfm", "write_ply", "fuse_reference_view")}

    def once(mode):
        sw = Stopwatch()
        fusion.read_scan_image = sw.wrap("image_decode", plain["read_scan_image"])
        fusion.read_pfm = sw.wrap("pfm_read", plain["read_pfm"])
        if mode == "host":                         # its upload + kernel end in a synchronise anyway (the mask means follow)
            fusion.write_ply = sw.wrap("file_write", plain["write_ply"])
            fusion.fuse_reference_view = sw.wrap("upload_and_gpu_kernels", plain["fuse_reference_view"], sync=True)
        info = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = fusion.filter_depth(scan, out, os.path.join(root, mode + ".ply"), 1.0, 0.01, a.photo_thres, device="cuda",
                                    img_wh=(w, h), points=mode, info=info)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        for n, f in plain.items():
            setattr(fusion, n, f)
        split = dict(sw.seconds)
        if mode == "device":
            # "upload" holds the depth-map uploads of filter_depth as well: they are part of pfm_read's callers, not of fuse_scan
            split.update({k: v for k, v in info["seconds"].items()})
        else:
            split["host_numpy_download_unproject_colour"] = total - sum(split.values())
        split["unaccounted"] = total - sum(split.values())
        return total, split, stats, info

    for mode in ("host", "device"):                # warm-up: code objects, pinned staging, the allocator's blocks
        once(mode)
    runs = {"host": [], "device": []}
    for _ in range(a.repeats):
        for mode in ("host", "device"):
            runs[mode].append(once(mode))
    ply = {m: open(os.path.join(root, m + ".ply"), "rb").read() for m in runs}
    head_h, body_h = ply["host"].split(b"end_header\n", 1)
    head_d, body_d = ply["device"].split(b"end_header\n", 1)
    rec = np.dtype([("xyz", "<u4", (3,)), ("rgb", "u1", (3,))])
    ph, pd = np.frombuffer(body_h, rec), np.frombuffer(body_d, rec)
    same_layout = head_h == head_d and len(ph) == len(pd)
    out_json = {"metric": "filter_depth end to end, seconds per scan (files on disk -> PLY)", "unit": "s/scan",
                "config": {"workload": f"{a.views} views, {a.src} source views each, {w}x{h}, synthetic plane scene, photo_thres {a.photo_thres}",
                           "repeats": a.repeats, "scan_folder_build_s": built},
                "vertices": int(len(pd)), "kept_share": len(pd) / float(a.views * h * w), "ply_bytes": len(ply["device"]),
                "device_vs_host": {"same_header_and_count": bool(same_layout),
                                   "colours_equal": bool(same_layout and np.array_equal(ph["rgb"], pd["rgb"])),
                                   "coordinate_words_differing": int((ph["xyz"] != pd["xyz"]).sum()) if same_layout else None}}
    for mode, rs in runs.items():
        tot = sorted(r[0] for r in rs)
        keys = sorted({k for r in rs for k in r[1]})
        out_json[mode] = {"seconds_per_scan": [r[0] for r in rs], "median": tot[len(tot) // 2], "spread": tot[-1] - tot[0],
                          "split_median_s": {k: sorted(r[1].get(k, 0.0) for r in rs)[len(rs) // 2] for k in keys}}
    out_json["device"]["groups"] = len(runs["device"][0][3]["groups"])
    out_json["device"]["synchronisations"] = runs["device"][0][3]["synchronisations"]
    out_json["value"] = out_json["device"]["median"]
    print(json.dumps(out_json))
    import shutil
    shutil.rmtree(root, ignore_errors=True)


def run_trace(a):
    """N reference views through fuse_depth + fuse_points, nothing timed: the subject of a kernel trace"""
    from test_fusion import _scene
    h, w = a.height, a.width
    views = _scene(h, w, a.src + 1, 0, 0.002)
    dev = torch.device("cuda")
    k, e, d, conf = views[0]
    mats = torch.from_numpy(np.stack([fusion.pair_matrices(k, e, v[0], v[1]) for v in views[1:]])).to(dev)
    dref, cref = torch.from_numpy(d).to(dev), torch.from_numpy(conf).to(dev)
    srcs = [torch.from_numpy(v[2]).to(dev) for v in views[1:]]
    cam = torch.from_numpy(np.concatenate([np.linalg.inv(k).reshape(-1), np.linalg.inv(e)[:3].reshape(-1)])).to(dev)
    rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8).to(dev)
    records = torch.empty(a.trace_views * h * w * ops.POINT_RECORD_BYTES, device=dev, dtype=torch.uint8)
    cursor = torch.zeros(1, device=dev, dtype=torch.int64)
    counts = torch.zeros((a.trace_views, 4), device=dev, dtype=torch.int64)
    for i in range(a.trace_views):
        avg, photo, geo, final, _ = ops.fuse_depth(dref, cref, srcs, mats, 1.0, 0.01, a.photo_thres, 3)
        ops.fuse_points(avg, final, cam, rgb, records, cursor, counts, i, photo, geo)
    torch.cuda.synchronize()
    print(json.dumps({"trace_views": a.trace_views, "vertices_per_view": int(counts[0, 2]), "pixels_per_view": h * w,
                      "algorithmic_bytes_per_view_new_kernels": int(2 * 9 * h * w + 15 * int(counts[0, 2]))}))


def run_dynamic(a):
    """the dynamic leg: both kernels on one set of inputs (the noisy plane scene, so that the levels differ between pixels)"""
    from test_fusion import _scene
    views = _scene(a.height, a.width, a.src + 1, 0, 0.002)
    dev = torch.device("cuda")
    k, e, d, conf = views[0]
    mats = torch.from_numpy(np.stack([fusion.pair_matrices(k, e, v[0], v[1]) for v in views[1:]])).to(dev)
    dref, cref = torch.from_numpy(d).to(dev), torch.from_numpy(conf).to(dev)
    srcs = [torch.from_numpy(v[2]).to(dev) for v in views[1:]]
    runs = {"fuse_depth": lambda: ops.fuse_depth(dref, cref, srcs, mats), "fuse_depth_dynamic": lambda: ops.fuse_depth_dynamic(dref, cref, srcs, mats)}
    for run in runs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    level = runs["fuse_depth_dynamic"]()[5]
    if a.trace_views:                            # nothing timed here: the kernels' own durations come from the trace around it
        for run in runs.values():
            for _ in range(a.trace_views):
                run()
        torch.cuda.synchronize()
        print(json.dumps({"trace_views": a.trace_views, "config": {"width": a.width, "height": a.height, "src": a.src}}))
        return
    ms = {name: [] for name in runs}
    for _ in range(a.repeats):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    print(json.dumps({"metric": "ms per call of ops.fuse_depth / ops.fuse_depth_dynamic, back to back (Python, allocation of the outputs and launch included)",
                      "config": {"width": a.width, "height": a.height, "src": a.src, "steps": a.steps, "repeats": a.repeats},
                      "ms_per_call": ms, "median_ms": med, "spread_ms": {n: max(v) - min(v) for n, v in ms.items()},
                      "dynamic_over_static": med["fuse_depth_dynamic"] / med["fuse_depth"],
                      "level_histogram": torch.bincount(level.reshape(-1).long(), minlength=11).tolist()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", action="store_true", help="time filter_depth end to end, points='host' against points='device'")
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--photo_thres", type=float, default=0.55)
    ap.add_argument("--trace-views", type=int, default=0)
    ap.add_argument("--height", type=int, default=1152)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--src", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dynamic", action="store_true", help="time itermvs_fuse_depth_dynamic against itermvs_fuse_depth")
    a = ap.parse_args()
    if a.scan:
        return run_scan(a)
    if a.dynamic:
        return run_dynamic(a)
    if a.trace_views:
        return run_trace(a)
    from test_fusion import _scene
    views = _scene(a.height, a.width, a.src + 1, 0, 0.002)
    dev = torch.device("cuda")
    k, e, d, conf = views[0]
    mats = torch.from_numpy(np.stack([fusion.pair_matrices(k, e, v[0], v[1]) for v in views[1:]])).to(dev)
    dref, cref = torch.from_numpy(d).to(dev), torch.from_numpy(conf).to(dev)
    srcs = [torch.from_numpy(v[2]).to(dev) for v in views[1:]]
    run = lambda: ops.fuse_depth(dref, cref, srcs, mats)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    px = a.height * a.width
    alg = px * ((2 + a.src) * 4 + 8 + 3 + 4)          # maps read once; float64 average, three masks and the count written
    out = {"metric": "reference views fused per second (geometric + photometric filter, eval.py:154-269)",
           "value": 1e3 / ms, "unit": "ref-views/s", "ms_per_view": ms, "dtype": "f64 geometry, f32 maps",
           "config": {"workload": f"{a.src} source views, {a.width}x{a.height} depth maps, synthetic plane scene"},
           "roofline": {"bound": "hbm", "achieved": alg / (ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": alg / (ms * 1e-3) / 1e9 / 8000.0, "algorithmic_bytes_per_launch": alg, "traffic": None}}
    if not a.no_cpu_baseline:
        from oracle import fusion_oracle as FO
        n_src = min(a.src, 2)                        # bounded sample: two source views, scaled to all of them
        t0 = time.perf_counter()
        FO.fuse_reference_view(d, conf, k, e, [v[2] for v in views[1:1 + n_src]], [v[0] for v in views[1:1 + n_src]],
                               [v[1] for v in views[1:1 + n_src]])
        dt = (time.perf_counter() - t0) * a.src / n_src
        out["cpu_baseline"] = {"value": 1.0 / dt, "unit": "ref-views/s", "cores": 1, "kind": "port",
                               "sample": f"numpy restatement on {n_src} of the {a.src} source views, scaled linearly"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

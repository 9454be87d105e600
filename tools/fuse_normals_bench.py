#!/usr/bin/env python3
"""``--ply_normals`` on one MI355X, on the synthetic scan of ``tools/fusion_bench.py`` (49 views, 10 source views each) held in
memory: seconds per scan of ``fusion.fuse_scan`` without and with ``normals`` (alternating, ``--repeats`` each after a warm-up of
both; wall clock around calls that end in a synchronise; the PLY goes to a temporary folder), PLY bytes and flush groups both
ways, and the per-view time of the three launches of ``itermvs_fuse_points`` against ``itermvs_fuse_points_normals`` on the
scan's first reference view (HIP events around ``--steps`` calls; count and scan are the same kernels, so the difference is the
emit kernels').  One JSON line.
``--trace-views N``: no timing, N calls of each entry point for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...),
which gives the two emit kernels' own times.
usage: fuse_normals_bench.py [--height 1152 --width 1600 --views 49 --src 10 --repeats 3 --steps 200]"""
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
from fusion_bench import scan_views  # noqa: E402
from itermvs_amd import fusion, ops  # noqa: E402


def one_view(views, n_src, photo_thres):
    """view 0 fused against its n_src neighbours -> what one emit call needs, on the device"""
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                # noqa: E731
    k, e, d, conf = views[0]
    h, w = d.shape
    mats = t(np.stack([fusion.pair_matrices(k, e, v[0], v[1]) for v in views[1:1 + n_src]]))
    avg, photo, geo, final, _ = ops.fuse_depth(t(d), t(conf), [t(v[2]) for v in views[1:1 + n_src]], mats, 1.0, 0.01, photo_thres, 3)
    cam = t(np.concatenate([np.linalg.inv(k).reshape(-1), np.linalg.inv(e)[:3].reshape(-1)]).astype(np.float32))
    rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8).to(dev)
    records = torch.empty(h * w * ops.POINT_NORMAL_RECORD_BYTES, device=dev, dtype=torch.uint8)
    cursor = torch.zeros(1, device=dev, dtype=torch.int64)
    counts = torch.zeros((1, 4), device=dev, dtype=torch.int64)
    workspace = torch.empty(ops.fuse_points_workspace_bytes(h, w), device=dev, dtype=torch.uint8)

    def call(normals):
        cursor.zero_()                                                             # every call writes the same records
        emit = ops.fuse_points_normals if normals else ops.fuse_points
        emit(avg, final, cam, rgb, records, cursor, counts, 0, photo, geo, workspace=workspace)

    return call, counts


def emit_times(call, steps, repeats):
    """ms per view of the three launches (and the cursor reset), [plain, normals] alternating"""
    def timed(normals):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            call(normals)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    for normals in (False, True):
        timed(normals)
    out = {"fuse_points": [], "fuse_points_normals": []}
    for _ in range(repeats):
        out["fuse_points"].append(timed(False))
        out["fuse_points_normals"].append(timed(True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--src", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--photo_thres", type=float, default=0.55)
    ap.add_argument("--height", type=int, default=1152)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--trace-views", type=int, default=0)
    a = ap.parse_args()
    h, w = a.height, a.width
    if not torch.cuda.is_available():
        raise SystemExit("fuse_normals_bench.py measures on an MI355X; no GPU here")
    if a.trace_views:
        call, counts = one_view(scan_views(a.src + 1, h, w), a.src, a.photo_thres)
        for _ in range(a.trace_views):
            call(False)
            call(True)
        torch.cuda.synchronize()
        print(json.dumps({"trace_views": a.trace_views, "vertices_per_view": int(counts[0, 2]), "pixels_per_view": h * w}))
        return
    views = scan_views(a.views, h, w)
    n = len(views)
    pairs = [(v, sorted((u for u in range(n) if u != v), key=lambda u: (abs(u - v), u))[:a.src]) for v in range(n)]
    dev = torch.device("cuda")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                # noqa: E731
    cams = {v: (views[v][0], views[v][1]) for v in range(n)}
    depths = {v: t(views[v][2]) for v in range(n)}                                 # as scan_fuse hands them over: on the device
    confs = {v: t(views[v][3]) for v in range(n)}
    rgb = {v: torch.randint(0, 256, (h, w, 3), dtype=torch.uint8).to(dev) for v in range(n)}
    root = tempfile.mkdtemp(prefix="fuse_normals_bench_")

    def once(normals):
        info = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fusion.fuse_scan(pairs, cams, depths, confs, rgb, os.path.join(root, f"normals_{int(normals)}.ply"), 1.0, 0.01,
                         a.photo_thres, device="cuda", info=info, normals=normals)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, info

    for normals in (False, True):
        once(normals)
    runs = {False: [], True: []}
    for _ in range(a.repeats):
        for normals in (False, True):
            runs[normals].append(once(normals))
    result = {"metric": "fuse_scan (maps in GPU memory -> PLY), seconds per scan, without / with normals", "unit": "s/scan",
              "config": {"workload": f"{a.views} views, {a.src} source views each, {w}x{h}, synthetic plane scene, photo_thres "
                                     f"{a.photo_thres}", "repeats": a.repeats, "steps": a.steps}}
    for normals, name in ((False, "plain"), (True, "normals")):
        tot = sorted(r[0] for r in runs[normals])
        infos = [r[1] for r in runs[normals]]
        mid = lambda key: sorted(i["seconds"][key] for i in infos)[len(infos) // 2]      # noqa: E731
        result[name] = {"seconds_per_scan": [r[0] for r in runs[normals]], "median": tot[len(tot) // 2], "spread": tot[-1] - tot[0],
                        "vertices": infos[0]["vertices"], "groups": len(infos[0]["groups"]),
                        "ply_bytes": os.path.getsize(os.path.join(root, f"normals_{int(normals)}.ply")),
                        "split_median_s": {key: mid(key) for key in sorted(infos[0]["seconds"])}}
    shutil.rmtree(root, ignore_errors=True)
    del depths, confs, rgb
    call, _ = one_view(views, a.src, a.photo_thres)
    result["three_launches_ms_per_view"] = emit_times(call, a.steps, a.repeats)
    result["value"] = result["normals"]["median"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()

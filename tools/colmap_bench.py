#!/usr/bin/env python3
"""The COLMAP converter (itermvs_amd/colmap.py) on one MI355X at three model sizes, (images V, observations per image n) =
(40, 1000), (300, 5000), (1000, 5000): the two kernels by HIP events, ``colmap.convert`` end to end by wall clock with its
stages, and the numpy restatement of the same arithmetic (tests/colmap_reference.py) on this host beside them.  Prints a
Markdown report.  usage: colmap_bench.py [--sizes 40x1000,300x5000,1000x5000] [--host_pairs 3000] [--repeats 5]

Models are synthetic: cameras on an arc, P = V n / 5 Gaussian points sorted by the direction they are best seen from, every
image observing ~n of them drawn from a window around its own direction (so far pairs share nothing), plus 5 % entries
without a 3-D point.  The restatement is timed on ``--host_pairs`` randomly chosen image pairs and scaled to all V (V - 1) / 2
(marked "extrapolated") when a size has more pairs than that."""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colmap_reference as CR  # noqa: E402
from itermvs_amd import colmap, ops  # noqa: E402


def make_model(v, n, seed=0):
    rng = np.random.default_rng(seed)
    p = max(v * n // 5, n)
    xyz = rng.normal(0.0, 60.0, (p, 3))
    span = 80.0                                                     # degrees of arc; point k is best seen from -span/2 + span k / p
    width = max(2.5 * n, p * 12.0 / span)                           # window: ~12 degrees of arc, never narrower than the list
    cams = {1: colmap.Camera(1, "PINHOLE", 640, 512, np.array([1446.1, 1446.1, 331.6, 265.6]))}
    images = []
    for i in range(v):
        az_deg = -span / 2 + span * (i + 0.5) / v
        az, el = math.radians(az_deg), math.radians(3.0 * ((i % 3) - 1))
        c = 680.0 * np.array([math.sin(az) * math.cos(el), math.sin(el), -math.cos(az) * math.cos(el)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        rot = np.stack([x, np.cross(z, x), z])
        mid = p * (i + 0.5) / v
        ids = rng.permutation(np.unique(np.clip(np.rint(rng.normal(mid, width / 4, int(1.15 * n))), 0, p - 1).astype(np.int64)))[:n]
        ids = np.concatenate([ids + 1, np.full(n // 20, -1, np.int64)])                 # COLMAP ids start at 1
        images.append(colmap.Image(i + 1, colmap.rotation_matrix_to_quaternion(rot), -rot @ c, 1, "%06d.jpg" % i, ids[rng.permutation(len(ids))]))
    return colmap.Model(cams, images, np.arange(1, p + 1, dtype=np.int64), xyz)


def time_kernels(model, repeats):
    offsets, point = colmap.observation_csr(model)
    ext = colmap.extrinsic_matrices(model.images)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    off_h = torch.from_numpy(offsets)
    off, pt, xyz, centre, row2 = up(offsets), up(point), up(model.xyz), up(colmap.camera_centres(ext)), up(ext[:, 2, :])
    out = {}
    for name, fn in (("view_scores", lambda: ops.view_scores(off_h, pt, xyz, centre, offsets_dev=off)),
                     ("depth_ranges", lambda: ops.depth_ranges(off_h, pt, xyz, row2, offsets_dev=off))):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name] = (sorted(ms)[len(ms) // 2], min(ms), max(ms))
    return out, (offsets, point, colmap.camera_centres(ext), np.ascontiguousarray(ext[:, 2, :])), res.cpu().numpy()


def time_host(model, inputs, host_pairs, seed=1):
    offsets, point, centre, row2 = inputs
    v = len(model.images)
    iu = np.stack(np.triu_indices(v, 1), 1)
    pick = iu if len(iu) <= host_pairs else iu[np.random.default_rng(seed).choice(len(iu), host_pairs, replace=False)]
    lists = [point[offsets[i]:offsets[i + 1]] for i in range(v)]
    t0 = time.perf_counter()
    for i, j in pick:
        float(CR.pair_terms(lists[i], lists[j], model.xyz, centre[i], centre[j]).sum())
    t_pairs = time.perf_counter() - t0
    t0 = time.perf_counter()
    CR.depth_ranges(offsets, point, model.xyz, row2)
    t_ranges = time.perf_counter() - t0
    return t_pairs * len(iu) / len(pick), len(pick), len(iu), t_ranges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40x1000,300x5000,1000x5000")
    ap.add_argument("--host_pairs", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    print("| V x n | points | observations | view_scores ms (median, min .. max) | depth_ranges ms | convert s (read / device / write) | "
          "numpy restatement: scores s | ranges s |")
    print("|---|---|---|---|---|---|---|---|")
    for size in a.sizes.split(","):
        v, n = (int(x) for x in size.split("x"))
        model = make_model(v, n)
        k, inputs, _ = time_kernels(model, a.repeats)
        with tempfile.TemporaryDirectory() as tmp:
            colmap.write_model(os.path.join(tmp, "sparse"), model, ".bin")
            os.makedirs(os.path.join(tmp, "images"))
            for im in model.images:
                with open(os.path.join(tmp, "images", im.name), "wb") as f:
                    f.write(b"\xff\xd8\xff\xd9")
            walls = []
            for _ in range(2):                                   # the second run: file cache warm, library loaded
                info = {}
                t0 = time.perf_counter()
                colmap.convert(tmp, device="cuda", info=info)
                walls.append(time.perf_counter() - t0)
        host_s, timed, pairs, host_r = time_host(model, inputs, a.host_pairs)
        note = "" if timed == pairs else f" (extrapolated from {timed} of {pairs} pairs)"
        vs, dr = k["view_scores"], k["depth_ranges"]
        print(f"| {v} x {n} | {len(model.point_ids)} | {sum(len(im.point3d_ids) for im in model.images)} | {vs[0]:.3f} ({vs[1]:.3f} .. {vs[2]:.3f}) | "
              f"{dr[0]:.3f} ({dr[1]:.3f} .. {dr[2]:.3f}) | {walls[1]:.3f} ({info['read_s']:.3f} / {info['device_s']:.3f} / {info['write_s']:.3f}) | "
              f"{host_s:.2f}{note} | {host_r:.3f} |", flush=True)


if __name__ == "__main__":
    main()

"""Small training-data trees in the reference's on-disk layouts (datasets/dtu_yao.py:37, 152-157; datasets/blendedmvs.py:37,
135-137) at the real file sizes, generated from seeds: what the training input side's tests and tools/train_input_bench.py read.
Cameras come from :func:`synthetic.camera_parameters`; images are smooth textures plus noise, depths smooth ramps plus noise."""
from __future__ import annotations

import os

import numpy as np

from .data_io import save_pfm


def _rows(m):
    return "\n".join(" ".join(repr(float(x)) for x in r) for r in m)


def _cam_text(ext, k, dmin, dmax):
    return f"extrinsic\n{_rows(ext)}\n\nintrinsic\n{_rows(k)}\n\n{dmin} 2.5 192 {dmax}\n"


def _image(rng, h, w, v):
    """a smooth random-phase texture (so the network sees structure) plus noise, uint8 RGB"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 127 + 80 * np.sin(xs * (0.05 + 0.01 * v) + ys * 0.03)[..., None] * np.array([1.0, 0.8, 0.6], np.float32)
    return np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)


def _pair_lines(n_views, n_src):
    lines = [str(n_views)]
    for v in range(n_views):
        srcs = [(v + k) % n_views for k in range(1, n_src + 1)]
        lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} {100.0 - u:.1f}" for u in srcs)]
    return "\n".join(lines) + "\n"


def write_dtu_tree(root: str, scans=("scan1",), n_views: int = 5, n_src: int = 4, seed: int = 0, lights=range(7),
                   img_hw=(512, 640), depth_hw=(1200, 1600)):
    """a DTU training tree (dtu_yao.py:37, 152-157) at the real file sizes"""
    from PIL import Image
    from . import synthetic
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "Cameras_1"), exist_ok=True)
    with open(os.path.join(root, "Cameras_1", "pair.txt"), "w") as f:
        f.write(_pair_lines(n_views, n_src))
    h, w = img_hw
    k0, exts = synthetic.camera_parameters(n_views, h, w)
    for scan in scans:
        for d in (f"Cameras_1/{scan}_train", f"Rectified/{scan}_train", f"Depths_raw/{scan}"):
            os.makedirs(os.path.join(root, d), exist_ok=True)
        for v in range(n_views):
            k = np.array(k0, np.float64)
            k[:2] /= 4                                                  # the files hold the 160 x 128 intrinsics
            with open(os.path.join(root, f"Cameras_1/{scan}_train/{v:08d}_cam.txt"), "w") as f:
                f.write(_cam_text(exts[v], k, 425.0, 935.0))
            for light in lights:
                Image.fromarray(_image(rng, h, w, v + light)).save(
                    os.path.join(root, f"Rectified/{scan}_train/rect_{v + 1:03d}_{light}_r5000.png"))
            dh, dw = depth_hw
            ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float32)
            depth = (500.0 + 0.1 * xs + 0.05 * ys + rng.normal(0, 1.0, (dh, dw))).astype(np.float32)
            depth[rng.random((dh, dw)) < 0.1] = 0.0
            save_pfm(os.path.join(root, f"Depths_raw/{scan}/depth_map_{v:04d}.pfm"), depth)
            Image.fromarray(rng.integers(0, 40, (dh, dw), dtype=np.uint8)).save(
                os.path.join(root, f"Depths_raw/{scan}/depth_visual_{v:04d}.png"))
    return list(scans)


def write_blended_tree(root: str, scans=("5a3ca9cb270f0e3f14d0eddb",), n_views: int = 6, src_counts=None, seed: int = 0,
                       img_hw=(576, 768), depth_min0: float = 2.0):
    """a BlendedMVS tree (blendedmvs.py:37, 135-137) at the real low-res size; ``src_counts``: sources per view"""
    from PIL import Image
    from . import synthetic
    rng = np.random.default_rng(seed)
    h, w = img_hw
    k0, exts = synthetic.camera_parameters(n_views, h, w)
    counts = src_counts or [n_views - 1] * n_views
    for si, scan in enumerate(scans):
        for d in ("cams", "blended_images", "rendered_depth_maps"):
            os.makedirs(os.path.join(root, scan, d), exist_ok=True)
        lines = [str(n_views)]
        for v in range(n_views):
            srcs = [(v + k) % n_views for k in range(1, counts[v] + 1)]
            lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} {50.0 - u:.1f}" for u in srcs)]
        with open(os.path.join(root, scan, "cams", "pair.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        for v in range(n_views):
            dmin = depth_min0 * (1 + 0.1 * v) * (si + 1)
            e = exts[v].copy()
            e[:3, 3] /= 100.0                                            # BlendedMVS scenes are in their own units
            with open(os.path.join(root, scan, "cams", f"{v:08d}_cam.txt"), "w") as f:
                f.write(_cam_text(e, k0, dmin, dmin * 3.0))
            Image.fromarray(_image(rng, h, w, v)).save(os.path.join(root, scan, "blended_images", f"{v:08d}.jpg"), quality=95)
            depth = (dmin * (0.8 + 2.6 * rng.random((h, w)))).astype(np.float32)
            save_pfm(os.path.join(root, scan, "rendered_depth_maps", f"{v:08d}.pfm"), depth)
    return list(scans)

#!/usr/bin/env python3
"""Generate tests/golden/colmap_cases.npz from the REAL reference converter (CPU only; never run on the GPU box).

The reference's ``colmap_input.py`` (found under $ITERMVS_REFERENCE, like tests/golden/make_golden.py) is a script that imports
``cv2`` at the top and does everything under ``__main__``.  It runs unmodified through ``runpy.run_path`` with an empty stand-in
module for cv2 (only ``--convert_format`` touches it, and that stays off); ``run_path`` returns the script's globals, so its
``score``, ``depth_ranges``, ``extrinsic`` are taken in full float64 beside the files it wrote.  Its code never ships: the fixture
holds data only -- the synthetic model as arrays and the reference's results.

Models: cameras on the arc of itermvs_amd/synthetic.py (radius 680, looking at the origin, elevation +-3 deg), a Gaussian point
cloud, per-image visibility that falls off with the angular distance between the image and the point's preferred direction (cut
off, so far pairs share nothing).  Cases:

* ``small``  12 images x ~100 observations: -1 entries, shuffled lists, pairs without a common point, one image whose list
             repeats point ids, non-contiguous COLMAP image / point ids in non-sorted file order, a SIMPLE_RADIAL and a PINHOLE camera;
* ``mid``    40 images x ~1000 observations, 8000 points;
* ``params`` ``small`` with --theta0 8 --sigma1 2 --sigma2 6 --num_src_images 5.

Per case ``score_floor`` = max over pairs of |reference score - the same sum with every operation in np.longdouble| /
max(1, reference score): how far the reference's own float64 result is from the exact value.  The tests' tolerances are
multiples of it.  Conditions asserted here, on the reference alone: every score finite; every image has a valid observation; in
every pair.txt row at least 90 % of the adjacent pairs among the non-zero scores differ by more than the tie margin
2 x 32 x score_floor x max(1, score), so the order check of the tests cannot pass vacuously.
"""
import math
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("ITERMVS_REFERENCE", "/root/reference")

import colmap_reference as CR  # noqa: E402
from itermvs_amd import colmap, synthetic  # noqa: E402


def make_model(n_images, n_obs, n_points, az_step_deg, sight_deg, seed, quirks):
    """-> itermvs_amd.colmap.Model"""
    rng = np.random.default_rng(seed)
    point_ids = np.sort(rng.choice(np.arange(1, 6 * n_points), n_points, replace=False))[rng.permutation(n_points)].astype(np.int64)
    xyz = rng.normal(0.0, 60.0, (n_points, 3))
    pref = rng.uniform(-1.0, 1.0, n_points) * az_step_deg * (n_images // 2 + 1)       # the direction a point is best seen from
    # the reference prints intrinsic[1] (colmap_input.py:306): a camera with id 1 must exist
    cams = {1: colmap.Camera(1, "SIMPLE_RADIAL", 640, 512, np.array([1446.1, 331.6, 265.6, -0.0123])),
            8: colmap.Camera(8, "PINHOLE", 640, 512, np.array([1440.0, 1452.5, 329.0, 262.25]))}
    images = []
    for v in range(n_images):
        step = (v + 1) // 2 * (1 if v % 2 else -1)
        az, el = math.radians(az_step_deg * step), math.radians(3.0 * ((v % 3) - 1))
        c = 680.0 * np.array([math.sin(az) * math.cos(el), math.sin(el), -math.cos(az) * math.cos(el)])
        rot = synthetic._look_at_origin(c)
        d = (pref - az_step_deg * step) / sight_deg
        w = np.where(np.abs(d) < 2.0, np.exp(-0.5 * d * d), 0.0)
        n = min(n_obs + int(rng.integers(-n_obs // 10, n_obs // 10 + 1)), int((w > 0).sum()))
        seen = rng.choice(n_points, n, replace=False, p=w / w.sum())
        ids = point_ids[seen]
        if quirks:
            ids = np.concatenate([ids, np.full(max(1, n // 6), -1, np.int64)])
            if v == 4:
                ids = np.concatenate([ids, ids[:7], ids[:2]])                       # repeated point ids (one of them three times)
            ids = ids[rng.permutation(len(ids))]
        images.append(colmap.Image(7 + 3 * v, colmap.rotation_matrix_to_quaternion(rot), -rot @ c, 1 if v % 2 else 8, "IMG_%04d.JPG" % (900 - 7 * v), ids))
    if quirks:
        images = [images[i] for i in rng.permutation(n_images)]                     # file order is neither arc nor id order
    return colmap.Model(cams, images, point_ids, xyz)


def run_reference(model, flags):
    with tempfile.TemporaryDirectory() as tmp:
        colmap.write_model(os.path.join(tmp, "sparse"), model, ".bin")
        os.makedirs(os.path.join(tmp, "images"))
        for im in model.images:
            with open(os.path.join(tmp, "images", im.name), "wb") as f:
                f.write(b"x")
        argv, mods = sys.argv, sys.modules.get("cv2")
        sys.modules["cv2"] = types.ModuleType("cv2")
        sys.argv = ["colmap_input.py", "--input_folder", tmp] + flags
        try:
            g = runpy.run_path(os.path.join(REF, "colmap_input.py"), run_name="__main__")
        finally:
            sys.argv = argv
            if mods is None:
                del sys.modules["cv2"]
            else:
                sys.modules["cv2"] = mods
        with open(os.path.join(tmp, "pair.txt")) as f:
            pair = f.read()
        cam_txt = []
        for i in range(len(model.images)):
            with open(os.path.join(tmp, "cams_1", "%08d_cam.txt" % i)) as f:
                cam_txt.append(f.read())
    return np.array(g["score"]), np.array(g["depth_ranges"]), np.stack(g["extrinsic"]), pair, cam_txt


def pack(case, model, flags):
    score, ranges, extrinsic, pair, cam_txt = run_reference(model, flags)
    assert np.isfinite(score).all() and np.isfinite(ranges).all()
    a = colmap.build_parser().parse_args(["--input_folder", "x"] + flags)
    offsets, point = colmap.observation_csr(model)
    ld = np.longdouble
    e = extrinsic.astype(ld)
    centre = np.stack([-(e[i, :3, :3].T @ e[i, :3, 3]) for i in range(len(e))])
    exact = CR.view_scores(offsets, point, model.xyz, centre, a.theta0, a.sigma1, a.sigma2, dtype=ld)
    floor = float(np.max(np.abs(score.astype(ld) - exact) / np.maximum(1, score)))
    # our own extrinsics / centres equal the reference's bit for bit (same expressions), so the fixture need not store them
    assert np.array_equal(colmap.extrinsic_matrices(model.images), extrinsic)
    ordered = total = 0
    for i, row in enumerate(CR.pair_rows(pair)):
        s = np.array([score[i, k] for k, _ in row])
        nz = s[s != 0]
        gaps = np.abs(np.diff(nz)) > 2 * 32 * floor * np.maximum(1, np.maximum(nz[:-1], nz[1:]))
        assert len(gaps) == 0 or gaps.mean() >= 0.9, (case, i, gaps.mean())
        ordered, total = ordered + int(gaps.sum()), total + len(gaps)
    iu = np.triu_indices(len(score), 1)
    print(f"{case}: V = {len(score)}, observations = {len(point)}, score max {score.max():.3f}, zero pairs {(score[iu] == 0).sum()} of "
          f"{len(iu[0])}, score_floor {floor:.3e}, {ordered} of {total} adjacent non-zero pairs ordered by the tie rule")
    cams = list(model.cameras.values())
    out = {"names": np.array([im.name for im in model.images]), "image_ids": np.array([im.id for im in model.images], np.int64),
           "qvec": np.stack([im.qvec for im in model.images]), "tvec": np.stack([im.tvec for im in model.images]),
           "camera_ids": np.array([im.camera_id for im in model.images], np.int64),
           "obs_len": np.array([len(im.point3d_ids) for im in model.images], np.int64),
           "obs_ids": np.concatenate([im.point3d_ids for im in model.images]),
           "cam_ids": np.array([c.id for c in cams], np.int64), "cam_models": np.array([c.model for c in cams]),
           "cam_wh": np.array([[c.width, c.height] for c in cams], np.int64),
           "cam_nparams": np.array([len(c.params) for c in cams], np.int64), "cam_params": np.concatenate([c.params for c in cams]),
           "point_ids": model.point_ids, "xyz": model.xyz, "score": score, "depth_ranges": ranges, "pair_txt": np.array(pair),
           "cam_txt": np.array(cam_txt), "score_floor": np.array(floor),
           "args": np.array([a.theta0, a.sigma1, a.sigma2, a.num_src_images], np.float64)}
    return {f"{case}.{k}": v for k, v in out.items()}, score


def main():
    small = make_model(12, 100, 700, 8.0, 14.0, seed=11, quirks=True)
    mid = make_model(40, 1000, 8000, 2.0, 12.0, seed=12, quirks=False)
    out = {}
    d, s_small = pack("small", small, [])
    out.update(d)
    iu = np.triu_indices(12, 1)
    assert (s_small[iu] == 0).any(), "small: no pair without a common point"
    reps = [np.unique(im.point3d_ids[im.point3d_ids >= 0], return_counts=True)[1].max() for im in small.images]
    assert max(reps) >= 2
    out.update(pack("mid", mid, [])[0])
    out.update(pack("params", small, ["--theta0", "8", "--sigma1", "2", "--sigma2", "6", "--num_src_images", "5"])[0])
    path = os.path.join(HERE, "colmap_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""COLMAP converter on the MI355X: itermvs_view_scores / itermvs_depth_ranges against the reference's own output
(tests/golden/colmap_cases.npz) and against the numpy restatement (tests/colmap_reference.py), and colmap_input.py -> eval.py end
to end.  Score tolerance: |got - ref| <= 32 x score_floor x max(1, ref), score_floor read from the fixture (the distance of the
reference's float64 sum from the same sum in extended precision); 32 is the allowance for the device's acos / exp and for a
tree-shaped instead of a serial sum."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import colmap_reference as CR
from conftest import ROOT, load_weights
from test_colmap_cpu import CASES, kernel_inputs, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK_POINTS = 64 * 1024 * 8          # kMaxChunkBits of csrc/colmap.hip: points per LDS bitmap chunk of itermvs_view_scores


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scores(offsets, point, xyz, centre, *params):
    from itermvs_amd import ops
    return ops.view_scores(torch.from_numpy(offsets), _up(point), _up(xyz), _up(centre), *params).cpu().numpy()


def _ranges(offsets, point, xyz, row2):
    from itermvs_amd import ops
    return ops.depth_ranges(torch.from_numpy(offsets), _up(point), _up(xyz), _up(row2)).cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_view_scores_against_the_reference(case):
    model, ref = load_case(case)
    offsets, point, xyz, centre, _, _ = kernel_inputs(model)
    params = (ref["theta0"], ref["sigma1"], ref["sigma2"])
    got = _scores(offsets, point, xyz, centre, *params)
    want, floor = ref["score"], ref["score_floor"]
    ratio = np.abs(got - want) / (floor * np.maximum(1, want))
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{case}: score_floor {floor:.3e}; worst |got - ref| / (score_floor x max(1, ref)) = {ratio.max():.2f} at pair ({i}, {j}), "
          f"ref {want[i, j]:.6f}, got - ref {got[i, j] - want[i, j]:.3e}")
    assert ratio.max() <= 32
    assert (got[want == 0] == 0).all() and (np.diag(got) == 0).all()                  # exact zeros stay exact zeros
    assert np.array_equal(got.view(np.int64), got.T.copy().view(np.int64))            # bitwise symmetric
    again = _scores(offsets, point, xyz, centre, *params)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))                   # two runs: the same bits


@pytest.mark.parametrize("case", CASES)
def test_depth_ranges_against_the_reference(case):
    model, ref = load_case(case)
    offsets, point, xyz, _, row2, _ = kernel_inputs(model)
    got = _ranges(offsets, point, xyz, row2)
    own, mags = CR.depth_ranges(offsets, point, xyz, row2)
    assert np.array_equal(got.view(np.int64), own.view(np.int64))       # the order statistic of the kernel's own z values, exactly
    err = np.abs(got - ref["depth_ranges"])
    print(f"{case}: depth ranges, worst |got - ref| / (8 x 2^-53 x sum |e_k x_k|) = {(err / (8 * 2.0 ** -53 * mags)).max():.3f}")
    assert (err <= 8 * 2.0 ** -53 * mags).all()


def test_multiplicity_and_missing_points_in_closed_form():
    """three images whose scores are integers: every common point sees its two camera centres under theta0 exactly (to ~1e-13
    degrees, where the Gaussian rounds to 1.0), so a pair's score is the number of matching entries of the LOWER image's list"""
    theta0 = 5.0
    a = 40.0
    d = a / math.tan(math.radians(theta0 / 2))
    c0, c1 = np.array([-a, 0.0, 0.0]), np.array([a, 0.0, 0.0])
    p1, p2, p3 = np.array([0.0, 0.0, d]), np.array([0.0, d, 0.0]), np.array([3.0, 0.0, -500.0])        # p1, p2: symmetric about the chord
    t = math.radians(theta0)
    rot_y = np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]])
    c2 = p3 + 1.3 * (rot_y @ (c0 - p3))                                     # the angle c0 - p3 - c2 is theta0 by construction
    xyz = np.stack([np.array([9.0, 9.0, 9.0]), p1, p2, p3, np.array([1.0, 2.0, 3.0]), np.array([5.0, 5.0, 50.0])])
    lists = [[1, 0, 1, -1, 2, 3, 4],         # image 0: point 1 twice
             [2, -1, 1, 2, 5, -1],           # image 1: points 1, 2 (2 twice: the higher image's repeats do not count), not 0, 3, 4
             [3, 3, -1, 3]]                  # image 2: point 3 three times (counts once: image 0 lists it once)
    offsets = np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)
    point = np.concatenate(lists).astype(np.int32)
    centre = np.stack([c0, c1, c2])
    got = _scores(offsets, point, xyz, centre, theta0, 1.0, 10.0)
    assert np.array_equal(got, np.array([[0.0, 3.0, 1.0], [3.0, 0.0, 0.0], [1.0, 0.0, 0.0]])), got
    assert np.array_equal(CR.view_scores(offsets, point, xyz, centre, theta0, 1.0, 10.0), got)
    # a list of -1 only / an empty list: scores 0, NaN range (the host turns it into a ValueError)
    offsets2 = np.array([0, 7, 9, 9], np.int64)
    point2 = np.concatenate([lists[0], [-1, -1]]).astype(np.int32)
    assert not _scores(offsets2, point2, xyz, centre, theta0, 1.0, 10.0).any()
    rng = _ranges(offsets2, point2, xyz, np.tile([0.0, 0.0, 1.0, 10.0], (3, 1)))
    assert np.isfinite(rng[0]).all() and np.isnan(rng[1:]).all()
    # order statistics with repeats: z = xyz_z + 10 over the entries 1, 0, 1, 2, 3, 4 -> int(6 * .01) = 0, int(6 * .99) = 5
    z = np.sort(xyz[[1, 0, 1, 2, 3, 4], 2] + 10)
    assert rng[0].tolist() == [z[0], z[5]]


def test_more_points_than_one_bitmap_chunk():
    """P > CHUNK_POINTS: the membership bitmap is built chunk by chunk; common points on both sides of the boundary (the two
    indices next to it included) against the restatement, within 32 x the restatement's own distance from extended precision"""
    rng = np.random.default_rng(5)
    p_total = CHUNK_POINTS + 70001
    xyz = rng.normal(0.0, 60.0, (p_total, 3))
    common = np.concatenate([rng.choice(p_total, 1500, replace=False), [CHUNK_POINTS - 1, CHUNK_POINTS, 0, p_total - 1]])
    lists, centre = [], []
    for v in range(5):
        own = rng.choice(p_total, 800, replace=False)
        ids = np.concatenate([common[rng.random(len(common)) < 0.6], own, np.full(50, -1)])
        lists.append(ids[rng.permutation(len(ids))])
        az = math.radians(4.0 * v)
        centre.append(680.0 * np.array([math.sin(az), 0.02 * v, -math.cos(az)]))
    lists[1] = np.concatenate([lists[1], [CHUNK_POINTS - 1, CHUNK_POINTS]])
    lists[3] = np.concatenate([lists[3], [CHUNK_POINTS - 1, CHUNK_POINTS]])
    offsets = np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)
    point, centre = np.concatenate(lists).astype(np.int32), np.stack(centre)
    got = _scores(offsets, point, xyz, centre, 5.0, 1.0, 10.0)
    want = CR.view_scores(offsets, point, xyz, centre)
    exact = CR.view_scores(offsets, point, xyz, centre, dtype=np.longdouble)
    floor = max(float(np.max(np.abs(want - exact) / np.maximum(1, want))), 2.0 ** -52)
    both = [len(set(a[a >= CHUNK_POINTS]) & set(b)) > 0 and len(set(a[(a >= 0) & (a < CHUNK_POINTS)]) & set(b)) > 0
            for a in lists for b in lists if a is not b]
    assert all(both) and want[np.triu_indices(5, 1)].min() > 1.0          # every pair has common points in both chunks
    ratio = float(np.max(np.abs(got - want) / (floor * np.maximum(1, want))))
    print(f"P = {p_total} (two chunks of {CHUNK_POINTS}): floor {floor:.3e}, worst ratio {ratio:.2f}")
    assert ratio <= 32 and np.array_equal(got, got.T) and np.array_equal(got, _scores(offsets, point, xyz, centre, 5.0, 1.0, 10.0))
    row2 = np.tile([0.1, -0.2, 0.97, 700.0], (5, 1))
    assert np.array_equal(_ranges(offsets, point, xyz, row2), CR.depth_ranges(offsets, point, xyz, row2)[0])


@pytest.mark.parametrize("case", ["small", "params"])
def test_convert_writes_the_reference_files(case, tmp_path):
    """itermvs_amd.colmap.convert on the fixture model written as .bin: camera files (range line to the %f digit's last place),
    pair.txt under the ties rule, images copied under their new names"""
    from itermvs_amd import colmap
    model, ref = load_case(case)
    colmap.write_model(str(tmp_path / "sparse"), model, ".bin" if case == "small" else ".txt")
    (tmp_path / "images").mkdir()
    for im in model.images:
        (tmp_path / "images" / im.name).write_bytes(im.name.encode())
    info = {}
    colmap.convert(str(tmp_path), None, ref["num_src_images"], ref["theta0"], ref["sigma1"], ref["sigma2"], device=DEV, info=info)
    assert info["images"] == 12 and info["device_s"] > 0
    for i, want in enumerate(ref["cam_txt"]):
        got = open(str(tmp_path / "cams_1" / ("%08d_cam.txt" % i))).read()
        assert got.split("\n")[:11] == want.split("\n")[:11], i
        g, w = [float(x) for x in got.split("\n")[11].split()], [float(x) for x in want.split("\n")[11].split()]
        assert len(g) == 2 and max(abs(g[0] - w[0]), abs(g[1] - w[1])) <= 1.5e-6, i
        assert (tmp_path / "images" / ("%08d.jpg" % i)).read_bytes() == model.images[i].name.encode()
    checked = CR.compare_pair_text(open(str(tmp_path / "pair.txt")).read(), ref["pair_txt"], ref["score"], ref["score_floor"])
    assert checked > 0
    # an image whose observations are all -1: ValueError naming it, instead of the reference's IndexError
    model.images[3].point3d_ids[:] = -1
    colmap.write_model(str(tmp_path / "sparse"), model, ".bin")
    with pytest.raises(ValueError, match=model.images[3].name):
        colmap.convert(str(tmp_path), device=DEV)


def _plane_depths(proj):
    """make_scene_sample's plane seen through K[R|t] = proj (float64 [4,4]) -> (depth map function inputs) centre, ray matrix, normal"""
    t = math.radians(20.0)
    normal = np.array([math.sin(t), 0.3 * math.sin(t), -math.cos(t)])
    normal /= np.linalg.norm(normal)
    minv = np.linalg.inv(proj[:3, :3])
    return -minv @ proj[:3, 3], minv, normal


def test_colmap_input_then_eval_end_to_end(tmp_path):
    """somebody's own photographs: the photo-consistent synthetic scene (itermvs_amd/synthetic.py: the textured plane the trained
    network really reconstructs; the flat-colour scan of tests/test_fusion.py gives a network nothing to match) described as a
    COLMAP model -- true cameras, 3-D points sampled uniformly on the plane, observations by projection -- then
    ``colmap_input.py`` and ``eval.py --dataset folder --filter`` in child processes: a PFM per view, a non-empty PLY, and every
    cam.txt range brackets the view's true depths at the 1 % / 99 % level.  Bound: at most 3 % of the true depth map outside on
    either side.  Points uniform on the plane are denser per pixel where the plane is farther, by at most (depth_max /
    depth_min)^2 < 2.2 in these views, so the 1 % order statistic of the observations cuts between 0.45 % and 2.2 % of the
    pixels; ~2000 observations per view add a sampling error of 0.3 % (one sigma at 2 %)."""
    from PIL import Image
    from itermvs_amd import colmap, synthetic
    h, w, n_views = 512, 640, 5
    s = synthetic.make_scene_sample(num_views=n_views, height=h, width=w, seed=0)
    k0, exts = synthetic.camera_parameters(n_views, h, w, ref_shift=0)
    scan = tmp_path / "data" / "scan1"
    (scan / "images").mkdir(parents=True)
    rng = np.random.default_rng(3)
    projs = [s["proj_matrices"]["level_0"][0, v].numpy().astype(np.float64) for v in range(n_views)]
    dense = []
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    for v in range(n_views):
        img = ((s["imgs"]["level_0"][0, v].permute(1, 2, 0).numpy() + 1) * 127.5).round().clip(0, 255).astype(np.uint8)
        Image.fromarray(img).save(str(scan / "images" / f"photo_{v}.png"))
        centre, minv, normal = _plane_depths(projs[v])
        dirs = np.stack([xs, ys, np.ones_like(xs)], -1) @ minv.T
        dense.append(-(centre @ normal) / (dirs @ normal))                 # the view's true depth map (make_scene_sample's `s`)
    e1 = np.cross(normal, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(normal, e1)
    xyz = rng.uniform(-260, 260, (6000, 1)) * e1 + rng.uniform(-230, 230, (6000, 1)) * e2      # covers every view's footprint
    point_ids = (np.arange(len(xyz)) * 3 + 11).astype(np.int64)
    images = []
    for v in range(n_views):
        cam = projs[v][:3, :3] @ xyz.T + projs[v][:3, 3:4]
        u, vv = cam[0] / cam[2], cam[1] / cam[2]
        seen = (u >= 0) & (u <= w - 1) & (vv >= 0) & (vv <= h - 1) & (cam[2] > 0)
        ids = np.concatenate([point_ids[seen], np.full(40, -1)])[rng.permutation(int(seen.sum()) + 40)]
        e = exts[v].astype(np.float64)
        images.append(colmap.Image(20 + v, colmap.rotation_matrix_to_quaternion(e[:3, :3]), e[:3, 3], 1, f"photo_{v}.png", ids))
    cams = {1: colmap.Camera(1, "PINHOLE", w, h, np.array([k0[0, 0], k0[1, 1], k0[0, 2], k0[1, 2]]))}
    colmap.write_model(str(scan / "sparse"), colmap.Model(cams, images, point_ids, xyz), ".bin")
    ckpt = str(tmp_path / "dtu.ckpt")
    torch.save({"model": {"module." + k: v for k, v in load_weights("dtu").items()}}, ckpt)
    run = lambda *a: subprocess.run([sys.executable] + list(a), cwd=ROOT, capture_output=True, text=True, timeout=600)      # noqa: E731
    r = run("colmap_input.py", "--input_folder", str(scan))
    assert r.returncode == 0, r.stderr[-2000:]
    from itermvs_amd.scan_dataset import read_cam_file
    for v in range(n_views):
        _, e, dmin, dmax = read_cam_file(str(scan / "cams_1" / ("%08d_cam.txt" % v)))
        assert np.abs(e - exts[v]).max() < 1e-3
        d = dense[v]
        below, above = float((d < dmin).mean()), float((d > dmax).mean())
        print(f"view {v}: range {dmin:.2f} .. {dmax:.2f}, true depths {d.min():.2f} .. {d.max():.2f}, outside {below:.4f} / {above:.4f}")
        assert d.min() - 0.05 <= dmin < np.median(d) < dmax <= d.max() + 0.05 and below <= 0.03 and above <= 0.03
        assert 1500 < len(images[v].point3d_ids) - 40
        assert (scan / "images" / ("%08d.jpg" % v)).is_file()
    rows = CR.pair_rows((scan / "pair.txt").read_text())
    assert len(rows) == n_views and all(len(r_) == n_views for r_ in rows)
    assert all(float(r_[0][1]) > 0 and r_[-1] == (i, "0.000000") for i, r_ in enumerate(rows))      # image i itself: score 0, last
    out = tmp_path / "outputs"
    r = run("eval.py", "--dataset", "folder", "--testpath", str(tmp_path / "data"), "--outdir", str(out), "--n_views", str(n_views),
            "--img_wh", str(w), str(h), "--loadckpt", ckpt, "--filter")
    assert r.returncode == 0, r.stderr[-2000:]
    for v in range(n_views):
        assert (out / "scan1" / "depth_est" / ("%08d.pfm" % v)).is_file() and (out / "scan1" / "confidence" / ("%08d.pfm" % v)).is_file()
    head = (out / "scan1.ply").read_bytes().split(b"end_header\n")[0]
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    print(f"fused cloud: {n} vertices")
    assert n > 0

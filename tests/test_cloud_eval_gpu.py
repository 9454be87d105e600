"""The DTU evaluator on the GPU against the numpy yardstick (tests/cloud_eval_reference.py): equality, not tolerances, on the
reduction's keep mask, the capped nearest-neighbour distances, the mask and plane tests, counts and medians; the means and
variances within the worst-case bound of a reordered fp64 sum; the driver end to end."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_eval_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"

STAT_KEYS = ("nData", "nStl", "MeanData", "MedData", "VarData", "MeanStl", "MedStl", "VarStl")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_reduce(pts, dst, seed):
    from itermvs_amd import cloud_eval as CE
    order = np.random.default_rng(seed).permutation(pts.shape[0])
    want = R.reduce_points(pts, dst, order)
    info, info2 = {}, {}
    got = CE.reduce_points(dev(pts), dst, order=torch.from_numpy(order), info=info)
    again = CE.reduce_points(dev(pts), dst, order=torch.from_numpy(order), rounds_per_sync=1, info=info2)
    print(f"reduce_points: n = {pts.shape[0]}, dst = {dst}, kept = {info['kept']}, rounds = {info['rounds']} / {info2['rounds']}, "
          f"non-finite = {info['non_finite']}")
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, again)
    assert info["kept"] == int(want.sum()) and info["non_finite"] == int((~np.isfinite(pts).all(1)).sum())
    assert 1 <= info2["rounds"] <= pts.shape[0] and 1 <= info["rounds"]      # (a round may see another's stores: the count can vary)
    return info


@pytest.mark.parametrize("seed,dst", [(0, 0.2), (1, 0.2), (2, 0.35), (3, 0.07)])
def test_reduce_points_equals_the_sequential_loop(seed, dst):
    s = R.make_scene(seed)
    info = check_reduce(s["pred"], dst, seed + 100)
    assert 0 < info["kept"] < s["pred"].shape[0] and info["non_finite"] == 4


def test_reduce_points_one_cell_no_neighbours_and_exact_radius():
    from itermvs_amd import cloud_eval as CE
    gen = np.random.default_rng(5)
    one_cell = (5.0 + gen.random((3000, 3)) * 0.19).astype(np.float32)       # everything inside one cell of edge 0.2
    info = check_reduce(one_cell, 0.2, 1)
    assert info["kept"] < 40
    g = np.arange(12) * 3.0
    apart = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)      # nobody has a neighbour
    assert check_reduce(apart, 0.2, 2)["kept"] == apart.shape[0]
    # spacing exactly dst: the inclusive radius removes the four axis neighbours (raster order keeps one colour)
    gx, gy = np.meshgrid(np.arange(9) * 0.25, np.arange(9) * 0.25, indexing="ij")
    lat = np.stack([gx.ravel(), gy.ravel(), np.zeros(81)], 1).astype(np.float32)
    keep = CE.reduce_points(dev(lat), 0.25, order=torch.arange(81)).cpu().numpy()
    assert np.array_equal(keep, np.array([(i + j) % 2 == 0 for i in range(9) for j in range(9)]))
    assert CE.reduce_points(dev(lat), 0.2499, order=torch.arange(81)).all()
    # the default order is the seeded CPU permutation
    a = CE.reduce_points(dev(one_cell), 0.05, seed=7)
    b = CE.reduce_points(dev(one_cell), 0.05, order=CE.default_order(3000, 7))
    assert torch.equal(a, b) and not torch.equal(a, CE.reduce_points(dev(one_cell), 0.05, seed=8))
    # nothing but non-finite points, and no points at all
    assert not CE.reduce_points(dev(np.full((5, 3), np.nan, np.float32)), 0.2).any()
    assert CE.reduce_points(torch.zeros((0, 3), device=DEV), 0.2).numel() == 0
    with pytest.raises(ValueError, match="cell key"):                        # an extent beyond 2^21 cells per axis
        CE.reduce_points(dev(np.array([[0, 0, 0], [1e6, 0, 0]], np.float32)), 0.2)


def test_reduce_points_200k():
    s = R.make_scene(11, n_gt=10, n_pred=200000, extent=120.0)
    info = check_reduce(s["pred"], 0.2, 12)
    assert info["rounds"] < 64


def check_nn(q_from, q_to, bb, cap, block_wise=True):
    from itermvs_amd import cloud_eval as CE
    info = {}
    got = CE.capped_nn_distance(dev(q_from), dev(q_to), bb, cap, info=info).cpu().numpy()
    want = R.capped_nn(q_from, q_to, bb, cap)
    print(f"capped_nn_distance: {q_from.shape[0]} x {q_to.shape[0]}, cap = {cap}, below cap: {int((want < cap).sum())}, "
          f"second pass: {info['second_pass']}")
    assert got.dtype == np.float64 and np.array_equal(got, want)             # bit for bit, all points
    if block_wise:
        blk = R.max_dist_cp(q_to, q_from, bb, cap)
        below = blk < cap
        assert np.array_equal(got[below], blk[below]) and (got[~below] == cap).all()
    return got, info


@pytest.mark.parametrize("seed,extent,cap", [(0, 24.0, 4.0), (1, 24.0, 4.0), (2, 240.0, 60.0)])
def test_capped_nn_distance_bit_equal_both_directions(seed, extent, cap):
    s = R.make_scene(seed, n_gt=5000, n_pred=5000, extent=extent, cap=cap)
    bb = s["bb"]
    for q_from, q_to in ((s["pred"], s["gt"]), (s["gt"], s["pred"])):
        got, _ = check_nn(q_from, q_to, bb, cap)
        assert (got < cap).any() and ((got == cap).any() or q_from is s["gt"])     # the prediction has outliers and NaN rows
        assert (got[~R.covered(q_from, bb, cap)] == cap).all()              # outside the covered region (NaN rows included)


def test_capped_nn_distance_edge_cases():
    from itermvs_amd import cloud_eval as CE
    s = R.make_scene(4, n_gt=800, n_pred=800)
    pred, gt, bb = s["pred"], s["gt"], s["bb"]
    none = CE.capped_nn_distance(dev(pred), torch.zeros((0, 3), device=DEV), bb, 4.0)
    assert none.shape == (pred.shape[0],) and (none == 4.0).all()            # empty q_to
    assert CE.capped_nn_distance(torch.zeros((0, 3), device=DEV), dev(gt), bb, 4.0).numel() == 0
    nan_targets = np.concatenate([gt, np.full((3, 3), np.nan, np.float32), np.array([[np.inf, 0, 0]], np.float32)])
    a, _ = check_nn(pred, nan_targets, bb, 4.0, block_wise=False)            # non-finite targets never win
    b, _ = check_nn(pred, gt, bb, 4.0, block_wise=False)
    assert np.array_equal(a, b)
    far_bb = np.array([[1000.0, 1000.0, 1000.0], [1100.0, 1100.0, 1100.0]])  # a region nobody is in
    assert (CE.capped_nn_distance(dev(pred), dev(gt), far_bb, 4.0) == 4.0).all()
    neg_bb = np.array([[0.0, 0.0, 0.0], [10.0, -5.0, 10.0]])                 # a negative Range: the block loops never run
    assert (CE.capped_nn_distance(dev(pred), dev(gt), neg_bb, 4.0) == 4.0).all()
    check_nn(gt, gt, bb, 4.0)                                                 # every point its own neighbour: 0 where covered
    check_nn(pred, gt[:1], bb, 4.0)                                           # a single target
    for cell in (0.3, 2.5, 9.0):                                              # the result does not depend on the grid
        got = CE.capped_nn_distance(dev(pred), dev(gt), bb, 4.0, cell=cell).cpu().numpy()
        assert np.array_equal(got, b), cell


def test_capped_nn_distance_one_million_targets():
    from itermvs_amd import cloud_eval as CE
    gen = np.random.default_rng(21)
    gt = R.wavy_surface(1_000_000, gen, extent=300.0, z0=40.0)
    s = R.make_scene(22, n_gt=10, n_pred=60000, extent=300.0, cap=60.0)
    pred = s["pred"]
    pred[:, 2] += 34.0                                                       # onto the large surface's height
    bb = np.array([[-30.0, -30.0, 0.0], [330.0, 330.0, 110.0]])
    info = {}
    got = CE.capped_nn_distance(dev(pred), dev(gt), bb, 60.0, info=info).cpu().numpy()
    pick = np.random.default_rng(23).choice(pred.shape[0], 4096, replace=False)
    far = np.array([[150.0, 150.0, 105.0], [-29.0, -29.0, 1.0], [329.0, 150.0, 100.0]], np.float32)   # covered, far from the surface
    queries = np.concatenate([pred[pick], far])

    def brute(q):
        """brute force over ALL targets: the squared distances with torch's fp64 elementwise operations (one rounding each, in
        the fixed order), their minimum, numpy's sqrt"""
        t, out = dev(gt).double(), []
        for a in range(0, q.shape[0], 64):
            qq = dev(q[a:a + 64]).double()[:, None, :]
            dx, dy, dz = qq[..., 0] - t[None, :, 0], qq[..., 1] - t[None, :, 1], qq[..., 2] - t[None, :, 2]
            d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
            out.append(torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2).min(1).values.cpu().numpy())
        return np.sqrt(np.concatenate(out))

    assert np.array_equal(brute(queries[:48]), R.nn_brute(queries[:48], gt, chunk=8))             # the same numbers as the yardstick's
    want = np.where(R.covered(queries, bb, 60.0), np.minimum(brute(queries), 60.0), 60.0)
    print(f"1M targets: sampled queries below cap: {int((want < 60).sum())}, at cap: {int((want == 60).sum())}, "
          f"second pass: {info['second_pass']} of {pred.shape[0]}")
    assert np.array_equal(got[pick], want[:4096])                             # every sampled query
    got_far = CE.capped_nn_distance(dev(far), dev(gt), bb, 60.0).cpu().numpy()
    assert np.array_equal(got_far, want[4096:]) and (got_far > 4.0).all() and (got_far < 60.0).any()


@pytest.mark.parametrize("seed", [0, 3])
def test_points_in_mask_and_above_plane(seed):
    from itermvs_amd import cloud_eval as CE
    s = R.make_scene(seed)
    pts = np.concatenate([s["pred"], s["gt"]])
    got = CE.points_in_mask(dev(pts), dev(s["obs_mask"]), s["bb"], s["res"]).cpu().numpy()
    want = R.points_in_mask(pts, s["obs_mask"], s["bb"], s["res"])
    assert np.array_equal(got, want) and want.any() and (~want).any()
    # half-way cases: v = k + 0.5 exactly goes up (MATLAB's round), also below zero; the mask's first and last voxels
    mask = np.ones((3, 3, 3), dtype=np.uint8)
    bb = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    xs = np.array([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.24, 1.25, 1.5, -0.26], np.float32)       # res 0.5: v = 2 x + 1
    half = np.stack([xs, np.zeros_like(xs), np.ones_like(xs)], 1)
    got = CE.points_in_mask(dev(half), dev(mask), bb, 0.5).cpu().numpy()
    assert np.array_equal(got, R.points_in_mask(half, mask, bb, 0.5))
    assert got.tolist() == [False, False, True, True, True, True, True, True, True, False, False, False]
    assert not CE.points_in_mask(dev(half), dev(np.zeros((3, 3, 3), np.uint8)), bb, 0.5).any()
    above = CE.above_plane(dev(pts), s["plane"]).cpu().numpy()
    assert np.array_equal(above, R.above_plane(pts, s["plane"])) and above.any() and (~above).any()
    on = np.array([[0.0, 0.0, 6.2], [0.0, 0.0, 6.25], [0.0, 0.0, 6.0]], np.float32)
    assert np.array_equal(CE.above_plane(dev(on), s["plane"]).cpu().numpy(), R.above_plane(on, s["plane"]))


@pytest.mark.parametrize("seed,extent,cap", [(5, 24.0, 4.0), (6, 240.0, 60.0)])
def test_compare_points_and_statistics_end_to_end(seed, extent, cap):
    from itermvs_amd import cloud_eval as CE
    s = R.make_scene(seed, n_gt=6000, n_pred=8000, extent=extent, cap=cap)
    bb, res, max_dist = s["bb"], s["res"], cap / 3.0
    order = np.random.default_rng(seed).permutation(s["pred"].shape[0])
    want = R.compare_points(s["pred"], s["gt"], s["obs_mask"], bb, res, s["plane"], 0.2, order, cap=cap)
    got = CE.compare_points(dev(s["pred"]), dev(s["gt"]), dev(s["obs_mask"]), bb, res, s["plane"], dst=0.2,
                            order=torch.from_numpy(order), cap=cap)
    assert np.array_equal(got["keep"].cpu().numpy(), want["keep"]) and got["n_reduced"] == int(want["keep"].sum())
    assert got["downsample_factor"] == s["pred"].shape[0] / want["keep"].sum()
    for k in ("Ddata", "Dstl", "DataInMask", "StlAbovePlane"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    st = CE.scan_statistics(got["Ddata"], got["Dstl"], got["DataInMask"], got["StlAbovePlane"], max_dist)
    ref = R.scan_statistics(want["Ddata"], want["Dstl"], want["DataInMask"], want["StlAbovePlane"], max_dist)
    print("statistics:", st, "reference:", ref)
    assert st["nData"] == ref["nData"] > 100 and st["nStl"] == ref["nStl"] > 100
    assert st["MedData"] == ref["MedData"] and st["MedStl"] == ref["MedStl"]
    for side in ("Data", "Stl"):
        n = ref["n" + side]
        bound = n * 2.0 ** -53 * max_dist          # n values below max_dist summed in another order, then divided by n
        print(f"{side}: mean differs by {abs(st['Mean' + side] - ref['Mean' + side]):.3e} (bound {bound:.3e}), "
              f"variance by {abs(st['Var' + side] - ref['Var' + side]):.3e} (bound {bound * 2 * max_dist:.3e})")
        assert abs(st["Mean" + side] - ref["Mean" + side]) <= bound
        assert abs(st["Var" + side] - ref["Var" + side]) <= bound * 2 * max_dist


# ---- the drivers -----------------------------------------------------------------------------------------------------------

def write_dtu_tree(root, scans, seed=0):
    """Points/stl/stl<N>_total.ply, ObsMask/ObsMask<N>_10.npz, ObsMask/Plane<N>.npz and predictions (the first scan under the
    script's name, the others as scan<N>.ply) -> {scan: scene}"""
    from itermvs_amd import fusion
    data, ply = os.path.join(root, "MVS Data"), os.path.join(root, "outputs")
    os.makedirs(os.path.join(data, "Points", "stl"))
    os.makedirs(os.path.join(data, "ObsMask"))
    os.makedirs(ply)
    scenes = {}
    for i, n in enumerate(scans):
        s = R.make_scene(seed + n, n_gt=3000, n_pred=4000, extent=240.0, cap=60.0)
        grey = np.full((s["gt"].shape[0], 3), 128, np.uint8)
        fusion.write_ply(os.path.join(data, "Points", "stl", "stl{:03d}_total.ply".format(n)), s["gt"], grey)
        np.savez(os.path.join(data, "ObsMask", "ObsMask{}_10.npz".format(n)), ObsMask=s["obs_mask"], BB=s["bb"], Res=s["res"])
        np.savez(os.path.join(data, "ObsMask", "Plane{}.npz".format(n)), P=s["plane"].reshape(4, 1))
        name = "itermvs{:03d}_l3.ply".format(n) if i == 0 else "scan{}.ply".format(n)
        fusion.write_ply(os.path.join(ply, name), s["pred"], np.zeros((s["pred"].shape[0], 3), np.uint8))
        scenes[n] = s
    return data, ply, scenes


def run_driver(*argv, timeout=900):
    return subprocess.run([sys.executable, os.path.join(ROOT, argv[0])] + [str(a) for a in argv[1:]], cwd=ROOT, capture_output=True,
                          text=True, timeout=timeout)


def test_dtu_eval_driver_two_scans(tmp_path):
    sys.path.insert(0, ROOT)
    import dtu_eval
    from itermvs_amd import cloud_eval as CE
    data, ply, scenes = write_dtu_tree(str(tmp_path), [1, 4])
    out = tmp_path / "results" / "dtu.json"
    r = run_driver("dtu_eval.py", "--data_path", data, "--ply_path", ply, "--scans", 1, 4, "--seed", 3, "--out", out)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert [s["scan"] for s in res["scans"]] == [1, 4] and res["seed"] == 3
    assert res["scans"][0]["file"].endswith("itermvs001_l3.ply") and res["scans"][1]["file"].endswith("scan4.ply")
    per = []
    for got, n in zip(res["scans"], (1, 4)):
        s = scenes[n]
        want = CE.evaluate_scan(data, ply, n, seed=3, device=DEV)
        for k in STAT_KEYS + ("n_pred", "n_reduced", "n_stl", "downsample_factor", "non_finite"):
            assert got[k] == want[k] or (isinstance(want[k], float) and math.isnan(want[k]) and math.isnan(got[k])), k
        assert set(got["seconds"]) >= {"read", "reduce_sort", "reduce_rounds", "data_to_stl", "stl_to_data", "mask_plane", "total"}
        # and the in-process result is the reference pipeline's for the same order
        order = CE.default_order(s["pred"].shape[0], 3).numpy()
        c = R.compare_points(s["pred"], s["gt"], s["obs_mask"], s["bb"], s["res"], s["plane"], 0.2, order)
        ref = R.scan_statistics(c["Ddata"], c["Dstl"], c["DataInMask"], c["StlAbovePlane"])
        assert all(want[k] == ref[k] for k in ("nData", "nStl", "MedData", "MedStl")) and want["n_reduced"] == int(c["keep"].sum())
        assert got["nData"] > 50 and got["nStl"] > 50 and math.isfinite(got["MeanData"]) and math.isfinite(got["MeanStl"])
        per.append(got)
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("final evaluation result on all scans: acc.: ")
    summ = dtu_eval.parse_final_line(lines[-1])
    assert res["summary"] == CE.summary(per)
    for k in ("acc", "comp", "overall"):
        assert abs(summ[k] - res["summary"][k]) <= 5e-7                       # %f prints six decimals
    assert sum(line.startswith("mean/median Data (acc.) ") for line in lines) == 2
    assert sum(line.startswith("mean/median Stl (comp.) ") for line in lines) == 2
    missing = run_driver("dtu_eval.py", "--data_path", data, "--ply_path", ply, "--scans", 9)
    assert missing.returncode != 0 and "itermvs009_l3.ply" in missing.stderr


def _plane_views(h, w, n_views=5):
    """a tilted plane 0.1 x - 0.05 y + z = 700 seen by cameras on an arc: per view (K, E, depth map)"""
    k = np.array([[1.2 * w, 0, w / 2 + 1.3], [0, 1.2 * w, h / 2 - 0.7], [0, 0, 1]], np.float32)
    normal, offset = np.array([0.1, -0.05, 1.0]), 700.0
    views = []
    for v in range(n_views):
        ang = np.deg2rad(6.0 * (v - n_views // 2))
        r = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        c = np.array([120.0 * np.sin(ang), 4.0 * v, 0.0])
        e = np.eye(4)
        e[:3, :3], e[:3, 3] = r, -r @ c
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        rays = np.linalg.inv(k.astype(np.float64)) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
        t = (offset - normal @ c) / (normal @ (r.T @ rays))
        views.append((k.copy(), e.astype(np.float32), t.reshape(h, w).astype(np.float32)))
    return views


def test_fusion_with_geo_mask_thres_4_then_dtu_eval(tmp_path):
    """the chain a user runs: eval.py's fusion stage with the reference's DTU threshold writes scan1.ply, dtu_eval.py scores
    it against a ground truth sampled from the same plane"""
    from PIL import Image
    sys.path.insert(0, ROOT)
    import eval as E
    from itermvs_amd import fusion
    from itermvs_amd.data_io import read_ply_xyz, save_pfm
    h, w = 64, 96
    scan, out = tmp_path / "data" / "scan1", tmp_path / "outputs" / "scan1"
    for d in (scan / "cams_1", scan / "images", out / "depth_est", out / "confidence"):
        d.mkdir(parents=True)
    lines = ["5"]
    for v, (k, e, d) in enumerate(_plane_views(h, w)):
        rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)                          # noqa: E731
        (scan / "cams_1" / "{:0>8}_cam.txt".format(v)).write_text(f"extrinsic\n{rows(e)}\n\nintrinsic\n{rows(k)}\n\n425 2.5\n")
        Image.fromarray(np.full((h, w, 3), 90, np.uint8)).save(str(scan / "images" / "{:0>8}.png".format(v)))
        save_pfm(str(out / "depth_est" / "{:0>8}.pfm".format(v)), d)
        save_pfm(str(out / "confidence" / "{:0>8}.pfm".format(v)), np.full_like(d, 0.9))
        srcs = [u for u in range(5) if u != v]
        lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} 1.0" for u in srcs)]
    (scan / "pair.txt").write_text("\n".join(lines) + "\n")
    common = ["--dataset", "folder", "--testpath", str(tmp_path / "data"), "--outdir", str(tmp_path / "outputs"), "--img_wh", str(w), str(h),
              "--filter", "--fuse_points", "device"]
    assert E.fuse_scans(E.build_parser().parse_args(common + ["--geo_mask_thres", "4"])) == 1
    cloud4 = read_ply_xyz(str(tmp_path / "outputs" / "scan1.ply"))
    strict = (tmp_path / "outputs" / "scan1.ply").read_bytes()
    assert E.fuse_scans(E.build_parser().parse_args(common)) == 1                                           # the default: 3, as before
    fusion.filter_depth(str(scan), str(out), str(tmp_path / "lib.ply"), 1.0, 0.01, 0.3, device=DEV, img_wh=(w, h), points="device")
    assert (tmp_path / "outputs" / "scan1.ply").read_bytes() == (tmp_path / "lib.ply").read_bytes()
    assert 1000 < cloud4.shape[0] < read_ply_xyz(str(tmp_path / "lib.ply")).shape[0]                        # 4 of 4 views is stricter
    (tmp_path / "outputs" / "scan1.ply").write_bytes(strict)
    # the ground truth: a 2 mm lattice on the plane; everything observable, everything above the table
    data = tmp_path / "MVS Data"
    (data / "Points" / "stl").mkdir(parents=True)
    (data / "ObsMask").mkdir()
    gx, gy = np.meshgrid(np.arange(-360, 360, 2.0), np.arange(-260, 260, 2.0), indexing="ij")
    gt = np.stack([gx.ravel(), gy.ravel(), 700.0 - 0.1 * gx.ravel() + 0.05 * gy.ravel()], 1).astype(np.float32)
    fusion.write_ply(str(data / "Points" / "stl" / "stl001_total.ply"), gt, np.zeros((gt.shape[0], 3), np.uint8))
    np.savez(str(data / "ObsMask" / "ObsMask1_10.npz"), ObsMask=np.ones((101, 76, 26), np.uint8),
             BB=np.array([[-400.0, -300.0, 600.0], [400.0, 300.0, 800.0]]), Res=8.0)
    np.savez(str(data / "ObsMask" / "Plane1.npz"), P=np.array([0.1, -0.05, 1.0, -650.0]))
    r = run_driver("dtu_eval.py", "--data_path", data, "--ply_path", tmp_path / "outputs", "--scans", 1, "--out", tmp_path / "r.json")
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads((tmp_path / "r.json").read_text())
    st = res["scans"][0]
    print("chain:", {k: st[k] for k in STAT_KEYS}, res["summary"])
    assert st["n_pred"] == cloud4.shape[0] and st["nData"] > 1000 and st["nStl"] > 1000
    assert 0.0 < st["MeanData"] < 1.5 and 0.0 < st["MeanStl"] < 10.0          # a 2 mm lattice: nobody is farther than sqrt(2) from it
    assert math.isfinite(res["summary"]["overall"]) and res["summary"]["overall"] == (st["MeanData"] + st["MeanStl"]) / 2

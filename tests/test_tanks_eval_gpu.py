"""The Tanks and Temples evaluator on the MI355X: every pass of csrc/cloud_register.hip through the ctypes library against the
numpy yardstick (tests/tanks_eval_reference.py), the ICP loop, and the driver end to end as a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tanks_eval_reference as R
from conftest import ROOT
from itermvs_amd import cloud_grid as CG, cloud_register as CR, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * k + (1 - np.cos(r)) * (k @ k)


def similarity(axis, deg, scale, shift):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * rotation(axis, deg), shift
    return T


def gpu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


CONCAVE = np.array([[0.0, 0.0], [2.0, 0.25], [4.0, 0.0], [3.0, 2.0], [4.0, 4.0], [2.0, 3.0], [0.5, 4.0]])    # 7 vertices, two notches


# ---- crop ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_crop_equals_the_restatement(axis):
    u, v = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    gen = np.random.default_rng(10 + axis)
    poly = np.zeros((7, 3))
    poly[:, u], poly[:, v], poly[:, axis] = CONCAVE[:, 0], CONCAVE[:, 1], gen.normal(0, 1, 7)      # the w column must be ignored
    T = similarity([1, -2, 0.5], 7.0, 1.25, [0.3, -0.2, 0.1])
    inv = np.linalg.inv(T)
    c = gen.uniform(-1.0, 5.0, (5000, 3))
    c[:, axis] = gen.uniform(-0.5, 1.5, 5000)
    c[:40, v] = np.repeat(CONCAVE[:, 1], 6)[:40]                                                   # at the height of vertices
    pts = (c @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    pts[100], pts[101], pts[102] = [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]
    for T_case, lo, hi in ((T, 0.0, 1.0), (np.eye(4), -0.25, 0.5)):
        p = pts.copy()
        if T_case is not T:                                                                        # identity: points exactly on both bounds
            p = c.astype(np.float32)
            p[200:230, axis], p[230:260, axis] = np.float32(lo), np.float32(hi)
            p[100] = [np.nan, 0, 0]
        want = R.crop_mask(p, T_case, axis, lo, hi, poly)
        got = ops.cloud_crop(gpu(p), T_case, axis, lo, hi, poly)
        assert 500 < int(want.sum()) < 4500
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        if T_case is not T:
            assert want[200:260].sum() > 10                                                        # the inclusive bounds are exercised
    big = np.zeros((1024, 3))
    ang = np.linspace(0, 2 * np.pi, 1024, endpoint=False)
    big[:, u], big[:, v] = 2 + 2 * np.cos(ang) * (1 + 0.3 * np.sin(9 * ang)), 2 + 2 * np.sin(ang) * (1 + 0.3 * np.sin(9 * ang))
    p = c.astype(np.float32)
    assert torch.equal(ops.cloud_crop(gpu(p), np.eye(4), axis, 0.0, 1.0, big).cpu(),
                       torch.from_numpy(R.crop_mask(p, np.eye(4), axis, 0.0, 1.0, big)))          # every upload chunk, all of the LDS


# ---- voxel mean ------------------------------------------------------------------------------------------------------------

def test_voxel_mean_equals_the_restatement_bit_for_bit():
    gen = np.random.default_rng(3)
    voxel = 0.25
    pts = gen.uniform(0.0, 3.0, (20000, 3)).astype(np.float32)                                    # 12 voxels per axis (+1 from the half-voxel origin)
    pts[0] = [0.0, 0.0, 0.0]                                                                       # fixes min_bound: faces at k * 0.25 - 0.125
    pts[1] = [3.0, 3.0, 3.0]
    pts[2:3002] = (np.array([0.9, 1.4, 1.9]) + gen.uniform(0.0, 0.2, (3000, 3))).astype(np.float32)   # inside one voxel ([0.875, 1.125) ...): 3 000 points, the wave path
    pts[3002:3072] = (np.array([1.9, 0.4, 0.4]) + gen.uniform(0.0, 0.2, (70, 3))).astype(np.float32)  # inside one voxel: 70+ points, just past the bound
    faces = np.arange(0, 12) * 0.25 + 0.125
    pts[4000:4012, 0], pts[4012:4024, 1], pts[4024:4036, 2] = faces, faces, faces                  # exactly on voxel faces
    pts[5000] = [np.nan, 1, 1]
    want = R.voxel_mean(pts, voxel)
    keys, _ = R.voxel_keys(pts[np.isfinite(pts).all(1)], voxel)
    counts = np.unique(keys, return_counts=True)[1]
    assert counts.max() >= 3000 and ((counts > 64) & (counts < 200)).any() and (counts <= 64).any()
    got = CR.voxel_down_sample(gpu(pts), voxel)
    again = CR.voxel_down_sample(gpu(pts), voxel)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                            # the same bytes on two runs
    out_keys, _ = R.voxel_keys(np.vstack([got.cpu().numpy(), pts[:2]]), voxel)                    # same min_bound / extent as the input
    assert (np.diff(out_keys[:-2]) > 0).all()                                                      # ascending voxel key
    one = np.array([[0.3, -0.7, 11.0]], dtype=np.float32)
    assert np.array_equal(CR.voxel_down_sample(gpu(one), voxel).cpu().numpy(), one)
    blob = (np.array([5.0, 5.0, 5.0]) + gen.uniform(0, 0.1, (777, 3))).astype(np.float32)
    got = CR.voxel_down_sample(gpu(blob), 1.0).cpu().numpy()
    assert got.shape == (1, 3) and np.array_equal(got.view(np.uint32), R.voxel_mean(blob, 1.0).view(np.uint32))


# ---- nearest-neighbour index -----------------------------------------------------------------------------------------------

def nn_case():
    gen = np.random.default_rng(4)
    t = gen.uniform(0.0, 1.0, (6000, 3)).astype(np.float32)
    t[3000:3200] = t[100:300]                                                                      # duplicated targets: ties
    t[5990] = [0.0, 0.0, 2.0]
    q = gen.uniform(0.0, 1.0, (4000, 3)).astype(np.float32)
    q[:150] = t[100:250]                                                                           # d2 = 0 on a duplicated target
    q[150:200] = gen.uniform(3.0, 9.0, (50, 3)).astype(np.float32)                                 # far outside the grid
    q[200:220] = gen.uniform(-9.0, -3.0, (20, 3)).astype(np.float32)
    q[220] = [np.nan, 0.5, 0.5]
    return q, t


@pytest.mark.parametrize("with_T", [False, True])
def test_nn_index_equals_brute_force(with_T):
    q, t = nn_case()
    T = similarity([0.2, 1, -0.4], 5.0, 1.02, [0.01, -0.02, 0.015]) if with_T else np.eye(4)
    max_dist = 0.036                                                                               # about a third stay unmatched
    if with_T:
        inv = np.linalg.inv(T)
        q = (q.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    want_idx, want_d2 = R.nn_index(R.apply_transform(T, q), t, max_dist)
    unmatched = float((want_idx < 0).mean())
    assert 0.28 < unmatched < 0.40, unmatched
    for edge in (max_dist / 8, max_dist, 0.3):                                                     # many rings, one ring, fat cells
        tg = CR.build_target_grid(gpu(t), edge)
        idx, d2 = ops.cloud_nn_index(gpu(q), T, tg.sorted, tg.keys, tg.perm, tg.grid, max_dist, CG.max_ring(max_dist, edge))
        assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)), edge
        assert np.array_equal(d2.cpu().numpy().view(np.uint64), want_d2.view(np.uint64)), edge
    if not with_T:
        assert (want_idx[:150] == np.arange(100, 250)).all()                                       # the lower of the two duplicates


def test_nn_index_bound_is_exclusive_and_empty_targets():
    t = np.array([[0.0, 0.0, 0.0], [4.0, 4.0, 4.0]], dtype=np.float32)
    q = np.array([[0.375, 0.5, 0.0], [0.375, 0.5, 2.0 ** -20]], dtype=np.float32)                  # exactly 0.625 away, and a hair more
    tg = CR.build_target_grid(gpu(t), 0.25)
    for max_dist, want in ((0.625, [-1, -1]), (0.6250001, [0, 0]), (0.62, [-1, -1])):
        idx, d2 = ops.cloud_nn_index(gpu(q), np.eye(4), tg.sorted, tg.keys, tg.perm, tg.grid, max_dist, CG.max_ring(max_dist, 0.25))
        assert idx.tolist() == want and R.nn_index(q.astype(np.float64), t, max_dist)[0].tolist() == want
        assert d2[0].item() == (0.390625 if want[0] == 0 else float("inf"))
    empty = CR.build_target_grid(torch.zeros((0, 3), device=DEV), 0.25)
    idx, d2 = ops.cloud_nn_index(gpu(q), np.eye(4), empty.sorted, empty.keys, empty.perm, empty.grid, 1.0, 5)
    assert idx.tolist() == [-1, -1] and torch.isinf(d2).all()


# ---- the sums --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 50000])
def test_umeyama_sums_within_the_summation_bound(n):
    """counts exact; every other sum within n * 2^-53 * sum |terms| of the restatement (any order of n additions); the same bytes
    on two runs.  2048 is one workgroup's slice."""
    gen = np.random.default_rng(n)
    q = gen.normal(0, 1, (n, 3)).astype(np.float32)
    target = gen.normal(0.5, 2, (max(n // 2, 3), 3)).astype(np.float32)
    idx = gen.integers(0, len(target), n)
    idx[gen.random(n) < 0.3] = -1
    if n == 1:
        idx[:] = 0
    d2 = gen.random(n)
    T = similarity([1, 1, 0], 12.0, 0.9, [0.1, 0.2, -0.3])
    terms = R.umeyama_terms(q, T, idx, d2, target)
    want = R.ordered_sum(terms)
    args = (gpu(q), T, gpu(idx, torch.int64), gpu(d2, torch.float64), gpu(target))
    got = ops.cloud_umeyama_sums(*args).cpu().numpy()
    again = ops.cloud_umeyama_sums(*args).cpu().numpy()
    assert got[0] == float((idx >= 0).sum()) == want[0]
    bound = n * 2.0 ** -53 * np.abs(terms).sum(0)
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    bad = idx.copy()
    bad[0] = len(target) + 7                                                                       # not an index into the targets: skipped
    skipped = ops.cloud_umeyama_sums(args[0], T, gpu(bad, torch.int64), args[3], args[4]).cpu().numpy()
    assert skipped[0] == float((idx[1:] >= 0).sum())


# ---- ICP -------------------------------------------------------------------------------------------------------------------

def bumpy(gen, n, extent=1.0):
    xy = gen.uniform(0.0, extent, (n, 2))
    z = 0.08 * np.sin(7 * xy[:, 0]) * np.cos(5 * xy[:, 1]) + 0.05 * np.sin(13 * xy[:, 1] + 1.0) + 0.03 * np.cos(17 * xy[:, 0])
    return np.column_stack([xy, z])


def test_icp_equals_the_restatement():
    """target: 8 000 points of a bumpy surface; source: 6 000 of them moved by the inverse of a known similarity (2 degrees,
    scale 1.01, a shift of half of tau = 0.01) plus 10 % outliers.  The tolerance is measured here, not fixed: delta =
    the largest element difference of the restatement's final T between adding the correspondences forwards and reversed;
    the GPU's reduction tree is a third order and ICP carries round-off through at most 20 iterations, so it gets 10 * delta.
    Measured on the CPU when this test was written: delta = 6.1e-15, allowance 6.1e-14, 10 updates in both orders (a delta of 0
    would make the allowance one ulp of the largest element instead)."""
    gen = np.random.default_rng(8)
    tau = 0.01
    target = bumpy(gen, 8000).astype(np.float32)
    S = similarity([0.3, -0.5, 1.0], 2.0, 1.01, [0.5 * tau, -0.5 * tau, 0.25 * tau])
    inv = np.linalg.inv(S)
    src = target[gen.permutation(8000)[:6000]].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
    src[gen.permutation(6000)[:600]] += gen.normal(0, 0.3, (600, 3))
    src = src.astype(np.float32)
    max_dist = 8 * tau
    fwd = R.icp(src, target, np.eye(4), max_dist, 20)
    rev = R.icp(src, target, np.eye(4), max_dist, 20, reverse=True)
    delta = float(np.abs(fwd[0] - rev[0]).max())
    allow = 10 * delta if delta > 0 else float(np.spacing(np.abs(fwd[0]).max()))
    print("icp: delta %.3e allowance %.3e iterations %d fitness %.4f rmse %.3e" % (delta, allow, fwd[3], fwd[1], fwd[2]))
    assert fwd[3] == rev[3] and 2 <= fwd[3] <= 20
    assert np.abs(fwd[0] - S).max() < 1e-3                                                         # it does recover the similarity
    T, fitness, rmse, it = CR.icp(gpu(src), CR.build_target_grid(gpu(target), max_dist / 8), None, max_dist, 20)
    print("icp: gpu max |T - restatement| %.3e" % np.abs(T - fwd[0]).max())
    assert it == fwd[3]
    assert np.abs(T - fwd[0]).max() <= allow
    assert abs(fitness - fwd[1]) < 1e-12 and abs(rmse - fwd[2]) <= 1e-9 * fwd[2]


# ---- the driver end to end -------------------------------------------------------------------------------------------------

TAU = 0.04


def bumpy_sphere(gen, n):
    """points of a closed bumpy surface around (0.5, 0.5, 0): a closed shape pins the scale, which a near-planar patch does not
    (nearest-neighbour matches slide along a plane, and any outlier then rewards shrinking)"""
    d = gen.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 0.45 * (1 + 0.08 * np.sin(5 * np.arctan2(d[:, 1], d[:, 0])) * np.cos(4 * np.arccos(np.clip(d[:, 2], -1, 1))))
    return d * r[:, None] + np.array([0.5, 0.5, 0.0]), d


def write_scene(folder, seed):
    from itermvs_amd.fusion import write_ply
    gen = np.random.default_rng(seed)
    gt64, _ = bumpy_sphere(gen, 30000)
    gt = gt64.astype(np.float32)
    poly = [[-0.05, -0.05, 0.0], [0.5, -0.02, 0.0], [1.05, -0.05, 0.0], [1.02, 0.5, 0.0], [1.05, 1.05, 0.0], [0.5, 1.02, 0.0], [-0.05, 1.05, 0.0]]
    vol = {"axis_max": 0.75, "axis_min": -0.75, "bounding_polygon": poly, "class_name": "SelectionPolygonVolume",
           "orthogonal_axis": "Z", "version_major": 1, "version_minor": 0}
    covered = gt64[gt64[:, 0] < np.quantile(gt64[:, 0], 0.7)]                                      # 70 % of the scene
    n_in = int(0.9 * len(covered))
    pred = covered[gen.permutation(len(covered))[:n_in]] + gen.normal(0, 0.1 * TAU, (n_in, 3))
    n_out = int(0.15 * n_in / 0.85)                                                                # 15 % of the prediction
    base, normal = bumpy_sphere(gen, n_out)
    outliers = base + normal * (gen.uniform(2.5 * TAU, 4 * TAU, n_out) * gen.choice([-1.0, 1.0], n_out))[:, None]
    pred = np.vstack([pred, outliers[outliers[:, 0] < np.quantile(gt64[:, 0], 0.7)], outliers[outliers[:, 0] >= np.quantile(gt64[:, 0], 0.7)]])
    user_to_ref = similarity([0.2, 1.0, 0.1], 30.0, 2.5, [1.0, -2.0, 0.5])                        # the user's frame -> the COLMAP frame
    gt_trans_true = similarity([1.0, 0.1, -0.3], 10.0, 0.8, [0.2, 0.1, -0.4])                     # the COLMAP frame -> the scan's frame
    gt_trans = similarity([0.1, 0.3, 1.0], 3.0, 1.03, [0.4 * TAU, -0.4 * TAU, 0.3 * TAU]) @ gt_trans_true    # as published: slightly off
    inv = np.linalg.inv(gt_trans_true @ user_to_ref)
    pred_user = (pred @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    grey = np.full((1, 3), 128, dtype=np.uint8)
    write_ply(os.path.join(folder, "X.ply"), gt, np.repeat(grey, len(gt), 0))
    os.makedirs(os.path.join(folder, "out"), exist_ok=True)
    write_ply(os.path.join(folder, "out", "X.ply"), pred_user, np.repeat(grey, len(pred_user), 0))
    with open(os.path.join(folder, "X.json"), "w") as f:
        json.dump(vol, f)
    np.savetxt(os.path.join(folder, "X_trans.txt"), gt_trans, fmt="%.17g")
    cams = np.tile(np.eye(4), (15, 1, 1))
    cams[:, :3, 3] = gen.normal(0, 3, (15, 3))                                                     # reference log: COLMAP frame
    user = cams.copy()
    iu = np.linalg.inv(user_to_ref)
    user[:, :3, 3] = cams[:, :3, 3] @ iu[:3, :3].T + iu[:3, 3]
    for name, log in (("X_COLMAP_SfM.log", cams), ("user.log", user)):
        with open(os.path.join(folder, name), "w") as f:
            for i, m in enumerate(log):
                f.write("%d %d %d\n" % (i, i, i + 1))
                for row in m:
                    f.write(" ".join("%.17g" % x for x in row) + "\n")


def run_driver(folder, scenes, extra):
    out = os.path.join(folder, "res%d.json" % len(extra))
    cmd = [sys.executable, os.path.join(ROOT, "tanks_eval.py"), "--scene"] + scenes + ["--gt_dir", folder, "--ply_path",
           os.path.join(folder, "out"), "--traj_path", os.path.join(folder, "user.log"), "--tau", str(TAU), "--out", out] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.count("X: precision") == len(scenes) and "f-score" in p.stdout
    assert ("mean over %d scenes" % len(scenes) in p.stdout) == (len(scenes) > 1)
    with open(out) as f:
        return json.load(f)


def reference_scene(folder, refine):
    from itermvs_amd.data_io import read_ply_xyz
    pred, gt = read_ply_xyz(os.path.join(folder, "out", "X.ply")), read_ply_xyz(os.path.join(folder, "X.ply"))
    init = CR.trajectory_alignment(CR.read_trajectory_log(os.path.join(folder, "user.log")),
                                   CR.read_trajectory_log(os.path.join(folder, "X_COLMAP_SfM.log")),
                                   np.loadtxt(os.path.join(folder, "X_trans.txt")).reshape(4, 4))
    return R.evaluate_scene(pred, gt, R.read_volume(os.path.join(folder, "X.json")), init, TAU, refine)


def margin_ok(ref):
    """no distance within 1e-9 * tau of tau or of a bin edge: a condition on the input under the restatement's T"""
    marks = np.sort(np.concatenate([[TAU], ref["edges"]]))
    for d in (ref["d_pred"], ref["d_gt"]):
        d = d[d < R.PLOT_STRETCH * TAU]                                                             # capped distances sit on the last edge by construction
        pos = np.clip(np.searchsorted(marks, d), 1, len(marks) - 1)
        if len(d) and np.minimum(np.abs(d - marks[pos - 1]), np.abs(d - marks[pos])).min() <= 1e-9 * TAU:
            return False
    return True


def test_driver_end_to_end_against_the_restatement(tmp_path):
    """a synthetic scene of 30 000 scan points; the prediction covers 70 % of it (x below the 0.7 quantile), carries 15 % outliers
    and lives in a similarity-transformed frame; the published alignment is off by 3 degrees, 3 % of scale and 0.4 tau, which
    the three ICP rounds repair.  Without refinement (run with the scene named twice, which also exercises the averaged line)
    every figure equals the restatement's exactly.  With refinement the iteration counts are equal, the transform agrees within
    1e-9 tau / 2 -- a point of this scene (coordinates below 1) then moves by less than 1e-9 tau, the margin that margin_ok()
    asserts around tau and every bin edge -- and so the counts, both curves, precision and recall are equal.
    The restatement on the CPU: without refinement P 0.6859 R 0.7340 F 0.7091 (9 697 / 7 877 points), with it P 0.6918 R 0.7422
    F 0.7161 (9 296 / 7 877 points, 11 / 10 / 15 updates), no distance within 1e-9 tau of tau or a bin edge."""
    folder = str(tmp_path)
    write_scene(folder, seed=21)
    both = run_driver(folder, ["X", "X"], ["--no_refine"])
    plain, refined = both["scenes"][0], run_driver(folder, ["X"], [])["scenes"][0]
    assert {k: v for k, v in both["scenes"][1].items() if k != "seconds"} == {k: v for k, v in plain.items() if k != "seconds"}
    assert both["mean"] == {"scenes": 2, "precision": plain["precision"], "recall": plain["recall"], "fscore": plain["fscore"]}
    ref_plain, ref_refined = reference_scene(folder, False), reference_scene(folder, True)
    for k in ("n_pred", "n_gt", "n_pred_below", "n_gt_below", "precision", "recall", "fscore"):
        assert plain[k] == ref_plain[k], k
    assert plain["curve_pred"] == ref_plain["curve_pred"].tolist() and plain["curve_gt"] == ref_plain["curve_gt"].tolist()
    t_diff = float(np.abs(np.array(refined["transform"]) - ref_refined["transform"]).max())
    iterations = [r["iterations"] for r in refined["rounds"]]
    print("e2e: no_refine P %.4f R %.4f F %.4f | refined P %.4f R %.4f F %.4f | max |T - restatement| %.3e | iterations %s vs %s" % (
        plain["precision"], plain["recall"], plain["fscore"], refined["precision"], refined["recall"], refined["fscore"], t_diff,
        iterations, ref_refined["iterations"]))
    assert margin_ok(ref_refined)
    assert iterations == ref_refined["iterations"]
    assert t_diff <= 1e-9 * TAU / 2
    for k in ("n_pred", "n_gt", "n_pred_below", "n_gt_below", "precision", "recall", "fscore"):
        assert refined[k] == ref_refined[k], k
    assert refined["curve_pred"] == ref_refined["curve_pred"].tolist() and refined["curve_gt"] == ref_refined["curve_gt"].tolist()
    assert refined["precision"] == refined["curve_pred"][99] and refined["recall"] == refined["curve_gt"][99]      # edge 100 is tau to an ulp; nothing lies that close
    assert refined["fscore"] >= plain["fscore"]
    assert abs(refined["recall"] - 0.7) < 0.05

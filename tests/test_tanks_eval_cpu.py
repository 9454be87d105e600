"""The Tanks and Temples evaluator without a GPU: the numpy yardstick (tests/tanks_eval_reference.py) and the host code against
analytic cases, the file readers, the validation codes of the new entry points and their declarations."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tanks_eval_reference as R
from conftest import ROOT
from itermvs_amd import cloud_register as CR

NEW_SYMBOLS = ("itermvs_cloud_crop", "itermvs_cloud_voxel_heads", "itermvs_cloud_voxel_mean", "itermvs_cloud_nn_index",
               "itermvs_cloud_umeyama_groups", "itermvs_cloud_umeyama_sums")


# ---- crop ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_crop_square_prism_faces_and_vertex_height(axis):
    """unit square [0,1]^2 in (u, v), axis range [-1, 2] (inclusive).  The crossing rule counts an edge for a_v > c_v XOR
    b_v > c_v, so v = 0 (the lower face, also the height of two vertices) is inside and v = 1 is outside; u = 0 is inside
    (c_u < 1 only) and u = 1 outside."""
    u, v = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    sq = np.zeros((4, 3))
    sq[:, u], sq[:, v] = [0, 1, 1, 0], [0, 0, 1, 1]
    cases = [((0.5, 0.5, 0.0), 1), ((0.5, 0.5, -1.0), 1), ((0.5, 0.5, 2.0), 1), ((0.5, 0.5, 2.5), 0), ((0.5, 0.5, -1.5), 0),
             ((0.0, 0.5, 0.0), 1), ((1.0, 0.5, 0.0), 0), ((0.5, 0.0, 0.0), 1), ((0.5, 1.0, 0.0), 0), ((-0.25, 0.5, 0.0), 0),
             ((1.25, 0.5, 0.0), 0), ((0.5, -0.25, 0.0), 0), ((0.5, 1.25, 0.0), 0), ((-0.5, 0.0, 0.0), 0), ((-0.5, 1.0, 0.0), 0),
             ((0.0, 0.0, 0.0), 1), ((1.0, 1.0, 0.0), 0), ((float("nan"), 0.5, 0.0), 0), ((0.5, float("inf"), 0.0), 0)]
    pts = np.zeros((len(cases), 3), dtype=np.float32)
    for i, ((cu, cv, cw), _) in enumerate(cases):
        pts[i, u], pts[i, v], pts[i, axis] = cu, cv, cw
    got = R.crop_mask(pts, np.eye(4), axis, -1.0, 2.0, sq)
    assert got.tolist() == [want for _, want in cases]
    shift = np.eye(4)
    shift[u, 3] = 10.0                                                                           # T moves everything out of the square
    assert R.crop_mask(pts, shift, axis, -1.0, 2.0, sq).sum() == 0


# ---- voxel mean ------------------------------------------------------------------------------------------------------------

def test_voxel_mean_points_on_faces():
    """voxel 0.5, min_bound 0 -> origin -0.25: faces at -0.25, 0.25, 0.75 (exact in binary).  A point on a face belongs to
    the voxel above it (floor)."""
    pts = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0], [0.75, 0.0, 0.0], [0.0, 0.25, 0.0]],
                   dtype=np.float32)
    out = R.voxel_mean(pts, 0.5)
    want = np.array([[0.0625, 0.0, 0.0], [0.0, 0.25, 0.0], [0.375, 0.0, 0.0], [0.75, 0.0, 0.0]], dtype=np.float32)   # key order: x, then y
    assert out.tolist() == want.tolist()
    assert R.voxel_mean(pts[:1], 0.5).tolist() == pts[:1].tolist()
    assert R.voxel_mean(np.array([[np.nan, 0, 0]], dtype=np.float32), 0.5).shape == (0, 3)


# ---- Umeyama ---------------------------------------------------------------------------------------------------------------

def _rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * k + (1 - np.cos(r)) * (k @ k)


def test_umeyama_recovers_a_known_similarity():
    """exact correspondences t = s R p + b.  The covariance of p has condition number < 10 (unit-variance axes scaled by 1,
    1.5, 2.5: eigenvalue ratio about 6.25) and the centroid lies within one standard deviation of the origin, so forming the
    covariance from raw sums costs less than a digit: agreement to 1e-12 relative is fp64 SVD round-off."""
    gen = np.random.default_rng(5)
    p = gen.normal(0, 1, (400, 3)) * np.array([1.0, 1.5, 2.5]) + np.array([0.3, -0.2, 0.5])
    assert np.linalg.cond(np.cov(p.T)) < 10
    rot, s, b = _rotation([1, 2, 3], 25.0), 1.7, np.array([0.4, -1.1, 2.0])
    t = s * p @ rot.T + b
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = s * rot, b
    for fit in (CR.umeyama, R.umeyama):
        got = fit(_sums(p, t), True)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        rigid = fit(_sums(p, t), False)[:3, :3]
        assert np.abs(rigid @ rigid.T - np.eye(3)).max() < 1e-12 and np.abs(rigid - rot).max() < 1e-12
    assert np.abs(R.umeyama_from_points(p, t) - want).max() <= 1e-12 * np.abs(want).max()


def test_umeyama_reflection_case_returns_a_proper_rotation():
    """mirrored data (t = s R M p + b, M = diag(1, 1, -1)): det(U) det(V) < 0, and S = diag(1, 1, -1) must turn the answer into
    the best PROPER rotation: determinant > 0, orthonormal up to the scale, scale = (d1 + d2 - d3) / var_p, and a residual no
    larger than that of nearby proper rotations."""
    gen = np.random.default_rng(6)
    p = gen.normal(0, 1, (400, 3)) * np.array([1.0, 1.5, 2.5]) + np.array([0.3, -0.2, 0.5])
    rot, s, b = _rotation([1, 2, 3], 25.0), 1.7, np.array([0.4, -1.1, 2.0])
    t = s * p @ (rot @ np.diag([1.0, 1.0, -1.0])).T + b
    sums = _sums(p, t)
    got = CR.umeyama(sums, True)
    assert np.array_equal(got, R.umeyama(sums, True))
    m = got[:3, :3]
    scale = np.cbrt(np.linalg.det(m))
    assert scale > 0 and np.abs((m / scale) @ (m / scale).T - np.eye(3)).max() < 1e-12
    n = sums[0]
    cov = sums[7:16].reshape(3, 3) / n - np.outer(sums[4:7] / n, sums[1:4] / n)
    d = np.linalg.svd(cov, compute_uv=False)
    var_p = sums[16] / n - (sums[1:4] / n) @ (sums[1:4] / n)
    assert abs(scale - (d[0] + d[1] - d[2]) / var_p) <= 1e-12 * scale
    residual = lambda mat: np.linalg.norm((p - p.mean(0)) @ mat.T - (t - t.mean(0)))            # noqa: E731
    for ax in ([1, 0, 0], [0, 1, 0], [0, 0, 1]):
        for deg in (-2.0, 2.0):
            assert residual(m) <= residual(m @ _rotation(ax, deg))


def _sums(p, t):
    s = np.zeros(18)
    s[0], s[1:4], s[4:7] = len(p), p.sum(0), t.sum(0)
    s[7:16] = (t[:, :, None] * p[:, None, :]).sum(0).reshape(-1)
    s[16] = (p * p).sum()
    return s


def test_trajectory_alignment_from_camera_centres():
    gen = np.random.default_rng(2)
    ref = np.tile(np.eye(4), (12, 1, 1))
    ref[:, :3, 3] = gen.normal(0, 2, (12, 3))
    sim = np.eye(4)
    sim[:3, :3], sim[:3, 3] = 0.5 * _rotation([0, 1, 1], 40.0), [1.0, 2.0, 3.0]
    user = ref.copy()
    user[:, :3, 3] = (ref[:, :3, 3] - sim[:3, 3]) @ np.linalg.inv(sim[:3, :3]).T               # ref = sim * user
    gt_trans = np.eye(4)
    gt_trans[:3, 3] = [5.0, 0.0, -1.0]
    got = CR.trajectory_alignment(user, ref, gt_trans)
    assert np.abs(got - gt_trans @ sim).max() < 1e-12 * 5
    assert np.array_equal(CR.trajectory_alignment(None, ref, gt_trans), gt_trans)
    with pytest.raises(ValueError, match="equal counts"):
        CR.trajectory_alignment(user[:5], ref, gt_trans)


# ---- the restatement's search ----------------------------------------------------------------------------------------------

def test_nn_index_ties_bound_and_prefilter():
    t = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=np.float32)
    q = np.array([[0.375, 0.5, 0.0], [0.9, 0, 0], [0.5, 0, 0], [5, 5, 5], [np.nan, 0, 0]], dtype=np.float64)
    idx, d2 = R.nn_index(q, t, 0.625)
    assert idx.tolist() == [-1, 1, 0, -1, -1]                       # exactly max_dist away: no match; ties: the lowest index
    assert d2[1] == (0.9 - 1.0) ** 2 and d2[2] == 0.25 and np.isinf(d2[[0, 3, 4]]).all()
    assert R.nn_index(q, t, 0.6251)[0][0] == 0
    gen = np.random.default_rng(0)
    tt, qq = gen.random((500, 3)).astype(np.float32), gen.random((300, 3))
    full = ((qq[:, None, :] - tt[None].astype(np.float64)) ** 2)
    dd = (full[..., 0] + full[..., 1]) + full[..., 2]
    idx, d2 = R.nn_index(qq, tt, 0.08)
    hit = dd.min(1) < 0.08 * 0.08
    assert np.array_equal(idx >= 0, hit) and np.array_equal(idx[hit], dd.argmin(1)[hit]) and np.array_equal(d2[hit], dd.min(1)[hit])


# ---- readers ---------------------------------------------------------------------------------------------------------------

def test_readers_round_trip(tmp_path):
    vol = {"axis_max": 2.5, "axis_min": -1.25, "bounding_polygon": [[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.5, 0.0, 2.0]],
           "class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "version_major": 1, "version_minor": 0}
    (tmp_path / "X.json").write_text(json.dumps(vol))
    v = CR.read_selection_volume(str(tmp_path / "X.json"))
    assert (v.axis, v.axis_min, v.axis_max) == (1, -1.25, 2.5) and v.polygon.tolist() == vol["bounding_polygon"]
    ref = R.read_volume(str(tmp_path / "X.json"))
    assert ref["axis"] == 1 and ref["polygon"].tolist() == vol["bounding_polygon"]
    (tmp_path / "bad.json").write_text(json.dumps(dict(vol, orthogonal_axis="W")))
    with pytest.raises(ValueError, match="orthogonal_axis"):
        CR.read_selection_volume(str(tmp_path / "bad.json"))
    mats = np.random.default_rng(1).normal(0, 3, (3, 4, 4))
    with open(tmp_path / "t.log", "w") as f:
        for i, m in enumerate(mats):
            f.write("%d %d %d\n" % (i, i, i + 1))
            for row in m:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
    got = CR.read_trajectory_log(str(tmp_path / "t.log"))
    assert got.shape == (3, 4, 4) and np.array_equal(got, mats)
    (tmp_path / "short.log").write_text("0 0 1\n1 0 0 0\n")
    with pytest.raises(ValueError, match="records"):
        CR.read_trajectory_log(str(tmp_path / "short.log"))
    assert CR.uniform_stride(16_000_000) == 1 and CR.uniform_stride(40_000_000) == 2 and CR.uniform_stride(24_000_001) == 2
    assert CR.uniform_down_sample(torch.arange(30.0).reshape(10, 3), 4)[:, 0].tolist() == [0.0, 12.0, 24.0]
    assert set(CR.SCENE_TAU) == {"Barn", "Caterpillar", "Church", "Courthouse", "Ignatius", "Meetingroom", "Truck"}


# ---- validation before any launch ------------------------------------------------------------------------------------------

def test_register_entry_points_validate_before_touching_the_gpu():
    from itermvs_amd import _lib, ops
    lib = _lib.load()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    eye = (C.c_double * 16)(*np.eye(4).reshape(-1))
    nan_t = (C.c_double * 16)(*([float("nan")] + [0.0] * 15))
    poly = (C.c_double * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0)
    NULL, DIMS = -1, -2
    crop = lambda **k: lib.itermvs_cloud_crop(*[k.get(n, d) for n, d in (                        # noqa: E731
        ("xyz", a), ("n", 4), ("T", eye), ("axis", 2), ("lo", 0.0), ("hi", 1.0), ("poly", poly), ("n_poly", 3), ("ws", a), ("out", a),
        ("stream", None))])
    for name in ("xyz", "T", "poly", "ws", "out"):
        assert crop(**{name: None}) == NULL, name
    for bad in (dict(n=0), dict(n=1 << 31), dict(axis=3), dict(axis=-1), dict(n_poly=2), dict(n_poly=1025), dict(T=nan_t),
                dict(lo=float("nan")), dict(poly=(C.c_double * 9)(0, 0, 0, float("inf"), 0, 0, 0, 1, 0))):
        assert crop(**bad) == DIMS, bad
    assert lib.itermvs_cloud_voxel_heads(None, 4, a, None) == NULL
    assert lib.itermvs_cloud_voxel_heads(a, 0, a, None) == DIMS
    assert lib.itermvs_cloud_voxel_mean(a, a, None, 4, 2, a, None) == NULL
    for n, n_out in ((0, 1), (4, 0), (4, 5), (1 << 31, 1)):
        assert lib.itermvs_cloud_voxel_mean(a, a, a, n, n_out, a, None) == DIMS
    nn = lambda **k: lib.itermvs_cloud_nn_index(*[k.get(n, d) for n, d in (                       # noqa: E731
        ("q", a), ("nq", 4), ("T", eye), ("t", a), ("keys", a), ("perm", a), ("nt", 4), ("ox", 0.0), ("oy", 0.0), ("oz", 0.0),
        ("nx", 4), ("ny", 4), ("nz", 4), ("edge", 1.0), ("max_dist", 1.0), ("rings", 3), ("idx", a), ("d2", a), ("stream", None))])
    for name in ("q", "T", "t", "keys", "perm", "idx", "d2"):
        assert nn(**{name: None}) == NULL, name
    for bad in (dict(nq=0), dict(nt=-1), dict(max_dist=0.0), dict(max_dist=float("inf")), dict(rings=0), dict(rings=(1 << 21) + 1),
                dict(nx=0), dict(edge=0.0), dict(T=nan_t), dict(ox=float("nan"))):
        assert nn(**bad) == DIMS, bad
    sums = lambda **k: lib.itermvs_cloud_umeyama_sums(*[k.get(n, d) for n, d in (                 # noqa: E731
        ("q", a), ("n", 4), ("T", eye), ("idx", a), ("d2", a), ("target", a), ("nt", 4), ("partials", a), ("sums", a), ("stream", None))])
    for name in ("q", "T", "idx", "d2", "target", "partials", "sums"):
        assert sums(**{name: None}) == NULL, name
    for bad in (dict(n=0), dict(n=1 << 31), dict(nt=-1), dict(T=nan_t)):
        assert sums(**bad) == DIMS, bad
    # the grid size is a pure function of n
    assert [lib.itermvs_cloud_umeyama_groups(n) for n in (1, 2048, 2049, 4096, 4097, 1 << 30)] == [1, 1, 2, 2, 3, 1024]
    assert lib.itermvs_cloud_umeyama_groups(0) == DIMS
    for call in (lambda: ops.cloud_crop(torch.zeros(4, 3), np.eye(4), 2, 0.0, 1.0, np.zeros((3, 3))),
                 lambda: ops.cloud_voxel_heads(torch.zeros(4, dtype=torch.int64)),
                 lambda: ops.cloud_umeyama_sums(torch.zeros(4, 3), np.eye(4), torch.zeros(4, dtype=torch.int64),
                                                torch.zeros(4, dtype=torch.float64), torch.zeros(4, 3)),
                 lambda: CR.voxel_down_sample(torch.zeros(4, 3), 0.5), lambda: CR.crop(torch.zeros(4, 3), None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ---- declarations ----------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_bound_and_exported():
    from itermvs_amd import _lib
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert "#define ITERMVS_ABI_VERSION 20" in header and lib.itermvs_version() == 20
    mk = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert mk.count("cloud_register.hip") == 2


def test_tanks_eval_help():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tanks_eval.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0
    for flag in ("--scene", "--gt_dir", "--ply_path", "--traj_path", "--tau", "--no_refine", "--device", "--out"):
        assert flag in p.stdout

"""The yardstick of the outlier removal (tests/cloud_filter_reference.py) against a per-point Python loop and hand-computed
cases, the census of the GPU tests' inputs, ``clean_ply`` on the project's two record sizes, and the argument errors of
``eval.py --clean_cloud`` and ``clean_cloud.py``.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_filter_reference as R
from conftest import ROOT


def loop_knn(pts, k, cap):
    """one point at a time, one distance at a time, Python floats (IEEE doubles)"""
    x = [[float(np.float32(c)) for c in p] for p in pts]
    n = len(x)
    m, isolated = [], []
    for i in range(n):
        d2 = []
        for j in range(n):
            if j == i or not all(math.isfinite(c) for c in x[j]):
                continue
            dx, dy, dz = x[i][0] - x[j][0], x[i][1] - x[j][1], x[i][2] - x[j][2]
            d2.append(((dx * dx) + (dy * dy)) + (dz * dz))
        d2.sort()
        ok = all(math.isfinite(c) for c in x[i]) and len(d2) >= k and d2[k - 1] <= cap * cap
        s = 0.0
        for v in d2[:k] if ok else []:
            s = s + math.sqrt(v)
        m.append(s / k if ok else math.inf)
        isolated.append(not ok)
    return np.array(m), np.array(isolated)


def loop_radius(pts, r, limit):
    x = [[float(np.float32(c)) for c in p] for p in pts]
    out = []
    for i in range(len(x)):
        c = 0
        for j in range(len(x)):
            if j != i and all(math.isfinite(v) for v in x[i] + x[j]):
                dx, dy, dz = x[i][0] - x[j][0], x[i][1] - x[j][1], x[i][2] - x[j][2]
                c += ((dx * dx) + (dy * dy)) + (dz * dz) <= r * r
        out.append(min(c, limit))
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("k,cap", [(1, 0.2), (5, 0.12), (20, 0.3)])
def test_the_restatement_equals_a_per_point_loop(k, cap):
    pts = R.make_cloud(3, n_surface=180, n_floaters=25, n_far=3, n_duplicates=6)
    pts[7] = [np.nan, 0.5, 0.5]
    pts[19] = [0.2, np.inf, 0.1]
    m, iso = R.knn_mean(pts, k, cap)
    lm, liso = loop_knn(pts, k, cap)
    assert np.array_equal(iso, liso) and iso[7] and iso[19] and 0 < iso.sum() < len(pts)
    assert np.array_equal(m.view(np.int64), lm.view(np.int64))
    for limit in (2, 1000):
        assert np.array_equal(R.radius_count(pts, cap / 2, limit), loop_radius(pts, cap / 2, limit))


def test_lattice_duplicates_and_a_point_at_the_cap_by_hand():
    g = np.arange(3.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    centre = 13                                                    # (1, 1, 1): 6 neighbours at 1, 12 at sqrt 2, 8 at sqrt 3
    corner = 0                                                     # (0, 0, 0): 3 at 1, 3 at sqrt 2, 1 at sqrt 3, 3 at 2, ...
    m, iso = R.knn_mean(lat, 6, 10.0)
    assert not iso.any() and m[centre] == 1.0                      # the k-th distance ties with twelve farther ones: still 1
    assert m[corner] == (((((1.0 + 1.0) + 1.0) + math.sqrt(2.0)) + math.sqrt(2.0)) + math.sqrt(2.0)) / 6.0
    m7, _ = R.knn_mean(lat, 7, 10.0)
    assert m7[centre] == (6.0 + math.sqrt(2.0)) / 7.0              # one of twelve tied 7th neighbours
    m, iso = R.knn_mean(lat, 7, 1.0)                               # nobody has 7 others within 1
    assert iso.all() and np.isinf(m).all()
    m, iso = R.knn_mean(lat, 6, 1.0)                               # the centre alone has 6 within exactly 1 (inclusive)
    assert np.array_equal(np.nonzero(~iso)[0], [centre])
    assert R.radius_count(lat, 1.0, 100)[centre] == 6 and R.radius_count(lat, 1.0, 4)[centre] == 4
    assert math.sqrt(2.0) * math.sqrt(2.0) > 2.0 and R.radius_count(lat, math.sqrt(2.0), 100)[corner] == 6     # by the rounded product
    # two coincident points and a third: the duplicate is a neighbour at distance 0, the point itself is not
    pts = np.array([[0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.25, 0.5, 1.75]], dtype=np.float32)
    m, iso = R.knn_mean(pts, 1, 0.5)
    assert m.tolist() == [0.0, 0.0, math.inf] and iso.tolist() == [False, False, True]
    m, iso = R.knn_mean(pts, 2, 1.0)
    assert m.tolist() == [0.5, 0.5, 1.0] and not iso.any()
    assert R.radius_count(pts, 0.5, 9).tolist() == [1, 1, 0]
    # a point exactly at the cap is a neighbour, one float32 ulp beyond is not
    cap = float(np.float32(0.3))
    beyond = float(np.nextafter(np.float32(0.3), np.float32(1.0)))
    pts = np.array([[0, 0, 0], [cap, 0, 0], [0, 8, 0], [beyond, 8, 0]], dtype=np.float32)
    m, iso = R.knn_mean(pts, 1, cap)
    assert iso.tolist() == [False, False, True, True] and m[0] == math.sqrt(cap * cap)
    assert R.radius_count(pts, cap, 5).tolist() == [1, 1, 0, 0]
    mu, sigma, t = R.statistics(np.array([1.0, 2.0, 3.0, math.inf]), np.array([False, False, False, True]), 2.0)
    assert (mu, sigma, t) == (2.0, 1.0, 4.0)


@pytest.mark.parametrize("case", R.CENSUS, ids=[f"seed{c[0]}-k{c[1]}" for c in R.CENSUS])
def test_census_of_the_gpu_inputs(case):
    from itermvs_amd.cloud_filter import threshold_bound
    c = R.census(case)
    n = len(c["pts"])
    removed = int((~c["keep"]).sum())
    bound = threshold_bound(n, c["t"])
    closest = float(np.abs(c["m"][~c["isolated"]] - c["t"]).min())
    print(f"n = {n}, removed = {removed}, isolated = {int(c['isolated'].sum())}, cap = {c['cap']:.6g}, t = {c['t']:.9g}, "
          f"bound = {bound:.3g}, closest m to t = {closest:.3g}")
    assert n <= 5000 and 0.01 * n <= removed <= 0.5 * n
    assert c["isolated"].sum() >= 1 and (~c["isolated"]).sum() > n // 2
    assert int((np.abs(c["m"][~c["isolated"]] - c["t"]) <= bound).sum()) == 0          # a condition on the inputs: seeds picked for it
    assert len(np.unique(c["pts"], axis=0)) < n                                      # duplicates are in


def _ply(path, n, normals, seed=0):
    from itermvs_amd.fusion import ply_header
    g = np.random.default_rng(seed)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals else []) + \
             [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.zeros(n, dtype=fields)
    for name, _ in fields:
        v[name] = g.integers(0, 256, n) if name in ("red", "green", "blue") else g.normal(0, 1, n)
    with open(path, "wb") as f:
        f.write(ply_header(n, normals))
        f.write(v.tobytes())
    return v


@pytest.mark.parametrize("normals,size", [(False, 15), (True, 27)])
def test_clean_ply_copies_the_kept_records(tmp_path, normals, size):
    from itermvs_amd.cloud_filter import clean_ply
    from itermvs_amd.data_io import read_ply_xyz
    from itermvs_amd.fusion import ply_header
    src, dst = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    v = _ply(src, 41, normals)
    assert v.dtype.itemsize == size
    keep = np.random.default_rng(1).random(41) < 0.6
    seen = []

    def fn(xyz):
        seen.append(xyz)
        return keep

    got = clean_ply(src, dst, fn)
    assert got == {"vertices": 41, "kept": int(keep.sum()), "removed": int((~keep).sum()), "record_bytes": size}
    assert seen[0].dtype == np.float32 and np.array_equal(seen[0], read_ply_xyz(src))
    with open(dst, "rb") as f:
        out = f.read()
    assert out == ply_header(int(keep.sum()), normals) + v[keep].tobytes()
    import torch
    clean_ply(src, dst, lambda xyz: torch.from_numpy(keep))                    # a tensor mask is taken too
    with open(dst, "rb") as f:
        assert f.read() == out
    clean_ply(src, dst, lambda xyz: np.zeros(41, dtype=bool))                  # nothing kept: a valid empty cloud
    with open(dst, "rb") as f:
        assert f.read() == ply_header(0, normals)
    assert read_ply_xyz(dst).shape == (0, 3)
    clean_ply(src, dst, lambda xyz: np.ones(41, dtype=bool))
    with open(dst, "rb") as f, open(src, "rb") as g:
        assert f.read() == g.read()
    for bad in (np.ones(40, dtype=bool), np.ones(41, dtype=np.uint8)):
        with pytest.raises(ValueError, match="mask_fn"):
            clean_ply(src, dst, lambda xyz: bad)
    assert not os.path.exists(dst) or read_ply_xyz(dst).shape[0] == 41         # a refused mask leaves no half-written file


def test_clean_ply_other_properties_and_bad_files(tmp_path):
    from itermvs_amd.cloud_filter import clean_ply
    src, dst = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    head = b"ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement vertex 3\nproperty double z\nproperty short q\n" \
           b"property float x\nproperty float y\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n"
    v = np.zeros(3, dtype=[("z", "<f8"), ("q", "<i2"), ("x", "<f4"), ("y", "<f4")])
    v["z"], v["q"], v["x"], v["y"] = [1, 2, 3], [7, 8, 9], [4, 5, 6], [0.5, 1.5, 2.5]
    with open(src, "wb") as f:
        f.write(head + v.tobytes())
    got = clean_ply(src, dst, lambda xyz: xyz[:, 2] != 2)              # z is read through its own property
    assert got["kept"] == 2 and got["record_bytes"] == 18
    with open(dst, "rb") as f:
        assert f.read() == head.replace(b"vertex 3", b"vertex 2") + v[[0, 2]].tobytes()

    def write(text: bytes, body: bytes = b""):
        with open(src, "wb") as f:
            f.write(text + body)

    xyz = b"property float x\nproperty float y\nproperty float z\n"
    cases = [(b"plx\n", "not a PLY"), (b"ply\nformat binary_little_endian 1.0\nelement vertex 1\n" + xyz, "end_header"),
             (b"ply\nformat binary_big_endian 1.0\nelement vertex 0\n" + xyz + b"end_header\n", "not supported"),
             (b"ply\nformat ascii 1.0\nelement vertex 0\n" + xyz + b"end_header\n", "not supported"),
             (b"ply\nformat binary_little_endian 1.0\nelement face 0\nelement vertex 0\n" + xyz + b"end_header\n", "first element"),
             (b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty list uchar int x\nend_header\n", "list property"),
             (b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty half x\nend_header\n", "unknown vertex property"),
             (b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nend_header\n", "x, y and z"),
             (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\n" + xyz + b"end_header\n" + b"\0" * 12, "short"),
             (b"ply\nformat binary_little_endian 1.0\nelement vertex 1\n" + xyz + b"element face 1\nproperty list uchar int "
              b"vertex_indices\nend_header\n" + b"\0" * 25, "faces")]
    for text, why in cases:
        write(text)
        with pytest.raises(ValueError, match=why):
            clean_ply(src, dst, lambda xyz: np.ones(len(xyz), dtype=bool))
    with pytest.raises(FileNotFoundError):
        clean_ply(str(tmp_path / "none.ply"), dst, lambda xyz: None)


def _load(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return __import__(name)


@pytest.mark.parametrize("argv,why", [
    (["--filter", "--clean_cloud", "radius"], "needs --clean_radius"),
    (["--filter", "--clean_k", "8"], "--clean_k needs --clean_cloud"),
    (["--filter", "--clean_radius", "0.5"], "--clean_radius needs --clean_cloud"),
    (["--filter", "--clean_std_ratio", "1"], "--clean_std_ratio needs --clean_cloud"),
    (["--filter", "--clean_max_dist", "1"], "--clean_max_dist needs --clean_cloud"),
    (["--filter", "--clean_min_neighbours", "3"], "--clean_min_neighbours needs --clean_cloud"),
    (["--clean_cloud", "statistical"], "needs --filter"),
    (["--filter", "--clean_cloud", "statistical", "--clean_k", "33"], "--clean_k must lie in 1 .. 32"),
    (["--filter", "--clean_cloud", "radius", "--clean_radius", "0"], "--clean_radius must be positive"),
    (["--filter", "--clean_cloud", "median"], "invalid choice")])
def test_eval_argument_errors(argv, why, capsys):
    E = _load("eval")
    with pytest.raises(SystemExit) as e:
        E.check_clean_cloud(E.build_parser().parse_args(argv))
    assert e.value.code == 2 and why in capsys.readouterr().err


@pytest.mark.parametrize("argv,why", [
    (["--method", "radius"], "needs --radius"),
    (["--radius", "0.5"], "--radius belongs to --method radius"),
    (["--method", "radius", "--radius", "0.5", "--k", "3"], "--k belongs to --method statistical"),
    (["--k", "0"], "--k must lie in 1 .. 32"),
    (["--std_ratio", "nan"], "--std_ratio must be finite"),
    (["--max_dist", "-1"], "--max_dist must be positive"),
    (["--method", "radius", "--radius", "1", "--min_neighbours", "0"], "--min_neighbours must be at least 1"),
    (["--method", "nearest"], "invalid choice")])
def test_clean_cloud_argument_errors(argv, why, tmp_path, capsys):
    CC = _load("clean_cloud")
    with pytest.raises(SystemExit) as e:
        CC.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), *argv])
    assert e.value.code == 2 and why in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out.ply")


def test_eval_accepts_the_clean_flags_and_one_driver_run_as_a_process():
    E = _load("eval")
    a = E.build_parser().parse_args(["--filter", "--clean_cloud", "radius", "--clean_radius", "2.5", "--clean_min_neighbours", "3"])
    assert E.check_clean_cloud(a) == "radius"
    assert E.check_clean_cloud(E.build_parser().parse_args(["--filter", "--clean_cloud", "statistical", "--clean_k", "32"])) == "statistical"
    assert E.check_clean_cloud(E.build_parser().parse_args(["--filter"])) is None
    got = subprocess.run([sys.executable, os.path.join(ROOT, "clean_cloud.py"), "in.ply", "in.ply"], capture_output=True, text=True)
    assert got.returncode == 2 and "must not be IN.ply" in got.stderr, got.stderr[-400:]

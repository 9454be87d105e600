"""Outlier removal on the GPU (csrc/cloud_filter.hip, itermvs_amd/cloud_filter.py) against the numpy yardstick
(tests/cloud_filter_reference.py): equality of bits, not tolerances, on the k-nearest means, the flags, the radius counts and the
masks; the threshold within the stated bound of a reordered fp64 sum; the drivers end to end."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import cloud_filter_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the shared census arrays are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_knn(pts, k, cap, edge=None):
    from itermvs_amd import cloud_filter as CF
    info = {}
    m, iso = CF.knn_mean_distance(dev(pts), k, cap, edge=edge, info=info)
    wm, wiso = R.knn_mean(pts, k, cap)
    assert m.dtype == torch.float64 and iso.dtype == torch.bool
    assert np.array_equal(iso.cpu().numpy(), wiso), (k, cap, edge)
    assert np.array_equal(bits(m.cpu().numpy()), bits(wm)), (k, cap, edge)
    assert info["isolated"] == int(wiso.sum())
    return m, iso, info


def check_radius(pts, r, limit):
    from itermvs_amd import cloud_filter as CF
    got = CF.radius_neighbour_count(dev(pts), r, limit)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.radius_count(pts, r, limit)), (r, limit)
    return got


@pytest.mark.parametrize("k", [1, 8, 20, 32])
def test_means_and_flags_are_bit_equal(k):
    c = R.census(R.CENSUS[0])
    _, iso, info = check_knn(c["pts"], k, 0.15)
    print(f"k = {k}: edge {info['edge']:.4g}, coarse pass {info['second_pass']}, isolated {info['isolated']}")
    assert 0 < int(iso.sum()) < len(c["pts"])
    if k == c["k"]:
        assert np.array_equal(iso.cpu().numpy(), c["isolated"])


def test_radius_counts_with_the_limit_below_and_above():
    pts = R.census(R.CENSUS[1])["pts"]
    true = R.radius_count(pts, 0.05, 10 ** 6)
    assert true.min() == 0 and true.max() > 40
    for limit in (1, 5, int(true.max()) + 7):
        check_radius(pts, 0.05, limit)
    check_radius(pts, 0.004, 3)


def test_minimum_size_and_chunk_seams():
    from itermvs_amd import cloud_filter as CF
    from itermvs_amd import ops
    g = np.random.default_rng(21)
    for k in (1, 8, 32):
        pts = g.random((k + 1, 3)).astype(np.float32)
        _, iso, _ = check_knn(pts, k, 4.0)                         # n = k + 1: every other point is a neighbour
        assert not iso.any()
        with pytest.raises(ValueError, match="exceed k"):
            CF.knn_mean_distance(dev(pts[:k]), k, 4.0)
        xs = dev(pts[:k])                                          # the entry point itself refuses n = k before any launch
        keys = torch.zeros((k,), device=DEV, dtype=torch.int64)
        with pytest.raises(RuntimeError, match="status -2"):
            ops.cloud_knn_mean(xs, keys, torch.arange(k, device=DEV), ops.CloudGrid((0.0, 0.0, 0.0), (1, 1, 1), 2.0), k, 4.0, 2,
                               torch.zeros((k,), device=DEV, dtype=torch.float64), torch.zeros((k,), device=DEV, dtype=torch.uint8))
    for n in (255, 256, 257):
        pts = g.random((n, 3)).astype(np.float32)
        check_knn(pts, 8, 0.3)
        check_knn(pts, 20, 0.25, edge=0.11)
        check_radius(pts, 0.2, 12)


def test_one_cell_and_a_crowded_cell_next_to_empty_ones():
    g = np.random.default_rng(22)
    one_cell = (5.0 + g.random((2500, 3)) * 0.19).astype(np.float32)
    _, iso, info = check_knn(one_cell, 20, 0.05, edge=0.2)
    assert not iso.all()
    crowd = np.concatenate([(g.random((3000, 3)) * 0.01 + 2.0), g.random((60, 3)) * 40.0 - 20.0]).astype(np.float32)
    _, iso, info = check_knn(crowd, 32, 0.5, edge=0.5)             # thousands in one cell, the rest one per cell or none
    assert 0 < int(iso.sum()) <= 60
    check_knn(crowd, 8, 3.0)
    check_radius(crowd, 0.004, 50)
    check_radius(crowd, 6.0, 4)


def test_the_result_does_not_depend_on_the_grid():
    from itermvs_amd import cloud_filter as CF
    c = R.census(R.CENSUS[0])
    pts, n = c["pts"], len(c["pts"])
    runs = {}
    for name, edge in (("one cell", 1000.0), ("default", None), ("tiny", 0.002)):
        m, iso, info = check_knn(pts, c["k"], c["cap"], edge=edge)
        runs[name] = (bits(m.cpu().numpy()), iso.cpu().numpy(), info)
        print(f"{name}: edge {info['edge']:.4g}, coarse edge {info['coarse_edge']}, coarse pass {info['second_pass']} of {n}")
    for name in ("default", "tiny"):
        assert np.array_equal(runs[name][0], runs["one cell"][0]) and np.array_equal(runs[name][1], runs["one cell"][1])
    assert runs["one cell"][2]["second_pass"] == 0
    assert runs["tiny"][2]["second_pass"] > n // 2 and runs["tiny"][2]["coarse_edge"] == c["cap"] / 8        # the coarse pass settled most
    assert 0.002 < runs["default"][2]["edge"] <= c["cap"]
    assert runs["default"][2]["edge"] == CF.default_edge(dev(pts), c["k"], c["cap"])


def test_cell_boundaries_duplicates_ties_and_the_exact_cap():
    g = np.arange(6.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)       # every point on a cell corner
    lat = np.concatenate([lat, lat[::7], lat[::35]])                                                # duplicates, some threefold
    for k, cap, edge in ((6, 1.0, 1.0), (7, 1.0, 1.0), (8, 10.0, 1.0), (20, 1.5, 0.5), (32, 2.0, 2.0), (6, 1.0, None)):
        check_knn(lat, k, cap, edge=edge)                                                           # the k-th distance is tied
    for r, limit in ((1.0, 100), (1.0, 3), (float(np.sqrt(2.0)), 100), (0.999, 5)):
        check_radius(lat, r, limit)
    cap = float(np.float32(0.3))
    beyond = float(np.nextafter(np.float32(0.3), np.float32(1.0)))
    pts = np.array([[0, 0, 0], [cap, 0, 0], [0, 8, 0], [beyond, 8, 0]], dtype=np.float32)
    for edge in (None, 0.05, 0.3, 100.0):
        _, iso, _ = check_knn(pts, 1, cap, edge=edge)
        assert iso.cpu().tolist() == [False, False, True, True]                  # at the cap: kept; one ulp beyond: isolated
    assert check_radius(pts, cap, 5).cpu().tolist() == [1, 1, 0, 0]


def test_non_finite_points_are_isolated_and_nobodys_neighbour():
    from itermvs_amd import cloud_filter as CF
    pts = R.make_cloud(5, n_surface=900, n_floaters=40, n_far=3, n_duplicates=5).copy()
    pts[3] = [np.nan, 0.2, 0.1]
    pts[77] = [0.5, np.inf, 0.0]
    pts[500] = [-np.inf, np.nan, np.inf]
    pts[901, 2] = np.nan
    m, iso, info = check_knn(pts, 8, 0.2)
    assert info["non_finite"] == 4 and iso[[3, 77, 500, 901]].all()
    assert check_radius(pts, 0.1, 6)[[3, 77, 500, 901]].sum() == 0
    keep = CF.statistical_outlier_mask(dev(pts), 8, 2.0, 0.2)
    assert np.array_equal(keep.cpu().numpy(), R.statistical_mask(pts, 8, 2.0, 0.2)[0]) and not keep[[3, 77, 500, 901]].any()
    nothing = np.full((12, 3), np.nan, dtype=np.float32)
    m, iso = CF.knn_mean_distance(dev(nothing), 3, 1.0)
    assert iso.all() and torch.isinf(m).all()
    assert not CF.statistical_outlier_mask(dev(nothing), 3, 2.0, 1.0).any()
    assert not CF.radius_outlier_mask(dev(nothing), 1.0, 1).any()


def test_outputs_sit_between_guard_bytes_and_layouts_are_refused_or_copied():
    from itermvs_amd import cloud_filter as CF
    from itermvs_amd import cloud_grid as CG
    from itermvs_amd import ops
    c = R.census(R.CENSUS[1])
    pts, n, k, cap = c["pts"], len(c["pts"]), c["k"], c["cap"]
    x = dev(pts)
    xs, keys, perm, grid = CG.sort_into_cells(x, 0.03, "test", extent=x)
    pad = 64
    mean = torch.full((n + 2 * pad,), -7.25, device=DEV, dtype=torch.float64)
    flag = torch.full((n + 2 * pad,), 0xA5, device=DEV, dtype=torch.uint8)
    count = torch.full((n + 2 * pad,), -1234567, device=DEV, dtype=torch.int32)
    ops.cloud_knn_mean(xs, keys, perm, grid, k, cap, CG.max_ring(cap, 0.03), mean[pad:pad + n], flag[pad:pad + n])
    ops.cloud_radius_count(xs, keys, perm, grid, 0.05, 9, count[pad:pad + n])
    for buf, fill in ((mean, -7.25), (flag, 0xA5), (count, -1234567)):
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all())
    assert np.array_equal(bits(mean[pad:pad + n].cpu().numpy()), bits(c["m"]))
    assert np.array_equal(flag[pad:pad + n].cpu().numpy() != 0, c["isolated"]) and int(flag[pad:pad + n].max()) <= 1
    assert np.array_equal(count[pad:pad + n].cpu().numpy(), R.radius_count(pts, 0.05, 9))
    # an index list writes its own queries only
    flag2 = torch.full((n,), 0xA5, device=DEV, dtype=torch.uint8)
    mean2 = torch.full((n,), -7.25, device=DEV, dtype=torch.float64)
    index = torch.arange(0, n, 3, device=DEV, dtype=torch.int64)
    ops.cloud_knn_mean(xs, keys, perm, grid, k, cap, CG.max_ring(cap, 0.03), mean2, flag2, index=index)
    touched = torch.zeros((n,), device=DEV, dtype=torch.bool)
    touched[perm[index]] = True
    assert bool((flag2[~touched] == 0xA5).all()) and torch.equal(flag2[touched], flag[pad:pad + n][touched])
    assert torch.equal(mean2[touched], mean[pad:pad + n][touched]) and bool((mean2[~touched] == -7.25).all())
    # layouts: the public functions copy like cloud_grid.points does, the entry wrappers refuse
    wide = torch.zeros((n, 4), device=DEV, dtype=torch.float32)
    wide[:, :3] = x
    m, iso = CF.knn_mean_distance(wide[:, :3], k, cap)
    assert not wide[:, :3].is_contiguous() and np.array_equal(bits(m.cpu().numpy()), bits(c["m"]))
    assert torch.equal(CF.radius_neighbour_count(wide[:, :3], 0.05, 9), count[pad:pad + n])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.cloud_knn_mean(wide[:, :3], keys, perm, grid, k, cap, 4, mean[:n], flag[:n])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.cloud_radius_count(xs, keys, perm, grid, 0.05, 9, count[::2][:n])
    for bad in (x.double(), x.cpu(), x[:, :2]):
        with pytest.raises(RuntimeError):
            CF.knn_mean_distance(bad, k, cap)


@pytest.mark.parametrize("case", R.CENSUS, ids=[f"seed{c[0]}-k{c[1]}" for c in R.CENSUS])
def test_statistical_mask_equals_the_restatement(case):
    from itermvs_amd import cloud_filter as CF
    c = R.census(case)
    info = {}
    keep = CF.statistical_outlier_mask(dev(c["pts"]), c["k"], c["std_ratio"], None if case[3] is None else c["cap"], info=info)
    bound = CF.threshold_bound(len(c["pts"]), c["t"])
    print(f"t = {info['threshold']!r} against fsum {c['t']!r}: off by {abs(info['threshold'] - c['t']):.3g}, bound {bound:.3g}; "
          f"kept {info['kept']}, removed {info['removed']}, isolated {info['isolated']}")
    assert info["cap"] == c["cap"]                                 # the default cap, bit for bit
    assert abs(info["threshold"] - c["t"]) <= bound
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), c["keep"])
    assert info["kept"] == int(c["keep"].sum()) and info["isolated"] == int(c["isolated"].sum())


def test_radius_mask():
    from itermvs_amd import cloud_filter as CF
    pts = R.census(R.CENSUS[0])["pts"]
    for r, need in ((0.05, 6), (0.02, 1)):
        keep = CF.radius_outlier_mask(dev(pts), r, need)
        want = R.radius_count(pts, r, 10 ** 6) >= need
        assert np.array_equal(keep.cpu().numpy(), want) and 0 < int(want.sum()) < len(pts)


# -- the drivers ----------------------------------------------------------------------------------------------------------------
def _tree(out):
    got = {}
    for dp, _, files in os.walk(out):
        for f in files:
            with open(os.path.join(dp, f), "rb") as fh:
                got[os.path.relpath(os.path.join(dp, f), out)] = fh.read()
    return got


def _split(ply: bytes):
    head, body = ply.split(b"end_header\n", 1)
    return head + b"end_header\n", body, int(re.search(rb"element vertex (\d+)", head).group(1))


def _masked(ply: bytes, keep: np.ndarray) -> bytes:
    head, body, n = _split(ply)
    size = len(body) // n
    rec = np.frombuffer(body, dtype=np.uint8).reshape(n, size)
    return head.replace(b"element vertex %d" % n, b"element vertex %d" % int(keep.sum())) + rec[keep].tobytes()


def _xyz(ply: bytes) -> np.ndarray:
    _, body, n = _split(ply)
    rec = np.frombuffer(body, dtype=np.uint8).reshape(n, len(body) // n)
    return np.ascontiguousarray(rec[:, :12]).view("<f4").reshape(n, 3)


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    import test_fuse_memory_gpu as FM
    root = tmp_path_factory.mktemp("clean_scans")
    FM.write_scans(str(root))
    return root


def test_eval_two_passes_with_normals_writes_the_masked_sub_sequence(scans, tmp_path):
    import test_fuse_memory_gpu as FM
    from itermvs_amd import cloud_filter as CF
    E = FM._eval_module()
    flags = ["--fuse_points", "device", "--ply_normals", "--save_masks"]
    clean = ["--clean_cloud", "statistical", "--clean_k", "8", "--clean_std_ratio", "1.0"]
    for out, extra in ((tmp_path / "a", flags), (tmp_path / "b", flags + clean)):
        args = FM._args(scans, out, extra)
        assert E.check_clean_cloud(args) == ("statistical" if extra is not flags else None)
        E.save_depth(args)
        assert E.fuse_scans(args) == 2
    a, b = _tree(tmp_path / "a"), _tree(tmp_path / "b")
    assert sorted(set(b) - set(a)) == ["scan1_clean.ply", "scan2_clean.ply"]
    assert any(n.endswith(".pfm") for n in a) and any(n.endswith(".png") for n in a)
    for name, data in a.items():
        assert b[name] == data, name                               # <scan>.ply, the PFMs and the masks: byte for byte
    for scan in ("scan1", "scan2"):
        head, body, n = _split(a[scan + ".ply"])
        assert n >= 1000 and len(body) == n * 27
        info = {}
        keep = CF.statistical_outlier_mask(dev(_xyz(a[scan + ".ply"])), 8, 1.0, info=info).cpu().numpy()
        print(scan, n, "vertices, kept", int(keep.sum()), "isolated", info["isolated"])
        assert 0 < keep.sum() < n
        assert b[scan + "_clean.ply"] == _masked(a[scan + ".ply"], keep)


def test_eval_from_memory_and_clean_cloud_py(scans, tmp_path, capsys):
    import test_fuse_memory_gpu as FM
    from itermvs_amd import cloud_filter as CF
    E = FM._eval_module()
    clean = ["--clean_cloud", "radius", "--clean_radius", "6.0", "--clean_min_neighbours", "12"]
    for out, extra in ((tmp_path / "a", []), (tmp_path / "b", clean)):
        E.fuse_memory(FM._args(scans, out, ["--fuse_source", "memory"] + extra))
    a, b = _tree(tmp_path / "a"), _tree(tmp_path / "b")
    assert sorted(set(b) - set(a)) == ["scan1_clean.ply", "scan2_clean.ply"]
    for name, data in a.items():
        assert b[name] == data, name
    for scan in ("scan1", "scan2"):
        _, body, n = _split(a[scan + ".ply"])
        assert n >= 1000 and len(body) == n * 15
        keep = CF.radius_outlier_mask(dev(_xyz(a[scan + ".ply"])), 6.0, 12).cpu().numpy()
        print(scan, n, "vertices, kept", int(keep.sum()))
        assert b[scan + "_clean.ply"] == _masked(a[scan + ".ply"], keep)
    # clean_cloud.py on the same file, both methods
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import clean_cloud as CC
    src = str(tmp_path / "a" / "scan1.ply")
    capsys.readouterr()
    got = CC.main([src, str(tmp_path / "r.ply"), "--method", "radius", "--radius", "6.0", "--min_neighbours", "12"])
    with open(tmp_path / "r.ply", "rb") as f:
        assert f.read() == b["scan1_clean.ply"]
    got = CC.main([src, str(tmp_path / "s.ply"), "--k", "8"])
    text = capsys.readouterr().out
    keep = CF.statistical_outlier_mask(dev(_xyz(a["scan1.ply"])), 8, 2.0).cpu().numpy()
    with open(tmp_path / "s.ply", "rb") as f:
        assert f.read() == _masked(a["scan1.ply"], keep)
    assert got["kept"] == int(keep.sum()) and got["removed"] == int((~keep).sum())
    for word in ("kept", "removed", "isolated", "threshold", "seconds: sort"):
        assert word in text, text

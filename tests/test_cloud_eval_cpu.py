"""The DTU evaluator without a GPU: the numpy yardstick (tests/cloud_eval_reference.py) against itself and against analytic
cases, the PLY / mask / plane readers, the statistics on CPU tensors, the validation codes of the cloud_* entry points and
the driver's command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_eval_reference as R
from conftest import ROOT
from itermvs_amd import cloud_eval as CE
from itermvs_amd.data_io import read_ply_xyz


# ---- the yardstick against itself ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_block_wise_restatement_equals_capped_brute_force_below_the_cap(seed):
    """the argument for capping: MaxDistCP's block-wise answer equals min(nearest neighbour, cap) wherever that is < cap and is
    >= cap elsewhere (every target closer than cap lies inside the enlarged block), in both directions"""
    s = R.make_scene(seed, n_gt=900, n_pred=1200)
    pred = s["pred"][np.isfinite(s["pred"]).all(1)]
    for q_from, q_to in ((pred, s["gt"]), (s["gt"], pred)):
        block = R.max_dist_cp(q_to, q_from, s["bb"], s["cap"])
        want = R.capped_nn(q_from, q_to, s["bb"], s["cap"])
        below = want < s["cap"]
        assert below.any() and (~below).any()
        assert np.array_equal(block[below], want[below])
        assert (block[~below] >= s["cap"]).all()
    assert (R.max_dist_cp(np.zeros((0, 3)), pred, s["bb"], s["cap"]) == s["cap"]).all()


@pytest.mark.parametrize("seed,dst", [(0, 0.2), (1, 0.35), (2, 0.1)])
def test_round_formulation_equals_sequential_greedy(seed, dst):
    s = R.make_scene(seed, n_gt=10, n_pred=2500)
    order = np.random.default_rng(seed + 10).permutation(s["pred"].shape[0])
    idx = R.range_search(s["pred"], dst)
    seq = R.reduce_points(s["pred"], dst, order, idx)
    par, sweeps = R.reduce_points_rounds(s["pred"], dst, order, idx)
    assert np.array_equal(seq, par) and 1 <= sweeps < 64
    kept = s["pred"][seq].astype(np.float64)
    assert np.isfinite(kept).all() and 0 < seq.sum() < np.isfinite(s["pred"]).all(1).sum()
    for i in range(0, kept.shape[0], 37):                                    # no two kept points within dst
        d2 = R.d2_to_all(kept[i], kept)
        assert (np.delete(d2, i) > dst * dst).all()
    removed = np.nonzero(~seq & np.isfinite(s["pred"]).all(1))[0][::29]        # every removed point has a kept point within dst
    for i in removed:
        assert (R.d2_to_all(s["pred"][i].astype(np.float64), kept) <= dst * dst).any()


def test_matlab_round_is_half_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.4999, -2.5001, 0.0, 7.0])
    assert R.matlab_round(x).tolist() == [1.0, 2.0, 3.0, -1.0, -2.0, -3.0, 2.0, -3.0, 0.0, 7.0]
    assert np.round(x).tolist() != R.matlab_round(x).tolist()                # numpy: half to even
    # a point half-way between two voxels goes to the upper one; on a 1-voxel mask that decides membership
    mask = np.ones((1, 1, 1), dtype=np.uint8)
    bb = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    pts = np.array([[-0.5, 0, 0], [0.49, 0, 0], [0.5, 0, 0], [-0.51, 0, 0]])  # v = 0.5 -> 1, 1.49 -> 1, 1.5 -> 2, 0.49 -> 0
    assert R.points_in_mask(pts, mask, bb, 1.0).tolist() == [True, True, False, False]


# ---- analytic cases --------------------------------------------------------------------------------------------------------

def lattice(n, spacing, z=0.0):
    g = np.arange(n) * spacing
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(n * n, z)], 1).astype(np.float32)


def test_lifted_lattice_gives_a_quarter_everywhere():
    gt, pred = lattice(20, 0.5), lattice(20, 0.5, 0.25)
    bb = np.array([[-1.0, -1.0, -1.0], [11.0, 11.0, 1.0]])
    mask = np.ones((25, 25, 5), dtype=np.uint8)
    order = np.random.default_rng(0).permutation(pred.shape[0])
    c = R.compare_points(pred, gt, mask, bb, 0.5, [0, 0, 1, 1], 0.2, order)
    assert c["keep"].all() and c["DataInMask"].all() and c["StlAbovePlane"].all()
    assert (c["Ddata"] == 0.25).all() and (c["Dstl"] == 0.25).all()
    st = R.scan_statistics(c["Ddata"], c["Dstl"], c["DataInMask"], c["StlAbovePlane"])
    assert st["MeanData"] == st["MedData"] == st["MeanStl"] == st["MedStl"] == 0.25
    assert st["VarData"] == st["VarStl"] == 0.0 and st["nData"] == st["nStl"] == 400
    blk = R.compare_points(pred, gt, mask, bb, 0.5, [0, 0, 1, 1], 0.2, order, block_wise=True)
    assert np.array_equal(blk["Ddata"], c["Ddata"]) and np.array_equal(blk["Dstl"], c["Dstl"])
    # the statistics of the product on the same numbers
    got = CE.scan_statistics(torch.from_numpy(c["Ddata"]), torch.from_numpy(c["Dstl"]), torch.from_numpy(c["DataInMask"]),
                             torch.from_numpy(c["StlAbovePlane"]))
    assert got == st
    assert CE.summary([got, got]) == {"acc": 0.25, "comp": 0.25, "overall": 0.25}


def test_lattice_with_spacing_dst_loses_its_neighbours():
    """rangesearch is inclusive: on a lattice whose spacing IS dst a kept point removes its four axis neighbours"""
    pts = lattice(9, 0.25)                                                   # 0.25 is exact in float32 and float64
    n = pts.shape[0]
    keep = R.reduce_points(pts, 0.25, np.arange(n))
    want = np.array([(i + j) % 2 == 0 for i in range(9) for j in range(9)])   # visiting in raster order keeps one colour
    assert np.array_equal(keep, want)
    assert R.reduce_points(pts, 0.2499, np.arange(n)).all()                  # just below the spacing nothing is removed


# ---- readers ---------------------------------------------------------------------------------------------------------------

def test_read_ply_xyz_formats_and_errors(tmp_path):
    from itermvs_amd import fusion
    gen = np.random.default_rng(0)
    xyz = gen.normal(0, 100, (57, 3)).astype(np.float32)
    rgb = gen.integers(0, 256, (57, 3)).astype(np.uint8)
    own = str(tmp_path / "own.ply")
    fusion.write_ply(own, xyz, rgb)                                          # this project's 15-byte records
    assert np.array_equal(read_ply_xyz(own), xyz)
    # binary, DTU style: normals and colours around the coordinates, doubles for y, a face element afterwards
    dt = np.dtype([("nx", "<f4"), ("x", "<f4"), ("y", "<f8"), ("z", "<f4"), ("red", "u1"), ("alpha", "<i2")])
    v = np.zeros(57, dtype=dt)
    v["x"], v["y"], v["z"], v["nx"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 7
    head = ("ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex 57\nproperty float nx\nproperty float x\n"
            "property double y\nproperty float z\nproperty uchar red\nproperty short alpha\nelement face 2\n"
            "property list uchar int vertex_indices\nend_header\n")
    f1 = tmp_path / "dtu.ply"
    f1.write_bytes(head.encode() + v.tobytes() + bytes([3]) + np.array([0, 1, 2], "<i4").tobytes() * 2)
    assert np.array_equal(read_ply_xyz(str(f1)), xyz)
    # ascii with extra properties and faces
    f2 = tmp_path / "ascii.ply"
    lines = ["ply", "format ascii 1.0", "element vertex 3", "property float x", "property float y", "property float z",
             "property uchar red", "element face 1", "property list uchar int vertex_indices", "end_header",
             "1.5 -2 3e2 255", "0 0 0 0", "-1e-3 4 5 9", "3 0 1 2"]
    f2.write_text("\n".join(lines) + "\n")
    assert np.array_equal(read_ply_xyz(str(f2)), np.array([[1.5, -2, 300], [0, 0, 0], [-1e-3, 4, 5]], dtype=np.float32))
    assert read_ply_xyz(str(f2)).dtype == np.float32
    # errors name the file
    cases = {"big.ply": head.replace("binary_little_endian", "binary_big_endian").encode() + v.tobytes(),
             "list.ply": head.replace("property short alpha\n", "property list uchar float w\n").encode() + v.tobytes(),
             "short.ply": head.encode() + v.tobytes()[:-40],
             "short_ascii.ply": ("\n".join(lines[:12]) + "\n").encode(),
             "noxyz.ply": head.replace("property float z\n", "").encode() + v.tobytes(),
             "nohead.ply": b"ply\nformat ascii 1.0\nelement vertex 1\n",
             "notply.ply": b"P5\n1 1\n255\n0"}
    for name, data in cases.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            read_ply_xyz(str(tmp_path / name))


def test_load_obs_mask_and_plane_npz(tmp_path):
    mask = (np.random.default_rng(1).random((4, 5, 6)) > 0.5)
    bb = np.array([[-1.0, 2.0, 3.0], [4.0, 5.0, 6.5]])
    np.savez(tmp_path / "ObsMask3_10.npz", ObsMask=mask, BB=bb.astype(np.float32), Res=np.array([[0.5]]))
    np.savez(tmp_path / "Plane3.npz", P=np.array([[0.1], [0.2], [0.3], [-4.0]]))
    m, b, res = CE.load_obs_mask(CE.resolve_file(str(tmp_path), "ObsMask3_10"))
    assert m.dtype == torch.uint8 and tuple(m.shape) == (4, 5, 6) and np.array_equal(m.numpy(), mask.astype(np.uint8))
    assert b.dtype == np.float64 and np.array_equal(b, bb) and res == 0.5
    assert CE.load_plane(CE.resolve_file(str(tmp_path), "Plane3")).tolist() == [0.1, 0.2, 0.3, -4.0]
    np.savez(tmp_path / "bad.npz", BB=bb)
    with pytest.raises(ValueError, match="ObsMask"):
        CE.load_obs_mask(str(tmp_path / "bad.npz"))
    with pytest.raises(FileNotFoundError):
        CE.resolve_file(str(tmp_path), "Plane4")


def test_load_obs_mask_and_plane_mat(tmp_path):
    sio = pytest.importorskip("scipy.io")
    mask = (np.random.default_rng(2).random((3, 4, 5)) > 0.4)
    bb = np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]])
    sio.savemat(str(tmp_path / "ObsMask7_10.mat"), {"ObsMask": mask, "BB": bb, "Res": 0.25})
    sio.savemat(str(tmp_path / "Plane7.mat"), {"P": np.array([[1.0], [0.0], [0.5], [-2.0]])})
    m, b, res = CE.load_obs_mask(CE.resolve_file(str(tmp_path), "ObsMask7_10"))
    assert np.array_equal(m.numpy(), mask.astype(np.uint8)) and np.array_equal(b, bb) and res == 0.25
    assert CE.load_plane(str(tmp_path / "Plane7.mat")).tolist() == [1.0, 0.0, 0.5, -2.0]


# ---- statistics on CPU tensors ---------------------------------------------------------------------------------------------

def test_scan_statistics_medians_variance_and_empty_selections():
    d = torch.tensor([3.0, 1.0, 25.0, 2.0, 4.0, 100.0], dtype=torch.float64)
    in_mask = torch.tensor([True, True, True, True, True, False])
    s = torch.tensor([5.0, 1.0, 2.0, 20.0, 7.0], dtype=torch.float64)
    above = torch.tensor([True, True, True, True, False])
    st = CE.scan_statistics(d, s, in_mask, above)                            # data: 3 1 2 4 (even), stl: 5 1 2 (odd; 20 is not < 20)
    assert st["nData"] == 4 and st["MedData"] == 2.5 and st["MeanData"] == 2.5
    assert st["VarData"] == pytest.approx(5.0 / 3.0, rel=1e-15)              # sum of squares 5, n - 1 = 3
    assert st["nStl"] == 3 and st["MedStl"] == 2.0 and st["MeanStl"] == pytest.approx(8.0 / 3.0, rel=1e-15)
    assert st == R.scan_statistics(d.numpy(), s.numpy(), in_mask.numpy(), above.numpy())
    assert torch.median(d[:4]).item() == 2.0 and CE.matlab_median(d[:4]) == 2.5      # torch takes the lower middle value
    empty = CE.scan_statistics(d, s, torch.zeros(6, dtype=torch.bool), above, max_dist=0.5)
    for k in ("MeanData", "MedData", "VarData", "MeanStl", "MedStl", "VarStl"):
        assert np.isnan(empty[k]), k
    assert empty["nData"] == empty["nStl"] == 0
    one = CE.scan_statistics(d, s, in_mask, above, max_dist=1.5)
    assert one["nData"] == 1 and one["VarData"] == 0.0 and one["MedData"] == 1.0
    assert np.isnan(CE.summary([])["overall"])
    assert CE.summary([{"MeanData": 1.0, "MeanStl": 2.0}, {"MeanData": 2.0, "MeanStl": 4.0}]) == {"acc": 1.5, "comp": 3.0, "overall": 2.25}


def test_above_plane_and_host_side_helpers():
    pts = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [float("nan"), 0.0, 9.0]])
    assert CE.above_plane(pts, [0.0, 0.0, 1.0, -1.0]).tolist() == [False, True, False]           # strictly above
    lo, hi = CE.covered_region([[0.0, 0.0, 0.0], [130.0, 59.0, 60.0]], 60.0)
    assert lo.tolist() == [0.0, 0.0, 0.0] and hi.tolist() == [180.0, 60.0, 120.0]
    lo, hi = CE.covered_region([[0.0, 0.0, 0.0], [10.0, -1.0, 10.0]], 60.0)                       # a negative Range: no block at all
    assert (hi == lo).all()
    rank = CE.inverse_permutation(torch.tensor([2, 0, 1]), 3)
    assert rank.dtype == torch.int32 and rank.tolist() == [1, 2, 0]
    for bad in (torch.tensor([0, 0, 1]), torch.tensor([0, 1, 3]), torch.tensor([0, 1])):
        with pytest.raises(ValueError):
            CE.inverse_permutation(bad, 3)
    assert torch.equal(CE.default_order(50, 3), torch.randperm(50, generator=torch.Generator().manual_seed(3)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        CE.reduce_points(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        CE.capped_nn_distance(torch.zeros(4, 3), torch.zeros(4, 3), [[0, 0, 0], [1, 1, 1]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        CE.points_in_mask(torch.zeros(4, 3), torch.ones(2, 2, 2, dtype=torch.uint8), [[0, 0, 0], [1, 1, 1]], 0.5)


# ---- C ABI validation ------------------------------------------------------------------------------------------------------

def test_cloud_entry_points_validate_before_touching_the_gpu():
    from itermvs_amd import _lib, ops
    lib = _lib.load()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    grid = (0.0, 0.0, 0.0, 4, 4, 4, 0.25)
    reg = (C.c_double * 6)(0, 0, 0, 1, 1, 1)
    NULL, DIMS = -1, -2
    assert lib.itermvs_cloud_cell_keys(None, 4, *grid, a, None) == NULL
    assert lib.itermvs_cloud_cell_keys(a, 4, *grid, None, None) == NULL
    assert lib.itermvs_cloud_cell_keys(a, 0, *grid, a, None) == DIMS
    assert lib.itermvs_cloud_cell_keys(a, -3, *grid, a, None) == DIMS
    assert lib.itermvs_cloud_cell_keys(a, 4, 0.0, 0.0, 0.0, 4, 4, 4, 0.0, a, None) == DIMS                      # edge <= 0
    assert lib.itermvs_cloud_cell_keys(a, 4, float("nan"), 0.0, 0.0, 4, 4, 4, 0.25, a, None) == DIMS
    assert lib.itermvs_cloud_cell_keys(a, 4, 0.0, 0.0, 0.0, (1 << 21) + 1, 4, 4, 0.25, a, None) == DIMS         # oversized extent
    assert lib.itermvs_cloud_cell_keys(a, 4, 0.0, 0.0, 0.0, 4, 0, 4, 0.25, a, None) == DIMS
    assert lib.itermvs_cloud_cell_keys(a, 1 << 31, *grid, a, None) == DIMS                                      # 32-bit ranks
    assert lib.itermvs_cloud_reduce_round(a, a, None, 4, *grid, 0.2, a, a, None) == NULL
    assert lib.itermvs_cloud_reduce_round(a, a, a, 4, *grid, 0.2, a, None, None) == NULL
    assert lib.itermvs_cloud_reduce_round(a, a, a, 0, *grid, 0.2, a, a, None) == DIMS
    assert lib.itermvs_cloud_reduce_round(a, a, a, 4, *grid, 0.0, a, a, None) == DIMS                           # dst <= 0
    assert lib.itermvs_cloud_reduce_round(a, a, a, 4, *grid, -1.0, a, a, None) == DIMS
    assert lib.itermvs_cloud_reduce_round(a, a, a, 4, *grid, 0.3, a, a, None) == DIMS                           # cells narrower than dst
    assert lib.itermvs_cloud_reduce_round(a, a, a, 4, 0.0, 0.0, 0.0, 4, 4, 1 << 22, 0.25, 0.2, a, a, None) == DIMS
    nn = lambda **k: lib.itermvs_cloud_nn_distance(*[k.get(n, d) for n, d in (                                  # noqa: E731
        ("q", a), ("nq", 4), ("index", None), ("n_index", 0), ("t", a), ("keys", a), ("nt", 4), ("ox", 0.0), ("oy", 0.0), ("oz", 0.0),
        ("nx", 4), ("ny", 4), ("nz", 4), ("edge", 1.0), ("region", reg), ("cap", 60.0), ("rings", 4), ("best", a), ("done", a),
        ("dist", a), ("stream", None))])
    for name in ("q", "t", "keys", "region", "best", "done", "dist"):
        assert nn(**{name: None}) == NULL, name
    for bad in (dict(nq=0), dict(nt=0), dict(nt=-1), dict(cap=0.0), dict(cap=float("inf")), dict(rings=0), dict(rings=(1 << 21) + 1),
                dict(nx=(1 << 21) + 1), dict(edge=-1.0), dict(index=a, n_index=0), dict(index=a, n_index=5)):
        assert nn(**bad) == DIMS, bad
    assert lib.itermvs_cloud_in_mask(a, 4, None, 2, 2, 2, 0.0, 0.0, 0.0, 0.5, a, None) == NULL
    assert lib.itermvs_cloud_in_mask(a, 0, a, 2, 2, 2, 0.0, 0.0, 0.0, 0.5, a, None) == DIMS
    assert lib.itermvs_cloud_in_mask(a, 4, a, 2, 0, 2, 0.0, 0.0, 0.0, 0.5, a, None) == DIMS
    assert lib.itermvs_cloud_in_mask(a, 4, a, 2, 2, 2, 0.0, 0.0, 0.0, 0.0, a, None) == DIMS
    assert lib.itermvs_cloud_in_mask(a, 4, a, 2, 2, 2, 0.0, float("inf"), 0.0, 0.5, a, None) == DIMS
    # the tensor-level wrappers refuse CPU tensors before anything is launched
    g = ops.CloudGrid((0.0, 0.0, 0.0), (4, 4, 4), 0.25)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cloud_cell_keys(torch.zeros(4, 3), g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cloud_in_mask(torch.zeros(4, 3), torch.ones(2, 2, 2, dtype=torch.uint8), (0, 0, 0), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cloud_reduce_round(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), g, 0.2,
                               torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cloud_nn_distance(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), g, [0] * 6, 60.0, 4,
                              torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.float64))


# ---- the driver ------------------------------------------------------------------------------------------------------------

def test_dtu_eval_help_defaults_and_file_names(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "dtu_eval.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--data_path" in p.stdout and "--ply_path" in p.stdout and "--testlist" in p.stdout
    import dtu_eval
    a = dtu_eval.build_parser().parse_args(["--data_path", "d", "--ply_path", "p"])
    assert (a.method, a.light, a.dst, a.max_dist, a.seed) == ("itermvs", "l3", 0.2, 20.0, 0)
    assert dtu_eval.scan_numbers(a) == list(CE.USED_SETS) and len(CE.USED_SETS) == 22
    a = dtu_eval.build_parser().parse_args(["--data_path", "d", "--ply_path", "p", "--scans", "9", "1"])
    assert dtu_eval.scan_numbers(a) == [9, 1]
    lst = tmp_path / "test.txt"
    lst.write_text("scan1\nscan114\n\n")
    a = dtu_eval.build_parser().parse_args(["--data_path", "d", "--ply_path", "p", "--testlist", str(lst)])
    assert dtu_eval.scan_numbers(a) == [1, 114]
    (tmp_path / "scan4.ply").write_bytes(b"")
    (tmp_path / "itermvs009_l3.ply").write_bytes(b"")
    (tmp_path / "scan9.ply").write_bytes(b"")
    assert CE.prediction_path(str(tmp_path), 9) == str(tmp_path / "itermvs009_l3.ply")           # the script's name first
    assert CE.prediction_path(str(tmp_path), 4) == str(tmp_path / "scan4.ply")
    assert CE.prediction_path(str(tmp_path), 9, "Other", "l7") == str(tmp_path / "scan9.ply")
    with pytest.raises(FileNotFoundError, match="itermvs001_l3.ply"):
        CE.prediction_path(str(tmp_path), 1)
    st = {"MeanData": 0.5, "MedData": 0.25, "MeanStl": 1.5, "MedStl": 1.0}
    assert dtu_eval.scan_lines(st) == ["mean/median Data (acc.) 0.500000/0.250000", "mean/median Stl (comp.) 1.500000/1.000000"]
    line = dtu_eval.final_line({"acc": 0.5, "comp": 1.5, "overall": 1.0})
    assert line == "final evaluation result on all scans: acc.: 0.500000, comp.: 1.500000, overall: 1.000000"
    assert dtu_eval.parse_final_line(line) == {"acc": 0.5, "comp": 1.5, "overall": 1.0}
    assert json.loads(json.dumps(dtu_eval.final_line({"acc": float("nan"), "comp": 1.0, "overall": float("nan")}))).startswith("final")


def test_eval_driver_takes_geo_mask_thres():
    import eval as ev
    assert ev.build_parser().parse_args([]).geo_mask_thres == 3                                    # today's clouds
    assert ev.build_parser().parse_args(["--geo_mask_thres", "4"]).geo_mask_thres == 4             # the reference's value for DTU

"""Per-vertex normals of the fused cloud (itermvs_fuse_points_normals, eval.py --ply_normals), the parts that need no GPU: what
the numpy restatement tests/fuse_normals_reference.py MEANS (an exact plane, a depth step, the degenerate inputs), the host
plumbing (header, grouping, the flag checks) and the statuses of the C entry point for arguments it refuses before any launch."""
import ctypes as C
import sys

import numpy as np
import pytest

import fuse_normals_reference as NR
from conftest import ROOT
from oracle import fusion_oracle as FO


def _camera(f=300.0, cx=29.3, cy=18.6):
    """a non-trivial float32 K and E: off-centre principal point, rotation about a skew axis, translation"""
    k = np.array([[f, 0, cx], [0, 1.07 * f, cy], [0, 0, 1]], np.float32)
    axis = np.array([0.3, -0.8, 0.52])
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(33.0)
    cross = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + np.sin(a) * cross + (1 - np.cos(a)) * cross @ cross
    e = np.eye(4)
    e[:3, :3], e[:3, 3] = r, [0.4, -1.1, 2.3]
    return k, e.astype(np.float32)


def _world_frame(k, e):
    """what the kernel holds of the camera, upcast: (inv(K), rotation part of inv(E), camera centre), float64"""
    ki, ei = np.linalg.inv(k).astype(np.float64), np.linalg.inv(e).astype(np.float64)
    return ki, ei[:3, :3], ei[:3, 3]


def _unit(v):
    return v / np.linalg.norm(v)


def test_exact_plane_every_pixel_borders_included():
    """depth_avg = the float64 depth at which the ray of every pixel, through the float32 matrices the kernel uses, meets a tilted
    world plane.  Bound 1e-6 on the dot product and the length: three float32 components with at most 2^-24 relative rounding
    each (about 2e-7 together); the float64 differencing error of neighbouring points is about 1e-13; the float32 inverse of E is
    orthogonal to about 1e-7, which tilts a normal by that angle and moves the dot product by its square."""
    h, w = 40, 56
    k, e = _camera()
    ki, rot, centre = _world_frame(k, e)
    n_plane, offset = _unit(np.array([0.35, -0.2, 1.0])), 9.0
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rays = rot @ (ki @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)]))           # X = centre + d * ray
    depth = ((offset - n_plane @ centre) / (n_plane @ rays)).reshape(h, w)
    assert depth.dtype == np.float64 and (depth > 1).all()
    mask = np.ones((h, w), bool)
    n = NR.normals(depth, mask, k, e, 0.01).astype(np.float64)
    pts = FO.unproject_points(depth, mask, k, e)
    assert n.shape == pts.shape == (h * w, 3)
    assert np.abs(pts @ n_plane - offset).max() < 1e-9                               # the scene is the plane
    facing = n_plane if n_plane @ (centre - pts[0]) > 0 else -n_plane
    dots, lengths = n @ facing, np.linalg.norm(n, axis=1)
    print("exact plane: min dot", dots.min(), "max | |n| - 1 |", np.abs(lengths - 1).max())
    assert dots.min() >= 1 - 1e-6
    assert np.abs(lengths - 1).max() <= 1e-6
    assert (np.einsum("ij,ij->i", n, centre - pts) > 0).all()                        # towards the camera that saw the point


def _step_scene(h=12, w=16):
    k, e = _camera()
    depth = np.full((h, w), 1.0)
    depth[:, w // 2:] = 1.2                                                          # a vertical step between columns 7 and 8
    return k, e, depth


def test_depth_step_the_threshold_protects_the_columns_beside_it():
    k, e, depth = _step_scene()
    h, w = depth.shape
    _, rot, _ = _world_frame(k, e)
    plane = _unit(rot @ np.array([0.0, 0.0, -1.0]))                                  # fronto-parallel, facing the camera
    beside = [w // 2 - 1, w // 2]
    n = NR.normal_map(depth, k, e, 0.01).astype(np.float64)
    assert (n.reshape(-1, 3) @ plane >= 1 - 1e-6).all()                              # every pixel, one-sided at the step
    assert (n[:, beside] @ plane >= 1 - 1e-6).all()
    loose = NR.normal_map(depth, k, e, 0.5).astype(np.float64)
    tilted = loose[:, beside] @ plane
    print("depth step, edge_thres 0.5: cos of the tilt beside the step", tilted.min(), tilted.max())
    assert (tilted < np.cos(np.deg2rad(45.0))).all()                                 # the central difference spans the step
    away = [c for c in range(w) if c not in beside]
    assert (loose[:, away] @ plane >= 1 - 1e-6).all()


def _vertices_and_normals(depth, mask, edge=0.01):
    k, e = _camera()
    with np.errstate(all="ignore"):
        return FO.unproject_points(depth, mask, k, e), NR.normals(depth, mask, k, e, edge)


def test_degenerate_inputs_give_zero_normals_and_keep_the_vertex():
    # a 1 x 1 image
    pts, n = _vertices_and_normals(np.full((1, 1), 2.0), np.ones((1, 1), bool))
    assert pts.shape == (1, 3) and np.isfinite(pts).all() and n.dtype == np.float32 and n.tolist() == [[0.0, 0.0, 0.0]]
    # all four neighbours across an edge
    depth = np.full((3, 3), 1.0)
    depth[1, 1] = 2.0
    pts, n = _vertices_and_normals(depth, np.ones((3, 3), bool))
    assert pts.shape == (9, 3) and n[4].tolist() == [0.0, 0.0, 0.0]
    # d = 0, NaN, Inf at the centre; the neighbours lose that neighbour and keep a one-sided normal
    for bad in (0.0, np.nan, np.inf):
        depth = np.full((5, 5), 1.5)
        depth[2, 2] = bad
        pts, n = _vertices_and_normals(depth, np.ones((5, 5), bool))
        assert pts.shape == (25, 3) and n.shape == (25, 3)
        assert n[12].tolist() == [0.0, 0.0, 0.0], bad
        others = np.delete(n, 12, axis=0).astype(np.float64)
        assert np.abs(np.linalg.norm(others, axis=1) - 1).max() <= 1e-6, bad
    # one row, one column: a tangent is missing everywhere
    for shape in ((1, 5), (5, 1)):
        pts, n = _vertices_and_normals(np.full(shape, 3.0), np.ones(shape, bool))
        assert pts.shape == (5, 3) and not n.any(), shape
    # the mask selects, in row-major order
    mask = np.zeros((3, 3), bool)
    mask[0, 2] = mask[2, 0] = True
    full = NR.normal_map(np.full((3, 3), 1.5), *_camera(), 0.01)
    assert np.array_equal(NR.normals(np.full((3, 3), 1.5), mask, *_camera(), 0.01), np.stack([full[0, 2], full[2, 0]]))


# -- host plumbing ----------------------------------------------------------------------------------------------------------
def test_ply_header_with_and_without_normals():
    from itermvs_amd import fusion
    plain = (b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
             b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert fusion.ply_header(7) == fusion.ply_header(7, normals=False) == plain
    assert fusion.ply_header(7, normals=True) == plain.replace(
        b"property float z\n", b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\n")


def test_group_views_with_the_larger_record():
    from itermvs_amd import fusion, ops
    assert ops.POINT_NORMAL_RECORD_BYTES == 27 and ops.POINT_RECORD_BYTES == 15
    h, w = 70, 90
    budget = 5 * h * w * 15
    assert fusion.group_views(5, h, w, budget) == fusion.group_views(5, h, w, budget, record_bytes=15) == [(0, 5)]
    assert fusion.group_views(5, h, w, budget, record_bytes=27) == [(0, 2), (2, 4), (4, 5)]      # 75 // 27 = 2 views per group
    with pytest.raises(ValueError, match="below one"):
        fusion.group_views(5, h, w, h * w * 27 - 1, record_bytes=27)


def test_filter_depth_refuses_normals_on_the_host_path(tmp_path):
    from itermvs_amd import fusion
    for kw in (dict(points="host"), dict()):
        with pytest.raises(ValueError, match="normals=True needs points='device'"):      # no pair.txt there: the check comes first
            fusion.filter_depth(str(tmp_path / "none"), str(tmp_path / "none"), str(tmp_path / "x.ply"), 1.0, 0.01, 0.3,
                                img_wh=(8, 8), normals=True, **kw)
    assert not (tmp_path / "x.ply").exists()


def test_ops_fuse_points_normals_refuses_cpu_tensors():
    import torch
    from itermvs_amd import ops
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)                      # noqa: E731
    with pytest.raises(RuntimeError, match="fuse_points_normals: .*no CPU path"):
        ops.fuse_points_normals(z(4, 4, dt=torch.float64), z(4, 4), z(21, dt=torch.float32), z(4, 4, 3), z(16 * 27),
                                z(1, dt=torch.int64), z(1, 4, dt=torch.int64), 0)


def _eval():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


@pytest.mark.parametrize("argv,names", [
    (["--fuse_points", "device", "--ply_normals"], ["--ply_normals", "--filter"]),
    (["--filter", "--ply_normals"], ["--ply_normals", "--fuse_points device", "--fuse_source memory"]),
    (["--filter", "--fuse_points", "host", "--ply_normals"], ["--ply_normals", "--fuse_points device", "--fuse_source memory"]),
    (["--ply_normals"], ["--ply_normals", "--filter", "--fuse_points device", "--fuse_source memory"]),
    (["--filter", "--fuse_points", "device", "--ply_normals", "--normal_edge_thres", "0"], ["--normal_edge_thres"]),
    (["--filter", "--fuse_points", "device", "--ply_normals", "--normal_edge_thres", "-0.01"], ["--normal_edge_thres"]),
    (["--filter", "--fuse_points", "device", "--ply_normals", "--normal_edge_thres", "nan"], ["--normal_edge_thres"]),
    (["--filter", "--fuse_points", "device", "--ply_normals", "--normal_edge_thres", "inf"], ["--normal_edge_thres"]),
])
def test_eval_refuses_normals_without_their_flags(argv, names):
    E = _eval()
    a = E.build_parser().parse_args(argv)
    with pytest.raises(SystemExit) as e:
        E.check_ply_normals(a)
    for name in names:
        assert name in str(e.value), (name, str(e.value))
    with pytest.raises(SystemExit) as e2:              # the filter stage refuses before it touches a device
        E.fuse_scans(a)
    assert str(e2.value) == str(e.value)


def test_eval_accepts_normals_with_either_gpu_assembly_and_explains_them():
    E = _eval()
    a = E.build_parser().parse_args([])
    assert a.ply_normals is False and a.normal_edge_thres == 0.01 and E.check_ply_normals(a) is False
    for argv in (["--filter", "--fuse_points", "device"], ["--dataset", "folder", "--filter", "--fuse_source", "memory"]):
        a = E.build_parser().parse_args(argv + ["--ply_normals", "--normal_edge_thres", "0.02", "--fuse_dedupe"])
        assert a.ply_normals is True and a.normal_edge_thres == 0.02 and E.check_ply_normals(a) is True
    text = " ".join(E.build_parser().format_help().split())
    about = text.split("--ply_normals")[2]
    assert "unit normal" in about and "facing the reference camera" in about and "every byte as before" in about
    assert "not a measured optimum" in text.split("--normal_edge_thres")[2]


# -- the C entry point ------------------------------------------------------------------------------------------------------
NULL, DIMS = -1, -2


def test_entry_status_without_a_launch():
    """every expected status is a rejection that precedes the first launch, so these calls are safe without a device; a fully
    valid argument list is never passed"""
    from itermvs_amd import _lib
    lib = _lib.load()
    assert len(_lib.PROTOTYPES["itermvs_fuse_points_normals"][1]) == 16
    buf = (C.c_uint8 * 256)()
    a = C.addressof(buf)
    ok = dict(depth_avg=a, final_mask=a, photo_mask=None, geo_mask=None, cam=a, rgb=a, H=4, W=4, edge_thres=0.01, records=a,
              capacity=4, cursor=a, view_counts=a, view=0, workspace=a, stream=None)
    call = lambda **kw: lib.itermvs_fuse_points_normals(*{**ok, **kw}.values())      # noqa: E731
    for name in ("depth_avg", "final_mask", "cam", "rgb", "records", "cursor", "view_counts", "workspace"):
        assert call(**{name: None}) == NULL, name
    for bad in (dict(H=0), dict(W=0), dict(H=-3), dict(capacity=-1), dict(view=-1), dict(H=46341, W=46341),
                dict(H=1, W=0x7fffff01)):
        assert call(**bad) == DIMS, bad
    for edge in (0.0, -0.01, float("nan"), float("inf"), -float("inf")):
        assert call(edge_thres=edge) == DIMS, edge
    # the checks of itermvs_fuse_points come first: a NULL pointer is reported whatever the threshold
    assert call(cam=None, edge_thres=0.0) == NULL

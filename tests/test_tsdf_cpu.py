"""The mesh of a scan (itermvs_tsdf_integrate, itermvs_tsdf_mesh, eval.py --mesh), the parts that need no GPU: the two marching-
tetrahedra tables through the library's host functions, the entry points' statuses before any launch, the numpy restatement on an
analytic sphere, the bounds rule, the budget error, the mesh PLY round trip and the argument checks of eval.py."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import tsdf_reference as R
from conftest import ROOT

NULL, DIMS, ALIGN = -1, -2, -5
_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16          # an aligned HOST address: every call below must be refused before it is used
CORNER = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], np.float64)


@pytest.fixture(scope="module")
def tables():
    from itermvs_amd import ops
    return ops.tsdf_tet_tables()


# -- 1. the case table -------------------------------------------------------------------------------------------------------
def test_tables_are_the_rule_of_the_header(tables):
    corners, cases = tables
    assert corners == R.tet_corners() and cases == R.tet_cases()


def test_case_table_counts_edges_and_winding(tables):
    corners, cases = tables
    assert len(cases) == 16
    tet = CORNER[corners[0]]                                       # any positively oriented tetrahedron
    assert np.linalg.det(tet[1:] - tet[0]) > 0
    for m, tris in enumerate(cases):
        inside = [(m >> p) & 1 for p in range(4)]
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(inside)]
        value = np.where(np.array(inside) == 1, -1.0, 1.0)         # linear field: -1 at inside, +1 at outside corners
        grad = np.linalg.solve(np.c_[tet, np.ones(4)], value)[:3]  # points from negative to positive
        for tri in tris:
            assert len(set(tri)) == 3
            for p, q in tri:
                assert p < q and inside[p] != inside[q]
            pts = np.array([(tet[p] + tet[q]) / 2 for p, q in tri])
            assert np.dot(np.cross(pts[1] - pts[0], pts[2] - pts[0]), grad) > 0, (m, tri)
        # the complementary pattern: the same edges, every triangle's normal reversed (checked above through grad's sign)
        assert {e for t in tris for e in t} == {e for t in cases[15 - m] for e in t}
        if len(tris) == 1:
            a, b = tris[0], cases[15 - m][0]
            assert any(b == a[i:] + a[:i] for i in range(3)) is False and any(b[::-1] == a[i:] + a[:i] for i in range(3))


def test_library_rejects_bad_table_arguments():
    from itermvs_amd import _lib
    lib = _lib.load()
    buf = (C.c_int32 * 12)()
    assert lib.itermvs_tsdf_tet_corners(6, buf) == DIMS and lib.itermvs_tsdf_tet_corners(-1, buf) == DIMS
    assert lib.itermvs_tsdf_tet_corners(0, None) == NULL
    assert lib.itermvs_tsdf_tet_case(16, buf) == DIMS and lib.itermvs_tsdf_tet_case(3, None) == NULL
    assert lib.itermvs_tsdf_tet_case(3, buf) == 2 and lib.itermvs_tsdf_tet_case(1, buf) == 1 and list(buf[6:]) == [-1] * 6


def test_six_tetrahedra_tile_the_cube(tables):
    corners, _ = tables
    tets = [CORNER[c] for c in corners]
    vols = [np.linalg.det(t[1:] - t[0]) / 6 for t in tets]
    assert all(v > 0 for v in vols) and abs(sum(vols) - 1) < 1e-12
    assert len({tuple(sorted(c)) for c in corners}) == 6 and all(c[0] == 0 and c[3] == 7 for c in corners)
    pts = np.random.default_rng(0).random((4000, 3))
    owners = np.zeros(len(pts), int)
    for t in tets:                                                 # barycentric coordinates strictly positive = in the interior
        bary = np.linalg.solve(np.c_[t, np.ones(4)].T, np.c_[pts, np.ones(len(pts))].T)
        owners += (bary > 1e-12).all(axis=0)
    assert (owners == 1).all()                                     # random points miss the measure-zero faces


def test_face_diagonals_match_across_cells(tables):
    corners, _ = tables
    edges = {tuple(sorted((t[p], t[q]))) for t in corners for p, q in itertools.combinations(range(4), 2)}
    assert len(edges) == 19 and all(lo & hi == lo for lo, hi in edges)        # every edge runs from a corner to one above it
    for axis in range(3):
        bit = 1 << axis
        low = {e for e in edges if not (e[0] | e[1]) & bit}                   # the face where the axis' coordinate is 0
        high = {(a ^ bit, b ^ bit) for a, b in edges if a & bit and b & bit}  # the opposite face, moved onto it
        assert low == high and len(low) == 5                                  # 4 sides + the same diagonal


# -- 2. statuses before any launch ---------------------------------------------------------------------------------------------
INTEGRATE = dict(state=A, nx=4, ny=5, nz=6, ox=0.0, oy=0.0, oz=0.0, voxel=0.5, trunc=1.5, depth=A, mask=A, cams=A, rgb=A, V=2, H=3, W=5,
                 stream=None)
MESH = dict(state=A, nx=4, ny=5, nz=6, ox=0.0, oy=0.0, oz=0.0, voxel=0.5, min_count=1, vertices=A, vertex_capacity=8, faces=A,
            face_capacity=8, totals=A, workspace=A, stream=None)
NAN, INF = float("nan"), float("inf")
PAST = dict(nx=65536, ny=65536, nz=1)                              # 2^32 voxels: one past what a launch can count (2^32 - 256)
VOLUME_CASES = ([(f"{n} 0", {n: 0}, DIMS) for n in ("nx", "ny", "nz")] + [("nx negative", {"nx": -3}, DIMS)] +
                [(f"voxel {v}", {"voxel": v}, DIMS) for v in (NAN, INF, 0.0, -0.5)] + [("origin nan", {"oy": NAN}, DIMS)] +
                [("voxels past the flat bound", PAST, DIMS), ("voxels past 64 bits", dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), DIMS)])
CASES = ([("itermvs_tsdf_integrate", INTEGRATE, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("state", "depth", "mask", "cams", "rgb")] + VOLUME_CASES +
          [(f"trunc {v}", {"trunc": v}, DIMS) for v in (NAN, INF, 0.0, -1.0)] + [(f"{n} 0", {n: 0}, DIMS) for n in ("V", "H", "W")] +
          [("pixels past int32", dict(H=46341, W=46341), DIMS), ("null before dims", dict(depth=None, nx=0), NULL)]] +
         [("itermvs_tsdf_mesh", MESH, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("state", "totals", "workspace", "vertices", "faces")] + VOLUME_CASES +
          [("min_count 0", {"min_count": 0}, DIMS), ("vertex capacity negative", {"vertex_capacity": -1}, DIMS),
           ("face capacity negative", {"face_capacity": -1}, DIMS), ("vertex capacity past int32", {"vertex_capacity": 2 ** 31}, DIMS),
           ("workspace unaligned", {"workspace": A + 4}, ALIGN)]])


@pytest.mark.parametrize("entry,valid,what,change,status", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_entry_status_before_any_launch(entry, valid, what, change, status):
    from itermvs_amd import _lib
    assert getattr(_lib.load(), entry)(*{**valid, **change}.values()) == status


def test_workspace_bytes_and_binding():
    from itermvs_amd import _lib, ops
    lib = _lib.load()
    assert ops.tsdf_mesh_workspace_bytes((1, 1, 1)) == 16 + 12 and ops.tsdf_mesh_workspace_bytes((16, 16, 2)) == 32 + 12 * 512
    assert ops.tsdf_mesh_workspace_bytes((512, 512, 512)) == 16 * 2 ** 19 + 12 * 2 ** 27
    n = C.c_int64(-1)
    assert lib.itermvs_tsdf_mesh_workspace_bytes(0, 4, 4, C.byref(n)) == DIMS and lib.itermvs_tsdf_mesh_workspace_bytes(4, 4, 4, None) == NULL
    assert lib.itermvs_tsdf_mesh_workspace_bytes(65536, 65536, 1, C.byref(n)) == DIMS and n.value == -1
    assert lib.itermvs_tsdf_mesh_workspace_bytes(65536, 65535, 1, C.byref(n)) == 0 and n.value > 0
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    for name in ("itermvs_tsdf_integrate", "itermvs_tsdf_mesh", "itermvs_tsdf_mesh_workspace_bytes", "itermvs_tsdf_tet_corners",
                 "itermvs_tsdf_tet_case"):
        assert name in _lib.PROTOTYPES and name + "(" in header and hasattr(lib, name)
    assert len(_lib.PROTOTYPES["itermvs_tsdf_integrate"][1]) == 17 and len(_lib.PROTOTYPES["itermvs_tsdf_mesh"][1]) == 16
    makefile = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert makefile.count("tsdf.hip") == 2                            # SRCS and the resource-usage list


def test_ops_refuse_cpu_tensors():
    import torch
    from itermvs_amd import ops
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)        # noqa: E731
    with pytest.raises(RuntimeError, match="tsdf_integrate: .*no CPU path"):
        ops.tsdf_integrate(z(8, 3, dt=torch.int32), (2, 2, 2), (0, 0, 0), 1.0, 3.0, z(1, 4, 4, dt=torch.float64), z(1, 4, 4),
                           z(1, 21, dt=torch.float32), z(1, 4, 4, 3))
    with pytest.raises(RuntimeError, match="tsdf_mesh: .*no CPU path"):
        ops.tsdf_mesh(z(8, 3, dt=torch.int32), (2, 2, 2), (0, 0, 0), 1.0, 1, z(15), z(3, dt=torch.int32), z(2, dt=torch.int64))


# -- 3. the restatement by itself ----------------------------------------------------------------------------------------------
SPHERE = dict(dims=(20, 20, 20), origin=(-1.0, -1.0, -1.0), voxel=0.1, centre=np.array([0.013, -0.021, 0.007]), radius=0.7)


def sphere_state(dims, origin, voxel, centre, radius):
    return R.sdf_state(dims, origin, voxel, lambda x, y, z: np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius)


def check_sphere(vertices, faces, voxel, centre, radius):
    """closed, one component of genus 0, outward, and every vertex within sqrt(3) * voxel of the sphere: a vertex and the true
    crossing of its grid edge lie on the same edge, and the longest edge is the cell's body diagonal"""
    uses, euler = R.topology(faces)
    assert len(faces) > 0 and (uses == 2).all() and euler == 2
    assert len(np.unique(faces)) == len(vertices)                  # every vertex is referenced
    p = np.stack([vertices["x"], vertices["y"], vertices["z"]], 1).astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3 - centre) > 0).all()
    assert np.abs(np.linalg.norm(p - centre, axis=1) - radius).max() <= np.sqrt(3) * voxel


def test_restatement_on_an_analytic_sphere():
    s = SPHERE
    state = sphere_state(**s)
    assert (state["sum"] > 0).sum() > 0 and (state["sum"][[0, -1]] > 0).all()      # the sphere is strictly inside the volume
    vertices, faces = R.mesh(state, s["dims"], s["origin"], s["voxel"], 1)
    check_sphere(vertices, faces, s["voxel"], s["centre"], s["radius"])
    assert (vertices["red"] == 200).all() and (vertices["green"] == 120).all() and (vertices["blue"] == 40).all()
    none, no_faces = R.mesh(state, s["dims"], s["origin"], s["voxel"], 2)          # count 1 < min_count 2: nothing is valid
    assert len(none) == 0 and no_faces.shape == (0, 3)


# -- 4. the host side ------------------------------------------------------------------------------------------------------
def test_bounds_rule_is_the_order_statistic():
    from itermvs_amd import fusion
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(1001, 3)).astype(np.float32)
    xyz[7] = np.nan                                                # a vertex that is not finite takes no part
    ok = np.sort(xyz[np.isfinite(xyz).all(1)], axis=0)
    for q, k in ((0.0, 0), (0.01, 9), (0.25, 249), (0.4999, 499)):
        got = fusion.mesh_bounds(xyz, q)
        assert got == tuple(float(v) for v in (*ok[k], *ok[len(ok) - 1 - k])), q
    import torch
    assert fusion.mesh_bounds(torch.from_numpy(xyz), 0.01) == fusion.mesh_bounds(xyz, 0.01)
    with pytest.raises(ValueError, match="no finite vertex"):
        fusion.mesh_bounds(np.full((3, 3), np.nan, np.float32), 0.01)


def test_plan_voxel_dims_and_budget():
    from itermvs_amd import fusion
    bounds = (0.0, 0.0, 0.0, 8.0, 4.0, 2.0)
    p = fusion.mesh_plan(bounds, resolution=64, trunc_voxels=3.0)
    assert p["voxel"] == 0.125 and p["trunc"] == 0.375 and p["origin"] == (-0.375, -0.375, -0.375) and p["dims"] == (70, 38, 22)
    p = fusion.mesh_plan(bounds, voxel=0.3, trunc_voxels=2.0, widen=False)
    assert p["voxel"] == 0.3 and p["origin"] == (0.0, 0.0, 0.0) and p["dims"] == (27, 14, 7)
    n = 27 * 14 * 7
    assert p["state_bytes"] == 12 * n and p["workspace_bytes"] == 16 * ((n + 255) // 256) + 12 * n
    from itermvs_amd import ops
    assert p["workspace_bytes"] == ops.tsdf_mesh_workspace_bytes((27, 14, 7))
    need = p["state_bytes"] + p["workspace_bytes"] + 1000
    assert fusion.mesh_plan(bounds, voxel=0.3, widen=False, budget_bytes=need, other_bytes=1000)["need_bytes"] == need
    with pytest.raises(ValueError, match=rf"needs {need} bytes.*budget is {need - 1}.*--mesh_resolution.*--mesh_budget_gb"):
        fusion.mesh_plan(bounds, voxel=0.3, widen=False, budget_bytes=need - 1, other_bytes=1000)
    with pytest.raises(ValueError, match="beyond the 4294967040 of one launch"):
        fusion.mesh_plan(bounds, resolution=4096)
    for bad in (dict(bounds=(0, 0, 0, 1, 0, 1)), dict(bounds_quantile=0.5), dict(voxel=0.0), dict(trunc_voxels=0.5), dict(min_count=0),
                dict(resolution=1), dict(bounds=(0, 0, 0, 1, float("nan"), 1))):
        with pytest.raises(ValueError, match="mesh: "):
            fusion.mesh_options(dict(path="m.ply", **bad))
    assert fusion.mesh_options(None) is None and fusion.mesh_options(dict(path="m.ply")).resolution == 256


def test_read_ply_mesh_round_trip(tmp_path):
    from itermvs_amd import data_io, fusion
    s = SPHERE
    vertices, faces = R.mesh(sphere_state(**s), s["dims"], s["origin"], s["voxel"], 1)
    path = str(tmp_path / "m.ply")
    fusion.write_ply_mesh(path, vertices, faces)
    assert os.path.getsize(path) == len(fusion.ply_mesh_header(len(vertices), len(faces))) + 15 * len(vertices) + 13 * len(faces)
    xyz, rgb, got = data_io.read_ply_mesh(path)
    assert np.array_equal(got, faces) and got.dtype == np.int32
    assert np.array_equal(xyz, np.stack([vertices["x"], vertices["y"], vertices["z"]], 1))
    assert np.array_equal(rgb, np.stack([vertices["red"], vertices["green"], vertices["blue"]], 1))
    assert np.array_equal(data_io.read_ply_xyz(path), xyz)          # the cloud reader skips the faces, as before
    fusion.write_ply_mesh(path, vertices[:0], faces[:0])            # an empty mesh is a valid file
    xyz, rgb, got = data_io.read_ply_mesh(path)
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and got.shape == (0, 3)
    fusion.write_ply_mesh(path, vertices, faces)
    raw = open(path, "rb").read()
    for broken, why in ((raw[:-5], "short"), (raw + b"x", "after the last face"), (raw.replace(b"binary_little_endian", b"ascii", 1), "format")):
        open(path, "wb").write(broken)
        with pytest.raises(ValueError, match=why):
            data_io.read_ply_mesh(path)
    bad = faces.copy()
    bad[3, 1] = len(vertices)
    fusion.write_ply_mesh(path, vertices, bad)
    with pytest.raises(ValueError, match="outside"):
        data_io.read_ply_mesh(path)


# -- 5. eval.py ------------------------------------------------------------------------------------------------------------
def _eval_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


@pytest.mark.parametrize("argv,needs", [
    (["--fuse_points", "device", "--mesh"], ["--mesh", "--filter"]),
    (["--filter", "--mesh"], ["--mesh", "--fuse_points device", "--fuse_source memory"]),
    (["--filter", "--fuse_points", "host", "--mesh"], ["--mesh", "--fuse_points device", "--fuse_source memory"]),
    (["--filter", "--fuse_points", "device", "--mesh", "--mesh_trunc", "0.5"], ["--mesh_trunc"]),
    (["--filter", "--fuse_points", "device", "--mesh", "--mesh_voxel", "0"], ["--mesh_voxel"]),
    (["--filter", "--fuse_points", "device", "--mesh", "--mesh_bounds_quantile", "0.5"], ["--mesh_bounds_quantile"]),
    (["--filter", "--fuse_points", "device", "--mesh", "--mesh_min_count", "0"], ["--mesh_min_count"]),
    (["--filter", "--fuse_points", "device", "--mesh", "--mesh_bounds", "0", "0", "0", "1", "1", "0"], ["--mesh_bounds"]),
])
def test_mesh_flag_is_refused_in_the_argument_check(argv, needs):
    E = _eval_module()
    with pytest.raises(SystemExit) as e:
        E.check_mesh(E.build_parser().parse_args(argv))
    for word in needs:
        assert word in str(e.value), (word, str(e.value))


def test_mesh_flags_parse_and_say_that_defaults_are_choices():
    E = _eval_module()
    a = E.build_parser().parse_args(["--filter", "--fuse_points", "device"])
    assert a.mesh is False and E.check_mesh(a) is False
    a = E.build_parser().parse_args(["--filter", "--fuse_source", "memory", "--dataset", "folder", "--mesh", "--mesh_resolution", "64",
                                     "--mesh_bounds", "0", "0", "0", "1", "2", "3"])
    assert E.check_mesh(a) is True and a.mesh_bounds == [0, 0, 0, 1, 2, 3] and a.mesh_resolution == 64
    from itermvs_amd import fusion
    m = fusion.mesh_options_from_args(a, "x_mesh.ply")
    assert m.path == "x_mesh.ply" and m.bounds == (0, 0, 0, 1, 2, 3) and m.trunc_voxels == 3.0 and m.min_count == 2
    helps = {s: act.help for act in E.build_parser()._actions for s in act.option_strings}
    for flag in ("--mesh_resolution", "--mesh_bounds_quantile", "--mesh_trunc", "--mesh_min_count", "--mesh_budget_gb"):
        assert "choice" in helps[flag], flag
    with pytest.raises(ValueError, match="points='device'"):
        fusion.filter_depth("scan", "out", "out.ply", 1, 0.01, 0.3, img_wh=(4, 4), points="host", mesh=dict(path="m.ply"))

"""itermvs_tsdf_integrate / itermvs_tsdf_mesh / eval.py --mesh on the MI355X: the volume state and the mesh bit for bit against the
numpy restatement (tests/tsdf_reference.py), and the drivers on a small synthetic scan folder."""
import numpy as np
import pytest
import torch

import tsdf_reference as R
from test_tsdf_cpu import SPHERE, check_sphere, sphere_state

pytestmark = pytest.mark.gpu
DEV = "cuda"

# a ragged volume (19 x 23 x 17, no multiple of the 256-voxel workgroup in any layer) of binary-exact geometry: voxel (9, 11, 8) has its
# centre at exactly (0, 0, 0)
DIMS, VOXEL = (19, 23, 17), 0.125
ORIGIN = (-9.5 * VOXEL, -11.5 * VOXEL, -8.5 * VOXEL)
TRUNC = 3 * VOXEL
RADIUS = 0.75
H, W = 40, 48


def _camera(rows, centre, f, cx, cy):
    r = np.array(rows, np.float64)
    e = np.c_[r, -r @ np.array(centre, np.float64)]
    k = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)
    return k, e, r, np.array(centre, np.float64)


def _depth(k, r, centre, wall):
    """analytic depth of the sphere of RADIUS at the world origin, ``wall`` where the ray misses it"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(x - k[0, 2]) / k[0, 0], (y - k[1, 2]) / k[1, 1], np.ones_like(x)], -1) @ r       # world direction per unit depth
    a, b, c = (d * d).sum(-1), 2 * (d @ centre), centre @ centre - RADIUS ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (t > 0), t, wall)


@pytest.fixture(scope="module")
def views():
    """3 views of 48 x 40: 0 looks along +z from z = -3 (its frustum misses the volume's upper and lower parts; the centre column of
    voxels projects to exactly (23.5, 19.5)), 1 sits INSIDE the volume at x = -1 looking along +x (the voxels behind it have pc.z <= 0),
    2 looks along +y from y = -3.  Masked pixels, NaN, 0 and negative depths in every view."""
    cams = [_camera([[1, 0, 0], [0, 1, 0], [0, 0, 1]], (0, 0, -3), 60, 23.5, 19.5),
            _camera([[0, 1, 0], [0, 0, 1], [1, 0, 0]], (-1, 0, 0), 20, 24.0, 20.0),
            _camera([[0, 0, 1], [1, 0, 0], [0, 1, 0]], (0, -3, 0), 60, 22.25, 18.75)]
    rng = np.random.default_rng(11)
    depth = np.stack([_depth(k, r, c, wall) for (k, _, r, c), wall in zip(cams, (4.0, 2.5, 4.0))])
    mask = (rng.random((3, H, W)) > 0.1).astype(np.uint8)
    mask[:, 10:13, 20:31] = 0
    for v in range(3):
        depth[v, 5 + v, 7] = np.nan
        depth[v, 20, 24 + v] = 0.0
        depth[v, 19, 23 - v] = -1.0
        depth[v, 30, 40] = np.inf
    mask[0, 20, 24] = mask[0, 19, 23] = mask[0, 5, 7] = 1          # the broken depths are reached, not masked away
    rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    cam = np.stack([np.concatenate([k.reshape(-1), e.reshape(-1)]) for k, e, _, _ in cams]).astype(np.float32)
    return depth, mask, cam, rgb


def _device(views):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in views]


def _integrate(views, batches):
    from itermvs_amd import ops
    depth, mask, cam, rgb = _device(views)
    state = ops.tsdf_volume(DIMS, DEV)
    for a, b in batches:
        ops.tsdf_integrate(state, DIMS, ORIGIN, VOXEL, TRUNC, depth[a:b], mask[a:b], cam[a:b], rgb[a:b])
    return state


@pytest.fixture(scope="module")
def integrated(views):
    """the restatement's volume after the three views, computed once and never changed"""
    state = R.integrate(R.empty_state(DIMS), DIMS, ORIGIN, VOXEL, TRUNC, *views)
    state.flags.writeable = False
    return state


def test_scene_holds_every_case_of_the_issue(views, integrated):
    depth, mask, cam, rgb = views
    cx, cy, cz = R._centres(DIMS, ORIGIN, VOXEL)
    seen = {"behind": 0, "outside": 0, "half": 0, "masked": 0, "nan": 0, "zero": 0, "negative": 0, "hidden": 0, "clamped": 0, "used": 0}
    for v in range(3):
        k, e = cam[v, :9].astype(np.float64), cam[v, 9:].astype(np.float64)
        px, py, pz = (e[4 * i] * cx + e[4 * i + 1] * cy + e[4 * i + 2] * cz + e[4 * i + 3] for i in range(3))
        front = pz > 0
        seen["behind"] += (~front).sum()
        with np.errstate(all="ignore"):
            ux, uy = (k[0] * px + k[1] * py + k[2] * pz) / pz, (k[3] * px + k[4] * py + k[5] * pz) / pz
        inside = front & (np.rint(ux) >= 0) & (np.rint(ux) <= W - 1) & (np.rint(uy) >= 0) & (np.rint(uy) <= H - 1)
        seen["outside"] += (front & ~inside).sum()
        with np.errstate(all="ignore"):
            seen["half"] += (inside & ((ux - np.floor(ux) == 0.5) | (uy - np.floor(uy) == 0.5))).sum()
        xi, yi = np.where(inside, np.rint(ux), 0).astype(int), np.where(inside, np.rint(uy), 0).astype(int)
        m, d = mask[v][yi, xi] != 0, depth[v][yi, xi]
        seen["masked"] += (inside & ~m).sum()
        ok = inside & m
        seen["nan"] += (ok & np.isnan(d)).sum()
        seen["zero"] += (ok & (d == 0)).sum()
        seen["negative"] += (ok & (d < 0)).sum()
        with np.errstate(invalid="ignore"):
            good = ok & np.isfinite(d) & (d > 0)
            seen["hidden"] += (good & (d - pz < -TRUNC)).sum()
            seen["clamped"] += (good & (d - pz > TRUNC)).sum()
            seen["used"] += (good & ~(d - pz < -TRUNC)).sum()
    assert all(n > 0 for n in seen.values()), seen
    assert seen["used"] == int(integrated["count"].sum())
    assert set(np.unique(integrated["count"])) == {0, 1, 2, 3}     # invalid voxels and every count up to the view number


def test_integrate_equals_the_restatement_bit_for_bit(views, integrated):
    got = _integrate(views, [(0, 3)]).cpu().numpy()
    want = R.state_words(integrated)
    assert got.dtype == want.dtype and np.array_equal(got, want), np.nonzero((got != want).any(1))[0][:10]


def test_integrate_in_batches_gives_the_same_bits(views):
    whole, split, single = (_integrate(views, b) for b in ([(0, 3)], [(0, 1), (1, 3)], [(0, 1), (1, 2), (2, 3)]))
    assert torch.equal(whole, split) and torch.equal(whole, single)


def test_integrate_saturates_at_257_views(views):
    from itermvs_amd import ops
    depth, mask, cam, rgb = (t[:1].expand(130, *t.shape[1:]).contiguous() for t in _device(views))
    state = ops.tsdf_volume(DIMS, DEV)
    for _ in range(2):                                             # 260 times view 0
        ops.tsdf_integrate(state, DIMS, ORIGIN, VOXEL, TRUNC, depth, mask, cam, rgb)
    got = state.cpu().numpy().view(R.STATE).reshape(-1)
    once = R.integrate(R.empty_state(DIMS), DIMS, ORIGIN, VOXEL, TRUNC, *(a[:1] for a in views))
    hit = once["count"] == 1
    assert hit.any() and (got["count"][hit] == 257).all() and (got["count"][~hit] == 0).all()
    for ch in "rgb":
        assert np.array_equal(got[ch][hit].astype(np.int64), once[ch][hit].astype(np.int64) * 257)      # no field wrapped


def _mesh(state_np, dims, origin, voxel, min_count, short=0):
    """the device's mesh of a restatement-made volume -> (vertices, faces, totals, guard bytes intact); ``short``: capacities that
    many below the totals"""
    from itermvs_amd import ops
    state = torch.from_numpy(R.state_words(np.ascontiguousarray(state_np)).copy()).to(DEV)
    totals = torch.zeros(2, device=DEV, dtype=torch.int64)
    ops.tsdf_mesh(state, dims, origin, voxel, min_count, torch.empty(0, device=DEV, dtype=torch.uint8),
                  torch.empty(0, device=DEV, dtype=torch.int32), totals)
    nv, nf = totals.tolist()
    vcap, fcap = max(nv - short, 0), max(nf - short, 0)
    guard = 64
    vertices = torch.full((vcap * 15 + guard,), 0xAB, device=DEV, dtype=torch.uint8)
    faces = torch.full((fcap * 3 + guard,), -7, device=DEV, dtype=torch.int32)
    again = torch.zeros(2, device=DEV, dtype=torch.int64)
    ops.tsdf_mesh(state, dims, origin, voxel, min_count, vertices, faces, again, vertex_capacity=vcap, face_capacity=fcap)
    intact = bool((vertices[vcap * 15:] == 0xAB).all()) and bool((faces[fcap * 3:] == -7).all())
    return (vertices[:vcap * 15].cpu().numpy().view(R.VERTEX), faces[:fcap * 3].cpu().numpy().reshape(-1, 3), (nv, nf), again.tolist(), intact)


def _assert_equal_mesh(got, want):
    vertices, faces, totals, again, intact = got
    assert intact and list(totals) == again == [len(want[0]), len(want[1])]
    assert np.array_equal(vertices.view(np.uint8), want[0].view(np.uint8)) and np.array_equal(faces, want[1]) and faces.dtype == np.int32


def test_mesh_of_the_integrated_volume(integrated):
    """invalid voxels and open boundaries; min_count 1 and 2 take different voxels"""
    sizes = []
    for min_count in (1, 2):
        want = R.mesh(integrated, DIMS, ORIGIN, VOXEL, min_count)
        _assert_equal_mesh(_mesh(integrated, DIMS, ORIGIN, VOXEL, min_count), want)
        sizes.append(len(want[1]))
        uses, _ = R.topology(want[1])
        assert (uses <= 2).all() and (uses == 1).any()             # a manifold with a boundary
    assert sizes[0] > sizes[1] > 0


def test_mesh_of_the_analytic_sphere():
    s = SPHERE
    state = sphere_state(**s)
    got = _mesh(state, s["dims"], s["origin"], s["voxel"], 1)
    _assert_equal_mesh(got, R.mesh(state, s["dims"], s["origin"], s["voxel"], 1))
    check_sphere(got[0], got[1], s["voxel"], s["centre"], s["radius"])


def test_mesh_with_exact_zeros_stays_closed():
    """a cube whose six faces are planes THROUGH voxel centres: the value is exactly 0 there, 0 counts as outside, the vertices on those
    edges coincide with the voxel centre (s = 1 or 0) and the surface is still closed"""
    dims, origin, voxel = (16, 14, 15), (-8 * 0.125, -7 * 0.125, -7.5 * 0.125), 0.125
    state = R.sdf_state(dims, origin, voxel, lambda x, y, z: np.maximum(np.maximum(np.abs(x - 0.0625), np.abs(y - 0.0625)), np.abs(z)) - 0.5)
    assert (state["sum"] == 0).sum() > 100
    want = R.mesh(state, dims, origin, voxel, 1)
    got = _mesh(state, dims, origin, voxel, 1)
    _assert_equal_mesh(got, want)
    uses, euler = R.topology(got[1])
    assert (uses == 2).all() and euler == 2


def test_mesh_of_an_all_positive_volume_is_empty(tmp_path):
    from itermvs_amd import data_io, fusion
    state = R.sdf_state((9, 7, 5), (0, 0, 0), 1.0, lambda x, y, z: x * 0 + 0.25)
    vertices, faces, totals, again, intact = _mesh(state, (9, 7, 5), (0, 0, 0), 1.0, 1)
    assert intact and list(totals) == again == [0, 0] and len(vertices) == 0 and faces.shape == (0, 3)
    path = str(tmp_path / "empty.ply")
    fusion.write_ply_mesh(path, vertices, faces)
    xyz, rgb, f = data_io.read_ply_mesh(path)
    assert xyz.shape == (0, 3) and f.shape == (0, 3)


def test_mesh_with_capacities_one_short(integrated):
    want = R.mesh(integrated, DIMS, ORIGIN, VOXEL, 1)
    vertices, faces, totals, again, intact = _mesh(integrated, DIMS, ORIGIN, VOXEL, 1, short=1)
    assert intact and list(totals) == again == [len(want[0]), len(want[1])]        # nothing past the capacities, the totals hold
    assert np.array_equal(vertices.view(np.uint8), want[0][:-1].view(np.uint8)) and np.array_equal(faces, want[1][:-1])


# -- the drivers ---------------------------------------------------------------------------------------------------------------
BOUNDS = ["--mesh_bounds", "-150", "-110", "-250", "150", "110", "250"]      # the rig looks at the origin from 680 away
MESH = ["--mesh", "--mesh_resolution", "40"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """eval.py's two drivers on the two six-view scans of tests/test_fuse_memory_gpu.py -> {name: {relative path: bytes}}"""
    from test_fuse_memory_gpu import _args, _eval_module, _files, write_scans
    data = tmp_path_factory.mktemp("mesh_scans")
    write_scans(str(data))
    E = _eval_module()
    out = {}
    for name, extra in (("plain", []), ("mesh", MESH), ("bounds", MESH + BOUNDS), ("bounds_dedupe", MESH + BOUNDS + ["--fuse_dedupe"])):
        folder = tmp_path_factory.mktemp(name)
        E.fuse_memory(_args(data, folder, ["--fuse_source", "memory", "--save_masks"] + extra))
        out[name] = _files(str(folder))
    folder = tmp_path_factory.mktemp("two_pass")
    args = _args(data, folder, ["--fuse_points", "device", "--save_masks"] + MESH)
    E.save_depth(args)
    assert E.fuse_scans(args) == 2
    out["two_pass"] = _files(str(folder))
    out["folders"] = (str(data), str(folder))
    return out


def test_driver_writes_a_mesh_and_changes_no_other_byte(runs, tmp_path):
    from itermvs_amd import data_io
    plain, mesh = runs["plain"], runs["mesh"]
    assert set(mesh) - set(plain) == {"scan1_mesh.ply", "scan2_mesh.ply"} and set(plain) <= set(mesh)
    assert any(f.endswith(".pfm") for f in plain) and any(f.endswith("_final.png") for f in plain) and "scan1.ply" in plain
    for name, raw in plain.items():
        assert mesh[name] == raw, name                             # cloud, PFMs and masks
    for scan in ("scan1", "scan2"):
        path = str(tmp_path / "m.ply")
        open(path, "wb").write(mesh[scan + "_mesh.ply"])
        xyz, rgb, faces = data_io.read_ply_mesh(path)              # parses; indices in range
        assert len(faces) > 0 and np.isfinite(xyz).all() and rgb.shape == xyz.shape
        assert np.array_equal(np.unique(faces), np.arange(len(xyz)))       # every vertex is referenced


def test_both_drivers_write_the_same_mesh(runs):
    for scan in ("scan1_mesh.ply", "scan2_mesh.ply"):
        assert runs["two_pass"][scan] == runs["mesh"][scan], scan
    assert runs["two_pass"]["scan1.ply"] == runs["mesh"]["scan1.ply"]


def test_mesh_with_given_bounds_does_not_depend_on_dedupe(runs):
    for scan in ("scan1", "scan2"):
        assert runs["bounds_dedupe"][scan + "_mesh.ply"] == runs["bounds"][scan + "_mesh.ply"], scan
        assert len(runs["bounds_dedupe"][scan + ".ply"]) < len(runs["bounds"][scan + ".ply"])      # the clouds do differ
        assert b"element face 0\n" not in runs["bounds"][scan + "_mesh.ply"]


def test_mesh_without_a_device_side_cloud_is_an_argument_error(runs):
    from test_fuse_memory_gpu import _args, _eval_module
    E = _eval_module()
    data, folder = runs["folders"]
    with pytest.raises(SystemExit, match="--mesh needs --fuse_points device or --fuse_source memory"):
        E.check_mesh(_args(data, folder, ["--mesh"]))

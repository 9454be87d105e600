"""The stream compaction of itermvs_fuse_points / itermvs_fuse_points_normals and of itermvs_tsdf_mesh at the seams of their
one-workgroup scans (csrc/wave_ops.hpp: block_scan_exclusive_chunked walks the per-workgroup counts 1024 at a time with a carry):
workgroup counts on both sides of one and of two chunks for the 32-bit scan of the point path, a volume of 1090 workgroups for the
64-bit scan of the mesh path.  Everything is compared bit for bit with the references the other GPU tests use."""
import numpy as np
import pytest
import torch

import fuse_normals_reference as NR
import test_fuse_normals_gpu as N
import test_fuse_points_gpu as P
import tsdf_reference as R
from oracle import fusion_oracle as FO
from test_tsdf_gpu import _assert_equal_mesh, _mesh

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK, CHUNK = 256, 1024                 # pixels (voxels) per workgroup, workgroups per chunk of the scan
# workgroups -> (H, W): 1, 4, one chunk, one chunk + 1, two chunks, two chunks + 1
SHAPES = {1: (8, 32), 4: (16, 64), 1024: (512, 512), 1025: (1, 262145), 2048: (512, 1024), 2049: (1, 524289)}
MASKS = ["all", "none", "last", "first", "block_heads", "random"]
N_VIEWS = 3


def _rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


@pytest.fixture(scope="module")
def views_of():
    """(h, w) -> the three views of that shape, built on first use and kept until the module is done"""
    made = {}
    yield lambda h, w: made[(h, w)] if (h, w) in made else made.setdefault((h, w), _views(h, w))
    made.clear()


def _views(h, w):
    """three views of h x w with their own K (fx != fy, skew) and general poses; per view the host arrays, the device tensors and
    the records of EVERY pixel from the references, computed once: both references are elementwise, so the records of a mask are
    the rows of its pixels"""
    assert -(-h * w // BLOCK) in SHAPES and SHAPES[-(-h * w // BLOCK)] == (h, w)
    rng = np.random.default_rng(h * 7 + w)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    every = np.ones((h, w), bool)
    views = []
    for v in range(N_VIEWS):
        f = 1.1 * max(w, 64) + 3 * v
        k = np.array([[f, 0.25, w / 2 + 1.3], [0, 1.07 * f, h / 2 - 0.7], [0, 0, 1]], np.float32)
        e = np.eye(4)
        e[:3, :3] = _rotation(0.05 * (v + 1), 0.1 * (v - 1), 0.03 * v)
        e[:3, 3] = (12.0 * v, -7.0, 30.0 + v)
        e = e.astype(np.float32)
        avg = (600.0 + 30.0 * np.sin(0.05 * xs + v) + 20.0 * np.cos(0.07 * ys)) * (1 + 0.004 * rng.standard_normal((h, w)))
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        photo, geo = rng.uniform(size=(h, w)) < 0.6, rng.uniform(size=(h, w)) < 0.3
        with np.errstate(all="ignore"):
            xyz = FO.unproject_points(avg, every, k, e).astype(np.float32).view(np.uint32)
        nrm = NR.normals(avg, every, k, e, 0.01).view(np.uint32)
        u8 = lambda m: torch.from_numpy(m.astype(np.uint8)).to(DEV)      # noqa: E731
        dev = (torch.from_numpy(avg).to(DEV), P._cam(k, e), torch.from_numpy(rgb).to(DEV), u8(photo), None if v == 1 else u8(geo))
        views.append(dict(xyz=xyz, nrm=nrm, rgb=rgb.reshape(-1, 3), photo=int(photo.sum()), geo=-1 if v == 1 else int(geo.sum()), dev=dev))
    return views


def _mask(kind, n, view):
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "first":
        m[0] = True
    elif kind == "block_heads":
        m[::BLOCK] = True
    elif kind == "random":
        m = np.random.default_rng(1000 + view).uniform(size=n) < 0.45
    else:
        assert kind == "none"
    return m


def _expected(views, masks, normals):
    """the records of the views back to back, and the rows of view_counts: photo, geo (-1: not given), final, first vertex"""
    mod = N if normals else P
    parts, rows, first = [], [], 0
    for view, m in zip(views, masks):
        rec = np.zeros(int(m.sum()), mod.RECORD)
        rec["xyz"], rec["rgb"] = view["xyz"][m], view["rgb"][m]
        if normals:
            rec["nrm"] = view["nrm"][m]
        parts.append(rec)
        rows.append([view["photo"], view["geo"], len(rec), first])
        first += len(rec)
    return np.concatenate(parts), rows


def _emit(views, masks, h, w, normals, capacity, guard):
    """the views through ONE cursor with no synchronisation in between -> (records below the capacity, guard bytes, cursor, counts)"""
    from itermvs_amd import ops
    size = 27 if normals else 15
    buf = torch.full((capacity * size + guard,), 0xA5, device=DEV, dtype=torch.uint8)
    cursor = torch.zeros(1, device=DEV, dtype=torch.int64)
    counts = torch.full((len(views), 4), -7, device=DEV, dtype=torch.int64)
    finals = [torch.from_numpy(m.reshape(h, w).astype(np.uint8)).to(DEV) for m in masks]
    call = ops.fuse_points_normals if normals else ops.fuse_points
    for i, (view, final) in enumerate(zip(views, finals)):
        avg, cam, rgb, photo, geo = view["dev"]
        call(avg, final, cam, rgb, buf, cursor, counts, i, photo, geo, capacity=capacity)
    host = buf.cpu().numpy()
    return host[:capacity * size], host[capacity * size:], int(cursor.item()), counts.cpu().numpy().tolist()


@pytest.mark.parametrize("blocks,kind", [(b, kind) for b in SHAPES for kind in MASKS])
def test_fuse_points_at_the_seams_of_the_scan(views_of, blocks, kind):
    h, w = SHAPES[blocks]
    views = views_of(h, w)
    masks = [_mask(kind, h * w, v) for v in range(N_VIEWS)]
    for normals in (False, True):
        want, rows = _expected(views, masks, normals)
        body, _, cursor, counts = _emit(views, masks, h, w, normals, len(want), 0)
        assert cursor == len(want) and counts == rows, (normals, counts, rows)
        mod = N if normals else P
        mod._same_records(np.frombuffer(body.tobytes(), mod.RECORD), want)


def test_fuse_points_capacity_one_short_of_the_total(views_of):
    """two chunks and one workgroup: the vertex that does not fit is the last one of the third view; every byte past the capacity
    keeps its fill and the totals count what exists"""
    h, w = SHAPES[2049]
    views = views_of(h, w)
    masks = [_mask("random", h * w, v) for v in range(N_VIEWS)]
    assert masks[-1][-CHUNK * BLOCK:].any()                               # the cut falls behind the second chunk's carry
    for normals in (False, True):
        want, rows = _expected(views, masks, normals)
        body, guard, cursor, counts = _emit(views, masks, h, w, normals, len(want) - 1, 4096)
        assert len(guard) == 4096 and (guard == 0xA5).all()
        assert cursor == len(want) and counts == rows
        mod = N if normals else P
        mod._same_records(np.frombuffer(body.tobytes(), mod.RECORD), want[:-1])


# -- the 64-bit scan of the mesh path ----------------------------------------------------------------------------------------------

DIMS, VOXEL, RADIUS = (65, 65, 66), 0.125, 3.9          # 278850 voxels = 1090 workgroups: workgroup 1024 starts at voxel 262144
ORIGIN = tuple(-0.5 * d * VOXEL for d in DIMS)


@pytest.fixture(scope="module")
def sphere():
    state = R.sdf_state(DIMS, ORIGIN, VOXEL, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - RADIUS)
    return state, R.mesh(state, DIMS, ORIGIN, VOXEL, 1)


def test_reference_mesh_lies_on_both_sides_of_the_chunk(sphere):
    """so that the device cannot be right with everything in one chunk.  Voxel 262144 lies in z-layer 62 (65 * 65 * 62 = 261950).  A
    vertex lies on an edge that starts at its owner voxel and runs towards +x, +y, +z: one with z above the centre of layer 63 has
    an owner in layer 63 or later (index >= 266175), one with z below the centre of layer 62 an owner before layer 62; a triangle is
    owned by the cell that holds its three vertices, by the same argument."""
    n = DIMS[0] * DIMS[1] * DIMS[2]
    assert -(-n // BLOCK) == 1090 and CHUNK * BLOCK == 262144 and 65 * 65 * 62 <= 262144 < 65 * 65 * 63
    vertices, faces = sphere[1]
    lo, hi = ORIGIN[2] + 62.5 * VOXEL, ORIGIN[2] + 63.5 * VOXEL
    z = vertices["z"].astype(np.float64)
    assert (z < lo).any() and (z > hi).any()
    fz = z[faces]
    assert (fz.max(axis=1) < lo).any() and (fz.min(axis=1) > hi).any()
    assert len(vertices) > 40000 and len(faces) > 80000


@pytest.mark.parametrize("short", [0, 1])
def test_tsdf_mesh_across_a_scan_chunk(sphere, short):
    state, want = sphere
    got = _mesh(state, DIMS, ORIGIN, VOXEL, 1, short=short)
    if short == 0:
        _assert_equal_mesh(got, want)
        return
    vertices, faces, totals, again, intact = got
    assert intact and list(totals) == again == [len(want[0]), len(want[1])]        # nothing past the capacities, the totals hold
    assert np.array_equal(vertices.view(np.uint8), want[0][:-1].view(np.uint8)) and np.array_equal(faces, want[1][:-1])

"""itermvs_mesh_simplify_* / fusion.simplify_mesh / fuse_scan(mesh=dict(simplify_voxels=...)) / eval.py --mesh_simplify /
simplify_mesh.py on the MI355X: vertex bytes and faces EQUAL to the restatement (tests/mesh_simplify_reference.py), every output
buffer between guard bytes."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

import mesh_simplify_reference as S
from conftest import ROOT
from test_mesh_simplify_cpu import RANDOM_CASES, corner_mesh, random_mesh, random_result, records_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
INT32_MAX = 2 ** 31 - 1


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def _upload(records, faces):
    records = np.ascontiguousarray(records, np.uint8)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    return records, faces, torch.from_numpy(records.reshape(-1).copy()).to(DEV), torch.from_numpy(faces.reshape(-1).copy()).to(DEV)


def device_simplify(records, faces, cell, origin=None, dims=None, vcap=None, fcap=None):
    """the sorts and launches of ``fusion.simplify_clusters``, then itermvs_mesh_simplify_emit into guarded buffers; capacities default
    to the true totals -> (vertex rows, faces, totals), what was stored below the capacities"""
    from itermvs_amd import fusion, ops
    records, faces, v, f = _upload(records, faces)
    nv, rec = records.shape
    xyz = v.view(nv, rec)[:, :12].contiguous().view(torch.float32) if nv else torch.empty((0, 3), device=DEV, dtype=torch.float32)
    if dims is None:
        grid = fusion.simplify_grid(xyz, cell, origin) if nv else ops.CloudGrid((0.0, 0.0, 0.0), (1, 1, 1), float(cell))
    else:
        grid = ops.CloudGrid(tuple(origin), tuple(dims), float(cell))
    reps, cluster, hi, lo, order, _ = fusion.simplify_clusters(v, f, rec, xyz, grid)
    totals = torch.zeros(2, device=DEV, dtype=torch.int64)
    emit = lambda *out, **cap: ops.mesh_simplify_emit(reps, rec, f, cluster, hi, lo, order, *out, **cap)      # noqa: E731
    emit(torch.empty(0, device=DEV, dtype=torch.uint8), torch.empty(0, device=DEV, dtype=torch.int32), totals)      # capacities 0
    kv, kf = totals.tolist()
    vcap, fcap = kv if vcap is None else vcap, kf if fcap is None else fcap
    vb, out_v = _guarded(vcap * rec, torch.uint8, 0xAB)
    fb, out_f = _guarded(fcap * 3, torch.int32, -7)
    tb, again = _guarded(2, torch.int64, -79)
    emit(out_v, out_f, again, vertex_capacity=vcap, face_capacity=fcap)
    torch.cuda.synchronize()
    assert _intact(vb, vcap * rec, 0xAB) and _intact(fb, fcap * 3, -7) and _intact(tb, 2, -79)
    assert again.tolist() == [kv, kf]
    got_v, got_f = out_v.cpu().numpy().reshape(-1, rec), out_f.cpu().numpy().reshape(-1, 3)
    return got_v[:min(vcap, kv)], got_f[:min(fcap, kf)], [kv, kf]


def check(records, faces, cell, origin=None, dims=None, want=None):
    """one mesh through the entry points and through ``fusion.simplify_mesh``, both equal to the restatement -> its result"""
    from itermvs_amd import fusion
    want_v, want_f, want_info = want if want is not None else S.simplify(records, faces, cell, origin, dims)
    got_v, got_f, totals = device_simplify(records, faces, cell, origin, dims)
    assert totals == [len(want_v), len(want_f)]
    assert got_f.dtype == np.int32 and np.array_equal(got_f, want_f)
    assert got_v.tobytes() == want_v.tobytes(), np.nonzero((got_v != want_v).any(1))[0][:10]
    records, faces, v, f = _upload(records, faces)
    info = {}
    out_v, out_f = fusion.simplify_mesh(v, f, cell, origin, info, record_bytes=records.shape[1], dims=dims)
    assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes()
    keys = ("vertices_before", "faces_before", "vertices", "faces", "clusters", "valid_faces", "degenerate_faces", "duplicate_faces",
            "cell", "origin", "dims")
    assert {k: info[k] for k in keys} == {k: want_info[k] for k in keys}
    return want_v, want_f, want_info


# -- tiny inputs ---------------------------------------------------------------------------------------------------------------
def test_tiny_inputs():
    none = np.zeros((0, 3), np.int32)
    v, f, info = check(np.zeros((0, 15), np.uint8), none, 0.5)
    assert len(v) == 0 and len(f) == 0 and info["clusters"] == 0
    v, f, info = check(np.zeros((0, 15), np.uint8), [[0, 1, 2], [0, 0, 0]], 0.5)                # no vertex: no face is valid
    assert len(f) == 0 and info["valid_faces"] == 0
    v, f, info = check(records_of(np.random.default_rng(0).random((7, 3))), none, 0.25)
    assert len(v) == 0 and info["clusters"] > 1
    rec = records_of([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 1.0, 0.5], [3.0, 3.0, 3.0]])
    v, f, info = check(rec, [[2, 0, 1]], 0.5)                                                    # one triangle
    assert f.tolist() == [[1, 0, 2]] and v.tobytes() == rec[[0, 2, 1]].tobytes()                # key order: x, then y, then z
    v, f, info = check(rec, [[2, 0, 1], [1, 2, 3]], 8.0)                                         # one cluster
    assert len(v) == 0 and len(f) == 0 and info["clusters"] == 1 and info["degenerate_faces"] == 2


# -- compaction seams: a strip with one vertex per cell -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip(n):
    """n vertices in n cells along x, numbered through a fixed permutation, n - 2 triangles; two unreferenced vertices and three
    invalid faces on top"""
    rng = np.random.default_rng(n)
    xyz = np.stack([np.arange(n) + 0.5, rng.random(n), rng.random(n)], 1)
    xyz = np.concatenate([xyz, [[n + 0.5, 0.5, 0.5], [n + 1.5, 0.5, 0.5]]])
    perm = rng.permutation(n + 2)
    inverse = np.argsort(perm)                                       # position along the strip -> vertex index
    i = np.arange(n - 2)
    faces = inverse[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)
    faces = np.insert(faces, [0, n // 2, n - 2], [[-1, 0, 1], [0, n + 2, 1], [0, 1, INT32_MAX]], axis=0)
    return records_of(xyz[perm], 15, n), faces


@pytest.mark.parametrize("count", [255, 256, 257, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, 70001])
@pytest.mark.parametrize("of", ["faces", "clusters"])
def test_compaction_seams(count, of):
    n = count + 2 if of == "faces" else count
    rec, faces = strip(n)
    v, f, info = check(rec, faces, 1.0, origin=(0.0, 0.0, 0.0))
    assert len(f) == n - 2 and len(v) == n and info["clusters"] == n + 2 and info["valid_faces"] == n - 2
    assert v.tobytes() == rec[np.argsort(S.coordinates(rec)[:, 0])][:n].tobytes()                # one member each: the records, in key order


# -- large clusters and long face segments ------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def fans():
    """for every size s: a cell (side 1) with s members and a fan of s triangles, each from a member to two of the 8 ring vertices in
    the 8 cells around it: s members and a face segment of s entries"""
    rng = np.random.default_rng(77)
    xyz, faces = [], []
    for k, s in enumerate(SIZES):
        base = len(xyz)
        corner = np.array([4.0 * k, 0.0, 0.0])
        xyz.extend(corner + 0.05 + 0.9 * rng.random((s, 3)))
        angle = np.arange(8) * np.pi / 4
        xyz.extend(corner + 0.5 + np.stack([np.cos(angle), np.sin(angle), 0.4 * rng.random(8) - 0.2], 1))
        ring = base + s
        faces.extend([base + j, ring + j % 8, ring + (j + 1) % 8] for j in range(s))
    perm = rng.permutation(len(xyz))
    return records_of(np.array(xyz)[perm], 15, 5), np.argsort(perm)[np.array(faces)].astype(np.int32)


def test_large_clusters_and_long_face_segments():
    rec, faces = fans()
    v, f, info = check(rec, faces, 1.0, origin=(-2.0, -2.0, -2.0))
    sizes = sorted(len(m) for m in info["members"])
    assert sizes == sorted(SIZES + (1,) * 8 * len(SIZES)) and info["degenerate_faces"] == 0
    assert len(v) == sum(1 + min(s + 1, 8) for s in SIZES)       # a fan of s triangles touches s + 1 ring vertices, 8 at the most
    assert len(f) == sum(min(s, 8) for s in SIZES)                  # a fan has 8 different triples, the rest repeat them
    again = device_simplify(rec, faces, 1.0, origin=(-2.0, -2.0, -2.0))                          # determinism: the same bytes
    assert again[0].tobytes() == v.tobytes() and again[1].tobytes() == f.tobytes()


def test_corner_mesh():
    rec, faces, cell, origin = corner_mesh()
    check(rec, faces, cell, origin=origin)


# -- odd content -----------------------------------------------------------------------------------------------------------------
def test_invalid_faces_bad_vertices_a_given_grid_degenerate_and_duplicate_faces():
    big = float(np.finfo(np.float32).max)
    xyz = [[0.2, 0.1, 0.1], [1.2, 0.1, 0.1], [2.2, 0.6, 0.1], [float("nan"), 0.0, 0.0], [0.3, 0.2, float("inf")], [-0.5, 0.1, 0.1],
           [2.4, 0.7, 0.3], [big, 0.5, 0.5], [0.5, -big, 0.5], [1.7, 0.9, 0.9], [3.0, 0.5, 0.5]]
    faces = [[0, 1, -1], [0, 1, 11], [INT32_MAX, 1, 2], [-2 ** 31, 0, 1], [0, 1, 3], [0, 4, 2], [0, 1, 5], [0, 1, 7], [8, 1, 2], [0, 1, 10],
             [2, 0, 1], [0, 1, 6], [1, 6, 0], [6, 1, 0], [0, 0, 1], [2, 6, 0], [1, 9, 2], [2, 2, 2]]
    v, f, info = check(records_of(xyz), faces, 1.0, origin=(0.0, 0.0, 0.0), dims=(3, 1, 1))
    assert info["cluster"].tolist() == [0, 1, 2, -1, -1, -1, 2, -1, -1, 1, -1]
    assert info["valid_faces"] == 8 and info["degenerate_faces"] == 4 and info["duplicate_faces"] == 2
    assert f.tolist() == [[2, 0, 1], [2, 1, 0]]
    # the default grid: the huge coordinates are vertices of it, and the products of the quadric leave the fp64 range
    v, f, info = check(records_of(xyz), faces + [[8, 0, 7], [7, 8, 1], [7, 1, 8]], 1e33)
    assert info["clusters"] == 3 and max(info["dims"]) > 300000 and f.tolist() == [[0, 1, 2], [2, 1, 0]]


def test_a_mesh_that_spans_too_many_cells_is_refused():
    from itermvs_amd import fusion
    rec, faces, v, f = _upload(records_of([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3e6, 0.0]]), [[0, 1, 2]])
    with pytest.raises(ValueError, match="spans .* cells of side 1.0; at most 2097152"):
        fusion.simplify_mesh(v, f, 1.0)


# -- capacities ------------------------------------------------------------------------------------------------------------------
def test_capacities_zero_exact_and_one_short():
    rec, faces, cell = random_mesh(2)
    rec, faces = np.concatenate([rec, strip(300)[0]]), np.concatenate([faces, strip(300)[1] + len(rec)])
    want_v, want_f, _ = S.simplify(rec, faces, cell)
    assert len(want_v) > 300 and len(want_f) > 298
    for vcap, fcap in ((0, 0), (None, None), (len(want_v) - 1, None), (None, len(want_f) - 1), (len(want_v) - 1, len(want_f) - 1),
                       (len(want_v) + 5, len(want_f) + 5)):
        got_v, got_f, totals = device_simplify(rec, faces, cell, vcap=vcap, fcap=fcap)           # the guards are checked inside
        assert totals == [len(want_v), len(want_f)]                                              # the totals stay true
        assert np.array_equal(got_v, want_v[:len(got_v)]) and len(got_v) == (len(want_v) if vcap is None else min(vcap, len(want_v)))
        assert np.array_equal(got_f, want_f[:len(got_f)]) and len(got_f) == (len(want_f) if fcap is None else min(fcap, len(want_f)))


# -- other records and inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec_bytes", [12, 15, 27, 64])
def test_record_sizes(rec_bytes):
    rec, faces, _ = random_mesh(9)
    v, f, info = check(records_of(S.coordinates(rec), rec_bytes, rec_bytes), faces, 0.3)
    assert v.shape[1] == rec_bytes and len(v) > 3 and max(len(m) for m in info["members"]) > 1


def test_the_random_meshes_of_the_cpu_file():
    for case in range(RANDOM_CASES):
        rec, faces, cell = random_mesh(case)
        check(rec, faces, cell, want=random_result(case))


# -- the whole scan ----------------------------------------------------------------------------------------------------------------
def _read(path):
    from itermvs_amd import fusion
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv, nf = int(re.search(rb"element vertex (\d+)", head).group(1)), int(re.search(rb"element face (\d+)", head).group(1))
    assert 15 * nv + 13 * nf == len(body)
    return raw, np.frombuffer(body[:15 * nv], np.uint8).reshape(nv, 15), np.frombuffer(body[15 * nv:], fusion.MESH_FACE)["v"]


def _fuse(tmp, name, **mesh):
    from itermvs_amd import fusion
    from test_mesh_components_cpu import SCENE as s, scan_arguments, scene_views
    views, _ = scene_views()
    info = {}
    path = os.path.join(tmp, name + "_mesh.ply")
    options = dict(path=path, bounds=s["bounds"], resolution=s["resolution"], min_count=s["min_count"], **mesh)
    fusion.fuse_scan(*scan_arguments(views), os.path.join(tmp, name + ".ply"), *(s["thresholds"][k] for k in
                     ("geo_pixel_thres", "geo_depth_thres", "photo_thres", "geo_mask_thres")), device=DEV, mesh=options, info=info)
    return path, open(os.path.join(tmp, name + ".ply"), "rb").read(), info["mesh"]


def _want_file(tmp, vertices, faces, cell):
    from itermvs_amd import fusion
    want_v, want_f, info = S.simplify(vertices, faces, cell)
    path = os.path.join(tmp, "want.ply")
    fusion.write_ply_mesh(path, want_v, want_f)
    return open(path, "rb").read(), info


def test_whole_scan_and_simplify_mesh_driver(tmp_path, capsys):
    from itermvs_amd import data_io, fusion
    tmp = str(tmp_path)
    plain_path, plain_cloud, plain_info = _fuse(tmp, "plain")
    capsys.readouterr()
    path, cloud, info = _fuse(tmp, "simple", simplify_voxels=2.0)
    line = [t for t in capsys.readouterr().out.splitlines() if t.startswith("simplified ")]
    raw, vertices, faces = _read(path)
    assert raw == open(plain_path, "rb").read() and cloud == plain_cloud                        # the mesh and the cloud keep their bytes
    assert not os.path.exists(fusion.simplified_path(plain_path)) and "simplified" not in plain_info
    cell = 2.0 * info["voxel"]
    want, want_info = _want_file(tmp, vertices, faces, cell)
    simplified = fusion.simplified_path(path)
    assert simplified.endswith("simple_mesh_simplified.ply") and open(simplified, "rb").read() == want
    assert 0 < want_info["faces"] < len(faces) / 4 and info["simplified"]["faces"] == want_info["faces"]
    assert len(line) == 1 and f"{len(faces)} -> {want_info['faces']} triangles" in line[0] and f"cell {cell!r}," in line[0]
    xyz, rgb, f = data_io.read_ply_mesh(simplified)                                              # reads back
    assert len(f) == want_info["faces"] and len(xyz) == want_info["vertices"] and np.isfinite(xyz).all()
    assert np.array_equal(np.unique(f), np.arange(len(xyz)))
    # simplify_mesh.py with the printed cell repeats the file
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import simplify_mesh
    out = os.path.join(tmp, "again.ply")
    got = simplify_mesh.main([path, out, "--cell", re.search(r"cell ([^,]+),", line[0]).group(1)])
    assert open(out, "rb").read() == want and got["faces"] == want_info["faces"]
    # with the component filter: the filtered mesh is the one that is simplified
    from test_mesh_components_cpu import SCENE
    kept_path, _, kept_info = _fuse(tmp, "kept", component_share=SCENE["component_share"], simplify_voxels=2.0)
    kept_raw, kept_vertices, kept_faces = _read(kept_path)
    assert len(kept_faces) < len(faces) and kept_info["faces"] == len(kept_faces)
    assert open(fusion.simplified_path(kept_path), "rb").read() == _want_file(tmp, kept_vertices, kept_faces, cell)[0]
    # a budget that holds the mesh but not the simplifier names the simplifier's buffers
    need = plain_info["need_bytes"] + len(vertices) * 15 + len(faces) * 12
    with pytest.raises(ValueError, match=r"simplifier of \d+ vertices and \d+ triangles needs \d+ bytes of keys and sort orders, "
                                         r"\d+ of representatives and \d+ of workspace .*budget is"):
        _fuse(tmp, "tight", simplify_voxels=2.0, budget_bytes=need + 1000)


def test_eval_driver_writes_the_simplified_mesh_beside_the_mesh(tmp_path, capsys):
    """eval.py --fuse_source memory --mesh --mesh_simplify 2 on a six-view scan of tests/test_fuse_memory_gpu.py"""
    from test_fuse_memory_gpu import _args, _eval_module, _files, write_scans
    from test_tsdf_gpu import BOUNDS, MESH
    data = tmp_path / "scans"
    data.mkdir()
    write_scans(str(data))
    E = _eval_module()
    runs = {}
    for name, extra in (("plain", []), ("simple", ["--mesh_simplify", "2"])):
        args = _args(data, tmp_path / name, ["--fuse_source", "memory"] + MESH + BOUNDS + extra)
        assert E.check_mesh(args) is True
        capsys.readouterr()
        E.fuse_memory(args)
        runs[name] = _files(str(tmp_path / name)), [t for t in capsys.readouterr().out.splitlines() if t.startswith("simplified ")]
    (plain, no_lines), (simple, lines) = runs["plain"], runs["simple"]
    assert set(simple) - set(plain) == {"scan1_mesh_simplified.ply", "scan2_mesh_simplified.ply"} and not no_lines and len(lines) == 2
    for name, raw in plain.items():
        assert simple[name] == raw, name                               # every other output byte
    for scan, line in zip(("scan1", "scan2"), lines):
        _, vertices, faces = _read(str(tmp_path / "simple" / (scan + "_mesh.ply")))
        cell = float(re.search(r"cell ([^,]+),", line).group(1))
        want, info = _want_file(str(tmp_path), vertices, faces, cell)
        assert simple[scan + "_mesh_simplified.ply"] == want and 0 < info["faces"] < len(faces)

"""itermvs_mesh_components / itermvs_mesh_keep / fusion.fuse_scan(mesh=dict(component_share=...)) / clean_mesh.py on the MI355X: labels,
counts, totals, kept vertex bytes and kept faces EQUAL to the restatement (tests/mesh_components_reference.py), every output buffer
between guard bytes.  The chain and the stars have no per-test time limit of their own (the suite has none): a walk that did not end
would stop at the time limit of the command that runs the suite."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import mesh_components_reference as M
from conftest import ROOT
from test_mesh_components_cpu import SCENE, check_census, scan_arguments, scene_views

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
INT32_MAX = 2 ** 31 - 1


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def _faces_on_device(faces):
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    return faces, torch.from_numpy(faces.reshape(-1).copy()).to(DEV)


def device_components(faces, nv):
    """itermvs_mesh_components through the C ABI into guarded buffers -> (label, face_count, totals) as numpy"""
    from itermvs_amd import _lib, ops
    faces, f = _faces_on_device(faces)
    lb, label = _guarded(nv, torch.int32, -77)
    cb, count = _guarded(nv, torch.int32, -78)
    tb, totals = _guarded(3, torch.int64, -79)
    at = lambda buf: buf.data_ptr() + GUARD * buf.element_size()   # noqa: E731  (an empty slice has no address of its own)
    _lib.check(_lib.load().itermvs_mesh_components(f.data_ptr() if len(faces) else None, len(faces), nv, at(lb), at(cb), at(tb),
                                                   ops._stream()), "itermvs_mesh_components")
    torch.cuda.synchronize()
    assert _intact(lb, nv, -77) and _intact(cb, nv, -78) and _intact(tb, 3, -79)
    return label.cpu().numpy(), count.cpu().numpy(), totals.tolist()


def device_keep(vertices, faces, label, count, min_faces, vcap=None, fcap=None):
    """itermvs_mesh_keep through ``ops.mesh_keep`` into guarded buffers; vertices uint8 [nv, record_bytes]; capacities default to the
    true totals -> (kept vertex rows, kept faces, totals), what was stored below the capacities"""
    from itermvs_amd import ops
    vertices = np.ascontiguousarray(vertices, np.uint8)
    nv, rec = vertices.shape
    faces, f = _faces_on_device(faces)
    v = torch.from_numpy(vertices.reshape(-1).copy()).to(DEV)
    lab, cnt = torch.from_numpy(np.ascontiguousarray(label, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(count, np.int32)).to(DEV)
    totals = torch.zeros(2, device=DEV, dtype=torch.int64)
    ops.mesh_keep(v, rec, f, lab, cnt, min_faces, torch.empty(0, device=DEV, dtype=torch.uint8), torch.empty(0, device=DEV, dtype=torch.int32),
                  totals)                                          # capacities 0: the totals alone
    kv, kf = totals.tolist()
    vcap, fcap = kv if vcap is None else vcap, kf if fcap is None else fcap
    vb, out_v = _guarded(vcap * rec, torch.uint8, 0xAB)
    fb, out_f = _guarded(fcap * 3, torch.int32, -7)
    tb, again = _guarded(2, torch.int64, -79)
    ops.mesh_keep(v, rec, f, lab, cnt, min_faces, out_v, out_f, again, vertex_capacity=vcap, face_capacity=fcap)
    torch.cuda.synchronize()
    assert _intact(vb, vcap * rec, 0xAB) and _intact(fb, fcap * 3, -7) and _intact(tb, 2, -79)
    assert again.tolist() == [kv, kf]
    got_v, got_f = out_v.cpu().numpy().reshape(-1, rec), out_f.cpu().numpy().reshape(-1, 3)
    return got_v[:min(vcap, kv)], got_f[:min(fcap, kf)], [kv, kf]


def records(nv, rec=15, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (nv, rec), dtype=np.uint8)


def check(faces, nv, min_faces=1, rec=15):
    """components and keep of one mesh, both equal to the restatement -> (label, count, totals, kept vertices, kept faces)"""
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    want = M.components(faces, nv)
    got = device_components(faces, nv)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), np.nonzero(got[0] != want[0])[0][:10]
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:10]
    assert got[2] == want[2]
    vertices = records(nv, rec)
    want_v, want_f = M.keep(vertices, faces, want[0], want[1], min_faces)
    got_v, got_f, totals = device_keep(vertices, faces, got[0], got[1], min_faces)
    assert totals == [len(want_v), len(want_f)]
    assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f) and got_f.dtype == np.int32
    return got + (got_v, got_f)


# -- tiny inputs ---------------------------------------------------------------------------------------------------------------
def test_tiny_inputs():
    label, count, totals, v, f = check(np.zeros((0, 3)), 0)
    assert len(label) == 0 and totals == [0, 0, 0] and len(v) == 0 and len(f) == 0
    assert check([[0, 0, 0], [1, 2, 3]], 0)[2] == [0, 0, 0]        # no vertex: no face is valid
    label, count, totals, v, f = check(np.zeros((0, 3)), 5)
    assert label.tolist() == [0, 1, 2, 3, 4] and count.tolist() == [0] * 5 and totals == [0, 0, 0] and len(v) == 0
    label, count, totals, v, f = check([[2, 0, 1]], 3)
    assert label.tolist() == [0, 0, 0] and count.tolist() == [1, 0, 0] and totals == [1, 1, 1] and f.tolist() == [[2, 0, 1]]
    label, count, totals, v, f = check([[5, 2, 3]], 8)
    assert label.tolist() == [0, 1, 2, 2, 4, 2, 6, 7] and count.tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and f.tolist() == [[2, 0, 1]]
    assert np.array_equal(v, records(8)[[2, 3, 5]])


def test_ops_wrapper_allocates_and_returns_the_same():
    from itermvs_amd import ops
    faces = np.array([[5, 2, 3], [0, 1, 1], [7, 7, 9]], np.int32)
    label, count, totals = ops.mesh_components(torch.from_numpy(faces).to(DEV), 8)
    want = M.components(faces, 8)
    assert label.cpu().tolist() == want[0].tolist() and count.cpu().tolist() == want[1].tolist() and totals.tolist() == want[2]
    label, count, totals = ops.mesh_components(torch.zeros(0, device=DEV, dtype=torch.int32), 0)
    assert label.numel() == 0 and count.numel() == 0 and totals.tolist() == [0, 0, 0]


# -- the chain: the largest diameter, the deepest trees ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip(permuted):
    n = 20000
    i = np.arange(n - 2, dtype=np.int32)
    faces = np.stack([i, i + 1, i + 2], 1)
    return (np.random.default_rng(20).permutation(n).astype(np.int32)[faces] if permuted else faces), n


@pytest.mark.parametrize("permuted", [False, True], ids=["along the strip", "permuted"])
def test_chain_of_20000_vertices(permuted):
    faces, n = strip(permuted)
    label, count, totals, v, f = check(faces, n)
    assert (label == 0).all() and count[0] == n - 2 and totals == [1, n - 2, n - 2] and len(v) == n and np.array_equal(f, faces)
    again = device_components(faces, n)                            # determinism: the same bytes
    assert again[0].tobytes() == label.tobytes() and again[1].tobytes() == count.tobytes() and again[2] == totals


# -- the stars: every hook lowers one root -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub_high", [False, True], ids=["hub 0", "hub highest"])
def test_star_of_10000_triangles(hub_high):
    n_tri = 10000
    nv = 2 * n_tri + 1
    i = np.arange(n_tri, dtype=np.int32)
    faces = np.stack([np.zeros_like(i), 2 * i + 1, 2 * i + 2], 1)
    if hub_high:
        faces = (nv - 1 - faces).astype(np.int32)
    label, count, totals, v, f = check(faces, nv)
    assert (label == 0).all() and count[0] == n_tri and totals == [1, n_tri, n_tri]
    again = device_components(faces, nv)
    assert again[0].tobytes() == label.tobytes() and again[1].tobytes() == count.tobytes() and again[2] == totals
    vertices = records(nv)
    a, b = (device_keep(vertices, faces, label, count, 1) for _ in range(2))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == [nv, n_tri]


# -- one shared vertex -------------------------------------------------------------------------------------------------------------
def _grid(rows, cols, first):
    """a triangulated rows x cols grid of vertices numbered from ``first``"""
    idx = first + np.arange(rows * cols).reshape(rows, cols)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)


def test_two_blobs_joined_by_one_vertex_and_the_same_with_it_duplicated():
    one, two = _grid(9, 11, 0), _grid(7, 13, 99)
    bridge = np.array([[98, 99, 100]], np.int32)                   # 98 is the first blob's last vertex, 99 and 100 the second's
    faces = np.concatenate([one, two, bridge])
    nv = 99 + 7 * 13
    label, count, totals, _, _ = check(faces, nv)
    assert (label == 0).all() and totals == [1, len(faces), len(faces)]
    apart = np.concatenate([one, two, np.array([[nv, 99, 100]], np.int32)])        # vertex 98 duplicated as a new last vertex
    label, count, totals, _, _ = check(apart, nv + 1)
    assert (label[:99] == 0).all() and (label[99:] == 99).all() and count[0] == len(one) and count[99] == len(two) + 1
    assert len(one) > len(two) + 1 and totals == [2, len(one), len(apart)]
    _, _, _, v, f = check(apart, nv + 1, min_faces=len(two) + 2)    # the second blob goes, with the duplicate
    assert len(v) == 99 and np.array_equal(f, one)


# -- many one-triangle components at the scan seams -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [255, 256, 257, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, 70001])
def test_one_triangle_components_at_the_scan_seams(nf):
    """component c owns the vertices 3c..3c+2 (numbered through a fixed permutation, so that neither the kept vertices nor the kept
    faces come in runs); every third has a second face, which alone passes min_faces = 2"""
    n_comp = nf                                                    # more than needed; the faces are cut at nf
    c = np.arange(n_comp, dtype=np.int64)
    first = np.stack([3 * c, 3 * c + 1, 3 * c + 2], 1)
    second = np.stack([3 * c + 2, 3 * c + 1, 3 * c], 1)[c % 3 == 0]
    order = np.argsort(np.concatenate([2 * c, 2 * c[c % 3 == 0] + 1]), kind="stable")      # the second face right after the first
    faces = np.concatenate([first, second])[order][:nf]
    nv = int(faces.max()) + 1 + 2                                  # and two unreferenced vertices at the end
    perm = np.random.default_rng(nf).permutation(nv)
    faces = perm[faces].astype(np.int32)
    label, count, totals, v, f = check(faces, nv, min_faces=2)
    doubles = int((count == 2).sum())
    assert totals[1] == 2 and totals[2] == nf and doubles in (nf // 4, nf // 4 + 1) and len(f) == 2 * doubles and len(v) == 3 * doubles


# -- invalid, degenerate and duplicate faces ----------------------------------------------------------------------------------------
def test_invalid_faces_are_ignored_and_degenerate_and_duplicate_faces_count():
    nv = 12
    faces = np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0],             # a face three times (once reversed): 3
                      [3, 3, 4], [4, 4, 4],                        # degenerate: (a, a, b) unites a and b, (a, a, a) unites nothing: 2
                      [5, 6, -1], [6, 7, nv], [7, 8, INT32_MAX], [-1, -1, -1], [nv, 0, 1], [INT32_MAX, 5, 6], [-2 ** 31, 9, 10],
                      [9, 9, 9]], np.int32)                        # the only valid face of vertex 9
    label, count, totals, v, f = check(faces, nv)
    assert label.tolist() == [0, 0, 0, 3, 3, 5, 6, 7, 8, 9, 10, 11]               # 5..8 and 10 are linked by invalid faces only
    assert count.tolist() == [3, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0] and totals == [3, 3, 6]
    assert f.tolist() == [[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [4, 4, 4], [5, 5, 5]] and len(v) == 6
    _, _, _, v, f = check(faces, nv, min_faces=2)
    assert f.tolist() == [[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [4, 4, 4]] and len(v) == 5


# -- thresholds ---------------------------------------------------------------------------------------------------------------------
def test_thresholds():
    faces = np.concatenate([_grid(3, 3, 0), _grid(4, 4, 9) + 0, _grid(2, 2, 25)])         # 8, 18 and 2 triangles; vertices 29..31 unreferenced
    nv = 32
    label, count, totals, v, f = check(faces, nv, min_faces=1)
    assert totals == [3, 18, 28] and len(v) == 29 and len(f) == 28                # min_faces 1 drops exactly the unreferenced vertices
    assert len(check(faces, nv, min_faces=8)[4]) == 26                            # count == min_faces is kept
    assert len(check(faces, nv, min_faces=9)[4]) == 18
    assert len(check(faces, nv, min_faces=18)[4]) == 18
    _, _, _, v, f = check(faces, nv, min_faces=totals[1] + 1)                     # largest + 1: nothing
    assert v.shape == (0, 15) and f.shape == (0, 3)
    _, _, kept = device_keep(records(nv), faces, label, count, INT32_MAX)
    assert kept == [0, 0]


# -- capacities ---------------------------------------------------------------------------------------------------------------------
def test_capacities_zero_exact_and_one_short():
    faces = np.concatenate([_grid(20, 30, 0), _grid(3, 3, 600), _grid(25, 17, 609)])
    nv = 609 + 25 * 17 + 3
    label, count, totals = M.components(faces, nv)
    vertices = records(nv)
    want_v, want_f = M.keep(vertices, faces, label, count, 9)
    assert 0 < len(want_v) < nv and 0 < len(want_f) < len(faces)
    for vcap, fcap in ((0, 0), (None, None), (len(want_v) - 1, None), (None, len(want_f) - 1), (len(want_v) - 1, len(want_f) - 1),
                       (len(want_v) + 5, len(want_f) + 5)):
        got_v, got_f, kept = device_keep(vertices, faces, label, count, 9, vcap, fcap)         # the guards are checked inside
        assert kept == [len(want_v), len(want_f)]                                              # the totals stay true
        assert np.array_equal(got_v, want_v[:len(got_v)]) and len(got_v) == (len(want_v) if vcap is None else min(vcap, len(want_v)))
        assert np.array_equal(got_f, want_f[:len(got_f)]) and len(got_f) == (len(want_f) if fcap is None else min(fcap, len(want_f)))


# -- record sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", [15, 27, 1, 64])
def test_record_sizes(rec):
    faces = np.concatenate([_grid(20, 30, 0), _grid(3, 3, 600), _grid(25, 17, 609)])
    _, _, _, v, f = check(faces, 609 + 25 * 17 + 3, min_faces=9, rec=rec)
    assert v.shape == (600 + 25 * 17, rec)


# -- the whole scan -------------------------------------------------------------------------------------------------------------
def _fuse(tmp, name, **mesh):
    from itermvs_amd import fusion
    s = SCENE
    views, _ = scene_views()
    info = {}
    path = os.path.join(tmp, name + "_mesh.ply")
    options = dict(path=path, bounds=s["bounds"], resolution=s["resolution"], min_count=s["min_count"], **mesh)
    fusion.fuse_scan(*scan_arguments(views), os.path.join(tmp, name + ".ply"), *(s["thresholds"][k] for k in
                     ("geo_pixel_thres", "geo_depth_thres", "photo_thres", "geo_mask_thres")), device=DEV, mesh=options, info=info)
    return open(path, "rb").read(), open(os.path.join(tmp, name + ".ply"), "rb").read(), info["mesh"]


def test_whole_scan_and_clean_mesh(tmp_path, capsys):
    from itermvs_amd import data_io, fusion
    tmp = str(tmp_path)
    plain_mesh, plain_cloud, plain_info = _fuse(tmp, "plain")
    share = SCENE["component_share"]
    kept_mesh, kept_cloud, info = _fuse(tmp, "kept", component_share=share)
    assert kept_cloud == plain_cloud                               # the cloud bytes are unchanged
    # the mesh file = write_ply_mesh of the restatement applied to the unfiltered mesh
    raw = plain_mesh.split(b"end_header\n", 1)[1]
    nv, nf = plain_info["vertices"], plain_info["faces"]
    vertices = np.frombuffer(raw[:15 * nv], fusion.MESH_VERTEX)
    faces = np.frombuffer(raw[15 * nv:], fusion.MESH_FACE)["v"]
    assert len(faces) == nf and 15 * nv + 13 * nf == len(raw)
    census = check_census(vertices, faces)                         # the GPU's mesh meets the conditions too
    want_v, want_f, want = M.clean(vertices, faces, 0, share)
    path = os.path.join(tmp, "want_mesh.ply")
    fusion.write_ply_mesh(path, want_v, want_f)
    assert kept_mesh == open(path, "rb").read() and len(kept_mesh) < len(plain_mesh)
    assert {k: info[k] for k in ("components", "largest", "min_faces", "kept_components", "vertices_before", "faces_before", "vertices",
                                 "faces")} == dict(components=want["components"], largest=want["largest"], min_faces=want["min_faces"],
                                                   kept_components=want["kept_components"], vertices_before=nv, faces_before=nf,
                                                   vertices=len(want_v), faces=len(want_f))
    assert "warning" not in info and "components" not in plain_info and census["min_faces"] == info["min_faces"]
    # both options 0: the bytes of a MeshOptions without the new fields
    off_mesh, off_cloud, off_info = _fuse(tmp, "off", min_component=0, component_share=0.0)
    assert off_mesh == plain_mesh and off_cloud == plain_cloud and "components" not in off_info
    # min_component alone, and the two together (a component must pass both)
    by_count, _, info_count = _fuse(tmp, "count", min_component=want["min_faces"])
    assert by_count == kept_mesh and info_count["min_faces"] == want["min_faces"]
    both, _, info_both = _fuse(tmp, "both", min_component=3, component_share=share)
    assert both == kept_mesh
    # everything removed: an empty mesh and a warning
    none, _, info_none = _fuse(tmp, "none", min_component=want["largest"] + 1)
    assert b"element vertex 0\n" in none and b"element face 0\n" in none and "empty mesh" in info_none["warning"]
    xyz, rgb, f = data_io.read_ply_mesh(os.path.join(tmp, "none_mesh.ply"))
    assert xyz.shape == (0, 3) and f.shape == (0, 3)
    # clean_mesh.py on the unfiltered file reproduces the filtered file
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import clean_mesh
    out = os.path.join(tmp, "cleaned.ply")
    got = clean_mesh.main([os.path.join(tmp, "plain_mesh.ply"), out, "--share", str(share)])
    assert open(out, "rb").read() == kept_mesh and got["faces"] == len(want_f)
    text = capsys.readouterr().out
    assert f"{want['components']} components" in text and f"at least {want['min_faces']} triangles" in text
    clean_mesh.main([os.path.join(tmp, "plain_mesh.ply"), out, "--min_faces", str(want["min_faces"])])
    assert open(out, "rb").read() == kept_mesh


def test_budget_names_the_labels_counts_and_workspace():
    from itermvs_amd import fusion
    faces = torch.from_numpy(_grid(20, 30, 0).reshape(-1)).to(DEV)
    vertices = torch.zeros(600 * 15, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"component filter .* 2400 bytes of labels, 2400 of counts and \d+ of workspace .*budget is 5000"):
        fusion.keep_mesh_components(vertices, faces, 1, 0.0, budget_bytes=5000, used_bytes=100)
    v, f = fusion.keep_mesh_components(vertices, faces, 1, 0.0, budget_bytes=1 << 20, used_bytes=100)
    assert v.numel() == 600 * 15 and f.numel() == faces.numel()

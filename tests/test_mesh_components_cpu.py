"""The component filter of the mesh (itermvs_mesh_components, itermvs_mesh_keep, eval.py --mesh_min_component / --mesh_component_share,
clean_mesh.py), the parts that need no GPU: the restatement (tests/mesh_components_reference.py) against scipy, the entry points'
statuses before any HIP call, the options and their formula, the argument checks, and the census of the scene that
tests/test_mesh_components_gpu.py fuses on the GPU."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import fusion_scenes as G
import mesh_components_reference as M
import tsdf_reference as T
from conftest import ROOT
from oracle import fusion_oracle as FO

NULL, DIMS, ALIGN = -1, -2, -5
_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16          # an aligned HOST address: every call below must be refused before it is used


# -- 1. the restatement against scipy ------------------------------------------------------------------------------------------
def random_mesh(rng, nv, nf, broken=0):
    """``nf`` random triangles over a random subset of the ``nv`` vertices (so that some stay unreferenced and the mesh falls into
    several components), ``broken`` of them with an index outside [0, nv)"""
    pool = rng.choice(nv, size=max(2, int(nv * rng.uniform(0.3, 1.0))), replace=False)
    blocks = np.array_split(rng.permutation(pool), rng.integers(1, 6))
    faces = np.stack([rng.choice(b, 3) for b in (blocks[i] for i in rng.integers(0, len(blocks), nf)) if len(b)]).astype(np.int32)
    for i in rng.choice(len(faces), size=min(broken, len(faces)), replace=False):
        faces[i, rng.integers(0, 3)] = rng.choice([-1, nv, 2 ** 31 - 1])
    return faces


def test_restatement_agrees_with_scipy():
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(5)
    several = 0
    for case in range(120):
        nv = int(rng.integers(2, 201))
        faces = random_mesh(rng, nv, int(rng.integers(1, 2 * nv)), broken=case % 3)
        label, count, totals = M.components(faces, nv)
        ok = faces[M.valid_faces(faces, nv)].astype(np.int64)
        rows, cols = np.concatenate([ok[:, 0], ok[:, 0]]), np.concatenate([ok[:, 1], ok[:, 2]])
        n, theirs = connected_components(sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv)), directed=False)
        # the same partition: each of their classes carries one of our labels and the numbers of classes agree
        assert len(np.unique(label)) == n
        assert all(len(np.unique(label[theirs == c])) == 1 for c in range(n))
        # and our label is the class minimum
        low = np.full(n, nv)
        np.minimum.at(low, theirs, np.arange(nv))
        assert np.array_equal(label, low[theirs].astype(np.int32)) and label.dtype == np.int32
        assert count.sum() == len(ok) == totals[2] and (count[label != np.arange(nv)] == 0).all()
        assert totals[0] == (count > 0).sum() and totals[1] == count.max()
        several += totals[0] > 1
    assert several > 60


def test_keep_rule_and_renumbering_by_hand():
    #            component {0,1,2,3}: 2 faces | vertex 4 unreferenced | component {5,6,7}: 1 face (with an invalid face beside it)
    faces = np.array([[2, 1, 0], [5, 6, 7], [3, 2, 2], [5, 6, 8], [-1, 0, 1]], np.int32)
    vertices = np.arange(8 * 15, dtype=np.uint8).reshape(8, 15)
    label, count, totals = M.components(faces, 8)
    assert label.tolist() == [0, 0, 0, 0, 4, 5, 5, 5] and count.tolist() == [2, 0, 0, 0, 0, 1, 0, 0] and totals == [2, 2, 3]
    v, f = M.keep(vertices, faces, label, count, 1)
    assert np.array_equal(v, vertices[[0, 1, 2, 3, 5, 6, 7]]) and f.tolist() == [[2, 1, 0], [4, 5, 6], [3, 2, 2]]
    v, f = M.keep(vertices, faces, label, count, 2)
    assert np.array_equal(v, vertices[:4]) and f.tolist() == [[2, 1, 0], [3, 2, 2]] and f.dtype == np.int32
    v, f = M.keep(vertices, faces, label, count, 3)
    assert len(v) == 0 and f.shape == (0, 3)


# -- 2. statuses before any HIP call -------------------------------------------------------------------------------------------
COMPONENTS = dict(faces=A, NF=4, NV=5, label=A, face_count=A, totals=A, stream=None)
KEEP = dict(vertices=A, NV=5, record_bytes=15, faces=A, NF=4, label=A, face_count=A, min_faces=1, out_vertices=A, vertex_capacity=2,
            out_faces=A, face_capacity=2, totals=A, workspace=A, stream=None)
SIZES = [("NV negative", dict(NV=-1), DIMS), ("NF negative", dict(NF=-1), DIMS), ("NF past the int32 flat bound", dict(NF=2 ** 31), DIMS),
         ("NF past 2^32", dict(NF=2 ** 32 + 4), DIMS)]
CASES = ([("itermvs_mesh_components", COMPONENTS, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("label", "face_count", "totals")] +
          [("faces null with NF 4", dict(faces=None), NULL), ("null before dims", dict(label=None, NV=-1), NULL),
           ("faces null with NF 0: still refused for NV", dict(faces=None, NF=0, NV=-2), DIMS)] + SIZES] +
         [("itermvs_mesh_keep", KEEP, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("vertices", "faces", "label", "face_count", "totals", "workspace", "out_vertices",
                                                    "out_faces")] +
          [("null before dims", dict(totals=None, record_bytes=0), NULL), ("faces null with NF 0: still refused for NV", dict(faces=None, NF=0, NV=-2), DIMS),
           ("vertices null with NV 0: still refused for min_faces", dict(vertices=None, NV=0, min_faces=0), DIMS)] + SIZES +
          [("record_bytes 0", dict(record_bytes=0), DIMS), ("record_bytes 65", dict(record_bytes=65), DIMS),
           ("min_faces 0", dict(min_faces=0), DIMS), ("min_faces negative", dict(min_faces=-4), DIMS),
           ("vertex capacity negative", dict(vertex_capacity=-1), DIMS), ("face capacity negative", dict(face_capacity=-1), DIMS),
           ("vertex capacity past int32", dict(vertex_capacity=2 ** 31), DIMS), ("dims before align", dict(workspace=A + 4, min_faces=0), DIMS),
           ("workspace unaligned", dict(workspace=A + 4), ALIGN)]])


@pytest.mark.parametrize("entry,valid,what,change,status", CASES, ids=[f"{c[0][8:]}-{c[2]}" for c in CASES])
def test_entry_status_before_any_hip_call(entry, valid, what, change, status):
    from itermvs_amd import _lib
    assert change, "a fully valid list is never passed"
    assert getattr(_lib.load(), entry)(*{**valid, **change}.values()) == status


def test_binding_header_makefile_and_workspace_bytes():
    from itermvs_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    for name, n_args in (("itermvs_mesh_components", 7), ("itermvs_mesh_keep_workspace_bytes", 3), ("itermvs_mesh_keep", 15)):
        assert name in _lib.PROTOTYPES and name + "(" in header and hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == n_args
    assert len(COMPONENTS) == 7 and len(KEEP) == 15
    assert _lib.ABI_VERSION == 20                                  # additions: the version stays
    makefile = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert makefile.count("mesh_components.hip") == 2              # SRCS and the resource-usage list
    assert ops.mesh_keep_workspace_bytes(0, 0) == 0 and ops.mesh_keep_workspace_bytes(1, 1) == 8 + 8 + 8
    assert ops.mesh_keep_workspace_bytes(256, 257) == 8 * 3 + 5 * 256 and ops.mesh_keep_workspace_bytes(257, 0) == 16 + 5 * 257 + 3
    n = C.c_int64(-1)
    assert lib.itermvs_mesh_keep_workspace_bytes(4, 4, None) == NULL and lib.itermvs_mesh_keep_workspace_bytes(-1, 4, C.byref(n)) == DIMS
    assert lib.itermvs_mesh_keep_workspace_bytes(4, 2 ** 31, C.byref(n)) == DIMS and n.value == -1
    assert lib.itermvs_mesh_keep_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, C.byref(n)) == 0 and n.value > 5 * (2 ** 31 - 1)


def test_ops_refuse_cpu_tensors():
    import torch
    from itermvs_amd import ops
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)        # noqa: E731
    with pytest.raises(RuntimeError, match="mesh_components: .*no CPU path"):
        ops.mesh_components(z(2, 3), 4)
    with pytest.raises(RuntimeError, match="mesh_keep: .*no CPU path"):
        ops.mesh_keep(z(60, dt=torch.uint8), 15, z(2, 3), z(4), z(4), 1, z(60, dt=torch.uint8), z(6), z(2, dt=torch.int64))


# -- 3. the options ------------------------------------------------------------------------------------------------------------
def test_mesh_options_validate_the_two_fields_and_off_changes_nothing():
    from itermvs_amd import fusion
    m = fusion.mesh_options(dict(path="m.ply"))
    assert m.min_component == 0 and m.component_share == 0.0       # off
    import dataclasses
    before = dict(path="m.ply", bounds=None, bounds_quantile=0.01, voxel=None, resolution=256, trunc_voxels=3.0, min_count=2,
                  budget_bytes=16 << 30, batch_views=4)
    assert {k: v for k, v in dataclasses.asdict(m).items() if k not in ("min_component", "component_share")} == before
    m = fusion.mesh_options(dict(path="m.ply", min_component=40, component_share=1.0))
    assert m.min_component == 40 and m.component_share == 1.0
    for bad in (dict(min_component=-1), dict(min_component=2.5), dict(min_component=True), dict(min_component=2 ** 31),
                dict(component_share=-0.01), dict(component_share=1.01), dict(component_share=float("nan")), dict(component_share="0.5"),
                dict(component_share=float("inf"))):
        with pytest.raises(ValueError, match="mesh: (min_component|component_share) must be"):
            fusion.mesh_options(dict(path="m.ply", **bad))


def test_min_faces_formula_at_ties():
    from itermvs_amd import fusion
    f = fusion.mesh_min_faces
    assert f(0, 0.5, 10) == 5 and f(0, 0.25, 12) == 3 and f(0, 1.0, 7) == 7          # share * largest an exact integer: that integer
    assert f(0, np.nextafter(0.5, 1.0), 10) == 6 and f(0, 0.5000001, 10) == 6         # just above one: the next
    assert f(0, np.nextafter(0.5, 0.0), 10) == 5
    assert f(0, 0.0, 10) == 1 and f(0, 0.5, 0) == 1 and f(0, 1e-9, 10) == 1           # never below 1
    assert f(7, 0.5, 10) == 7 and f(3, 0.5, 10) == 5 and f(4, 0.0, 0) == 4            # the larger of the two thresholds
    for args in ((0, 0.5, 10), (7, 0.3, 1001), (0, 1.0, 7), (2, 0.0, 5)):
        assert f(*args) == M.min_faces(*args)
    assert isinstance(f(0, 0.3, 1001), int) and f(0, 0.3, 1001) == 301


# -- 4. the argument checks ----------------------------------------------------------------------------------------------------
def _eval_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


ON_GPU = ["--filter", "--fuse_points", "device"]


@pytest.mark.parametrize("argv,word", [(ON_GPU + ["--mesh_min_component", "50"], "--mesh_min_component needs --mesh"),
                                       (ON_GPU + ["--mesh_component_share", "0.1"], "--mesh_component_share needs --mesh"),
                                       (ON_GPU + ["--mesh_component_share", "0"], "--mesh_component_share needs --mesh")])
def test_component_flags_without_mesh_are_argparse_errors(argv, word, capsys):
    E = _eval_module()
    with pytest.raises(SystemExit) as e:
        E.check_mesh(E.build_parser().parse_args(argv))
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_component_flags_reach_the_options_and_have_no_default():
    E = _eval_module()
    from itermvs_amd import fusion
    a = E.build_parser().parse_args(ON_GPU + ["--mesh"])
    assert a.mesh_min_component is None and a.mesh_component_share is None and E.check_mesh(a) is True
    m = fusion.mesh_options_from_args(a, "x.ply")
    assert m.min_component == 0 and m.component_share == 0.0
    a = E.build_parser().parse_args(ON_GPU + ["--mesh", "--mesh_min_component", "120", "--mesh_component_share", "0.02"])
    assert E.check_mesh(a) is True
    m = fusion.mesh_options_from_args(a, "x.ply")
    assert m.min_component == 120 and m.component_share == 0.02
    for bad, word in ((["--mesh_min_component", "-3"], "--mesh_min_component"), (["--mesh_component_share", "1.5"], "--mesh_component_share")):
        with pytest.raises(SystemExit) as e:
            E.check_mesh(E.build_parser().parse_args(ON_GPU + ["--mesh"] + bad))
        assert word in str(e.value)
    helps = {s: act.help for act in E.build_parser()._actions for s in act.option_strings}
    assert "No default" in helps["--mesh_min_component"] and "No default" in helps["--mesh_component_share"]
    assert "component filter" in helps["--mesh_budget_gb"]


def test_clean_mesh_needs_a_threshold(capsys):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import clean_mesh
    for argv, word in ((["a.ply", "b.ply"], "--min_faces N, --share F or both"), (["a.ply", "b.ply", "--share", "1.5"], "--share must be"),
                       (["a.ply", "b.ply", "--min_faces", "-2"], "--min_faces must be"), (["a.ply", "a.ply", "--share", "0.5"], "must not be IN.ply")):
        with pytest.raises(SystemExit) as e:
            clean_mesh.check_args(clean_mesh.build_parser().parse_args(argv))
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    clean_mesh.check_args(clean_mesh.build_parser().parse_args(["a.ply", "b.ply", "--min_faces", "3"]))


# -- 5. the scene of the GPU test and its census -----------------------------------------------------------------------------------
# tests/fusion_scenes.py's sphere (radius 55 at z = 400) in front of its wall, and a detached blob (radius 14) in front of the sphere.
# The volume holds the front of the sphere and the blob, not the wall.
SCENE = dict(h=48, w=80, views=6, seed=3, blob_centre=(40.0, -35.0, 300.0), blob_radius=14.0,
             bounds=(-75.0, -75.0, 270.0, 75.0, 75.0, 420.0), resolution=48, min_count=2, component_share=0.1,
             thresholds=dict(geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=2))


def scene_views():
    """``G.general_scene`` without noise, the blob ray-cast into every depth map it is nearer in -> (views, blob pixels per view)"""
    s = SCENE
    h, w = s["h"], s["w"]
    centre = np.array(s["blob_centre"])
    views, hits = [], []
    for (k, e, c), (k32, e32, d, _) in zip(G.cameras(h, w, s["views"], s["seed"]), G.general_scene(h, w, s["views"], s["seed"], 0.0)):
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        rw = e[:3, :3].T @ (np.linalg.inv(k) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)]))
        oc = c - centre
        qa, qb, qc = (rw * rw).sum(0), 2 * (oc @ rw), oc @ oc - s["blob_radius"] ** 2
        disc = qb * qb - 4 * qa * qc
        with np.errstate(invalid="ignore"):
            t = ((-qb - np.sqrt(disc)) / (2 * qa)).reshape(h, w)
        hit = (disc.reshape(h, w) > 0) & (t > 0) & (t < d)
        views.append((k32, e32, np.where(hit, t, d).astype(np.float32), np.full((h, w), 0.9, np.float32)))
        hits.append(int(hit.sum()))
    return views, hits


def scan_arguments(views):
    """the first five arguments of ``fusion.fuse_scan``"""
    n = len(views)
    pairs = [(v, [u for u in range(n) if u != v]) for v in range(n)]
    colours = {v: np.full((SCENE["h"], SCENE["w"], 3), 90 + 25 * v, np.uint8) for v in range(n)}
    return pairs, {v: views[v][:2] for v in range(n)}, {v: views[v][2] for v in range(n)}, {v: views[v][3] for v in range(n)}, colours


@functools.lru_cache(maxsize=1)
def scene_mesh():
    """the scene's mesh from the restatements alone (oracle/fusion_oracle.py, tests/tsdf_reference.py) -> (vertices, faces, hits)"""
    from itermvs_amd import fusion
    s = SCENE
    views, hits = scene_views()
    pairs, cams, _, _, colours = scan_arguments(views)
    depth, mask, cam, rgb = [], [], [], []
    for ref, _ in pairs:
        args, _ = G.split(views, ref)
        with np.errstate(all="ignore"):
            avg, photo, geo, _, _ = FO.fuse_reference_view(*args, **s["thresholds"])
        depth.append(avg.astype(np.float64))
        mask.append((photo & geo).astype(np.uint8))
        cam.append(np.concatenate([cams[ref][0].reshape(-1), cams[ref][1][:3].reshape(-1)]).astype(np.float32))
        rgb.append(colours[ref])
    plan = fusion.mesh_plan(s["bounds"], None, s["resolution"], 3.0, widen=False)
    state = T.integrate(T.empty_state(plan["dims"]), plan["dims"], plan["origin"], plan["voxel"], plan["trunc"], np.stack(depth),
                        np.stack(mask), np.stack(cam), np.stack(rgb))
    vertices, faces = T.mesh(state, plan["dims"], plan["origin"], plan["voxel"], s["min_count"])
    return vertices, faces, hits


def check_census(vertices, faces):
    """the conditions a mesh of the scene must meet for the filter to have something to do -> the restatement's info"""
    s = SCENE
    kept_v, kept_f, info = M.clean(vertices, faces, 0, s["component_share"])
    print(f"{len(vertices)} vertices, {len(faces)} triangles, {info['components']} components, largest {info['largest']}, min_faces "
          f"{info['min_faces']}, kept {info['kept_components']} components, {len(kept_v)} vertices, {len(kept_f)} triangles")
    assert info["components"] >= 2 and info["components"] - info["kept_components"] >= 1
    assert len(faces) - len(kept_f) >= 0.01 * len(faces) and len(kept_f) >= 0.5 * len(faces)
    # the blob is a component of its own and it is among the removed ones
    xyz = np.stack([vertices["x"], vertices["y"], vertices["z"]], 1).astype(np.float64)
    on_blob = np.linalg.norm(xyz - np.array(s["blob_centre"]), axis=1) < 1.5 * s["blob_radius"]
    blob = np.unique(info["label"][on_blob])
    assert on_blob.sum() > 50 and len(blob) >= 1
    assert (info["face_count"][blob] < info["min_faces"]).all() and info["face_count"][blob].max() > 100
    main = int(np.argmax(info["face_count"]))
    assert main not in blob.tolist()
    return info


def test_census_of_the_scene_fused_on_the_gpu():
    vertices, faces, hits = scene_mesh()
    assert sum(n > 20 for n in hits) >= SCENE["min_count"]         # the blob is seen by at least min_count views
    check_census(vertices, faces)

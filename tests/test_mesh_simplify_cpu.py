"""The mesh simplifier (itermvs_mesh_simplify_*, eval.py --mesh_simplify, simplify_mesh.py), the parts that need no GPU: the
restatement (tests/mesh_simplify_reference.py) on hand cases, properties over random meshes, a planar patch and a corner; the entry
points' statuses before any HIP call; the options and the argument checks."""
import ctypes as C
import fnmatch
import functools
import math
import os
import re
import sys

import numpy as np
import pytest

import mesh_simplify_reference as S
from conftest import ROOT

NULL, DIMS, ALIGN = -1, -2, -5
_BUF = (C.c_double * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16          # an aligned HOST address: every call below must be refused before it is used
INT32_MAX = 2 ** 31 - 1


def records_of(xyz, rec=15, seed=0):
    """uint8 [n, rec] records with the float32 coordinates ``xyz`` and random other bytes"""
    xyz = np.ascontiguousarray(xyz, "<f4").reshape(-1, 3)
    out = np.random.default_rng(seed).integers(0, 256, (len(xyz), rec), dtype=np.uint8)
    out[:, :12] = xyz.view(np.uint8).reshape(-1, 12)
    return out


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# -- 1. hand cases -------------------------------------------------------------------------------------------------------------
def test_two_triangles_in_one_cell_all_go():
    xyz = [[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1], [0.2, 0.2, 0.3]]
    v, f, info = S.simplify(records_of(xyz), [[0, 1, 2], [1, 3, 2]], 1.0, origin=(0.0, 0.0, 0.0))
    assert v.shape == (0, 15) and f.shape == (0, 3) and f.dtype == np.int32
    assert info["clusters"] == 1 and info["valid_faces"] == 2 and info["degenerate_faces"] == 2 and info["duplicate_faces"] == 0


def _three_cells(extra_faces):
    """vertices 0|1, 2|3, 4|5 pairwise in the cells 0, 1, 2 along x"""
    xyz = [[0.2, 0.1, 0.1], [0.4, 0.3, 0.1], [1.2, 0.1, 0.1], [1.4, 0.3, 0.2], [2.2, 0.6, 0.1], [2.4, 0.8, 0.3]]
    return S.simplify(records_of(xyz), extra_faces, 1.0, origin=(0.0, 0.0, 0.0))


def test_same_orientation_drops_the_later_and_the_opposite_orientation_stays():
    v, f, info = _three_cells([[0, 2, 4], [3, 5, 1], [5, 1, 2]])               # the same triple, rotated twice
    assert f.tolist() == [[0, 1, 2]] and len(v) == 3 and info["duplicate_faces"] == 2
    v, f, info = _three_cells([[3, 5, 1], [0, 4, 2], [4, 2, 1]])               # first face keeps ITS corner order; the twin is reversed
    assert f.tolist() == [[1, 2, 0], [0, 2, 1]] and info["duplicate_faces"] == 1 and info["degenerate_faces"] == 0


def test_invalid_faces_and_a_nan_vertex_are_ignored():
    xyz = [[0.2, 0.1, 0.1], [1.2, 0.1, 0.1], [2.2, 0.6, 0.1], [float("nan"), 0.0, 0.0], [0.3, 0.2, float("inf")], [-0.5, 0.1, 0.1]]
    faces = [[0, 1, -1], [0, 1, 6], [INT32_MAX, 1, 2], [0, 1, 3], [0, 4, 2], [0, 1, 5], [2, 0, 1]]
    v, f, info = S.simplify(records_of(xyz), faces, 1.0, origin=(0.0, 0.0, 0.0), dims=(3, 1, 1))
    assert info["valid_faces"] == 1 and f.tolist() == [[2, 0, 1]] and info["clusters"] == 3
    assert info["cluster"].tolist() == [0, 1, 2, -1, -1, -1]                    # NaN, inf and outside the given grid
    assert np.array_equal(v, records_of(xyz)[:3])


def test_one_member_cluster_keeps_its_15_bytes_and_a_larger_one_averages():
    xyz = [[0.2, 0.1, 0.1], [1.2, 0.1, 0.1], [2.2, 0.6, 0.1], [2.4, 0.8, 0.3]]
    rec = records_of(xyz)
    rec[2, 12:], rec[3, 12:] = (10, 11, 255), (13, 12, 254)
    v, f, info = S.simplify(rec, [[0, 1, 2], [0, 1, 3]], 1.0, origin=(0.0, 0.0, 0.0))
    assert np.array_equal(v[:2], rec[:2]) and f.tolist() == [[0, 1, 2]] and info["duplicate_faces"] == 1
    assert v[2, 12:].tolist() == [12, 12, 254]                                 # 11.5 -> 12, 11.5 -> 12, 254.5 -> 254: ties to even
    got = S.coordinates(v)[2]
    assert 2.0 <= got[0] <= 3.0 and 0.0 <= got[1] <= 1.0


def test_longer_records_copy_the_lowest_member_beyond_the_colours():
    xyz = [[0.2, 0.1, 0.1], [1.2, 0.1, 0.1], [2.4, 0.8, 0.3], [2.2, 0.6, 0.1]]
    for rec_bytes in (12, 14, 27):
        rec = records_of(xyz, rec_bytes, seed=rec_bytes)
        v, f, _ = S.simplify(rec, [[0, 1, 3]], 1.0, origin=(0.0, 0.0, 0.0))
        assert v.shape == (3, rec_bytes)
        keep_from = 15 if rec_bytes >= 15 else 12
        assert np.array_equal(v[2, keep_from:], rec[2, keep_from:])             # vertex 2 is the lowest member of its cell


# -- 2. properties over random meshes -----------------------------------------------------------------------------------------
def random_mesh(case):
    """-> (records uint8 [nv,15], faces int32 [nf,3], cell): NV 2..200 in the unit cube, some vertices not finite, some indices out of range"""
    rng = np.random.default_rng(1000 + case)
    nv = int(rng.integers(2, 201))
    xyz = rng.random((nv, 3)).astype(np.float32)
    if case % 4 == 1:
        xyz[rng.integers(0, nv)] = [np.nan, 0.5, 0.5]
        xyz[rng.integers(0, nv)] = [0.5, np.inf, 0.5]
    near = rng.integers(0, nv, (int(rng.integers(1, 3 * nv)), 1)) + rng.integers(-3, 4, (1, 3))
    faces = np.clip(near, 0, nv - 1).astype(np.int32) if case % 2 else rng.integers(0, nv, (len(near), 3)).astype(np.int32)
    for i in rng.choice(len(faces), size=min(case % 3, len(faces)), replace=False):
        faces[i, rng.integers(0, 3)] = rng.choice([-1, nv, INT32_MAX])
    return records_of(xyz, 15, case), faces, float(rng.choice([0.07, 0.15, 0.3, 0.55]))


RANDOM_CASES = 100


@functools.lru_cache(maxsize=None)
def random_result(case):
    rec, faces, cell = random_mesh(case)
    return S.simplify(rec, faces, cell)


def test_properties_of_random_meshes():
    dropped = 0
    for case in range(RANDOM_CASES):
        rec, faces, cell = random_mesh(case)
        v, f, info = random_result(case)
        assert f.dtype == np.int32 and v.dtype == np.uint8 and v.shape[1] == 15
        assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
        canonical = [tuple(np.roll(t, -int(np.argmin(t)))) for t in f]
        assert len(set(canonical)) == len(f)                                    # no two are cyclic rotations of each other
        assert np.array_equal(np.unique(f), np.arange(len(v)))                  # every output vertex is referenced
        # order: the survivors in ascending original face, the vertices in ascending cluster = ascending cell key
        cluster = info["cluster"]
        keys = S.cell_keys(S.coordinates(rec), info["origin"], info["dims"], cell)
        referenced = np.unique(cluster[cluster >= 0])[np.isin(np.unique(cluster[cluster >= 0]), [c for t in _cluster_triples(faces, cluster) for c in t])]
        want_faces = _survivors(faces, cluster)
        new = {int(c): i for i, c in enumerate(sorted({c for t in want_faces for c in t}))}
        assert f.tolist() == [[new[c] for c in t] for t in want_faces]
        first_key = {int(c): int(keys[cluster == c][0]) for c in new}
        assert sorted(first_key.values()) == [first_key[c] for c in sorted(new)] and set(new) <= set(referenced.tolist())
        # every representative lies within the cell's diagonal (plus one float32 ulp per axis) of each member: it is clamped to the cell
        out_xyz, xyz = S.coordinates(v).astype(np.float64), S.coordinates(rec).astype(np.float64)
        for c, i in new.items():
            members = xyz[info["members"][c]]
            slack = math.sqrt(3.0) * ulp32(np.abs(np.concatenate([members.ravel(), out_xyz[i]])).max())
            assert np.linalg.norm(members - out_xyz[i], axis=1).max() <= math.sqrt(3.0) * cell + slack
        assert info["faces"] == len(f) and info["vertices"] == len(v)
        assert info["valid_faces"] - info["degenerate_faces"] - info["duplicate_faces"] == len(f)
        dropped += info["degenerate_faces"] > 0 and info["duplicate_faces"] > 0
    assert dropped > 20                                                          # the cases do exercise both rules


def _cluster_triples(faces, cluster):
    nv = len(cluster)
    out = []
    for a, b, c in faces.tolist():
        if 0 <= a < nv and 0 <= b < nv and 0 <= c < nv and min(cluster[a], cluster[b], cluster[c]) >= 0:
            out.append((int(cluster[a]), int(cluster[b]), int(cluster[c])))
    return out


def _survivors(faces, cluster):
    """rule 5 once more, written differently: all three rotations of a kept triple are remembered"""
    kept, seen = [], set()
    for t in _cluster_triples(faces, cluster):
        if len(set(t)) == 3 and t not in seen:
            kept.append(t)
            seen.update({t, t[1:] + t[:1], t[2:] + t[:2]})
    return kept


def test_a_cell_below_the_vertex_spacing_returns_the_referenced_vertices_in_key_order():
    for case in range(20):
        rng = np.random.default_rng(case)
        lattice = rng.permutation(np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3))[:int(rng.integers(3, 100))]
        xyz = (lattice * 0.1 + rng.random(lattice.shape) * 0.02).astype(np.float32)      # two vertices differ by >= 0.06 on an axis
        rec = records_of(xyz, 15, case)
        faces = rng.integers(0, len(xyz), (3 * len(xyz), 3)).astype(np.int32)
        v, f, info = S.simplify(rec, faces, 0.03)
        assert info["clusters"] == len(xyz)
        used = np.unique(faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])])
        keys = S.cell_keys(xyz, info["origin"], info["dims"], 0.03)
        assert v.tobytes() == rec[used[np.argsort(keys[used], kind="stable")]].tobytes()


# -- 3. a planar patch and a corner --------------------------------------------------------------------------------------------
def _patch(n, at):
    """an n x n grid of vertices ``at(i, j)`` and its 2 (n - 1)^2 triangles"""
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    xyz = np.array([at(i, j) for i in range(n) for j in range(n)], np.float64)
    return xyz, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)


def test_planar_patch_stays_on_its_plane():
    e1, e2 = np.array([2.0, 1.0, 2.0]) / 3.0, np.array([-2.0, 2.0, 1.0]) / 3.0            # orthonormal; the normal is e1 x e2
    normal, p0, spacing = np.cross(e1, e2), np.array([3.0, -2.0, 5.0]), 0.37
    xyz, faces = _patch(8, lambda i, j: p0 + spacing * (i * e1 + j * e2))
    v, f, info = S.simplify(records_of(xyz), faces, 3 * spacing)
    assert 0 < len(f) < len(faces) and 3 < len(v) < 64
    # inputs are within (sqrt 3 / 2) ulp of the plane, so is a cell's mean; |y| is at most as much again (the right side is the
    # normal times offsets of that size, the matrix at least its square); the output is rounded once more: 3 ulp in all
    off = np.abs((S.coordinates(v).astype(np.float64) - p0) @ normal)
    assert off.max() <= 3 * ulp32(np.abs(xyz).max()), off.max()


def corner_mesh():
    """three 5 x 5 vertex patches (side 1, spacing 0.25) in the planes z = 0, x = 0, y = 0, each the cyclic image of the last, meeting
    at the origin; the cell [-0.125, 0.5)^3 holds the corner and 4 vertices of every patch"""
    parts, faces = [], []
    for k in range(3):
        xyz, f = _patch(5, lambda i, j: np.roll([0.25 * i, 0.25 * j, 0.0], k))
        faces.append(f + 25 * k)
        parts.append(xyz)
    return records_of(np.concatenate(parts)), np.concatenate(faces), 0.625, (-0.125, -0.125, -0.125)


def test_corner_is_kept_by_the_quadric_and_lost_by_the_mean():
    rec, faces, cell, origin = corner_mesh()
    v, f, info = S.simplify(rec, faces, cell, origin=origin)
    cluster = info["cluster"]
    at_corner = int(cluster[0])
    assert len(info["members"][at_corner]) == 12 and at_corner in np.unique(cluster[faces[_survivor_rows(faces, cluster)]])
    mu = S.coordinates(rec)[info["members"][at_corner]].astype(np.float64).mean(0)
    new = sorted({int(c) for t in _survivors(faces, cluster) for c in t}).index(at_corner)
    got = S.coordinates(v)[new].astype(np.float64)
    far = float(np.linalg.norm(mu))                                              # the corner is the origin
    # three equal eigenvalues s, lambda = 3 REG s: (s + lambda) y = s (corner - mu), so the rest is 3 REG / (1 + 3 REG) of |corner - mu|
    assert np.linalg.norm(got) <= 3 * S.REG / (1 + 3 * S.REG) * far + ulp32(0.125)
    # what the cell's mean would have cost: mu = (1/12, 1/12, 1/12), over 300 times farther from the corner
    assert abs(far - math.sqrt(3.0) / 12) < 1e-12 and np.linalg.norm(got) < far / 300


def _survivor_rows(faces, cluster):
    t = cluster[faces]
    return (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])


# -- 4. statuses before any HIP call -------------------------------------------------------------------------------------------
CORNERS = dict(faces=A, NF=4, NV=5, cluster=A, pair_cluster=A, key_hi=A, key_lo=A, stream=None)
CLUSTERS = dict(vertices=A, NV=5, record_bytes=15, faces=A, NF=4, keys_sorted=A, perm=A, cluster_sorted=A, pair_sorted=A, pair_face=A,
                ox=0.0, oy=0.0, oz=0.0, nx=4, ny=4, nz=4, cell=0.5, reps=A, stream=None)
EMIT = dict(reps=A, NV=5, record_bytes=15, faces=A, NF=4, cluster=A, key_hi_sorted=A, key_lo_sorted=A, order=A, out_vertices=A,
            vertex_capacity=2, out_faces=A, face_capacity=2, totals=A, workspace=A, stream=None)
SIZES = [("NV negative", dict(NV=-1), DIMS), ("NF negative", dict(NF=-1), DIMS), ("NF past a third of int32", dict(NF=INT32_MAX // 3 + 1), DIMS),
         ("NF past 2^32", dict(NF=2 ** 32 + 4), DIMS)]
RECORDS = [("record_bytes 11", dict(record_bytes=11), DIMS), ("record_bytes 65", dict(record_bytes=65), DIMS)]
CASES = ([("itermvs_mesh_simplify_corners", CORNERS, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("faces", "cluster", "pair_cluster", "key_hi", "key_lo")] +
          [("null before dims", dict(key_hi=None, NV=-1), NULL), ("faces null with NF 0: still refused for NV", dict(faces=None, NF=0, NV=-2), DIMS)] +
          SIZES] +
         [("itermvs_mesh_simplify_clusters", CLUSTERS, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("vertices", "faces", "keys_sorted", "perm", "cluster_sorted", "pair_sorted", "pair_face",
                                                    "reps")] +
          [("null before dims", dict(reps=None, cell=0.0), NULL)] + SIZES + RECORDS +
          [("cell 0", dict(cell=0.0), DIMS), ("cell negative", dict(cell=-1.0), DIMS), ("cell NaN", dict(cell=float("nan")), DIMS),
           ("cell inf", dict(cell=float("inf")), DIMS), ("origin NaN", dict(oy=float("nan")), DIMS), ("origin inf", dict(oz=float("-inf")), DIMS),
           ("grid dimension 0", dict(ny=0), DIMS), ("grid dimension 2^21 + 1", dict(nx=2 ** 21 + 1), DIMS)]] +
         [("itermvs_mesh_simplify_emit", EMIT, *c) for c in
          [(f"{n} null", {n: None}, NULL) for n in ("reps", "faces", "cluster", "key_hi_sorted", "key_lo_sorted", "order", "out_vertices",
                                                    "out_faces", "totals", "workspace")] +
          [("null before dims", dict(totals=None, record_bytes=0), NULL)] + SIZES + RECORDS +
          [("vertex capacity negative", dict(vertex_capacity=-1), DIMS), ("face capacity negative", dict(face_capacity=-1), DIMS),
           ("vertex capacity past int32", dict(vertex_capacity=2 ** 31), DIMS), ("dims before align", dict(workspace=A + 4, record_bytes=11), DIMS),
           ("workspace unaligned", dict(workspace=A + 4), ALIGN)]])


@pytest.mark.parametrize("entry,valid,what,change,status", CASES, ids=[f"{c[0][22:]}-{c[2]}" for c in CASES])
def test_entry_status_before_any_hip_call(entry, valid, what, change, status):
    from itermvs_amd import _lib
    assert change, "a fully valid list is never passed"
    assert getattr(_lib.load(), entry)(*{**valid, **change}.values()) == status


NAMES = (("itermvs_mesh_simplify_corners", CORNERS), ("itermvs_mesh_simplify_clusters", CLUSTERS), ("itermvs_mesh_simplify_emit", EMIT),
         ("itermvs_mesh_simplify_emit_workspace_bytes", dict(NV=0, NF=0, bytes=0)))


def test_binding_header_exports_makefile_and_workspace_bytes():
    from itermvs_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    exported = re.search(r"global:\s*([^;]+);", open(os.path.join(ROOT, "itermvs_amd", "csrc", "exports.map")).read()).group(1).split()
    for name, args in NAMES:
        assert name in _lib.PROTOTYPES and name + "(" in header and hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == len(args)
        assert any(fnmatch.fnmatchcase(name, pattern) for pattern in exported)
    assert _lib.ABI_VERSION == 20 and lib.itermvs_version() == 20                # additions: the version stays
    assert "#define ITERMVS_MESH_SIMPLIFY_REG 1e-3" in header and ops.MESH_SIMPLIFY_REG == S.REG == 1e-3
    makefile = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert makefile.count("mesh_simplify.hip") == 2                              # SRCS and the resource-usage list
    w = ops.mesh_simplify_emit_workspace_bytes
    assert w(0, 0) == 0 and w(1, 1) == 8 + 8 + 8 and w(256, 257) == 8 * 3 + 5 * 256 + 257 + 7 and w(257, 0) == 16 + 5 * 257 + 3
    n = C.c_int64(-1)
    q = lib.itermvs_mesh_simplify_emit_workspace_bytes
    assert q(4, 4, None) == NULL and q(-1, 4, C.byref(n)) == DIMS and q(4, INT32_MAX // 3 + 1, C.byref(n)) == DIMS and n.value == -1
    assert q(INT32_MAX, INT32_MAX // 3, C.byref(n)) == 0 and n.value > 5 * INT32_MAX


def test_ops_refuse_cpu_tensors():
    import torch
    from itermvs_amd import ops
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)        # noqa: E731
    with pytest.raises(RuntimeError, match="mesh_simplify_corners: .*no CPU path"):
        ops.mesh_simplify_corners(z(6), z(4))
    with pytest.raises(RuntimeError, match="mesh_simplify_clusters: .*no CPU path"):
        ops.mesh_simplify_clusters(z(60, dt=torch.uint8), 15, z(6), z(4, dt=torch.int64), z(4, dt=torch.int64), z(4), z(6), z(6),
                                   ops.CloudGrid((0.0, 0.0, 0.0), (1, 1, 1), 1.0))
    with pytest.raises(RuntimeError, match="mesh_simplify_emit: .*no CPU path"):
        ops.mesh_simplify_emit(z(60, dt=torch.uint8), 15, z(6), z(4), z(2, dt=torch.int64), z(2), z(2), z(60, dt=torch.uint8), z(6),
                               z(2, dt=torch.int64))


# -- 5. the options and the argument checks ------------------------------------------------------------------------------------
def test_simplify_problem_names_bad_options():
    from itermvs_amd import fusion
    p = fusion.simplify_problem
    assert p(0.5) is None and p(2, (0.0, 1, -3.5)) is None and p(np.float32(0.25), np.zeros(3)) is None
    for bad in (0, -1.0, float("nan"), float("inf"), "2", None, True):
        assert p(bad) == f"cell must be a finite number above 0, got {bad!r}"
    for bad in ((0.0, 1.0), (0.0, 1.0, float("nan")), (0.0, float("inf"), 1.0), "abc", 5, (0.0, 1.0, "2")):
        assert p(1.0, bad) == f"origin must be three finite numbers, got {bad!r}"
    with pytest.raises(ValueError, match="simplify_mesh: cell must be"):
        fusion.simplify_mesh(None, None, 0.0)
    with pytest.raises(ValueError, match="simplify_mesh: origin must be"):
        fusion.simplify_mesh(None, None, 1.0, origin=(1.0, 2.0))


def test_mesh_options_carry_simplify_voxels_and_off_changes_nothing():
    import dataclasses
    from itermvs_amd import fusion
    m = fusion.mesh_options(dict(path="out/scan_mesh.ply"))
    assert m.simplify_voxels == 0.0                                              # off
    m = fusion.mesh_options(dict(path="out/scan_mesh.ply", simplify_voxels=2, bounds=(0, 0, 0, 1, 1, 1)))
    assert m.simplify_voxels == 2 and fusion.simplified_path(m.path) == os.path.join("out", "scan_mesh_simplified.ply")
    assert "simplify_voxels" not in dataclasses.asdict(m)                        # the fields describe <scan>_mesh.ply, as before
    for bad in (-1.0, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="mesh: simplify_voxels must be a finite number above 0"):
            fusion.mesh_options(dict(path="m.ply", simplify_voxels=bad))


def _eval_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


ON_GPU = ["--filter", "--fuse_points", "device"]


@pytest.mark.parametrize("argv,word", [(ON_GPU + ["--mesh_simplify", "2"], "--mesh_simplify needs --mesh"),
                                       (ON_GPU + ["--mesh", "--mesh_simplify", "0"], "--mesh_simplify must be a finite cell side"),
                                       (ON_GPU + ["--mesh", "--mesh_simplify", "-2"], "--mesh_simplify must be a finite cell side"),
                                       (ON_GPU + ["--mesh", "--mesh_simplify", "nan"], "--mesh_simplify must be a finite cell side")])
def test_eval_flag_errors_are_argparse_errors(argv, word, capsys):
    E = _eval_module()
    with pytest.raises(SystemExit) as e:
        E.check_mesh(E.build_parser().parse_args(argv))
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_eval_flag_reaches_the_options_and_has_no_default():
    E = _eval_module()
    from itermvs_amd import fusion
    a = E.build_parser().parse_args(ON_GPU + ["--mesh"])
    assert a.mesh_simplify is None and E.check_mesh(a) is True and fusion.mesh_options_from_args(a, "x.ply").simplify_voxels == 0.0
    a = E.build_parser().parse_args(ON_GPU + ["--mesh", "--mesh_simplify", "1.5"])
    assert E.check_mesh(a) is True and fusion.mesh_options_from_args(a, "x.ply").simplify_voxels == 1.5
    helps = {s: act.help for act in E.build_parser()._actions for s in act.option_strings}
    assert "No default" in helps["--mesh_simplify"] and " 2 " in helps["--mesh_simplify"] and "simplifier" in helps["--mesh_budget_gb"]


def test_simplify_mesh_driver_argument_errors(capsys):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import simplify_mesh
    for argv, word in ((["a.ply", "b.ply"], "give --cell C"), (["a.ply", "b.ply", "--cell", "0"], "--cell must be a finite number above 0"),
                       (["a.ply", "b.ply", "--cell", "nan"], "--cell must be"), (["a.ply", "a.ply", "--cell", "0.5"], "must not be IN.ply")):
        with pytest.raises(SystemExit) as e:
            simplify_mesh.check_args(simplify_mesh.build_parser().parse_args(argv))
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    simplify_mesh.check_args(simplify_mesh.build_parser().parse_args(["a.ply", "b.ply", "--cell", "0.25"]))

"""numpy / Python restatement of the mesh simplifier (include/itermvs_hip.h: rules 1..6 of the itermvs_mesh_simplify_* section; host
side: itermvs_amd/fusion.py simplify_mesh), in the header's operation order: every sum and product is a Python float (IEEE fp64, one
rounding per operation, no contraction), taken in the written order; no ``linalg.solve``.  The outputs are compared with ``==``."""
import math

import numpy as np

REG = 1e-3                                 # ITERMVS_MESH_SIMPLIFY_REG
MAX_CELL_DIM = 1 << 21
NO_KEY = np.iinfo(np.int64).max


def coordinates(vertices):
    """uint8 [nv, record_bytes] records -> float32 [nv,3]"""
    vertices = np.ascontiguousarray(vertices, np.uint8)
    return np.ascontiguousarray(vertices[:, :12]).view("<f4").reshape(-1, 3)


def default_grid(xyz, cell, origin=None):
    """(origin, dims): the origin given or the per-axis minimum of the finite vertices; cells up to their maximum"""
    finite = xyz[np.isfinite(xyz).all(1)].astype(np.float64)
    if not len(finite):
        return (tuple(float(o) for o in origin) if origin is not None else (0.0, 0.0, 0.0)), (1, 1, 1)
    o = [float(v) for v in (finite.min(0) if origin is None else origin)]
    hi = finite.max(0)
    dims = [max(1, int(math.floor((float(hi[a]) - o[a]) / float(cell))) + 1) for a in range(3)]
    assert max(dims) <= MAX_CELL_DIM
    return tuple(o), tuple(dims)


def cell_keys(xyz, origin, dims, cell):
    """rule 1 and the key of csrc/cloud_grid.hpp: int64 [nv], NO_KEY for a vertex that is not finite or lies outside the grid"""
    with np.errstate(all="ignore"):
        c = np.floor((xyz.astype(np.float64) - np.array(origin, np.float64)) / np.float64(cell))
        inside = ((c >= 0) & (c < np.array(dims, np.float64))).all(1)                  # NaN: false
    ci = np.where(inside[:, None], c, 0).astype(np.int64)
    return np.where(inside, (ci[:, 0] * int(dims[1]) + ci[:, 1]) * int(dims[2]) + ci[:, 2], NO_KEY)


def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def representative(members, records, xyz, faces, face_list, cell_index, origin, cell):
    """rule 4 -> the record (uint8 [record_bytes]) of the cluster with ``members`` (ascending vertex indices) whose valid faces are
    ``face_list`` (ascending, once each)"""
    rec = records.shape[1]
    if len(members) == 1:
        return records[members[0]].copy()
    m = float(len(members))
    out = records[members[0]].copy()                                   # every byte from the 12th on: the lowest member's
    mu = []
    for axis in range(3):
        s = 0.0
        for v in members:
            s = s + float(xyz[v, axis])
        mu.append(s / m)
    if rec >= 15:
        for ch in (12, 13, 14):
            out[ch] = int(np.rint(float(sum(int(records[v, ch]) for v in members)) / m))
    axx = axy = axz = ayy = ayz = azz = rx = ry = rz = 0.0
    for f in face_list:
        a, b, c = (tuple(float(t) for t in xyz[i]) for i in faces[f])
        ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        vx, vy, vz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
        nx, ny, nz = (uy * vz) - (uz * vy), (uz * vx) - (ux * vz), (ux * vy) - (uy * vx)
        h = ((nx * (a[0] - mu[0])) + (ny * (a[1] - mu[1]))) + (nz * (a[2] - mu[2]))
        axx += nx * nx; axy += nx * ny; axz += nx * nz; ayy += ny * ny; ayz += ny * nz; azz += nz * nz      # noqa: E702
        rx += nx * h; ry += ny * h; rz += nz * h                                                            # noqa: E702
    trace = (axx + ayy) + azz
    lam = REG * trace
    a00, a11, a22 = axx + lam, ayy + lam, azz + lam
    c00, c01, c02 = (a11 * a22) - (ayz * ayz), (axz * ayz) - (axy * a22), (axy * ayz) - (axz * a11)
    c11, c12, c22 = (a00 * a22) - (axz * axz), (axy * axz) - (a00 * ayz), (a00 * a11) - (axy * axy)
    det = ((a00 * c00) + (axy * c01)) + (axz * c02)
    y = (0.0, 0.0, 0.0)
    if trace != 0.0 and math.isfinite(det) and det > 0.0:
        y = ((((c00 * rx) + (c01 * ry)) + (c02 * rz)) / det, (((c01 * rx) + (c11 * ry)) + (c12 * rz)) / det,
             (((c02 * rx) + (c12 * ry)) + (c22 * rz)) / det)
        if not all(math.isfinite(t) for t in y):
            y = (0.0, 0.0, 0.0)
    x = [clamp(mu[a] + y[a], origin[a] + float(cell_index[a]) * cell, origin[a] + float(cell_index[a] + 1) * cell) for a in range(3)]
    with np.errstate(over="ignore"):
        out[:12] = np.array(x, np.float64).astype("<f4").view(np.uint8)
    return out


def simplify(vertices, faces, cell, origin=None, dims=None):
    """rules 1..6 -> (vertices uint8 [k, record_bytes], faces int32 [m,3], info); ``vertices`` uint8 [nv, record_bytes]"""
    records = np.ascontiguousarray(vertices, np.uint8)
    nv = len(records)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    cell = float(cell)
    xyz = coordinates(records) if nv else np.zeros((0, 3), np.float32)
    if dims is None:
        origin, dims = default_grid(xyz, cell, origin)
    origin = tuple(float(o) for o in origin)
    keys = cell_keys(xyz, origin, dims, cell) if nv else np.zeros(0, np.int64)
    # rule 3: clusters in ascending key, members in ascending vertex index
    occupied = np.unique(keys[keys != NO_KEY])
    cluster = np.where(keys != NO_KEY, np.searchsorted(occupied, keys), -1)
    members = [[] for _ in occupied]
    for v in range(nv):
        if cluster[v] >= 0:
            members[cluster[v]].append(v)
    # rule 2, and every cluster's valid faces, once each, ascending
    face_lists = [[] for _ in occupied]
    triples = {}
    for f, (a, b, c) in enumerate(faces.tolist()):
        if not (0 <= a < nv and 0 <= b < nv and 0 <= c < nv) or min(cluster[a], cluster[b], cluster[c]) < 0:
            continue
        triples[f] = (int(cluster[a]), int(cluster[b]), int(cluster[c]))
        for k in dict.fromkeys(triples[f]):
            face_lists[k].append(f)
    # rule 5
    seen, survivors, degenerate = set(), [], 0
    for f, t in triples.items():                                        # ascending f
        if t[0] == t[1] or t[1] == t[2] or t[0] == t[2]:
            degenerate += 1
            continue
        k = t.index(min(t))
        canonical = t[k:] + t[:k]
        if canonical in seen:
            continue
        seen.add(canonical)
        survivors.append(t)
    # rule 6
    referenced = sorted({k for t in survivors for k in t})
    new = {k: i for i, k in enumerate(referenced)}
    out_faces = np.array([[new[k] for k in t] for t in survivors], np.int32).reshape(-1, 3)
    out_vertices = np.zeros((len(referenced), records.shape[1]), np.uint8)
    for i, k in enumerate(referenced):
        key = int(occupied[k])
        index = (key // dims[2] // dims[1], (key // dims[2]) % dims[1], key % dims[2])
        out_vertices[i] = representative(members[k], records, xyz, faces, face_lists[k], index, origin, cell)
    info = dict(vertices_before=nv, faces_before=len(faces), vertices=len(referenced), faces=len(survivors), clusters=len(occupied),
                valid_faces=len(triples), degenerate_faces=degenerate, duplicate_faces=len(triples) - degenerate - len(survivors),
                cell=cell, origin=origin, dims=tuple(int(d) for d in dims), cluster=cluster, members=members)
    return out_vertices, out_faces, info

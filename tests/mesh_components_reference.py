"""numpy / Python restatement of itermvs_mesh_components and itermvs_mesh_keep (include/itermvs_hip.h): a sequential union-find with
path halving that always keeps the smaller root, counts by ``np.bincount``, the keep rule and the renumbering.  TEST INFRASTRUCTURE
ONLY: nothing from the package.  tests/test_mesh_components_cpu.py checks it against scipy's connected_components."""
import math

import numpy as np


def valid_faces(faces, nv):
    """bool [NF]: all three indices in [0, nv)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < nv)).all(axis=1)


def labels(faces, nv):
    """-> int32 [nv]: the smallest vertex index of each vertex's component"""
    parent = list(range(nv))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]                          # path halving
            v = parent[v]
        return v

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for a, b, c in f[valid_faces(f, nv)].tolist():
        for x, y in ((a, b), (a, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)                  # the smaller root stays: the root is the set's minimum
    return np.array([find(v) for v in range(nv)], np.int32).reshape(nv)


def components(faces, nv):
    """-> (label int32 [nv], face_count int32 [nv], totals [3] = components with a face, largest count, valid faces)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    label = labels(f, nv)
    ok = valid_faces(f, nv)
    count = np.bincount(label[f[ok, 0]], minlength=nv).astype(np.int32) if nv else np.zeros(0, np.int32)
    return label, count, [int((count > 0).sum()), int(count.max()) if nv else 0, int(ok.sum())]


def min_faces(min_component, component_share, largest):
    return max(1, int(min_component), math.ceil(float(component_share) * largest))


def keep(vertices, faces, label, face_count, threshold):
    """vertices: any array with one row (or record) per vertex -> (kept vertices, kept faces int32 [m,3] renumbered)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(vertices)
    keep_v = face_count[label] >= threshold if nv else np.zeros(0, bool)
    rank = np.cumsum(keep_v) - keep_v
    ok = valid_faces(f, nv)
    ok[ok] = keep_v[f[ok, 0]]
    return vertices[keep_v], rank[f[ok]].astype(np.int32).reshape(-1, 3)


def clean(vertices, faces, min_component=0, component_share=0.0):
    """the whole filter -> (kept vertices, kept faces, info)"""
    label, count, totals = components(faces, len(vertices))
    threshold = min_faces(min_component, component_share, totals[1])
    v, f = keep(vertices, faces, label, count, threshold)
    return v, f, dict(components=totals[0], largest=totals[1], valid_faces=totals[2], min_faces=threshold,
                      kept_components=int((count >= threshold).sum()), label=label, face_count=count)

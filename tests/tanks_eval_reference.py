"""The yardstick of the Tanks and Temples evaluator: a numpy restatement of the passes of csrc/cloud_register.hip and of
itermvs_amd/cloud_register.py, written from their specification (fp64 on float32 coordinates, every expression in the stated
order of operations).  Not a test.  Nothing here uses a grid to decide a result: the nearest neighbour is brute force (a
bounding-box prefilter only drops targets that cannot be within the search radius)."""
import json
import math

import numpy as np

PLOT_STRETCH = 5
CURVE_BINS = 500
INT64_MAX = np.iinfo(np.int64).max


def apply_transform(T, pts):
    """float64 [n,3]: per row ((m0*x + m1*y) + m2*z) + m3"""
    m = np.asarray(T, dtype=np.float64)
    x, y, z = (np.asarray(pts)[:, a].astype(np.float64) for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], 1)


def crop_mask(pts, T, axis, axis_min, axis_max, polygon):
    """uint8 [n]: the even-odd crossing rule of include/itermvs_hip.h on c = T * p; a non-finite c is outside"""
    u, v = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    c = apply_transform(T, pts)
    poly = np.asarray(polygon, dtype=np.float64)
    ok = np.isfinite(c).all(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok &= (c[:, axis] >= axis_min) & (c[:, axis] <= axis_max)
        cu, cv = c[:, u], c[:, v]
        inside = np.zeros(len(c), dtype=bool)
        for k in range(len(poly)):
            a, b = poly[k], poly[(k + 1) % len(poly)]
            straddle = (a[v] > cv) != (b[v] > cv)
            if a[v] == b[v]:
                continue                                                  # never straddles: no division by zero to evaluate
            cross = cu < (((b[u] - a[u]) * (cv - a[v])) / (b[v] - a[v])) + a[u]
            inside ^= straddle & cross
    return (ok & inside).astype(np.uint8)


def voxel_keys(pts, voxel):
    """(keys int64 [n], dims): voxel floor((p - origin) / voxel), origin = min_bound - voxel / 2, key = (cx * ny + cy) * nz + cz"""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    origin = p.min(0) - voxel / 2
    dims = [int(math.floor((float(p[:, a].max()) - float(origin[a])) / voxel)) + 1 for a in range(3)]
    c = np.floor((p - origin) / voxel).astype(np.int64)
    assert (c >= 0).all() and (c < np.array(dims)).all()
    return (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2], dims


def voxel_mean(pts, voxel):
    """float32 [m,3] in ascending key order: per voxel the fp64 sum of its points in index order (from 0.0), divided by the
    count, rounded once.  A dict of index lists, summed one member at a time (vectorised across voxels, not within one)."""
    pts = np.asarray(pts, dtype=np.float32)
    pts = pts[np.isfinite(pts).all(1)]
    if len(pts) == 0:
        return pts
    keys, _ = voxel_keys(pts, voxel)
    members = {}
    for i, k in enumerate(keys.tolist()):
        members.setdefault(k, []).append(i)
    order = sorted(members)
    counts = np.array([len(members[k]) for k in order])
    sums = np.zeros((len(order), 3), dtype=np.float64)
    p64 = pts.astype(np.float64)
    for j in range(int(counts.max())):                                    # the j-th member of every voxel that has one
        rows = np.nonzero(counts > j)[0]
        sums[rows] = sums[rows] + p64[[members[order[r]][j] for r in rows]]
    return (sums / counts[:, None].astype(np.float64)).astype(np.float32)


def nn_index(queries64, targets, max_dist, chunk=128):
    """(idx int64 [nq], d2 float64 [nq]): the nearest target of each fp64 query with d2 < max_dist^2 (exclusive), the lowest
    index on a tie, else -1 / +Inf.  Brute force, for the queries of one cell of 2 * max_dist at a time, over the targets of a box around them."""
    q = np.asarray(queries64, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float32).astype(np.float64)
    nq = len(q)
    idx, d2 = np.full(nq, -1, dtype=np.int64), np.full(nq, np.inf)
    if len(t) == 0 or nq == 0:
        return idx, d2
    md2 = max_dist * max_dist
    finite = np.isfinite(q).all(1)
    cell = np.floor(np.where(finite[:, None], q, 0.0) / (2 * max_dist))
    _, group = np.unique(cell, axis=0, return_inverse=True)
    group = np.asarray(group).reshape(-1)
    order = np.argsort(group, kind="stable")
    order = order[finite[order]]
    cuts = np.nonzero(np.diff(group[order]))[0] + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(order)]])
    reach = max_dist * (1 + 1e-9) + 1e-300
    for a, e0 in zip(starts, ends):
        cell_rows = order[a:e0]
        cq = q[cell_rows]
        near = np.nonzero(((t >= cq.min(0) - reach) & (t <= cq.max(0) + reach)).all(1))[0]          # ascending original index
        if len(near) == 0:
            continue
        tt = np.ascontiguousarray(t[near].T)
        for s0 in range(0, len(cell_rows), chunk):
            rows = cell_rows[s0:s0 + chunk]
            qq = q[rows]
            dd = qq[:, 0:1] - tt[0][None, :]                                  # ((dx*dx) + (dy*dy)) + (dz*dz), in place
            dd *= dd
            for ax in (1, 2):
                da = qq[:, ax:ax + 1] - tt[ax][None, :]
                da *= da
                dd += da
            j = np.argmin(dd, 1)                                              # the first minimum: the lowest index
            best = dd[np.arange(len(rows)), j]
            hit = best < md2
            idx[rows[hit]], d2[rows[hit]] = near[j[hit]], best[hit]
    return idx, d2


def umeyama_terms(source, T, idx, d2, target):
    """float64 [m,18]: one row per correspondence idx >= 0, in query order: {1, p, t, t p^T (row t, column p), |p|^2, d2}"""
    rows = np.nonzero(idx >= 0)[0]
    p = apply_transform(T, np.asarray(source)[rows])
    t = np.asarray(target, dtype=np.float32)[idx[rows]].astype(np.float64)
    out = np.empty((len(rows), 18))
    out[:, 0] = 1.0
    out[:, 1:4], out[:, 4:7] = p, t
    for a in range(3):
        for b in range(3):
            out[:, 7 + a * 3 + b] = t[:, a] * p[:, b]
    out[:, 16] = ((p[:, 0] * p[:, 0]) + (p[:, 1] * p[:, 1])) + (p[:, 2] * p[:, 2])
    out[:, 17] = d2[rows]
    return out


def ordered_sum(terms, reverse=False):
    """the 18 sums, adding the rows one after the other in the given (or the reversed) order"""
    terms = terms[::-1] if reverse else terms
    acc = np.zeros(terms.shape[1])
    for block in range(0, len(terms), 4096):                              # cumsum adds sequentially; carry the accumulator across blocks
        acc = np.cumsum(np.vstack([acc[None], terms[block:block + 4096]]), 0)[-1]
    return acc


def umeyama(sums, with_scale=True):
    s = np.asarray(sums, dtype=np.float64)
    n = s[0]
    mu_p, mu_t = s[1:4] / n, s[4:7] / n
    cov = s[7:16].reshape(3, 3) / n - np.outer(mu_t, mu_p)
    var_p = s[16] / n - float(mu_p @ mu_p)
    u, d, vt = np.linalg.svd(cov)
    sgn = np.array([1.0, 1.0, 1.0 if np.linalg.det(u) * np.linalg.det(vt) >= 0 else -1.0])
    rot = (u * sgn) @ vt
    scale = float((d * sgn).sum() / var_p) if with_scale else 1.0
    out = np.eye(4)
    out[:3, :3] = scale * rot
    out[:3, 3] = mu_t - scale * (rot @ mu_p)
    return out


def umeyama_from_points(p, t, with_scale=True):
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    s = np.zeros(18)
    s[0], s[1:4], s[4:7] = len(p), p.sum(0), t.sum(0)
    s[7:16] = (t[:, :, None] * p[:, None, :]).sum(0).reshape(-1)
    s[16] = (p * p).sum()
    return umeyama(s, with_scale)


def icp(source, target, init, max_dist, max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6, reverse=False):
    """(T, fitness, rmse, updates): the loop of cloud_register.icp; ``reverse`` adds the correspondences in reversed order"""
    source = np.asarray(source, dtype=np.float32)
    T = np.array(init, dtype=np.float64)
    n = len(source)
    if n == 0:
        return T, 0.0, 0.0, 0
    prev, it = None, 0
    while True:
        idx, d2 = nn_index(apply_transform(T, source), target, max_dist)
        s = ordered_sum(umeyama_terms(source, T, idx, d2, target), reverse)
        m = s[0]
        fitness, rmse = float(m / n), (float(math.sqrt(s[17] / m)) if m > 0 else 0.0)
        if prev is not None and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            break
        if it >= max_iter or m < 3:
            break
        T = umeyama(s, True) @ T
        prev, it = (fitness, rmse), it + 1
    return T, fitness, rmse, it


def read_volume(json_path):
    with open(json_path) as f:
        d = json.load(f)
    return {"axis": "XYZ".index(d["orthogonal_axis"]), "axis_min": float(d["axis_min"]), "axis_max": float(d["axis_max"]),
            "polygon": np.asarray(d["bounding_polygon"], dtype=np.float64)}


def prepare(pts, vol, T, voxel):
    pts = np.asarray(pts, dtype=np.float32)
    keep = crop_mask(pts, np.eye(4) if T is None else T, vol["axis"], vol["axis_min"], vol["axis_max"], vol["polygon"]).astype(bool)
    kept = pts[keep]
    if T is not None:
        kept = apply_transform(T, kept).astype(np.float32)
    if voxel is not None:
        return voxel_mean(kept, voxel)
    stride = max(int(round(len(kept) / 16e6)), 1) if len(kept) > 16e6 else 1          # each cropped cloud by its own size
    return kept[::stride]


def capped_distance(src, dst, cap):
    """float64 [n]: min(distance to the nearest dst point, cap)"""
    _, d2 = nn_index(np.asarray(src, dtype=np.float32).astype(np.float64), dst, cap * (1 + 1e-6))
    return np.minimum(np.sqrt(d2), cap)


def cumulative_curve(dist, cap):
    edges = cap * (np.arange(1, CURVE_BINS + 1, dtype=np.float64) / CURVE_BINS)
    if len(dist) == 0:
        return np.zeros(CURVE_BINS), edges
    return np.searchsorted(np.sort(dist), edges, side="left").astype(np.float64) / len(dist), edges


def evaluate_scene(pred, gt, vol, init, tau, refine=True):
    T = np.array(init, dtype=np.float64)
    iterations = []
    if refine:
        for voxel, max_dist in ((tau, 80 * tau), (tau / 2, 20 * tau), (None, 2 * tau)):
            s, t = prepare(pred, vol, T, voxel), prepare(gt, vol, None, voxel)
            step, _, _, it = icp(s, t, np.eye(4), max_dist, 20)
            T = step @ T
            iterations.append(it)
    s, t = prepare(pred, vol, T, tau / 2), prepare(gt, vol, None, tau / 2)
    cap = PLOT_STRETCH * tau
    d_s, d_t = capped_distance(s, t, cap), capped_distance(t, s, cap)
    precision = float((d_s < tau).sum()) / len(s) if len(s) else 0.0
    recall = float((d_t < tau).sum()) / len(t) if len(t) else 0.0
    f = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    curve_s, edges = cumulative_curve(d_s, cap)
    curve_t, _ = cumulative_curve(d_t, cap)
    return {"precision": precision, "recall": recall, "fscore": f, "n_pred": len(s), "n_gt": len(t), "transform": T,
            "n_pred_below": int((d_s < tau).sum()), "n_gt_below": int((d_t < tau).sum()), "curve_pred": curve_s, "curve_gt": curve_t,
            "d_pred": d_s, "d_gt": d_t, "edges": edges, "iterations": iterations}

"""numpy restatement of the DTU evaluation scripts (evaluations/dtu/*.m of the reference), the yardstick of the cloud_eval
tests.  Written from the .m files and literal where it matters: the sequential loop of reducePts_haa.m over a dict-of-cells
neighbour list, the triple block loop of MaxDistCP.m with brute-force nearest neighbours per block, sub2ind indexing, the
filters of ComputeStat_web.m.  Clouds are [n,3] (the scripts hold them as 3 x n).  numpy only.

All arithmetic is float64 on float32 coordinates; the squared distance is ((dx*dx) + (dy*dy)) + (dz*dz), the distance its
sqrt (numpy evaluates the expression operation by operation, each correctly rounded)."""
import numpy as np


def d2_to_all(q, pts):
    """squared distances of one point q [3] to pts [m,3], float64, in the fixed order of operations"""
    dx, dy, dz = q[0] - pts[:, 0], q[1] - pts[:, 1], q[2] - pts[:, 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def matlab_round(x):
    """MATLAB's round: half away from zero (np.round rounds half to even)"""
    x = np.asarray(x, dtype=np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def cell_lists(pts, edge):
    """dict cell -> list of point indices, cells of edge ``edge`` anchored at the origin (finite points only)"""
    cells = {}
    c = np.floor(pts / edge)
    for i in range(pts.shape[0]):
        if np.isfinite(pts[i]).all():
            cells.setdefault((int(c[i, 0]), int(c[i, 1]), int(c[i, 2])), []).append(i)
    return cells, c


def range_search(pts, dst, edge_factor=1.5):
    """rangesearch(NS, pts', dst) for every point: idx[i] = the points with d2 <= dst*dst (the point itself included), from
    the 27 cells of edge 1.5 * dst around it.  A non-finite point has no neighbours and is nobody's neighbour."""
    pts = np.asarray(pts, dtype=np.float64)
    cells, c = cell_lists(pts, dst * edge_factor)
    idx = []
    for i in range(pts.shape[0]):
        if not np.isfinite(pts[i]).all():
            idx.append(np.zeros(0, dtype=np.int64))
            continue
        cand = []
        cx, cy, cz = int(c[i, 0]), int(c[i, 1]), int(c[i, 2])
        for x in (cx - 1, cx, cx + 1):
            for y in (cy - 1, cy, cy + 1):
                for z in (cz - 1, cz, cz + 1):
                    cand.extend(cells.get((x, y, z), ()))
        cand = np.asarray(cand, dtype=np.int64)
        idx.append(cand[d2_to_all(pts[i], pts[cand]) <= dst * dst])
    return idx


def reduce_points(pts, dst, order, idx=None):
    """reducePts_haa.m:8,24-30 with RandOrd = order: the sequential loop -> indexSet (bool [n]).  Non-finite points are never
    kept (the GPU evaluator's rule; the script does not meet them)."""
    pts = np.asarray(pts, dtype=np.float64)
    idx = range_search(pts, dst) if idx is None else idx
    index_set = np.isfinite(pts).all(1)
    for i in range(pts.shape[0]):
        ident = int(order[i])
        if index_set[ident]:
            index_set[idx[ident]] = False
            index_set[ident] = True
    return index_set


def reduce_points_rounds(pts, dst, order, idx=None):
    """the round formulation: all undecided points are updated once per sweep from the previous sweep's states -- kept when
    every earlier neighbour is removed, removed when some earlier neighbour is kept -> (indexSet, number of sweeps)"""
    pts = np.asarray(pts, dtype=np.float64)
    n = pts.shape[0]
    idx = range_search(pts, dst) if idx is None else idx
    rank = np.empty(n, dtype=np.int64)
    rank[np.asarray(order, dtype=np.int64)] = np.arange(n)
    state = np.where(np.isfinite(pts).all(1), 0, 2)           # 0 undecided, 1 kept, 2 removed
    sweeps = 0
    while (state == 0).any():
        new = state.copy()
        for i in np.nonzero(state == 0)[0]:
            earlier = idx[i][rank[idx[i]] < rank[i]]
            if (state[earlier] == 1).any():
                new[i] = 2
            elif (state[earlier] == 2).all():
                new[i] = 1
        state = new
        sweeps += 1
        assert sweeps <= n
    return state == 1, sweeps


def nn_brute(q_from, q_to, chunk=256):
    """distance of every q_from point to its nearest q_to point, brute force over all targets (inf without targets; NaN
    targets never win)"""
    q_from, q_to = np.asarray(q_from, dtype=np.float64), np.asarray(q_to, dtype=np.float64)
    q_to = q_to[np.isfinite(q_to).all(1)]
    out = np.full(q_from.shape[0], np.inf)
    if q_to.shape[0] == 0:
        return out
    for a in range(0, q_from.shape[0], chunk):
        q = q_from[a:a + chunk, None, :]
        dx, dy, dz = q[..., 0] - q_to[None, :, 0], q[..., 1] - q_to[None, :, 1], q[..., 2] - q_to[None, :, 2]
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        out[a:a + chunk] = np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(1))
    return out


def covered(q_from, bb, cap):
    """the queries some block of MaxDistCP.m looks at: bb[0] <= x < (bb[0] + Range * cap) + cap on every axis"""
    q_from, bb = np.asarray(q_from, dtype=np.float64), np.asarray(bb, dtype=np.float64)
    rng = np.floor((bb[1] - bb[0]) / cap)
    if (rng < 0).any():
        return np.zeros(q_from.shape[0], dtype=bool)
    hi = (bb[0] + rng * cap) + cap
    with np.errstate(invalid="ignore"):
        return ((q_from >= bb[0]) & (q_from < hi)).all(1)


def capped_nn(q_from, q_to, bb, cap):
    """what the GPU evaluator defines: min(brute-force nearest neighbour, cap) for covered queries, cap for the others"""
    d = np.minimum(nn_brute(q_from, q_to), cap)
    return np.where(covered(q_from, bb, cap), d, cap)


def max_dist_cp(q_to, q_from, bb, max_dist):
    """MaxDistCP.m, block by block: Dist(idxF) = distance to the nearest point of the block enlarged by MaxDist (knnsearch),
    MaxDist where that set is empty and for queries no block looks at.  Argument order as in the script (Qto, Qfrom)."""
    q_to, q_from, bb = np.asarray(q_to, dtype=np.float64), np.asarray(q_from, dtype=np.float64), np.asarray(bb, dtype=np.float64)
    dist = np.ones(q_from.shape[0]) * max_dist
    rng = np.floor((bb[1] - bb[0]) / max_dist)
    with np.errstate(invalid="ignore"):
        for x in range(0, int(rng[0]) + 1):
            for y in range(0, int(rng[1]) + 1):
                for z in range(0, int(rng[2]) + 1):
                    low = bb[0] + np.array([x, y, z], dtype=np.float64) * max_dist
                    high = low + max_dist
                    idx_f = np.nonzero(((q_from >= low) & (q_from < high)).all(1))[0]
                    low = low - max_dist
                    high = high + max_dist
                    idx_t = np.nonzero(((q_to >= low) & (q_to < high)).all(1))[0]
                    if idx_t.size == 0:
                        dist[idx_f] = max_dist
                    elif idx_f.size:
                        dist[idx_f] = nn_brute(q_from[idx_f], q_to[idx_t])
    return dist


def points_in_mask(pts, obs_mask, bb, res):
    """PointCompareMain.m:32-41 with sub2ind over size(ObsMask) (column-major linear index into the Fortran-order mask)"""
    pts, bb = np.asarray(pts, dtype=np.float64), np.asarray(bb, dtype=np.float64)
    sx, sy, sz = obs_mask.shape
    with np.errstate(invalid="ignore"):
        qv = matlab_round(((pts - bb[0]) / res) + 1)
        midx1 = np.nonzero((qv[:, 0] > 0) & (qv[:, 0] <= sx) & (qv[:, 1] > 0) & (qv[:, 1] <= sy) & (qv[:, 2] > 0) & (qv[:, 2] <= sz))[0]
    v = qv[midx1].astype(np.int64)
    midx_a = (v[:, 0] - 1) + sx * ((v[:, 1] - 1) + sy * (v[:, 2] - 1))          # sub2ind, zero-based
    flat = np.asarray(obs_mask).reshape(-1, order="F")
    midx2 = np.nonzero(flat[midx_a])[0]
    out = np.zeros(pts.shape[0], dtype=bool)
    out[midx1[midx2]] = True
    return out


def above_plane(pts, plane):
    """PointCompareMain.m:53: P' * [Qstl; 1] > 0, summed in the order ((P0*x + P1*y) + P2*z) + P3"""
    pts, p = np.asarray(pts, dtype=np.float64), np.asarray(plane, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (((p[0] * pts[:, 0] + p[1] * pts[:, 1]) + p[2] * pts[:, 2]) + p[3]) > 0


def compare_points(pred, gt, obs_mask, bb, res, plane, dst, order, cap=60.0, block_wise=False):
    """PointCompareMain.m -> dict(keep, Qdata, Ddata, Dstl, DataInMask, StlAbovePlane); ``block_wise``: the distances from the
    literal MaxDistCP restatement instead of min(brute force, cap)"""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    keep = reduce_points(pred, dst, order)
    qdata = pred[keep]
    if block_wise:
        ddata, dstl = max_dist_cp(gt, qdata, bb, cap), max_dist_cp(qdata, gt, bb, cap)
    else:
        ddata, dstl = capped_nn(qdata, gt, bb, cap), capped_nn(gt, qdata, bb, cap)
    return {"keep": keep, "Qdata": qdata, "Ddata": ddata, "Dstl": dstl, "DataInMask": points_in_mask(qdata, obs_mask, bb, res),
            "StlAbovePlane": above_plane(gt, plane)}


def matlab_median(x):
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    if n == 0:
        return float("nan")
    return float(x[n // 2]) if n % 2 else float((x[n // 2 - 1] + x[n // 2]) / 2)


def scan_statistics(ddata, dstl, data_in_mask, stl_above_plane, max_dist=20.0):
    """ComputeStat_web.m:52-68: mask / plane first, then < MaxDist; mean, var (n - 1), median"""
    d = np.asarray(ddata)[np.asarray(data_in_mask, dtype=bool)]
    d = d[d < max_dist]
    s = np.asarray(dstl)[np.asarray(stl_above_plane, dtype=bool)]
    s = s[s < max_dist]

    def mean(x):
        return float(np.mean(x)) if x.size else float("nan")

    def var(x):
        return float("nan") if x.size == 0 else (0.0 if x.size == 1 else float(np.var(x, ddof=1)))

    return {"nData": int(d.size), "nStl": int(s.size), "MeanData": mean(d), "MedData": matlab_median(d), "VarData": var(d),
            "MeanStl": mean(s), "MedStl": matlab_median(s), "VarStl": var(s)}


# ---- seeded scenes of the tests -------------------------------------------------------------------------------------------

def wavy_surface(n, gen, extent=24.0, z0=6.0, part=1.0):
    """n float32 samples of z = z0 + sin(x / 3) + cos(y / 4) over [0, part * extent) x [0, extent)"""
    xy = gen.random((n, 2)) * np.array([part * extent, extent])
    z = z0 + np.sin(xy[:, 0] / 3.0) + np.cos(xy[:, 1] / 4.0)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def make_scene(seed, n_gt=4000, n_pred=5000, extent=24.0, cap=4.0):
    """ground truth on a wavy surface; a prediction of 60 % of it (the rest of the ground truth is farther than cap from it) with near-duplicates, noise, outliers far outside bb, points on block and
    mask borders and a few NaN / Inf rows; a voxel mask that cuts the scene; a plane through it.  bb, res and cap are exactly
    representable, so the blocks of MaxDistCP have no rounding seams."""
    gen = np.random.default_rng(seed)
    gt = wavy_surface(n_gt, gen, extent)
    base = wavy_surface(max(n_pred // 5, 1), gen, extent, part=0.6)
    dup = np.repeat(base, 4, 0) + gen.normal(0, 0.05, (base.shape[0] * 4, 3))             # four near-duplicates per sample
    noisy = wavy_surface(max(n_pred // 10, 1), gen, extent, part=0.6) + gen.normal(0, 0.8, (max(n_pred // 10, 1), 3))
    far = gen.uniform(-300, 300, (max(n_pred // 50, 1), 3))
    f = extent / 24.0                                                          # bb and res grow with the scene
    bb = np.array([[-2.0, -2.0, 0.0], [26.0, 26.0, 12.0]]) * f
    res = 0.5 * f
    k = max(n_pred // 100, 4)
    on_blocks = np.stack([bb[0, 0] + cap * gen.integers(0, int(28 * f / cap) + 1, k), gen.uniform(0, extent, k), gen.uniform(3, 9, k)], 1)
    on_voxels = np.stack([bb[0, 0] + res * (gen.integers(-2, 60, k) - 0.5), bb[0, 1] + res * (gen.integers(-2, 60, k) + 0.5),
                          bb[0, 2] + res * (gen.integers(-2, 26, k) - 0.5)], 1)             # v = x.5 on every axis, some outside
    odd = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan, np.nan, np.nan]])
    pred = np.concatenate([dup, noisy, far, on_blocks, on_voxels, odd, bb[:1], bb[1:]], 0).astype(np.float32)
    pred = pred[gen.permutation(pred.shape[0])]
    size = np.floor((bb[1] - bb[0]) / res).astype(int) + 1
    gx, gy, gz = np.meshgrid(np.arange(size[0]), np.arange(size[1]), np.arange(size[2]), indexing="ij")
    obs_mask = (((gx + 2 * gy) % 7 != 0) & (gx > 4) & (gz < size[2] - 3)).astype(np.uint8)
    plane = np.array([0.05, -0.02, 1.0, -6.2])
    return {"gt": gt, "pred": pred, "bb": bb, "res": res, "obs_mask": obs_mask, "plane": plane, "cap": cap}

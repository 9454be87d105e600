"""A general scene for the fusion kernels, with the shape of result of tests/test_fusion.py:_scene, and the census that shows what
it holds.  TEST INFRASTRUCTURE ONLY: numpy and the restatements (oracle/fusion_oracle.py, tests/fuse_claim_reference.py), nothing
from the package.

``_scene`` is one tilted plane seen through ONE intrinsic matrix (fx == fy, no skew) by cameras that turn about the y axis only.
On it K_src and K_ref (and their inverses) can be swapped in a pair block without changing one output bit, 24 of a block's 60
floats are exactly zero, no pair has a depth edge and no point lies behind a camera.  ``general_scene`` has

  * per-view intrinsics: fx != fy in every view, skew in two views of three, distinct principal points;
  * look-at rotations from centres spread in x, y and z with a roll about the optical axis: no rotation block, no translation and
    no composed E_src inv(E_ref) holds an exact zero in rows 0..2;
  * a sphere in front of a tilted wall, ray-cast analytically in float64 (depth = camera-frame z), so that every front view sees
    the sphere's silhouette against the wall: depth edges and occlusion;
  * a LAST view behind the sphere, between it and the wall, looking at the wall: every sphere point has kz <= 0 in it (it alone
    does not see the silhouette: it is the view behind the surface).

The numbers differ from the first prototype of this scene in two places.  The sphere stands at z = 400 in front
of a wall at z ~ 1000 and the last view at z = 520 (prototype: 610, 700, 655): the last view is also used as a REFERENCE view, and
with 45 units between it and the wall a depth noise of 0.002 * 700 in the other maps is 3 % of its depth, so no pair would ever be
consistent with it; at 480 units it is 0.3 %.  And the prototype's centre (10, 5, 655) lies inside its sphere.
Views beyond the five base centres (and before the last) are jittered copies of them with intrinsics of their own.

``plant_edges`` writes the pixels that no ray-cast produces (special values, the clamp branch of ``remap_fixed``, a consistent
pixel whose nearest source pixel lies outside the map), ``census`` counts every case from the restatements alone."""
import numpy as np

import fuse_claim_reference as R
from oracle import fusion_oracle as FO

CENTRES = [(3.0, -2.0, 1.5), (90.0, 25.0, -20.0), (-80.0, 40.0, 15.0), (40.0, -70.0, 30.0), (-50.0, -45.0, -25.0)]
TARGET = (5.0, -3.0, 640.0)
SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 400.0]), 55.0
WALL_N, WALL_D = np.array([0.1, -0.05, 1.0]), 1000.0                # wall n.X = d in world coordinates
BEHIND_C, BEHIND_TARGET = (35.0, -20.0, 520.0), (-10.0, 12.0, 1000.0)
INT_MAX = 2.0 ** 31 - 1


def look_at(centre, target, roll_deg):
    """world -> camera [4,4] float64: optical axis towards ``target``, then a roll about it"""
    c, z = np.asarray(centre, np.float64), np.asarray(target, np.float64) - np.asarray(centre, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x = x / np.linalg.norm(x)
    r = np.stack([x, np.cross(z, x), z])
    a = np.deg2rad(roll_deg)
    r = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ r
    e = np.eye(4)
    e[:3, :3], e[:3, 3] = r, -r @ c
    return e


def cameras(h, w, n_views, seed):
    """-> [(K float64 [3,3], E float64 [4,4], centre)] of the n_views views; the last one (n_views >= 2) is the view behind"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for v in range(n_views):
        f = w * (1.1 + 0.07 * (v % 6) + 0.013 * (v // 6))
        k = np.array([[f, 0.8 * (v % 3), w / 2 + 1.3 - 0.37 * v], [0, f * (1 + 0.013 * (v + 1)), h / 2 - 0.7 + 0.53 * v], [0, 0, 1]])
        if v == n_views - 1 and n_views >= 2:
            k[0, 0], k[1, 1] = 0.55 * w, 0.55 * w * 1.021            # a wide view: it sees past every border of the front views
            c, e = np.array(BEHIND_C), look_at(BEHIND_C, BEHIND_TARGET, 7.0)
        else:
            c = np.array(CENTRES[v % 5]) + (rng.normal(0, 14.0, 3) if v >= 5 else 0.0)
            e = look_at(c, TARGET, 2.5 + 2.9 * v if v < 5 else rng.uniform(1.0, 15.0))
        out.append((k, e, c))
    return out


def general_scene(h, w, n_views, seed, noise):
    """-> per view (K float32 [3,3], E float32 [4,4], depth float32 [h,w], confidence float32 [h,w]), like ``_scene``"""
    rng = np.random.default_rng(seed)
    views = []
    for k, e, c in cameras(h, w, n_views, seed):
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        rays = np.linalg.inv(k) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
        rw = e[:3, :3].T @ rays                                     # world direction per unit of camera-frame z
        t_wall = (WALL_D - WALL_N @ c) / (WALL_N @ rw)
        oc = c - SPHERE_C
        qa, qb, qc = (rw * rw).sum(0), 2 * (oc @ rw), oc @ oc - SPHERE_R ** 2
        disc = qb * qb - 4 * qa * qc
        with np.errstate(invalid="ignore"):
            t_sph = (-qb - np.sqrt(disc)) / (2 * qa)                # the near intersection; X = c + t * rw, depth = t
        t = np.where((disc > 0) & (t_sph > 0) & (t_sph < t_wall), t_sph, t_wall)
        d = t.reshape(h, w).astype(np.float32)
        if noise:
            d = d * (1 + noise * rng.standard_normal(d.shape)).astype(np.float32)
        conf = rng.uniform(0, 1, (h, w)).astype(np.float32)
        views.append((k.astype(np.float32), e.astype(np.float32), d, conf))
    return views


def split(views, ref):
    """-> (the positional arguments of FO.fuse_reference_view / R.fuse_view_claim for views[ref] against all the others, others)"""
    k, e, d, conf = views[ref]
    others = [v for i, v in enumerate(views) if i != ref]
    return (d, conf, k, e, [o[2] for o in others], [o[0] for o in others], [o[1] for o in others]), others


def claim_maps(h, w, s, seed, planted=None):
    """the pre-filled claim maps of a case: (claimed_ref, 30 % marked; claimed_src, 10 % marked each); the reference pixels of
    ``planted`` are left unclaimed, so that they emit"""
    rng = np.random.default_rng(100 + seed)
    claimed_ref = (rng.uniform(size=(h, w)) < 0.3).astype(np.uint8)
    claimed_src = [(rng.uniform(size=(h, w)) < 0.1).astype(np.uint8) for _ in range(s)]
    for name, pos in (planted or {}).items():
        if isinstance(pos, tuple) and len(pos) == 2:
            claimed_ref[pos] = 0
    return claimed_ref, claimed_src


def pair_detail(d_ref, k_ref, e_ref, d_src, k_src, e_src):
    """one (reference, source) pair through the restatement's own functions -> dict of [H,W] maps: kz (float64, the source-space
    z the projection divides by), x_src, y_src (float32), dist (float32 pixel distance of the reprojection), rel (float32 relative
    depth difference)"""
    h, w = d_ref.shape
    m = FO.pair_matrices(k_ref, e_ref, k_src, e_src)
    x, y = np.meshgrid(np.arange(0, w), np.arange(0, h))
    d = d_ref.reshape(-1).astype(np.float64)
    with np.errstate(all="ignore"):
        kz = FO._mat3(m["k_src"], FO._mat4(m["t_rs"], FO._mat3(m["a_ref"], np.stack([x.reshape(-1) * d, y.reshape(-1) * d, d]))))[2]
        d_rep, x_rep, y_rep, x_src, y_src = FO.reproject_with_depth(d_ref, k_ref, e_ref, d_src, k_src, e_src)
        dist = np.sqrt((x_rep - x) ** 2 + (y_rep - y) ** 2)
        rel = np.abs(d_rep - d_ref) / d_ref
    return dict(kz=kz.reshape(h, w), x_src=x_src, y_src=y_src, dist=dist, rel=rel)


def _taps(x32, y32):
    """the four taps of FO.remap_bilinear at one float32 position -> [(iy, ix, float32 weight)]"""
    sx, sy = int(np.rint(np.float64(x32) * 32)), int(np.rint(np.float64(y32) * 32))
    ix, iy = sx >> 5, sy >> 5
    fx, fy = np.float32(sx & 31) * np.float32(1 / 32), np.float32(sy & 31) * np.float32(1 / 32)
    wx, wy = (np.float32(1) - fx, fx), (np.float32(1) - fy, fy)
    return [(iy + j, ix + i, wy[j] * wx[i]) for j in (0, 1) for i in (0, 1)]


def plant_edges(views, ref):
    """copies of the maps with the pixels written that the ray-cast cannot produce -> (views, planted): ``planted`` maps a name to
    the (y, x) it was written at in the REFERENCE map, or to (source index among the others, y, x) in a source map.
    Reference map (their confidence is set to 0.95, so that they pass every photometric threshold):
      nan, inf, zero, negative_zero, negative, tiny (1e-30): special depths;
      clamp: the float32 depth nearest to where the source-space z of that pixel vanishes for source 0 (sz = a * d + b is linear in
             d): the float64 source coordinate is then finite and far beyond 2^26 pixels, so ``remap_fixed`` saturates.
      The non-finite branch of ``remap_fixed`` is what ``nan`` and ``inf`` reach (inf * 0 and inf - inf in the products).
    Source maps 0 and 1 (one map when there is one): src_nan, src_zero, src_negative, src_inf at the first tap of four reference
      pixels that are consistent with that source under the strictest thresholds used (0.5 px, 0.005).
    outside: a reference pixel whose float32 source position rounds to a pixel OUTSIDE source map s, made consistent all the same:
      its taps inside the map are set to (true source depth) / (their weight sum), so the zero border is made up for.  Needs a
      reference pixel that projects into the half-pixel ring around a source map; None when the maps are too small to have one."""
    views = [(k.copy(), e.copy(), d.copy(), c.copy()) for k, e, d, c in views]
    (d, conf, k, e, srcs, ks, es), _ = split(views, ref)
    h, w = d.shape
    planted = {}
    free = [(y, x) for y in range(h) for x in range(w)]
    rng = np.random.default_rng(7 + h * w)
    rng.shuffle(free)
    detail = [pair_detail(d, k, e, ds, k2, e2) for ds, k2, e2 in zip(srcs, ks, es)]
    strict = [(p["dist"] < 0.5) & (p["rel"] < np.float32(0.005)) for p in detail]
    taken = set()

    def take(cond=lambda y, x: True):
        for y, x in free:
            if (y, x) not in taken and cond(y, x):
                taken.add((y, x))
                return y, x
        return None

    # a consistent pixel whose nearest source pixel is outside the map: first, it changes source pixels
    best = None
    for s, p in enumerate(detail):
        with np.errstate(invalid="ignore"):
            qx, qy = np.rint(p["x_src"]), np.rint(p["y_src"])
            ring = ((qx < 0) | (qx > w - 1) | (qy < 0) | (qy > h - 1)) & (p["x_src"] > -1) & (p["x_src"] < w) & (p["y_src"] > -1) \
                & (p["y_src"] < h) & (p["kz"] > 0)
        for y, x in zip(*np.nonzero(ring)):
            inside = [(ty, tx, wt) for ty, tx, wt in _taps(p["x_src"][y, x], p["y_src"][y, x]) if 0 <= ty < h and 0 <= tx < w and wt > 0]
            if not inside:
                continue
            support = sum(int(o[y, x]) for i, o in enumerate(strict) if i != s)
            weight = float(sum(wt for _, _, wt in inside))
            if best is None or (support, weight) > best[0]:
                best = ((support, weight), s, int(y), int(x), inside, float(p["kz"][y, x]))
    planted["outside"] = None
    if best is None:                                   # no such pixel: give one the depth that puts it at x_src = -0.75
        best = _solve_outside(d, k, e, srcs, ks, es, free)
    if best is not None:
        _, s, y, x, inside, kz = best
        for ty, tx, _ in inside:
            srcs[s][ty, tx] = np.float32(kz / sum(np.float64(wt) for _, _, wt in inside))
        taken.add((y, x))
        planted["outside"], planted["outside_source"] = (y, x), s
    # pixels of two source maps that consistent reference pixels sample
    for s in range(min(2, len(srcs))):
        for name, value in (("src_nan", np.nan), ("src_zero", 0.0), ("src_negative", -3.0), ("src_inf", np.inf)):
            p = detail[s]
            pos = take(lambda y, x: strict[s][y, x] and 1 <= p["x_src"][y, x] < w - 2 and 1 <= p["y_src"][y, x] < h - 2)
            if pos is None:
                continue
            ty, tx, _ = max(_taps(p["x_src"][pos], p["y_src"][pos]), key=lambda t: t[2])
            srcs[s][ty, tx] = np.float32(value)
            planted[f"{name}_{s}"] = (s, ty, tx)
            planted[f"{name}_{s}_sampled_by"] = pos
    # the reference map
    for name, value in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0), ("negative_zero", -0.0), ("negative", -250.0), ("tiny", 1e-30)):
        pos = take()
        if pos is not None:
            d[pos], planted[name] = np.float32(value), pos
    m = FO.pair_matrices(k, e, ks[0], es[0])
    a, t = m["a_ref"].astype(np.float64), m["t_rs"].astype(np.float64)
    planted["clamp"] = None
    for y, x in free:
        if (y, x) in taken:
            continue
        slope = t[2, :3] @ (a @ np.array([x, y, 1.0]))
        d0 = np.float32(-t[2, 3] / slope) if slope != 0 else np.float32(np.nan)
        if not np.isfinite(d0):
            continue
        trial = d.copy()
        trial[y, x] = d0
        p = pair_detail(trial, k, e, srcs[0], ks[0], es[0])
        if _branch(p["x_src"][y, x]) == "clamp" or _branch(p["y_src"][y, x]) == "clamp":
            d[y, x], planted["clamp"] = d0, (y, x)
            taken.add((y, x))
            break
    for name, pos in planted.items():
        if pos is not None and not name.startswith("src_") and name != "outside_source":
            conf[pos] = np.float32(0.95)
        if name.endswith("_sampled_by"):
            conf[pos] = np.float32(0.95)
    return views, planted


def _solve_outside(d, k, e, srcs, ks, es, free):
    """x_src = kx / kz with kx and kz linear in the reference depth: the depth at which a pixel lands at x_src = -0.75 in source 0,
    written into ``d`` for the first pixel where that depth is positive and the row lies inside -> the tuple ``plant_edges`` uses"""
    h, w = d.shape
    m = FO.pair_matrices(k, e, ks[0], es[0])
    a, t, k2 = m["a_ref"].astype(np.float64), m["t_rs"].astype(np.float64), m["k_src"].astype(np.float64)
    for y, x in free[:400]:
        u = t[:3, :3] @ (a @ np.array([x, y, 1.0]))
        den = k2[0] @ u + 0.75 * u[2]
        d0 = np.float32((-0.75 * t[2, 3] - k2[0] @ t[:3, 3]) / den) if den != 0 else np.float32(np.nan)
        if not (np.isfinite(d0) and d0 > 0):
            continue
        trial = d.copy()
        trial[y, x] = d0
        p = pair_detail(trial, k, e, srcs[0], ks[0], es[0])
        xs, ys, kz = p["x_src"][y, x], p["y_src"][y, x], p["kz"][y, x]
        if not (-1 < xs < -0.5 and 0 <= ys < h - 1 and kz > 0):
            continue
        inside = [(ty, tx, wt) for ty, tx, wt in _taps(xs, ys) if 0 <= ty < h and 0 <= tx < w and wt > 0]
        if inside:
            d[y, x] = d0
            return (0, 0.0), 0, int(y), int(x), inside, float(kz)
    return None


def _branch(c32):
    """which branch of ``remap_fixed`` a float32 coordinate takes: "nonfinite", "clamp" or "plain" """
    v = np.float64(c32) * 32.0
    if not np.isfinite(v):
        return "nonfinite"
    return "clamp" if abs(np.rint(v)) > INT_MAX else "plain"


def census(views, ref, thres, claimed_ref=None, edge_thres=0.01):
    """what the case holds, from the restatements alone -> dict of counts (pixels, or pixel-source pairs).  ``thres``: the four
    thresholds by name; claimed_ref: the claim map the reference view starts with (None: nothing is claimed)."""
    (d, conf, k, e, srcs, ks, es), _ = split(views, ref)
    h, w = d.shape
    s_n = len(srcs)
    with np.errstate(all="ignore"):
        avg, photo, geo, final, cnt = FO.fuse_reference_view(d, conf, k, e, srcs, ks, es, **thres)
    out = dict(histogram=np.bincount(cnt.ravel(), minlength=s_n + 1).tolist(), final_share=float(final.mean()))
    emit = final & (np.asarray(claimed_ref) == 0 if claimed_ref is not None else True)
    keys = ("behind", "outside_window", "clamp", "nonfinite", "only_distance", "only_depth", "edge_refused", "first_row_or_column",
            "last_row_or_column", "target_outside", "claims")
    out.update({key: 0 for key in keys})
    pix, dep = thres["geo_pixel_thres"], np.float32(thres["geo_depth_thres"])
    for ds, k2, e2 in zip(srcs, ks, es):
        p = pair_detail(d, k, e, ds, k2, e2)
        with np.errstate(all="ignore"):
            out["behind"] += int((p["kz"] <= 0).sum())
            window = (p["x_src"] > -1) & (p["x_src"] < w) & (p["y_src"] > -1) & (p["y_src"] < h)
            out["outside_window"] += int((np.isfinite(p["x_src"]) & np.isfinite(p["y_src"]) & ~window).sum())
            vx, vy = p["x_src"].astype(np.float64) * 32.0, p["y_src"].astype(np.float64) * 32.0
            out["nonfinite"] += int((~np.isfinite(vx) | ~np.isfinite(vy)).sum())
            out["clamp"] += int(((np.isfinite(vx) & (np.abs(np.rint(vx)) > INT_MAX)) | (np.isfinite(vy) & (np.abs(np.rint(vy)) > INT_MAX))).sum())
            near_px, near_d = p["dist"] < pix, p["rel"] < dep
            out["only_distance"] += int((~near_px & near_d).sum())
            out["only_depth"] += int((near_px & ~near_d).sum())
            ok, may, qy, qx = R.claim_targets(d, k, e, ds, k2, e2, pix, thres["geo_depth_thres"])
            _, loose, _, _ = R.claim_targets(d, k, e, ds, k2, e2, pix, thres["geo_depth_thres"], depth_condition=False)
            rx, ry = np.rint(p["x_src"]), np.rint(p["y_src"])
            inside = (rx >= 0) & (rx <= w - 1) & (ry >= 0) & (ry <= h - 1)
        assert np.array_equal(ok, near_px & near_d)
        out["edge_refused"] += int((emit & loose & ~may).sum())
        out["first_row_or_column"] += int((emit & may & ((qy == 0) | (qx == 0))).sum())
        out["last_row_or_column"] += int((emit & may & ((qy == h - 1) | (qx == w - 1))).sum())
        out["target_outside"] += int((emit & ok & ~inside).sum())
        out["claims"] += int((emit & may).sum())
    # the tangents of tests/fuse_normals_reference.py: which neighbours of an emitted pixel are usable
    with np.errstate(all="ignore"):
        a = avg.astype(np.float64)

        def usable(dy, dx):
            q = np.full((h, w), np.nan)
            ys, yd = (slice(1, h), slice(0, h - 1)) if dy == 1 else (slice(0, h - 1), slice(1, h)) if dy == -1 else (slice(0, h),) * 2
            xs, xd = (slice(1, w), slice(0, w - 1)) if dx == 1 else (slice(0, w - 1), slice(1, w)) if dx == -1 else (slice(0, w),) * 2
            q[yd, xd] = a[ys, xs]
            return np.isfinite(q) & (q > 0) & (np.abs(q - a) < edge_thres * a)

        good = final & np.isfinite(a) & (a > 0)
        for name, lo, hi in (("x", usable(0, -1), usable(0, 1)), ("y", usable(-1, 0), usable(1, 0))):
            out[f"normal_{name}_central"] = int((good & lo & hi).sum())
            out[f"normal_{name}_one_sided"] = int((good & (lo ^ hi)).sum())
            out[f"normal_{name}_none"] = int((good & ~lo & ~hi).sum())
    return out

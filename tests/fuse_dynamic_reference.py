"""numpy restatement of the level rule of ``itermvs_fuse_depth_dynamic`` (``eval.py --geo_consistency dynamic``) on top of
oracle/fusion_oracle.py and tests/fuse_claim_reference.py.  TEST INFRASTRUCTURE ONLY.  The reference project has no counterpart of
the rule; the per-source quantities are those of ``FO.check_geometric_consistency`` (eval.py:197-212), the average and the count
those of ``FO.fuse_reference_view`` (eval.py:238-269), the claim step that of ``R.fuse_view_claim``.

Contract, per reference pixel, with S source views (dtypes as in the kernel):
  dist_s  float64   sqrt((x_rep32 - x)^2 + (y_rep32 - y)^2), x and y int64                        eval.py:203
  rel_s   float32   |depth_rep32 - depth_ref32| / depth_ref32                                     eval.py:205-206
  ok_s              dist_s < geo_pixel_thres and rel_s < geo_depth_thres: average, count and claims, as without the rule
  pass_s(n)         dist_s < float64(n) * float64(a) and rel_s < float32(n) * float32(b)          strict; NaN fails
  c_n               number of s with pass_s(n)
  level             smallest n in [n_min, min(n_max, S)] with c_n >= n, else 0
  geo = level != 0; photo = conf > photo_thres; final = photo and geo and claimed_ref == 0"""
import numpy as np

import fuse_claim_reference as R
from oracle import fusion_oracle as FO

DEFAULTS = dict(a=0.25, b=float(np.float32(1.0 / 1300.0)), n_min=2, n_max=10)


def pair_errors(depth_ref, k_ref, e_ref, depth_src, k_src, e_src):
    """one (reference, source) pair -> (dist float64 [H,W], rel float32 [H,W]) by the expressions of
    ``FO.check_geometric_consistency``"""
    h, w = depth_ref.shape
    x_ref, y_ref = np.meshgrid(np.arange(0, w), np.arange(0, h))
    depth_rep, x_rep, y_rep, _, _ = FO.reproject_with_depth(depth_ref, k_ref, e_ref, depth_src, k_src, e_src)
    with np.errstate(all="ignore"):
        dist = np.sqrt((x_rep - x_ref) ** 2 + (y_rep - y_ref) ** 2)
        rel = np.abs(depth_rep - depth_ref) / depth_ref
    assert dist.dtype == np.float64 and rel.dtype == np.float32
    return dist, rel


def level_map(dists, rels, a, b, n_min, n_max):
    """the accepting level of every pixel (uint8 [H,W], 0: none) from the S pairs' (dist, rel)"""
    s = len(dists)
    level = np.zeros(dists[0].shape, np.uint8)
    for n in range(int(n_min), min(int(n_max), s) + 1):
        pixel, depth = np.float64(n) * np.float64(a), np.float32(n) * np.float32(b)
        assert pixel.dtype == np.float64 and depth.dtype == np.float32
        with np.errstate(invalid="ignore"):
            c_n = sum(((d < pixel) & (r < depth)).astype(np.int32) for d, r in zip(dists, rels))
        level = np.where((level == 0) & (c_n >= n), np.uint8(n), level).astype(np.uint8)
    return level


def fuse_view_dynamic(depth_ref, conf_ref, k_ref, e_ref, src_depths, src_ks, src_es, claimed_ref=None, claimed_src=None,
                      geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, a=DEFAULTS["a"], b=DEFAULTS["b"],
                      n_min=DEFAULTS["n_min"], n_max=DEFAULTS["n_max"]):
    """one reference view.  claimed_ref: uint8 [H,W] or None (all zero); claimed_src: S uint8 [H,W] maps or None (no claims).
    -> ((depth_avg float64, photo, geo, final bool, count int32, level uint8), updated COPIES of the source claim maps (None if
        not given), claims: per source (pixel index p of the claiming reference pixels, pixel index q they claim))"""
    h, w = depth_ref.shape
    with np.errstate(all="ignore"):
        avg, photo, _, _, cnt = FO.fuse_reference_view(depth_ref, conf_ref, k_ref, e_ref, src_depths, src_ks, src_es,
                                                       geo_pixel_thres, geo_depth_thres, photo_thres, 0)
        errors = [pair_errors(depth_ref, k_ref, e_ref, d, k, e) for d, k, e in zip(src_depths, src_ks, src_es)]
    level = level_map([d for d, _ in errors], [r for _, r in errors], a, b, n_min, n_max)
    geo = level != 0
    final = photo & geo
    if claimed_ref is not None:
        final = final & (np.asarray(claimed_ref) == 0)
    if claimed_src is None:
        return (avg, photo, geo, final, cnt, level), None, []
    out, claims = [np.array(c, dtype=np.uint8, copy=True) for c in claimed_src], []
    for s, (d_src, k_src, e_src) in enumerate(zip(src_depths, src_ks, src_es)):
        with np.errstate(all="ignore"):
            _, may, qy, qx = R.claim_targets(depth_ref, k_ref, e_ref, d_src, k_src, e_src, geo_pixel_thres, geo_depth_thres)
        sel = final & may
        out[s][qy[sel], qx[sel]] = 1
        claims.append((np.flatnonzero(sel), (qy[sel] * w + qx[sel])))
    return (avg, photo, geo, final, cnt, level), out, claims


def fuse_scan_dynamic(pairs, cams, depths, confidences, images, geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3,
                      dedupe=False, **rule):
    """a whole scan in ``pairs`` order (arguments as ``fusion.fuse_scan`` takes them, numpy; ``rule``: a, b, n_min, n_max).
    -> (PLY bytes, views: {ref: dict(final=emit mask, kept=photo & geo, geo, photo, level, records)}, claimed: {view: uint8 [H,W]}
        at the end of the scan)"""
    h, w = depths[pairs[0][0]].shape
    every = sorted({v for ref, srcs in pairs for v in (ref, *srcs)})
    claimed = {v: np.zeros((h, w), np.uint8) for v in every}
    views, parts = {}, []
    for ref, srcs in pairs:
        k, e = cams[ref]
        res, new, _ = fuse_view_dynamic(depths[ref], confidences[ref], k, e, [depths[v] for v in srcs], [cams[v][0] for v in srcs],
                                        [cams[v][1] for v in srcs], claimed[ref] if dedupe else None,
                                        [claimed[v] for v in srcs] if dedupe else None, geo_pixel_thres, geo_depth_thres,
                                        photo_thres, **rule)
        avg, photo, geo, final, _, level = res
        for v, c in zip(srcs, new or []):
            claimed[v] = c
        rec = R.records_of(avg, final, k, e, np.asarray(images[ref]))
        views[ref] = dict(final=final, kept=photo & geo, geo=geo, photo=photo, level=level, records=rec)
        parts.append(rec.tobytes())
    body = b"".join(parts)
    return R.ply_header(len(body) // R.RECORD.itemsize) + body, views, claimed

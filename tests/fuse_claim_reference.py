"""numpy restatement of the claim step of ``itermvs_fuse_depth_claim`` (``eval.py --fuse_dedupe``) on top of
oracle/fusion_oracle.py.  TEST INFRASTRUCTURE ONLY.  The reference project has no counterpart of the claim step; everything
else is ``FO.fuse_reference_view`` (eval.py:238-269) and ``FO.unproject_points`` (eval.py:287-296) unchanged.

Contract, per reference view r with its claim map ``claimed[r]`` and the claim maps of its sources:
  final[p] = photo[p] and geo[p] and claimed[r][p] == 0
  for every source s that is consistent with p (the mask of ``FO.check_geometric_consistency``), if final[p]:
      qx, qy = rint(x_src32), rint(y_src32)                        float32, round half to even
      inside  = 0 <= qx <= W-1 and 0 <= qy <= H-1                  compared in float32; NaN and inf fail
      near    = |depth_src[s][qy, qx] - smp32| / smp32 < geo_depth_thres      float32; false or NaN: no claim
      claimed[s][qy, qx] = 1 where inside and near
with smp32 the float32 bilinear sample of depth_src[s] at (x_src32, y_src32)."""
import numpy as np

from oracle import fusion_oracle as FO

RECORD = np.dtype([("xyz", "<u4", (3,)), ("rgb", "u1", (3,))])           # coordinates as bit patterns, 15 bytes


def ply_header(n: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n).encode("ascii")


def claim_targets(depth_ref, k_ref, e_ref, depth_src, k_src, e_src, geo_pixel_thres, geo_depth_thres, depth_condition=True):
    """one (reference, source) pair -> (ok [H,W] bool: the pair's consistency mask, may [H,W] bool: this reference pixel would
    claim if it emits, qy, qx [H,W] int64: the source pixel it would claim (0 where ``may`` is false)).
    ``depth_condition=False`` leaves the ``near`` test out (what the claim step would do without it)."""
    h, w = depth_ref.shape
    ok, _, x_src, y_src = FO.check_geometric_consistency(depth_ref, k_ref, e_ref, depth_src, k_src, e_src,
                                                         geo_pixel_thres, geo_depth_thres)
    smp = FO.remap_bilinear(depth_src, x_src, y_src)
    with np.errstate(all="ignore"):
        qx, qy = np.rint(x_src), np.rint(y_src)
        assert qx.dtype == np.float32 and smp.dtype == np.float32
        inside = (qx >= np.float32(0)) & (qx <= np.float32(w - 1)) & (qy >= np.float32(0)) & (qy <= np.float32(h - 1))
        ix = np.where(inside, qx, np.float32(0)).astype(np.int64)
        iy = np.where(inside, qy, np.float32(0)).astype(np.int64)
        near = np.abs(depth_src[iy, ix] - smp) / smp < np.float32(geo_depth_thres)
        assert (np.abs(depth_src[iy, ix] - smp) / smp).dtype == np.float32
    may = ok & inside & (near if depth_condition else True)
    return ok, may, np.where(may, iy, 0), np.where(may, ix, 0)


def fuse_view_claim(depth_ref, conf_ref, k_ref, e_ref, src_depths, src_ks, src_es, claimed_ref, claimed_src,
                    geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=3, depth_condition=True):
    """one reference view.  claimed_ref: uint8 [H,W] or None (all zero); claimed_src: S uint8 [H,W] maps or None (no claims).
    -> ((depth_avg float64, photo, geo, final bool, count int32), updated COPIES of the source claim maps (None if not given),
        claims: per source (pixel index p of the claiming reference pixels, pixel index q they claim))"""
    h, w = depth_ref.shape
    avg, photo, geo, final, cnt = FO.fuse_reference_view(depth_ref, conf_ref, k_ref, e_ref, src_depths, src_ks, src_es,
                                                         geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres)
    if claimed_ref is not None:
        final = final & (np.asarray(claimed_ref) == 0)
    if claimed_src is None:
        return (avg, photo, geo, final, cnt), None, []
    out, claims = [np.array(c, dtype=np.uint8, copy=True) for c in claimed_src], []
    for s, (d_src, k_src, e_src) in enumerate(zip(src_depths, src_ks, src_es)):
        _, may, qy, qx = claim_targets(depth_ref, k_ref, e_ref, d_src, k_src, e_src, geo_pixel_thres, geo_depth_thres,
                                       depth_condition)
        sel = final & may
        out[s][qy[sel], qx[sel]] = 1
        claims.append((np.flatnonzero(sel), (qy[sel] * w + qx[sel])))
    return (avg, photo, geo, final, cnt), out, claims


def records_of(avg, mask, k, e, rgb):
    """the vertex records the reference writes for one view: float32(unproject_points) bits and rgb[mask]"""
    with np.errstate(all="ignore"):
        xyz = FO.unproject_points(avg, mask, k, e).astype(np.float32)
    out = np.zeros(int(mask.sum()), RECORD)
    out["xyz"], out["rgb"] = xyz.view(np.uint32).reshape(-1, 3), rgb[mask]
    return out


def fuse_scan_claim(pairs, cams, depths, confidences, images, geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3,
                    geo_mask_thres=3, dedupe=True):
    """a whole scan in ``pairs`` order (pairs, cams, depths, confidences, images as ``fusion.fuse_scan`` takes them, numpy).
    -> (PLY bytes,
        claimer: {(view, pixel index): (claiming view, its pixel index)} for every SUPPRESSED pixel (photo and geo hold, the
                 pixel was claimed before its view's turn),
        views: {ref: dict(final=bool [H,W] emit mask, plain=bool [H,W] photo & geo, records=its vertex records)},
        claimed: {view: uint8 [H,W]} at the end of the scan)"""
    h, w = depths[pairs[0][0]].shape
    every = sorted({v for ref, srcs in pairs for v in (ref, *srcs)})
    claimed = {v: np.zeros((h, w), np.uint8) for v in every}
    by = {v: (np.full(h * w, -1, np.int64), np.full(h * w, -1, np.int64)) for v in every}      # first claimer: view, pixel
    claimer, views, parts = {}, {}, []
    for ref, srcs in pairs:
        k, e = cams[ref]
        res, new, claims = fuse_view_claim(depths[ref], confidences[ref], k, e, [depths[v] for v in srcs],
                                           [cams[v][0] for v in srcs], [cams[v][1] for v in srcs],
                                           claimed[ref] if dedupe else None, [claimed[v] for v in srcs] if dedupe else None,
                                           geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres)
        avg, photo, geo, final, _ = res
        for p in np.flatnonzero((photo & geo & ~final).reshape(-1)):
            claimer[(ref, int(p))] = (int(by[ref][0][p]), int(by[ref][1][p]))
        for v, c, (p_from, q_to) in zip(srcs, new or [], claims):
            fresh = by[v][0][q_to] < 0
            by[v][0][q_to[fresh]], by[v][1][q_to[fresh]] = ref, p_from[fresh]
            claimed[v] = c
        rec = records_of(avg, final, k, e, np.asarray(images[ref]))
        views[ref] = dict(final=final, plain=photo & geo, records=rec)
        parts.append(rec.tobytes())
    body = b"".join(parts)
    return ply_header(len(body) // RECORD.itemsize) + body, claimer, views, claimed

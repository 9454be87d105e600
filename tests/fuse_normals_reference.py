"""numpy restatement of the per-vertex normal of itermvs_fuse_points_normals (include/itermvs_hip.h, steps 1-8): float64
throughout, products and sums in the written order (numpy's elementwise operations round once each and never fuse), IEEE sqrt and
division, one conversion to float32 at the end.  Vectorised over the image; the neighbours are shifted copies of the maps, padded
with NaN depths so that a neighbour outside the image is never usable.  TEST INFRASTRUCTURE ONLY: imports nothing from the package;
the vertex coordinates keep coming from oracle/fusion_oracle.py:unproject_points."""
import numpy as np


def _mat3(m, p):
    """(3x3 float32 upcast) @ (3 x ... float64), k ascending, no FMA"""
    m = m.astype(np.float64)
    return np.stack([(m[i, 0] * p[0] + m[i, 1] * p[1]) + m[i, 2] * p[2] for i in range(3)])


def _shift(a, dy, dx, fill):
    """out[..., y, x] = a[..., y + dy, x + dx] where that lies inside the image, ``fill`` elsewhere (dy, dx in -1, 0, 1)"""
    h, w = a.shape[-2:]
    out = np.full(a.shape, fill, a.dtype)
    ys, yd = (slice(1, h), slice(0, h - 1)) if dy == 1 else (slice(0, h - 1), slice(1, h)) if dy == -1 else (slice(0, h),) * 2
    xs, xd = (slice(1, w), slice(0, w - 1)) if dx == 1 else (slice(0, w - 1), slice(1, w)) if dx == -1 else (slice(0, w),) * 2
    out[..., yd, xd] = a[..., ys, xs]
    return out


def camera_points(depth_avg, k_ref):
    """step 2: Pc [3,H,W] float64 = float32 inv(K_ref), upcast, applied to (x*d, y*d, d)"""
    h, w = depth_avg.shape
    x, y = np.meshgrid(np.arange(0, w), np.arange(0, h))
    d = depth_avg.astype(np.float64)
    return _mat3(np.linalg.inv(k_ref), np.stack([x * d, y * d, d]))


def normal_map(depth_avg, k_ref, e_ref, edge_thres=0.01):
    """-> float32 [H,W,3]: the normal of every pixel; k_ref [3,3], e_ref [4,4] float32 as the fusion holds them"""
    with np.errstate(all="ignore"):
        d = depth_avg.astype(np.float64)
        pc = camera_points(d, k_ref)
        ok = np.isfinite(d) & (d > 0)                                                  # step 1

        def tangent(dy, dx):
            """steps 3 and 4 along one axis -> (t [3,H,W], defined [H,W])"""
            use, pts = [], []
            for sign in (-1, 1):                                                        # lo, hi
                dq = _shift(d, sign * dy, sign * dx, np.nan)
                use.append(np.isfinite(dq) & (dq > 0) & (np.abs(dq - d) < edge_thres * d))
                pts.append(_shift(pc, sign * dy, sign * dx, 0.0))
            lo, hi = use
            return np.where(hi, pts[1], pc) - np.where(lo, pts[0], pc), lo | hi

        tx, has_x = tangent(0, 1)
        ty, has_y = tangent(1, 0)
        nc = np.stack([tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]])      # step 5
        s = (nc[0] * pc[0] + nc[1] * pc[1]) + nc[2] * pc[2]                            # step 6
        nc = np.where(s > 0, -nc, nc)
        n = _mat3(np.linalg.inv(e_ref)[:3, :3], nc)                                     # step 7
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])                     # step 8
        ok = ok & has_x & has_y & np.isfinite(length) & (length > 0)
        unit = (n / length).astype(np.float32)
    return np.where(ok, unit, np.float32(0.0)).transpose(1, 2, 0)


def normals(depth_avg, mask, k_ref, e_ref, edge_thres=0.01):
    """-> float32 [n,3]: the normals of the pixels in ``mask``, in the row-major order of the vertices"""
    return normal_map(depth_avg, k_ref, e_ref, edge_thres)[mask]

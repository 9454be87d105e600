"""Lens distortion of COLMAP's camera models on the host (numpy, float64, no GPU): the distortion functions that
``itermvs_undistort_rgb8`` evaluates per pixel, their iterative inverse, and the choice of the output pinhole camera.

Written from COLMAP's published behaviour (``src/colmap/sensor/models.h``: ``Distortion`` of every model and
``IterativeUndistortion``; ``src/colmap/image/undistortion.cc``: ``UndistortCamera`` with the default options of
``image_undistorter``).  Pixel centres are at half-integers: pixel (0, 0) covers [0, 1) x [0, 1).  Agreement with COLMAP's own
output files has not been verified byte for byte.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .colmap import CAMERA_MODEL_NAMES, SINGLE_FOCAL, Camera

PINHOLE_MODELS = ("SIMPLE_PINHOLE", "PINHOLE")
FISHEYE_MODELS = ("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
SUPPORTED_MODELS = PINHOLE_MODELS + ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV") + FISHEYE_MODELS
FISHEYE_EPS = float(np.finfo(np.float64).eps)      # below this radius the fisheye models have no distortion

NEWTON_ITERATIONS = 100
NEWTON_MAX_STEP = 1e-10
NEWTON_REL_STEP = 1e-6          # finite-difference step of the Jacobian, relative to the coordinate


def check_model(model: str) -> None:
    if model not in CAMERA_MODEL_NAMES:
        raise ValueError(f"unknown camera model {model}")
    if model not in SUPPORTED_MODELS:
        raise ValueError(f"camera model {model} is not supported by the undistortion (supported: {', '.join(SUPPORTED_MODELS)})")


def split_params(cam: Camera) -> Tuple[float, float, float, float, np.ndarray]:
    """fx, fy, cx, cy and the distortion parameters of the model's parameter list"""
    check_model(cam.model)
    p = np.asarray(cam.params, np.float64)
    if len(p) != CAMERA_MODEL_NAMES[cam.model][1]:
        raise ValueError(f"camera {cam.id} ({cam.model}) has {len(p)} parameters")
    if cam.model in SINGLE_FOCAL:
        return float(p[0]), float(p[0]), float(p[1]), float(p[2]), p[3:]
    return float(p[0]), float(p[1]), float(p[2]), float(p[3]), p[4:]


def distortion(model: str, k, u, v) -> Tuple[np.ndarray, np.ndarray]:
    """(du, dv) of normalised coordinates (u, v): the distorted point is (u + du, v + dv).  ``k``: the parameters after the
    focal lengths and the principal point.  The operation order is the kernel's (include/itermvs_hip.h)."""
    check_model(model)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    k = [float(x) for x in k]
    with np.errstate(all="ignore"):
        u2, v2 = u * u, v * v
        r2 = u2 + v2
        if model in PINHOLE_MODELS:
            return np.zeros_like(u), np.zeros_like(v)
        if model == "SIMPLE_RADIAL":
            radial = k[0] * r2
            return u * radial, v * radial
        if model == "RADIAL":
            radial = k[0] * r2 + k[1] * (r2 * r2)
            return u * radial, v * radial
        if model in ("OPENCV", "FULL_OPENCV"):
            r4, uv = r2 * r2, u * v
            if model == "OPENCV":
                radial = k[0] * r2 + k[1] * r4
            else:
                r6 = r4 * r2
                radial = (((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6) / (((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6)
            du = (u * radial + (2.0 * k[2]) * uv) + k[3] * (r2 + 2.0 * u2)
            dv = (v * radial + (2.0 * k[3]) * uv) + k[2] * (r2 + 2.0 * v2)
            return (du - u, dv - v) if model == "FULL_OPENCV" else (du, dv)
        r = np.sqrt(r2)
        t = np.arctan(r)
        t2 = t * t
        poly = 1.0 + k[0] * t2
        if model != "SIMPLE_RADIAL_FISHEYE":
            t4 = t2 * t2
            poly = poly + k[1] * t4
            if model == "OPENCV_FISHEYE":
                poly = (poly + k[2] * (t4 * t2)) + k[3] * (t4 * t4)
        td = t * poly
        far = r > FISHEYE_EPS
        safe = np.where(far, r, 1.0)
        return np.where(far, (u * td) / safe - u, 0.0), np.where(far, (v * td) / safe - v, 0.0)


def undistort_points(model: str, k, ud, vd) -> Tuple[np.ndarray, np.ndarray]:
    """solve (u, v) + distortion(u, v) = (ud, vd): Newton's method from (ud, vd) with a central-difference Jacobian, at most
    NEWTON_ITERATIONS steps, a point stops once its step is shorter than NEWTON_MAX_STEP"""
    ud, vd = np.atleast_1d(np.asarray(ud, np.float64)), np.atleast_1d(np.asarray(vd, np.float64))
    shape = ud.shape
    ud, vd = ud.ravel(), vd.ravel()
    u, v = ud.copy(), vd.copy()
    if model in PINHOLE_MODELS:
        check_model(model)
        return u.reshape(shape), v.reshape(shape)
    eps = np.finfo(np.float64).eps
    hu, hv = np.maximum(eps, np.abs(NEWTON_REL_STEP * ud)), np.maximum(eps, np.abs(NEWTON_REL_STEP * vd))
    live = np.ones(len(u), bool)

    def forward(a, b):
        da, db = distortion(model, k, a, b)
        return a + da, b + db

    with np.errstate(all="ignore"):
        for _ in range(NEWTON_ITERATIONS):
            i = np.nonzero(live)[0]
            if not len(i):
                break
            a, b, ha, hb = u[i], v[i], hu[i], hv[i]
            fu, fv = forward(a, b)
            pu, pv = forward(a + ha, b)
            mu, mv = forward(a - ha, b)
            j00, j10 = (pu - mu) / (2 * ha), (pv - mv) / (2 * ha)
            pu, pv = forward(a, b + hb)
            mu, mv = forward(a, b - hb)
            j01, j11 = (pu - mu) / (2 * hb), (pv - mv) / (2 * hb)
            ru, rv = fu - ud[i], fv - vd[i]
            det = j00 * j11 - j01 * j10
            su, sv = (j11 * ru - j01 * rv) / det, (j00 * rv - j10 * ru) / det
            ok = np.isfinite(su) & np.isfinite(sv)
            u[i[ok]] -= su[ok]
            v[i[ok]] -= sv[ok]
            live[i] = ok & (np.hypot(su, sv) >= NEWTON_MAX_STEP)
    return u.reshape(shape), v.reshape(shape)


def source_map(cam: Camera, out: Camera) -> np.ndarray:
    """float64 [Ho,Wo,2]: the coordinates (sx, sy) in ``cam``'s image, pixel (0, 0) at (0, 0), that the pixels of the pinhole
    camera ``out`` sample -- the map of ``itermvs_undistort_rgb8``"""
    fx, fy, cx, cy, k = split_params(cam)
    fxo, fyo, cxo, cyo, _ = split_params(out)
    x, y = np.meshgrid(np.arange(out.width, dtype=np.float64), np.arange(out.height, dtype=np.float64))
    with np.errstate(all="ignore"):
        u, v = ((x + 0.5) - cxo) / fxo, ((y + 0.5) - cyo) / fyo
        du, dv = distortion(cam.model, k, u, v)
        return np.stack([(fx * (u + du) + cx) - 0.5, (fy * (v + dv) + cy) - 0.5], -1)


def undistorted_camera(cam: Camera, blank_pixels: float = 0.0, min_scale: float = 0.2, max_scale: float = 2.0) -> Camera:
    """the pinhole camera an image of ``cam`` is resampled to: the rule of COLMAP's image_undistorter.  The focal lengths are
    kept; the image is scaled per axis so that the undistorted border of the source lies outside the output
    (``blank_pixels`` = 0: no blank pixel when the principal point is centred) or inside it (``blank_pixels`` = 1: every source
    pixel kept); the principal point is the output's centre.  A pinhole camera is returned as it is."""
    if cam.model in PINHOLE_MODELS:
        check_model(cam.model)
        return cam
    fx, fy, cx, cy, k = split_params(cam)
    w, h = int(cam.width), int(cam.height)
    if w < 1 or h < 1:
        raise ValueError(f"camera {cam.id}: size {w} x {h}")
    rows, cols = np.arange(h, dtype=np.float64) + 0.5, np.arange(w, dtype=np.float64) + 0.5

    def undistorted(px, py):                       # pixel -> pixel of the pinhole with the same fx, fy, cx, cy
        u, v = undistort_points(cam.model, k, (px - cx) / fx, (py - cy) / fy)
        return fx * u + cx, fy * v + cy

    left, _ = undistorted(np.full(h, 0.5), rows)
    right, _ = undistorted(np.full(h, w - 0.5), rows)
    _, top = undistorted(cols, np.full(w, 0.5))
    _, bottom = undistorted(cols, np.full(w, h - 0.5))
    with np.errstate(all="ignore"):
        min_x = min(cx / (cx - left.min()), (w - 0.5 - cx) / (right.max() - cx))
        max_x = max(cx / (cx - left.max()), (w - 0.5 - cx) / (right.min() - cx))
        min_y = min(cy / (cy - top.min()), (h - 0.5 - cy) / (bottom.max() - cy))
        max_y = max(cy / (cy - top.max()), (h - 0.5 - cy) / (bottom.min() - cy))
        scale_x = 1.0 / (min_x * blank_pixels + max_x * (1.0 - blank_pixels))
        scale_y = 1.0 / (min_y * blank_pixels + max_y * (1.0 - blank_pixels))
    if not (np.isfinite(scale_x) and np.isfinite(scale_y)):
        raise ValueError(f"camera {cam.id} ({cam.model}): the undistorted image border is degenerate")
    scale_x, scale_y = float(np.clip(scale_x, min_scale, max_scale)), float(np.clip(scale_y, min_scale, max_scale))
    wo, ho = max(1, int(scale_x * w)), max(1, int(scale_y * h))
    return Camera(cam.id, "PINHOLE", wo, ho, np.array([fx, fy, wo / 2.0, ho / 2.0]))

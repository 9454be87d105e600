"""numpy restatement of itermvs_undistort_rgb8 (include/itermvs_hip.h): the map from output pixels to source coordinates and the
bilinear sampling, written from the header's formulas and independent of itermvs_amd/undistort.py.  Everything is float64 and
every line is one rounding per operation in the header's order, so the polynomial models are comparable bit for bit."""
import numpy as np

# model -> (id, number of parameters, single focal length)
MODELS = {"SIMPLE_PINHOLE": (0, 3, True), "PINHOLE": (1, 4, False), "SIMPLE_RADIAL": (2, 4, True), "RADIAL": (3, 5, True),
          "OPENCV": (4, 8, False), "OPENCV_FISHEYE": (5, 8, False), "FULL_OPENCV": (6, 12, False),
          "SIMPLE_RADIAL_FISHEYE": (8, 4, True), "RADIAL_FISHEYE": (9, 5, True)}
POLYNOMIAL = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
ATAN = ("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
UNSUPPORTED = {"FOV": (7, 5), "THIN_PRISM_FISHEYE": (10, 12)}


def intrinsics(model, params):
    """-> fx, fy, cx, cy, [distortion parameters]"""
    p = [float(x) for x in params]
    _, n, single = MODELS[model]
    assert len(p) == n
    return (p[0], p[0], p[1], p[2], p[3:]) if single else (p[0], p[1], p[2], p[3], p[4:])


def delta(model, k, u, v):
    u2 = u * u
    v2 = v * v
    r2 = u2 + v2
    zero = np.zeros_like(u)
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return zero, zero
    if model == "SIMPLE_RADIAL":
        radial = k[0] * r2
        return u * radial, v * radial
    r4 = r2 * r2
    if model == "RADIAL":
        radial = k[0] * r2 + k[1] * r4
        return u * radial, v * radial
    uv = u * v
    if model == "OPENCV":
        k1, k2, p1, p2 = k
        radial = k1 * r2 + k2 * r4
        return (u * radial + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * u2), (v * radial + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * v2)
    if model == "FULL_OPENCV":
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        r6 = r4 * r2
        radial = (((1.0 + k1 * r2) + k2 * r4) + k3 * r6) / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6)
        return (((u * radial + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * u2)) - u,
                ((v * radial + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * v2)) - v)
    r = np.sqrt(r2)
    t = np.arctan(r)
    t2 = t * t
    t4 = t2 * t2
    if model == "SIMPLE_RADIAL_FISHEYE":
        td = t * (1.0 + k[0] * t2)
    elif model == "RADIAL_FISHEYE":
        td = t * ((1.0 + k[0] * t2) + k[1] * t4)
    else:
        assert model == "OPENCV_FISHEYE"
        t6 = t4 * t2
        t8 = t4 * t4
        td = t * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
    near = ~(r > 2.0 ** -52)
    rr = np.where(near, 1.0, r)
    du = (u * td) / rr - u
    dv = (v * td) / rr - v
    return np.where(near, 0.0, du), np.where(near, 0.0, dv)


def source_coords(model, params, out_camera, out_hw):
    """float64 [Ho,Wo,2]: (sx, sy) of every output pixel"""
    fx, fy, cx, cy, k = intrinsics(model, params)
    fxo, fyo, cxo, cyo = [float(x) for x in out_camera]
    ho, wo = out_hw
    x = np.broadcast_to(np.arange(wo, dtype=np.float64)[None, :], (ho, wo))
    y = np.broadcast_to(np.arange(ho, dtype=np.float64)[:, None], (ho, wo))
    with np.errstate(all="ignore"):
        u = ((x + 0.5) - cxo) / fxo
        v = ((y + 0.5) - cyo) / fyo
        du, dv = delta(model, k, u, v)
        sx = (fx * (u + du) + cx) - 0.5
        sy = (fy * (v + dv) + cy) - 0.5
    return np.stack([sx, sy], -1)


def filled(coords, src_hw):
    hs, ws = src_hw
    sx, sy = coords[..., 0], coords[..., 1]
    with np.errstate(all="ignore"):
        return (sx >= 0) & (sx <= ws - 1) & (sy >= 0) & (sy <= hs - 1)        # NaN compares false


def sample(src, coords):
    """uint8 [Hs,Ws,3] sampled at coords [Ho,Wo,2] -> uint8 [Ho,Wo,3]; pixels that are not filled are 0"""
    hs, ws, _ = src.shape
    ok = filled(coords, (hs, ws))
    sx = np.where(ok, coords[..., 0], 0.0)
    sy = np.where(ok, coords[..., 1], 0.0)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    wx, wy = (sx - fx0)[..., None], (sy - fy0)[..., None]
    s = src.astype(np.float64)
    top = (1.0 - wx) * s[y0, x0] + wx * s[y0, x1]
    bot = (1.0 - wx) * s[y1, x0] + wx * s[y1, x1]
    value = np.clip(np.floor(((1.0 - wy) * top + wy * bot) + 0.5), 0, 255).astype(np.uint8)
    return np.where(ok[..., None], value, np.uint8(0))


def make_image(h, w, seed=0):
    """smooth gradients plus noise: neighbouring pixels differ, so a wrong tap or weight shows"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


COEFFICIENTS = {"SIMPLE_PINHOLE": [], "PINHOLE": [], "SIMPLE_RADIAL": [0.1], "RADIAL": [0.1, -0.02],
                "OPENCV": [-0.12, 0.03, 0.004, -0.003], "FULL_OPENCV": [-0.12, 0.03, 0.004, -0.003, 0.01, 0.02, -0.01, 0.005],
                "OPENCV_FISHEYE": [0.05, -0.01, 0.002, 0.0], "SIMPLE_RADIAL_FISHEYE": [0.05], "RADIAL_FISHEYE": [0.05, -0.01]}
# (width, height, f, cx, cy): the two source shapes of the tests, principal point at the centre
SHAPES = {"64x48": (64, 48, 50.0, 32.0, 24.0), "37x29": (37, 29, 30.0, 18.5, 14.5)}


def params_of(model, f, cx, cy, coefficients=None):
    """COLMAP's parameter list of ``model`` with the given focal length, principal point and distortion coefficients"""
    k = COEFFICIENTS[model] if coefficients is None else list(coefficients)
    assert len(k) == len(COEFFICIENTS[model])
    return ([f, cx, cy] if MODELS[model][2] else [f, f, cx, cy]) + [float(x) for x in k]


def tiny_model(camera, names):
    """a COLMAP model of len(names) images of ``camera`` on a line, all observing the same 24 points in front of them"""
    from itermvs_amd import colmap
    rng = np.random.default_rng(3)
    xyz = np.concatenate([rng.uniform(-1, 1, (24, 2)), rng.uniform(4, 6, (24, 1))], 1)
    ids = np.arange(1, 25, dtype=np.int64)
    images = [colmap.Image(10 + i, np.array([1.0, 0.0, 0.0, 0.0]), np.array([-0.3 * i, 0.0, 0.0]), camera.id, name, ids.copy(),
                           np.zeros((24, 2))) for i, name in enumerate(names)]
    return colmap.Model({camera.id: camera}, images, ids, xyz)

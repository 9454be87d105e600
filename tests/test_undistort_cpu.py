"""--undistort of colmap_input.py, the parts that need no GPU: the distortion models (itermvs_amd/undistort.py and the restatement
tests/undistort_reference.py) against each other and against closed forms, the Newton inverse, the choice of the output camera,
the C ABI of itermvs_undistort_rgb8, the new flags, and the unchanged behaviour without the flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import undistort_reference as UR
from conftest import ROOT
from test_colmap_cpu import load_case

ULP = 2.0 ** -52


def _camera(model, shape="64x48", coefficients=None, centre=None):
    from itermvs_amd.colmap import Camera
    w, h, f, cx, cy = UR.SHAPES[shape]
    if centre is not None:
        cx, cy = centre
    return Camera(1, model, w, h, np.array(UR.params_of(model, f, cx, cy, coefficients)))


def _inside_share(cam, out):
    from itermvs_amd import undistort as U
    return float(UR.filled(U.source_map(cam, out), (cam.height, cam.width)).mean())


@pytest.mark.parametrize("model", UR.POLYNOMIAL)
def test_zero_coefficients_give_the_identity_map(model):
    """f = 64 and a principal point on the half-pixel grid: (x + 0.5 - cx) / f and its product with f are exact (a power of two
    only shifts the exponent), so sx = x and sy = y hold bit for bit, in the restatement and in the package's map alike"""
    from itermvs_amd import undistort as U
    from itermvs_amd.colmap import Camera
    for w, h, cx, cy in ((64, 48, 32.0, 24.0), (37, 29, 18.5, 14.5)):
        params = UR.params_of(model, 64.0, cx, cy, [0.0] * len(UR.COEFFICIENTS[model]))
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        want = np.stack([x, y], -1)
        assert np.array_equal(UR.source_coords(model, params, (64.0, 64.0, cx, cy), (h, w)), want)
        out = Camera(1, "PINHOLE", w, h, np.array([64.0, 64.0, cx, cy]))
        assert np.array_equal(U.source_map(Camera(1, model, w, h, np.array(params)), out), want)


@pytest.mark.parametrize("model", sorted(UR.MODELS))
@pytest.mark.parametrize("shape", sorted(UR.SHAPES))
def test_package_map_equals_the_restatement(model, shape):
    """two independent statements of the header's formulas: the same bits for the polynomial models AND for the atan ones
    (both call numpy's arctan)"""
    from itermvs_amd import undistort as U
    cam = _camera(model, shape)
    out = U.undistorted_camera(cam)
    got = U.source_map(cam, out)
    want = UR.source_coords(model, cam.params, U.split_params(out)[:4], (out.height, out.width))
    assert got.shape == (out.height, out.width, 2) and np.array_equal(got, want)


def test_model_chain():
    w, h, f, cx, cy = UR.SHAPES["64x48"]
    out, hw = (47.0, 52.0, 30.2, 25.9), (h, w)
    sr = UR.source_coords("SIMPLE_RADIAL", [f, cx, cy, 0.1], out, hw)
    r0 = UR.source_coords("RADIAL", [f, cx, cy, 0.1, 0.0], out, hw)
    assert np.array_equal(sr, r0)                                              # + 0 * r4 changes no bit
    r = UR.source_coords("RADIAL", [f, cx, cy, 0.1, -0.02], out, hw)
    o0 = UR.source_coords("OPENCV", [f, f, cx, cy, 0.1, -0.02, 0.0, 0.0], out, hw)
    assert np.array_equal(r, o0) and not np.array_equal(r, sr)                 # + 0 * uv + 0 * (...) changes no bit
    o = UR.source_coords("OPENCV", [f, f, cx, cy, -0.12, 0.03, 0.004, -0.003], out, hw)
    f0 = UR.source_coords("FULL_OPENCV", [f, f, cx, cy, -0.12, 0.03, 0.004, -0.003, 0, 0, 0, 0], out, hw)
    # FULL_OPENCV forms u * (1 + radial) + tangential - u where OPENCV forms u * radial + tangential: a few roundings of values
    # of the size of the normalised coordinate (|u| < 1), scaled by f = 50 into pixels of magnitude < 64: 8 ulp of 64
    assert np.abs(o - f0).max() <= 8 * 64 * ULP and not np.array_equal(o, r)


@pytest.mark.parametrize("model", UR.ATAN)
def test_fisheye_with_zero_coefficients_is_the_equidistant_map(model):
    w, h, f, cx, cy = UR.SHAPES["64x48"]
    out = (f, f, 32.5, 24.5)                                                   # pixel (32, 24) looks along the axis: r = 0 there
    got = UR.source_coords(model, UR.params_of(model, f, cx, cy, [0.0] * len(UR.COEFFICIENTS[model])), out, (h, w))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (x + 0.5 - 32.5) / f, (y + 0.5 - 24.5) / f
    r = np.hypot(u, v)
    scale = np.where(r > 0, np.arctan(r) / np.where(r > 0, r, 1.0), 1.0)
    want = np.stack([f * u * scale + cx - 0.5, f * v * scale + cy - 0.5], -1)
    assert np.abs(got - want).max() <= 8 * 64 * ULP                            # another expression of the same value
    assert np.array_equal(got[24, 32], [cx - 0.5, cy - 0.5])                   # r below epsilon: no distortion, no 0 / 0


@pytest.mark.parametrize("k", [0.1, -0.1])
def test_simple_radial_closed_form_on_the_axes(k):
    """on the row and the column through the principal point the other coordinate is 0: sx = f u (1 + k u^2) + cx - 0.5"""
    from itermvs_amd import undistort as U
    from itermvs_amd.colmap import Camera
    w, h, f, cx, cy = UR.SHAPES["64x48"]
    out = (f, f, 32.5, 24.5)                                                   # row 24 has v = 0, column 32 has u = 0
    cam, pin = Camera(1, "SIMPLE_RADIAL", w, h, np.array([f, cx, cy, k])), Camera(1, "PINHOLE", w, h, np.array(out))
    for coords in (UR.source_coords("SIMPLE_RADIAL", [f, cx, cy, k], out, (h, w)), U.source_map(cam, pin)):
        for x in (0, 1, 7, 31, 32, 33, 50, 63):
            u = (x - 32) / f
            assert abs(coords[24, x, 0] - (f * u * (1 + k * u ** 2) + cx - 0.5)) <= 8 * 64 * ULP
            assert coords[24, x, 1] == cy - 0.5
        for y in (0, 5, 23, 24, 25, 47):
            v = (y - 24) / f
            assert abs(coords[y, 32, 1] - (f * v * (1 + k * v ** 2) + cy - 0.5)) <= 8 * 64 * ULP
            assert coords[y, 32, 0] == cx - 0.5
    assert abs(coords[24, 63, 0] - (50 * 0.62 * (1 + k * 0.62 ** 2) + 31.5)) < 1e-9      # one pixel by hand: x = 63, u = 0.62


@pytest.mark.parametrize("model", [m for m in sorted(UR.MODELS) if "PINHOLE" not in m])
@pytest.mark.parametrize("shape", sorted(UR.SHAPES))
def test_newton_inverse_returns_the_border_points(model, shape):
    from itermvs_amd import undistort as U
    cam = _camera(model, shape)
    fx, fy, cx, cy, k = U.split_params(cam)
    w, h = cam.width, cam.height
    px = np.concatenate([np.full(h, 0.5), np.full(h, w - 0.5), np.arange(w) + 0.5, np.arange(w) + 0.5])
    py = np.concatenate([np.arange(h) + 0.5, np.arange(h) + 0.5, np.full(w, 0.5), np.full(w, h - 0.5)])
    ud, vd = (px - cx) / fx, (py - cy) / fy
    u, v = U.undistort_points(model, k, ud, vd)
    du, dv = UR.delta(model, list(k), u, v)                                     # distorted again by the restatement
    assert np.hypot(u + du - ud, v + dv - vd).max() <= 1e-9
    assert np.hypot(u - ud, v - vd).max() > 1e-3                                # and the inverse did move them


# the sizes follow from the rule: 1 / (largest ratio of the original to the undistorted half-extent), per axis, times the size
@pytest.mark.parametrize("model,coefficients,size", [
    ("SIMPLE_RADIAL", [0.1], (59, 44)), ("SIMPLE_RADIAL", [-0.1], (65, 48)), ("OPENCV", [-0.12, 0.03, 0.004, -0.003], (65, 48)),
    ("OPENCV_FISHEYE", [0.05, -0.01, 0.002, 0.0], (71, 50))])
def test_undistorted_camera_without_blank_pixels(model, coefficients, size):
    """blank_pixels = 0, centred principal point: every output pixel samples inside the source.

    The fisheye case gives 71 x 50 under the stated rule: on the row through the principal point the left border centre
    x = 0.5 undistorts to x = -3.62, ratio 32 / 35.62 = 0.898, the largest of the left and right ratios, and
    int(64 / 0.898) = 71.  A width of 77 would be 64 / 0.830, the SMALLEST ratio (the corners), which is what blank_pixels = 1
    selects, and at 77 x 52 the inside share is below 1."""
    from itermvs_amd import undistort as U
    from itermvs_amd.colmap import Camera
    cam = _camera(model, coefficients=coefficients)
    out = U.undistorted_camera(cam)
    print(model, coefficients, "->", out.width, "x", out.height, "inside share", _inside_share(cam, out))
    assert out.model == "PINHOLE" and out.id == cam.id and (out.width, out.height) == size
    assert list(out.params) == [50.0, 50.0, size[0] / 2, size[1] / 2]          # focal lengths kept, principal point centred
    assert _inside_share(cam, out) == 1.0
    if model == "OPENCV_FISHEYE":
        assert _inside_share(cam, Camera(1, "PINHOLE", 77, 52, np.array([50.0, 50.0, 38.5, 26.0]))) < 1.0


@pytest.mark.parametrize("model,coefficients", [("SIMPLE_RADIAL", [0.1]), ("SIMPLE_RADIAL", [-0.1]),
                                                ("OPENCV", [-0.12, 0.03, 0.004, -0.003]),
                                                ("OPENCV_FISHEYE", [0.05, -0.01, 0.002, 0.0])])
def test_undistorted_camera_with_blank_pixels(model, coefficients):
    from itermvs_amd import undistort as U
    cam = _camera(model, coefficients=coefficients)
    tight, loose = U.undistorted_camera(cam), U.undistorted_camera(cam, blank_pixels=1.0)
    assert loose.width > tight.width and loose.height > tight.height
    assert _inside_share(cam, loose) < 1.0                                     # all of the source is kept: the corners are blank
    half = U.undistorted_camera(cam, blank_pixels=0.5)
    assert tight.width <= half.width <= loose.width and tight.height <= half.height <= loose.height
    off = _camera(model, coefficients=coefficients, centre=(29.0, 24.0))       # the rule centres the output: blank pixels remain
    assert 0.9 < _inside_share(off, U.undistorted_camera(off)) < 1.0


def test_undistorted_camera_clips_the_scale_and_passes_pinholes_through():
    from itermvs_amd import undistort as U
    cam = _camera("SIMPLE_RADIAL", coefficients=[0.1])                          # unclipped: 59 x 44, scales 0.93 and 0.92
    out = U.undistorted_camera(cam, min_scale=1.0, max_scale=2.0)
    assert (out.width, out.height) == (64, 48)
    out = U.undistorted_camera(cam, min_scale=0.2, max_scale=0.5)
    assert (out.width, out.height) == (32, 24) and list(out.params[2:]) == [16.0, 12.0]
    out = U.undistorted_camera(_camera("SIMPLE_RADIAL", coefficients=[-0.1]), min_scale=0.2, max_scale=1.0)   # unclipped: 65 x 48
    assert (out.width, out.height) == (64, 48)
    for model in ("PINHOLE", "SIMPLE_PINHOLE"):
        cam = _camera(model)
        assert U.undistorted_camera(cam, blank_pixels=0.7) is cam


def test_sampling_restatement_on_known_maps():
    src = UR.make_image(29, 37)
    y, x = np.mgrid[0:29, 0:37].astype(np.float64)
    assert np.array_equal(UR.sample(src, np.stack([x, y], -1)), src)           # integer coordinates, the clamped last taps included
    half = UR.sample(src, np.stack([x + 0.5, y], -1))
    mean = np.floor((src[:, :-1].astype(np.float64) + src[:, 1:]) * 0.5 + 0.5).astype(np.uint8)
    assert np.array_equal(half[:, :-1], mean) and not half[:, -1].any()        # x + 0.5 > Ws - 1 in the last column: black
    bad = np.stack([np.where(x == 3, np.nan, x), np.where(y == 2, np.inf, y)], -1)
    got = UR.sample(src, bad)
    assert not got[2].any() and not got[:, 3].any() and np.array_equal(got[3:, 4:], src[3:, 4:])


@pytest.mark.parametrize("model", sorted(UR.UNSUPPORTED))
def test_unsupported_models_are_a_value_error_naming_the_model(model):
    import torch
    from itermvs_amd import ops, undistort as U
    from itermvs_amd.colmap import Camera
    n = UR.UNSUPPORTED[model][1]
    cam = Camera(1, model, 64, 48, np.array([50.0, 50.0, 32.0, 24.0] + [0.01] * (n - 4)))
    with pytest.raises(ValueError, match=model):
        U.undistorted_camera(cam)
    with pytest.raises(ValueError, match=model):
        U.distortion(model, [0.01], np.zeros(2), np.zeros(2))
    with pytest.raises(ValueError, match=model):
        ops.undistort_rgb8(torch.zeros((48, 64, 3), dtype=torch.uint8), model, cam.params, (50, 50, 32, 24), (48, 64))
    with pytest.raises(ValueError, match="NO_SUCH_MODEL"):
        ops.undistort_rgb8(torch.zeros((48, 64, 3), dtype=torch.uint8), "NO_SUCH_MODEL", [], (50, 50, 32, 24), (48, 64))


def test_ops_undistort_rgb8_checks_its_arguments_like_resize_rgb8():
    import torch
    from itermvs_amd import ops
    params = UR.params_of("SIMPLE_RADIAL", 50.0, 32.0, 24.0)
    with pytest.raises(RuntimeError, match="CUDA uint8"):
        ops.undistort_rgb8(torch.zeros((48, 64, 3), dtype=torch.uint8), "SIMPLE_RADIAL", params, (50, 50, 32, 24), (48, 64))
    with pytest.raises(ValueError, match="4 parameters"):
        ops.undistort_rgb8(torch.zeros((48, 64, 3), dtype=torch.uint8), "SIMPLE_RADIAL", params[:3], (50, 50, 32, 24), (48, 64))


def test_undistort_rgb8_is_declared_bound_and_exported():
    from itermvs_amd import _lib
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(itermvs_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    assert "itermvs_undistort_rgb8" in declared and "itermvs_undistort_rgb8" in _lib.PROTOTYPES
    assert hasattr(lib, "itermvs_undistort_rgb8") and len(_lib.PROTOTYPES["itermvs_undistort_rgb8"][1]) == 15
    assert "ITERMVS_ERR_MODEL = -9" in header and b"FOV" in lib.itermvs_error_string(-9)
    makefile = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert makefile.count("undistort.hip") == 2                 # SRCS and the resource-usage list


def test_undistort_rgb8_argument_validation_without_a_launch():
    """every check precedes the launch, so these calls are safe without a GPU"""
    from itermvs_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint8 * 256)()
    a = C.addressof(buf)
    k = (C.c_double * 12)(50.0, 32.0, 24.0, 0.1)
    ok = dict(src=a, Hs=4, Ws=4, model=2, params=k, n_params=4, fx=50.0, fy=50.0, cx=2.0, cy=2.0, Ho=4, Wo=4, out=a, map=None,
              stream=None)
    call = lambda **kw: lib.itermvs_undistort_rgb8(*{**ok, **kw}.values())       # noqa: E731
    for name in ("src", "params", "out"):
        assert call(**{name: None}) == -1, name                                  # ERR_NULL
    for model in (7, 10, 11, -1, 1000):
        assert call(model=model, n_params=5) == -9, model                        # ERR_MODEL: FOV, THIN_PRISM_FISHEYE, unknown ids
    for bad in (dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=0), dict(n_params=3), dict(n_params=5), dict(model=6, n_params=8),
                dict(Ho=0x7fffffff, Wo=0x7fffffff)):
        assert call(**bad) == -2, bad                                            # ERR_DIMS
    for name, (mid, n, _) in UR.MODELS.items():                                  # the table of the restatement is the library's
        assert call(model=mid, n_params=n + 1) == -2 and call(model=mid, n_params=n, Ho=0) == -2, name


def test_cli_accepts_the_new_flags_and_still_the_reference_flag_set():
    import colmap_input
    from itermvs_amd import colmap
    parse = colmap_input.build_parser().parse_args
    a = parse(["--input_folder", "in", "--output_folder", "out", "--num_src_images", "7", "--theta0", "6", "--sigma1", "2", "--sigma2", "8",
               "--convert_format"])
    assert (a.input_folder, a.output_folder, a.num_src_images, a.theta0, a.sigma1, a.sigma2, a.convert_format, a.device) == \
        ("in", "out", 7, 6.0, 2.0, 8.0, True, "cuda")
    assert (a.undistort, a.blank_pixels, a.min_scale, a.max_scale, a.num_workers) == (False, 0.0, 0.2, 2.0, 4)
    d = parse(["--input_folder", "in"])
    assert (d.output_folder, d.num_src_images, d.theta0, d.sigma1, d.sigma2, d.convert_format, d.undistort) == ("", -1, 5, 1, 10, False, False)
    u = parse(["--input_folder", "in", "--undistort", "--blank_pixels", "0.25", "--min_scale", "0.5", "--max_scale", "1.5", "--num_workers", "9"])
    assert (u.undistort, u.blank_pixels, u.min_scale, u.max_scale, u.num_workers) == (True, 0.25, 0.5, 1.5, 9)
    assert colmap.MAX_WORKERS == 16
    seen = {}
    real, colmap.convert = colmap.convert, lambda *args, **kw: seen.update(args=args, kw=kw)
    try:
        colmap.main(["--input_folder", "in", "--undistort", "--blank_pixels", "0.25", "--num_workers", "40"])
    finally:
        colmap.convert = real
    assert seen["args"] == ("in", "", -1, 5, 1, 10, False, "cuda")
    assert seen["kw"] == dict(undistort=True, blank_pixels=0.25, min_scale=0.2, max_scale=2.0, num_workers=40)


def test_convert_without_undistort_writes_todays_bytes(tmp_path, monkeypatch):
    """the device step replaced by the fixture's scores: convert() without the flag writes exactly what write_outputs and
    copy_images write for the model with its ORIGINAL cameras, and never touches the undistortion"""
    from itermvs_amd import colmap
    model, ref = load_case("params")
    assert any(c.model not in ("PINHOLE", "SIMPLE_PINHOLE") for c in model.cameras.values())
    monkeypatch.setattr(colmap, "device_scores_and_ranges", lambda *a, **kw: (ref["score"], ref["depth_ranges"]))
    monkeypatch.setattr(colmap, "undistort_images", lambda *a, **kw: pytest.fail("undistort_images called without --undistort"))
    scene, want = tmp_path / "scene", tmp_path / "want"
    (scene / "images").mkdir(parents=True)
    want.mkdir()
    colmap.write_model(str(scene / "sparse"), model, ".bin")
    for im in model.images:
        (scene / "images" / im.name).write_bytes(b"not an image: " + im.name.encode())
    model = colmap.read_model(str(scene / "sparse"))
    colmap.write_outputs(str(want), model, colmap.extrinsic_matrices(model.images), ref["score"], ref["depth_ranges"], 5)
    colmap.copy_images(str(scene / "images"), str(want / "images"), model.images)
    for name, kw in (("a", {}), ("b", dict(undistort=False, blank_pixels=1.0, num_workers=2))):
        out, info = tmp_path / name, {}
        out.mkdir()
        colmap.convert(str(scene), str(out), 5, device="cpu", info=info, **kw)
        assert sorted(info) == ["device_s", "images", "points", "read_s", "write_s"]
        files = sorted(os.path.relpath(os.path.join(d, f), str(out)) for d, _, fs in os.walk(str(out)) for f in fs)
        assert files == sorted(os.path.relpath(os.path.join(d, f), str(want)) for d, _, fs in os.walk(str(want)) for f in fs)
        assert len(files) == 2 * len(model.images) + 1
        for f in files:
            assert (out / f).read_bytes() == (want / f).read_bytes(), f

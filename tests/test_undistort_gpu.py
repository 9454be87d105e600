"""itermvs_undistort_rgb8 and colmap_input.py --undistort on the MI355X, against the numpy restatement
(tests/undistort_reference.py).

The kernel's own map of source coordinates is compared first: bit for bit for the polynomial models (+ - * / only, one rounding
each on both sides), within 1e-9 px for the three atan models (float64 carries about 1e-12 px per operation at these magnitudes
over a few dozen operations, and two atan implementations may differ by an ulp or two).  The image is then the restatement's
sampling of the KERNEL's map, bit for bit for every model: sampling has no transcendental function."""
import io

import numpy as np
import pytest
import torch

import undistort_reference as UR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATAN_TOLERANCE_PX = 1e-9


def _undistort(src, model, params, out_camera, out_hw):
    from itermvs_amd import ops
    img, coords = ops.undistort_rgb8(torch.from_numpy(src).to(DEV), model, params, out_camera, out_hw, want_map=True)
    plain = ops.undistort_rgb8(torch.from_numpy(src).to(DEV), model, params, out_camera, out_hw)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (*out_hw, 3) and tuple(coords.shape) == (*out_hw, 2)
    assert torch.equal(img, plain)                                   # the map is an extra output, not another path
    return img.cpu().numpy(), coords.cpu().numpy()


def _check(src, model, params, out_camera, out_hw):
    """the two comparisons of the module docstring -> (image, map, share of filled pixels)"""
    img, coords = _undistort(src, model, params, out_camera, out_hw)
    want = UR.source_coords(model, params, out_camera, out_hw)
    if model in UR.POLYNOMIAL:
        assert np.array_equal(coords, want, equal_nan=True)
    else:
        err = float(np.abs(coords - want).max())
        print(f"{model} {out_hw}: map, worst |kernel - restatement| = {err:.3e} px")
        assert err <= ATAN_TOLERANCE_PX
    assert np.array_equal(img, UR.sample(src, coords))
    return img, coords, float(UR.filled(coords, src.shape[:2]).mean())


def _cases():
    out = []
    for shape in sorted(UR.SHAPES):
        for model in sorted(UR.MODELS):
            out.append((shape, model, "same"))                       # the source's size: 64 columns take the 4-pixel path
            if "PINHOLE" not in model:
                out.append((shape, model, "rule"))                   # the size undistorted_camera chooses
    return out


@pytest.mark.parametrize("shape,model,size", _cases())
def test_map_and_image_equal_the_restatement(shape, model, size):
    from itermvs_amd import undistort as U
    from itermvs_amd.colmap import Camera
    w, h, f, cx, cy = UR.SHAPES[shape]
    params = UR.params_of(model, f, cx, cy)
    if size == "rule":
        out = U.undistorted_camera(Camera(1, model, w, h, np.array(params)))
        out_camera, out_hw = tuple(out.params), (out.height, out.width)
    else:
        out_camera, out_hw = (f, f, cx + 0.25, cy - 0.25), (h, w)
    _, _, share = _check(UR.make_image(h, w, seed=len(model)), model, params, out_camera, out_hw)
    assert share > 0.8                                               # the comparison is about pixels that were sampled


@pytest.mark.parametrize("model", ["PINHOLE", "SIMPLE_RADIAL", "FULL_OPENCV", "OPENCV"])
@pytest.mark.parametrize("w,h,cx,cy", [(64, 48, 32.0, 24.0), (37, 29, 18.5, 14.5)])
def test_zero_distortion_to_the_same_camera_returns_the_source_bytes(model, w, h, cx, cy):
    """f = 64: (x + 0.5 - cx) / f * f is exact, so sx = x and sy = y, the last row and column included (the clamped taps at
    sx = Ws - 1, sy = Hs - 1, weight 0)"""
    src = UR.make_image(h, w, seed=5)
    params = UR.params_of(model, 64.0, cx, cy, [0.0] * len(UR.COEFFICIENTS[model]))
    img, coords = _undistort(src, model, params, (64.0, 64.0, cx, cy), (h, w))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    assert np.array_equal(coords, np.stack([x, y], -1)) and np.array_equal(img, src)


@pytest.mark.parametrize("k", [0.1, -0.1])
def test_ramp_against_the_closed_form(k):
    """source value = x + 20 in every row; on the output row through the principal point (v = 0) the closed form
    sx = f u (1 + k u^2) + cx - 0.5 gives the value floor(sx + 20 + 0.5), and black where sx leaves [0, 63]"""
    w, h, f, cx, cy = UR.SHAPES["64x48"]
    src = np.broadcast_to((np.arange(w) + 20).astype(np.uint8)[None, :, None], (h, w, 3)).copy()
    img, coords, _ = _check(src, "SIMPLE_RADIAL", [f, cx, cy, k], (f, f, 32.5, 24.5), (h, w))
    u = (np.arange(w) - 32.0) / f
    sx = f * u * (1 + k * u ** 2) + cx - 0.5
    inside = (sx >= 0) & (sx <= w - 1)
    want = np.where(inside, np.floor(sx + 20 + 0.5), 0).astype(np.uint8)
    assert list(np.nonzero(~inside)[0]) == ([0, 1, 63] if k > 0 else [])      # k > 0: x = 1 -> sx = -0.69, x = 63 -> sx = 63.69
    assert np.array_equal(img[24], np.repeat(want[:, None], 3, 1))
    assert np.array_equal(coords[24, :, 1], np.full(w, cy - 0.5))


OUTSIDE = {
    # name: (model, parameters, output camera, output size (Ho, Wo)) on the 64 x 48 source
    "off-centre principal point": ("SIMPLE_RADIAL", [50.0, 29.0, 24.0, 0.1], None, 0.0),
    "blank_pixels = 1": ("OPENCV", UR.params_of("OPENCV", 50.0, 32.0, 24.0), None, 1.0),
    "coordinates of about 1e12": ("SIMPLE_RADIAL", [50.0, 32.0, 24.0, 1e11], (50.0, 50.0, 32.5, 24.5), (48, 64)),
    # 1 + k4 r2 = 0 exactly where (x - 32)^2 + (y - 24)^2 = 256 (r2 = 1/16, k4 = -16): radial = 1 / 0
    "vanishing denominator": ("FULL_OPENCV", UR.params_of("FULL_OPENCV", 64.0, 32.0, 24.0, [0, 0, 0, 0, 0, -16.0, 0, 0]),
                              (64.0, 64.0, 32.5, 24.5), (48, 64)),
}


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_pixels_outside_the_source_are_black(name):
    from itermvs_amd import undistort as U
    from itermvs_amd.colmap import Camera
    model, params, out_camera, extra = OUTSIDE[name]
    if out_camera is None:
        out = U.undistorted_camera(Camera(1, model, 64, 48, np.array(params)), blank_pixels=extra)
        out_camera, out_hw = tuple(out.params), (out.height, out.width)
    else:
        out_hw = extra
    src = np.maximum(UR.make_image(48, 64, seed=9), 1)               # no black pixel in the source: black means not filled
    img, coords, share = _check(src, model, params, out_camera, out_hw)
    ok = UR.filled(coords, (48, 64))
    print(f"{name}: {out_hw[1]} x {out_hw[0]}, filled share {share:.4f}")
    assert 0 < ok.sum() < ok.size
    assert not img[~ok].any() and img[ok].min() >= 1
    if name == "coordinates of about 1e12":
        assert np.nanmax(np.abs(coords)) > 1e11 and ok[24, 32]
    if name == "vanishing denominator":
        assert not np.isfinite(coords[24, 48]).all() and not np.isfinite(coords[8, 32]).all() and not ok[24, 48]


def test_ops_undistort_rgb8_refuses_bad_arguments():
    from itermvs_amd import ops
    params = UR.params_of("SIMPLE_RADIAL", 50.0, 32.0, 24.0)
    good = torch.zeros((48, 64, 3), dtype=torch.uint8, device=DEV)
    for bad in (good.float(), good[..., :2], good[None]):
        with pytest.raises(RuntimeError, match="undistort_rgb8"):
            ops.undistort_rgb8(bad, "SIMPLE_RADIAL", params, (50, 50, 32, 24), (48, 64))
    with pytest.raises(RuntimeError, match="positive"):
        ops.undistort_rgb8(good, "SIMPLE_RADIAL", params, (50, 50, 32, 24), (0, 64))
    with pytest.raises(ValueError, match="FOV"):
        ops.undistort_rgb8(good, "FOV", [50, 50, 32, 24, 0.1], (50, 50, 32, 24), (48, 64))
    by_id = ops.undistort_rgb8(good + 7, 2, params, (50, 50, 32, 24), (48, 64))              # COLMAP's model id for the name
    assert torch.equal(by_id, ops.undistort_rgb8(good + 7, "SIMPLE_RADIAL", params, (50, 50, 32, 24), (48, 64)))


def _jpeg(rgb):
    from PIL import Image as PILImage
    buf = io.BytesIO()
    PILImage.fromarray(rgb).save(buf, format="JPEG", quality=95)
    return buf.getvalue()


def test_convert_with_undistort_end_to_end(tmp_path):
    """four 64 x 48 images of one SIMPLE_RADIAL camera and a fifth of a PINHOLE camera: cam files with the output cameras, JPEGs of
    the restatement's images (SIMPLE_RADIAL's map is bit-equal, so the restatement's own map serves), the pinhole image copied,
    pair.txt and the depth ranges as without the flag"""
    from PIL import Image as PILImage
    from itermvs_amd import colmap, undistort as U
    cam = colmap.Camera(1, "SIMPLE_RADIAL", 64, 48, np.array([50.0, 32.0, 24.0, 0.1]))
    names = ["a.png", "b.png", "c.png", "d.png", "e.png"]
    model = UR.tiny_model(cam, names)
    model.cameras[2] = colmap.Camera(2, "PINHOLE", 64, 48, np.array([50.0, 50.0, 32.0, 24.0]))
    model.images[4].camera_id = 2
    scene = tmp_path / "scene"
    (scene / "images").mkdir(parents=True)
    colmap.write_model(str(scene / "sparse"), model, ".bin")
    sources = [UR.make_image(48, 64, seed=20 + i) for i in range(5)]
    for name, rgb in zip(names, sources):
        PILImage.fromarray(rgb).save(str(scene / "images" / name), format="PNG")
    plain, warped, info = tmp_path / "plain", tmp_path / "warped", {}
    plain.mkdir()
    warped.mkdir()
    colmap.convert(str(scene), str(plain), device=DEV)
    colmap.convert(str(scene), str(warped), device=DEV, info=info, undistort=True, num_workers=2)
    assert info["undistort_s"] > 0 and info["undistort_images"] == 4 and info["images"] == 5

    out = U.undistorted_camera(cam)
    assert (out.width, out.height) == (59, 44)
    coords = UR.source_coords("SIMPLE_RADIAL", cam.params, out.params, (44, 59))
    for i in range(5):
        text = open(str(warped / "cams_1" / ("%08d_cam.txt" % i))).read()
        before = open(str(plain / "cams_1" / ("%08d_cam.txt" % i))).read()
        k = colmap.intrinsic_matrix(out if i < 4 else model.cameras[2])
        want = colmap.cam_text(np.eye(4), k, 0.0, 1.0)
        block = lambda t: t.split("intrinsic\n")[1].split("\n")[:3]      # noqa: E731
        assert block(text) == block(want), i
        assert text.split("intrinsic\n")[0] == before.split("intrinsic\n")[0]              # the extrinsic block
        assert text.split("\n")[-2:] == before.split("\n")[-2:], i                        # the depth range line
        assert (block(text) == block(before)) == (i == 4)
        got = (warped / "images" / ("%08d.jpg" % i)).read_bytes()
        if i < 4:
            assert got == _jpeg(UR.sample(sources[i], coords)), i
            with PILImage.open(io.BytesIO(got)) as im:
                assert im.size == (59, 44)
        else:
            assert got == (scene / "images" / names[i]).read_bytes()                       # no distortion: copied as today
    assert (warped / "pair.txt").read_bytes() == (plain / "pair.txt").read_bytes()

    PILImage.fromarray(sources[2][:, :60].copy()).save(str(scene / "images" / "c.png"), format="PNG")
    with pytest.raises(ValueError, match=r"c\.png"):
        colmap.convert(str(scene), str(warped), device=DEV, undistort=True)

"""COLMAP converter, host side (itermvs_amd/colmap.py, colmap_input.py): the numpy restatement of the reference's arithmetic
(tests/colmap_reference.py) against the reference's own output (tests/golden/colmap_cases.npz, written by
tests/golden/make_colmap_golden.py from the real script), the model readers, the writers' text forms, the argument validation of
the two kernels' entry points and the command line.  Tolerances are multiples of ``score_floor``, the distance of the
reference's own float64 score from the same sum in extended precision, read from the fixture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import colmap_reference as CR
from conftest import ROOT, golden

CASES = ["small", "mid", "params"]


def load_case(case):
    """-> (itermvs_amd.colmap.Model, dict of the reference's results)"""
    from itermvs_amd import colmap
    g = golden("colmap_cases.npz")
    z = lambda k: g.np(f"{case}.{k}")      # noqa: E731
    cams, off = {}, 0
    for cid, model, wh, n in zip(z("cam_ids"), z("cam_models"), z("cam_wh"), z("cam_nparams")):
        cams[int(cid)] = colmap.Camera(int(cid), str(model), int(wh[0]), int(wh[1]), z("cam_params")[off:off + n].copy())
        off += int(n)
    images, off = [], 0
    for k, n in enumerate(z("obs_len")):
        images.append(colmap.Image(int(z("image_ids")[k]), z("qvec")[k].copy(), z("tvec")[k].copy(), int(z("camera_ids")[k]),
                                   str(z("names")[k]), z("obs_ids")[off:off + n].copy()))
        off += int(n)
    theta0, sigma1, sigma2, num_src = z("args")
    ref = {"score": z("score"), "depth_ranges": z("depth_ranges"), "pair_txt": str(z("pair_txt")), "cam_txt": [str(t) for t in z("cam_txt")],
           "score_floor": float(z("score_floor")), "theta0": float(theta0), "sigma1": float(sigma1), "sigma2": float(sigma2),
           "num_src_images": int(num_src)}
    return colmap.Model(cams, images, z("point_ids").copy(), z("xyz").copy()), ref


def kernel_inputs(model):
    """-> (offsets, point, xyz, centre, ext_row2, extrinsic): what convert() uploads"""
    from itermvs_amd import colmap
    offsets, point = colmap.observation_csr(model)
    ext = colmap.extrinsic_matrices(model.images)
    return offsets, point, model.xyz, colmap.camera_centres(ext), np.ascontiguousarray(ext[:, 2, :]), ext


def test_fixture_covers_what_it_claims():
    model, ref = load_case("small")
    offsets, point = kernel_inputs(model)[:2]
    iu = np.triu_indices(len(model.images), 1)
    assert (ref["score"][iu] == 0).any() and (ref["score"][iu] > 0).any() and (point == -1).any()
    assert max(np.unique(im.point3d_ids[im.point3d_ids >= 0], return_counts=True)[1].max() for im in model.images) >= 2
    ids = [im.id for im in model.images]
    assert ids != sorted(ids) and set(np.diff(sorted(ids))) != {1} and int(model.point_ids.max()) > len(model.point_ids)
    assert {c.model for c in model.cameras.values()} == {"SIMPLE_RADIAL", "PINHOLE"}
    assert 1e-17 < ref["score_floor"] < 1e-12
    mid, _ = load_case("mid")
    assert len(mid.images) == 40 and len(mid.point_ids) == 8000 and 900 < np.mean([len(im.point3d_ids) for im in mid.images]) < 1100
    assert load_case("params")[1]["num_src_images"] == 5


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference(case):
    model, ref = load_case(case)
    offsets, point, xyz, centre, row2, _ = kernel_inputs(model)
    got = CR.view_scores(offsets, point, xyz, centre, ref["theta0"], ref["sigma1"], ref["sigma2"])
    want = ref["score"]
    ratio = float(np.max(np.abs(got - want) / (ref["score_floor"] * np.maximum(1, want))))
    print(f"{case}: restatement against the reference, worst |got - ref| / (score_floor x max(1, ref)) = {ratio:.2f}")
    assert ratio <= 32
    assert np.array_equal(got == 0, want == 0) and np.array_equal(got, got.T)
    rng, mags = CR.depth_ranges(offsets, point, xyz, row2)
    assert (np.abs(rng - ref["depth_ranges"]) <= 8 * 2.0 ** -53 * mags).all()


@pytest.mark.parametrize("case", CASES)
def test_readers_return_the_fixture_model_from_both_formats(case, tmp_path):
    from itermvs_amd import colmap
    model, _ = load_case(case)
    for ext in (".bin", ".txt"):
        d = str(tmp_path / ext[1:])
        colmap.write_model(d, model, ext)
        back = colmap.read_model(d)
        assert list(back.cameras) == list(model.cameras)
        for cid, c in model.cameras.items():
            b = back.cameras[cid]
            assert (b.model, b.width, b.height) == (c.model, c.width, c.height) and np.array_equal(b.params, c.params)
        assert len(back.images) == len(model.images)
        for a, b in zip(model.images, back.images):
            assert (a.id, a.camera_id, a.name) == (b.id, b.camera_id, b.name)
            assert np.array_equal(a.qvec, b.qvec) and np.array_equal(a.tvec, b.tvec) and np.array_equal(a.point3d_ids, b.point3d_ids)
            assert b.point3d_ids.dtype == np.int64
        assert np.array_equal(back.point_ids, model.point_ids) and np.array_equal(back.xyz, model.xyz)
    # both present: the binary form is taken (the only one the reference reads)
    colmap.write_model(str(tmp_path / "bin"), colmap.Model(model.cameras, model.images[:1], model.point_ids, model.xyz), ".txt")
    assert len(colmap.read_model(str(tmp_path / "bin")).images) == len(model.images)
    assert len(colmap.read_model(str(tmp_path / "bin"), ".txt").images) == 1


def test_readers_refuse_truncated_files_and_unknown_camera_models(tmp_path):
    import struct
    from itermvs_amd import colmap
    model, _ = load_case("small")
    d = str(tmp_path / "m")
    colmap.write_model(d, model, ".bin")
    for name, cut in (("cameras.bin", 20), ("images.bin", 333), ("images.bin", 8 + 64 + 3), ("points3D.bin", 100), ("points3D.bin", 4)):
        raw = open(os.path.join(d, name), "rb").read()
        with open(os.path.join(d, name), "wb") as f:
            f.write(raw[:cut])
        with pytest.raises(ValueError, match="truncated"):
            colmap.read_model(d)
        with open(os.path.join(d, name), "wb") as f:
            f.write(raw)
    assert len(colmap.read_model(d).images) == 12
    with open(os.path.join(d, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<QiiQQ", 1, 1, 77, 640, 512) + b"\x00" * 32)
    with pytest.raises(ValueError, match="unknown camera model"):
        colmap.read_model(d)
    t = str(tmp_path / "t")
    colmap.write_model(t, model, ".txt")
    text = open(os.path.join(t, "cameras.txt")).read()
    with open(os.path.join(t, "cameras.txt"), "w") as f:
        f.write(text.replace("SIMPLE_RADIAL", "KANNALA_BRANDT"))
    with pytest.raises(ValueError, match="unknown camera model"):
        colmap.read_model(t)
    with open(os.path.join(t, "cameras.txt"), "w") as f:
        f.write(text)
    lines = open(os.path.join(t, "images.txt")).read().split("\n")
    with open(os.path.join(t, "images.txt"), "w") as f:
        f.write("\n".join(lines[:-2]))                         # the last image lost its observation line
    with pytest.raises(ValueError, match="truncated"):
        colmap.read_model(t)
    with pytest.raises(ValueError, match="neither"):
        colmap.read_model(str(tmp_path / "nothing"))
    # an observation of a point the model does not hold; an image without any valid observation
    bad = colmap.Model(model.cameras, model.images, model.point_ids[1:], model.xyz[1:])
    seen = np.concatenate([im.point3d_ids for im in model.images])
    if model.point_ids[0] in seen:
        with pytest.raises(ValueError, match="does not hold"):
            colmap.observation_csr(bad)
    ext = colmap.extrinsic_matrices(model.images)
    rng = np.tile([400.0, 900.0], (12, 1))
    rng[5] = np.nan
    with pytest.raises(ValueError, match=model.images[5].name):
        colmap.write_outputs(str(tmp_path), model, ext, np.zeros((12, 12)), rng)


def test_camera_model_table_and_matrices():
    from itermvs_amd import colmap
    assert len(colmap.CAMERA_MODELS) == 11 and colmap.CAMERA_MODELS[4] == ("OPENCV", 8) and colmap.CAMERA_MODELS[10][1] == 12
    k = colmap.intrinsic_matrix(colmap.Camera(1, "RADIAL", 10, 10, np.array([500.0, 320.0, 240.0, 0.1, 0.2])))
    assert np.array_equal(k, [[500, 0, 320], [0, 500, 240], [0, 0, 1]])
    k = colmap.intrinsic_matrix(colmap.Camera(1, "OPENCV", 10, 10, np.array([500.0, 510.0, 320.0, 240.0, 1, 2, 3, 4])))
    assert np.array_equal(k, [[500, 0, 320], [0, 510, 240], [0, 0, 1]])
    with pytest.raises(ValueError, match="unknown camera model"):
        colmap.intrinsic_matrix(colmap.Camera(1, "NOPE", 1, 1, np.zeros(4)))
    r = colmap.quaternion_to_rotation_matrix([np.cos(0.3), 0.0, np.sin(0.3), 0.0])            # 0.6 rad about y
    assert np.allclose(r, [[np.cos(0.6), 0, np.sin(0.6)], [0, 1, 0], [-np.sin(0.6), 0, np.cos(0.6)]], atol=1e-15)
    im = colmap.Image(1, np.array([np.cos(0.3), 0.0, np.sin(0.3), 0.0]), np.array([1.0, 2.0, 3.0]), 1, "a", np.zeros(0, np.int64))
    e = colmap.extrinsic_matrices([im])
    assert np.allclose(e[0, :3, :3] @ colmap.camera_centres(e)[0] + e[0, :3, 3], 0, atol=1e-14) and e[0, 3].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("case", CASES)
def test_writers_reproduce_the_reference_files(case, tmp_path):
    """fed the reference's own score / ranges: cams_1/*.txt byte for byte, pair.txt under the ties rule"""
    from itermvs_amd import colmap
    model, ref = load_case(case)
    ext = colmap.extrinsic_matrices(model.images)
    colmap.write_outputs(str(tmp_path), model, ext, ref["score"], ref["depth_ranges"], ref["num_src_images"])
    for i, want in enumerate(ref["cam_txt"]):
        assert open(str(tmp_path / "cams_1" / ("%08d_cam.txt" % i))).read() == want, i
    assert len(os.listdir(str(tmp_path / "cams_1"))) == len(model.images)
    got = open(str(tmp_path / "pair.txt")).read()
    checked = CR.compare_pair_text(got, ref["pair_txt"], ref["score"], ref["score_floor"])
    rows = CR.pair_rows(ref["pair_txt"])
    assert all(len(r) == (5 if case == "params" else len(model.images)) for r in rows)
    nonzero_adjacent = sum(max(0, sum(float(t) != 0 for _, t in r) - 1) for r in rows)
    assert checked >= 0.9 * nonzero_adjacent > 0
    # the scan-folder readers of the engine take the files as they are
    from itermvs_amd.scan_dataset import read_cam_file
    k, e, dmin, dmax = read_cam_file(str(tmp_path / "cams_1" / "00000000_cam.txt"))
    assert np.array_equal(e, ext[0].astype(np.float32)) and abs(dmin - ref["depth_ranges"][0, 0]) < 1e-6 < dmax - dmin
    assert np.array_equal(k, colmap.intrinsic_matrix(model.cameras[model.images[0].camera_id]).astype(np.float32))


def test_images_are_copied_or_reencoded(tmp_path):
    from PIL import Image as PILImage
    from itermvs_amd import colmap
    model, _ = load_case("small")
    src = tmp_path / "images"
    src.mkdir()
    for n, im in enumerate(model.images[:3]):
        PILImage.fromarray(np.full((8, 12, 3), 40 * n, np.uint8)).save(str(src / im.name), format="PNG")
    colmap.copy_images(str(src), str(tmp_path / "a"), model.images[:3])
    assert (tmp_path / "a" / "00000002.jpg").read_bytes() == (src / model.images[2].name).read_bytes()
    colmap.copy_images(str(src), str(tmp_path / "b"), model.images[:3], convert_format=True)
    with PILImage.open(str(tmp_path / "b" / "00000001.jpg")) as im:
        assert im.format == "JPEG" and im.size == (12, 8) and abs(int(np.asarray(im)[0, 0, 0]) - 40) <= 2


def test_argument_validation_of_the_entry_points():
    """validation happens before any launch: safe without a GPU"""
    from itermvs_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    assert lib.itermvs_view_scores(a, a, a, a, 2, 5, 5.0, 1.0, 10.0, None, None) == -1            # ERR_NULL
    assert lib.itermvs_view_scores(None, a, a, a, 2, 5, 5.0, 1.0, 10.0, a, None) == -1
    assert lib.itermvs_view_scores(a, None, a, a, 2, 5, 5.0, 1.0, 10.0, a, None) == -1
    assert lib.itermvs_view_scores(a, a, None, a, 2, 5, 5.0, 1.0, 10.0, a, None) == -1
    assert lib.itermvs_view_scores(a, a, a, None, 2, 5, 5.0, 1.0, 10.0, a, None) == -1
    assert lib.itermvs_view_scores(a, a, a, a, 0, 5, 5.0, 1.0, 10.0, a, None) == -2               # ERR_DIMS: V < 1
    assert lib.itermvs_view_scores(a, a, a, a, 2, 0, 5.0, 1.0, 10.0, a, None) == -2               # P < 1
    assert lib.itermvs_depth_ranges(a, a, a, a, 2, 5, None, None) == -1
    assert lib.itermvs_depth_ranges(None, a, a, a, 2, 5, a, None) == -1
    assert lib.itermvs_depth_ranges(a, a, a, None, 2, 5, a, None) == -1
    assert lib.itermvs_depth_ranges(a, a, a, a, -3, 5, a, None) == -2
    assert lib.itermvs_depth_ranges(a, a, a, a, 2, 0, a, None) == -2


def test_ops_refuse_cpu_tensors_and_check_offsets_on_the_host():
    from itermvs_amd import ops
    off, pt = torch.tensor([0, 2, 4]), torch.zeros(4, dtype=torch.int32)
    xyz, c, r2 = torch.zeros((3, 3), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.float64), torch.zeros((2, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.view_scores(off, pt, xyz, c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.depth_ranges(off, pt, xyz, r2)

    class OnDevice(torch.Tensor):              # a CPU tensor that claims to live on the device: reaches the host-side value checks
        is_cuda = True

    dev = lambda t: t.as_subclass(OnDevice)    # noqa: E731
    for bad in ([0, 3, 2], [-1, 2, 4], [0, 2, 5]):
        with pytest.raises(RuntimeError, match="offsets must ascend"):
            ops.view_scores(torch.tensor(bad), dev(pt), dev(xyz), dev(c))
        with pytest.raises(RuntimeError, match="offsets must ascend"):
            ops.depth_ranges(torch.tensor(bad), dev(pt), dev(xyz), dev(r2))
    with pytest.raises(RuntimeError, match="HOST"):
        ops.view_scores(off.int(), dev(pt), dev(xyz), dev(c))
    with pytest.raises(RuntimeError, match="int32"):
        ops.view_scores(off, dev(pt.long()), dev(xyz), dev(c))
    with pytest.raises(RuntimeError, match="per-view"):
        ops.depth_ranges(off, dev(pt), dev(xyz), dev(c))


def test_cli_accepts_the_reference_flag_set():
    import colmap_input
    a = colmap_input.build_parser().parse_args(["--input_folder", "in", "--output_folder", "out", "--num_src_images", "7", "--theta0", "6",
                                                "--sigma1", "2", "--sigma2", "8", "--convert_format"])
    assert (a.input_folder, a.output_folder, a.num_src_images, a.theta0, a.sigma1, a.sigma2, a.convert_format, a.device) == \
        ("in", "out", 7, 6.0, 2.0, 8.0, True, "cuda")
    d = colmap_input.build_parser().parse_args(["--input_folder", "in"])              # eval_custom.sh passes the input folder alone
    assert (d.output_folder, d.num_src_images, d.theta0, d.sigma1, d.sigma2, d.convert_format) == ("", -1, 5, 1, 10, False)
    assert colmap_input.build_parser().parse_args(["--input_folder", "in", "--device", "cuda:1"]).device == "cuda:1"
    from itermvs_amd import colmap
    with pytest.raises(ValueError, match="Invalid input folder"):
        colmap.convert(os.path.join(ROOT, "no", "such", "folder"))

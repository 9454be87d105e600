"""The host side of the fusion that needs no GPU: the one mapping from eval.py's flags to the keyword arguments of
``fusion.filter_depth`` / ``fusion.fuse_scan``, the one intrinsics rescale, and the header-last rule of the cloud's file."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT


def _eval():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


def test_flags_to_keywords_defaults():
    """what eval.fuse_scans and scan_fuse.fuse_scans_from_memory passed on without a fusion flag"""
    from itermvs_amd import fusion
    a = _eval().build_parser().parse_args([])
    assert fusion.fuse_keywords_from_args(a, "out/scan_mesh.ply") == dict(
        geo_pixel_thres=1, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=3, dedupe=False, normals=False, normal_edge_thres=0.01,
        mesh=None, consistency="static", dyn_pixel_step=0.25, dyn_depth_step=1.0 / 1300.0, dyn_n_min=2, dyn_n_max=10)
    b = _eval().build_parser().parse_args(["--geo_mask_thres", "2"])
    assert fusion.fuse_keywords_from_args(b, "x.ply")["geo_mask_thres"] == 2


def test_flags_to_keywords_with_every_flag_set():
    """--geo_mask_thres stays at its default: the driver refuses it beside --geo_consistency dynamic"""
    from itermvs_amd import fusion
    argv = ["--filter", "--fuse_points", "device", "--geo_pixel_thres", "0.5", "--geo_depth_thres", "0.02", "--photo_thres", "0.4",
            "--fuse_dedupe", "--ply_normals", "--normal_edge_thres", "0.02", "--geo_consistency", "dynamic", "--dyn_pixel_step", "0.4",
            "--dyn_depth_step", "0.0015", "--dyn_levels", "1", "3", "--mesh", "--mesh_resolution", "64", "--mesh_voxel", "0.5",
            "--mesh_bounds", "-1", "-2", "-3", "1", "2", "3", "--mesh_bounds_quantile", "0.05", "--mesh_trunc", "2", "--mesh_min_count", "3",
            "--mesh_min_component", "7", "--mesh_component_share", "0.25", "--mesh_budget_gb", "2"]
    a = _eval().build_parser().parse_args(argv)
    got = fusion.fuse_keywords_from_args(a, "out/scan_mesh.ply")
    assert got == dict(
        geo_pixel_thres=0.5, geo_depth_thres=0.02, photo_thres=0.4, geo_mask_thres=3, dedupe=True, normals=True, normal_edge_thres=0.02,
        mesh=fusion.MeshOptions(path="out/scan_mesh.ply", bounds=(-1.0, -2.0, -3.0, 1.0, 2.0, 3.0), bounds_quantile=0.05, voxel=0.5,
                                resolution=64, trunc_voxels=2.0, min_count=3, budget_bytes=2 << 30, batch_views=4, min_component=7,
                                component_share=0.25),
        consistency="dynamic", dyn_pixel_step=0.4, dyn_depth_step=0.0015, dyn_n_min=1, dyn_n_max=3)
    assert type(got["dedupe"]) is bool and type(got["normals"]) is bool and type(got["normal_edge_thres"]) is float
    fusion.dynamic_options(**{k: got[k] for k in ("consistency", "dyn_pixel_step", "dyn_depth_step", "dyn_n_min", "dyn_n_max")})


def test_intrinsics_rescale_is_the_in_place_float32_product(tmp_path):
    from itermvs_amd import fusion
    k = np.array([[2892.33, 0.1, 823.205], [0, 2883.175, 619.071], [0, 0, 1]], np.float32)
    e = np.random.default_rng(0).standard_normal((4, 4)).astype(np.float32)
    rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)      # noqa: E731
    os.makedirs(tmp_path / "cams_1")
    (tmp_path / "cams_1" / "00000007_cam.txt").write_text(f"extrinsic\n{rows(e)}\n\nintrinsic\n{rows(k)}\n\n425 2.5\n")
    sx, sy = 640 / 1600, 512 / 1200                    # neither is a float32, nor a double without rounding
    want = k.copy()
    want[0] *= sx
    want[1] *= sy
    got_k, got_e = fusion.read_scaled_camera(str(tmp_path), 7, sx, sy)
    assert got_k.dtype == np.float32 and got_k.tobytes() == want.tobytes() and got_k.tobytes() != k.tobytes()
    assert got_e.dtype == np.float32 and got_e.tobytes() == e.tobytes()
    plain_k, plain_e = fusion.read_camera_parameters(str(tmp_path / "cams_1" / "00000007_cam.txt"))
    assert plain_k.tobytes() == k.tobytes() and plain_e.tobytes() == e.tobytes()


def _fake_download(calls):
    def download(records, nbytes, write, seconds):
        calls.append(nbytes)
        if nbytes == 0:
            return 0
        write(np.frombuffer(records, np.uint8)[:nbytes])
        return 1
    return download


@pytest.mark.parametrize("normals", [False, True])
def test_ply_appender_writes_the_header_last_and_the_parts_in_order(tmp_path, normals):
    from itermvs_amd import fusion
    rec = 27 if normals else 15
    parts = [bytes(range(1, 2 * rec + 1)), b"", bytes(range(100, 100 + 3 * rec))]    # 2, 0 and 3 vertices
    seconds = {"download_wait": 0.0, "file_write": 0.0}
    calls = []
    path = str(tmp_path / "cloud.ply")
    with fusion._open_cloud(path, normals, seconds, download=_fake_download(calls)) as ply:
        for i, part in enumerate(parts):
            ply.append(part + b"\xa5" * 7, len(part) // rec, rec, last=i == 2)      # the buffer is longer than what the group emitted
            if i < 2:
                assert ply.f.tell() == 0                                            # nothing is written before the total is known
    assert open(path, "rb").read() == fusion.ply_header(5, normals) + b"".join(parts)
    assert ply.vertices == 5 and ply.chunks == 2 and calls == [2 * rec, 0, 3 * rec]


def test_ply_appender_without_groups_writes_the_empty_header(tmp_path):
    from itermvs_amd import fusion
    path = str(tmp_path / "empty.ply")
    with fusion._open_cloud(path, False, {"file_write": 0.0}, download=_fake_download([])) as ply:
        pass
    assert open(path, "rb").read() == fusion.ply_header(0) and ply.vertices == 0 and ply.chunks == 0


@pytest.mark.parametrize("spooled_groups", [0, 1])
def test_ply_appender_removes_the_file_when_the_fusion_raises(tmp_path, spooled_groups):
    from itermvs_amd import fusion
    path = str(tmp_path / "gone.ply")
    with pytest.raises(RuntimeError, match="the records buffer holds"):
        with fusion._open_cloud(path, False, {"file_write": 0.0}, download=_fake_download([])) as ply:
            for _ in range(spooled_groups):
                ply.append(bytes(15), 1, 15, last=False)
            assert os.path.exists(path)
            raise RuntimeError("fuse_scan: the records buffer holds too little")
    assert not os.path.exists(path)

"""Point-cloud emission on the GPU (itermvs_fuse_points, fusion.fuse_scan), the parts that need no GPU: the C ABI and its
argument checks, the grouping of reference views under a byte budget, the colour shortcut the kernel relies on, the PLY
assembly from raw vertex records, and the new keyword arguments of filter_depth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def test_fuse_points_is_declared_bound_and_exported():
    from itermvs_amd import _lib
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(itermvs_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in ("itermvs_fuse_points", "itermvs_fuse_points_workspace_bytes"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "eval.py:287-308" in header
    assert lib.itermvs_version() == _lib.ABI_VERSION == 20
    assert len(_lib.PROTOTYPES["itermvs_fuse_points"][1]) == 15
    makefile = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert makefile.count("fuse_points.hip") == 2                       # SRCS and the resource-usage list


def test_fuse_points_argument_validation_without_a_launch():
    """every check precedes the first launch, so these calls are safe without a GPU"""
    from itermvs_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint8 * 256)()
    a = C.addressof(buf)
    ok = dict(depth_avg=a, final_mask=a, photo_mask=None, geo_mask=None, cam=a, rgb=a, H=4, W=4, records=a, capacity=16,
              cursor=a, view_counts=a, view=0, workspace=a, stream=None)
    call = lambda **kw: lib.itermvs_fuse_points(*{**ok, **kw}.values())          # noqa: E731
    for name in ("depth_avg", "final_mask", "cam", "rgb", "records", "cursor", "view_counts", "workspace"):
        assert call(**{name: None}) == -1, name                                  # ERR_NULL
    for bad in (dict(H=0), dict(W=0), dict(H=-3), dict(capacity=-1), dict(view=-1), dict(H=46341, W=46341),
                dict(H=1, W=0x7fffff01)):
        assert call(**bad) == -2, bad                                            # ERR_DIMS
    assert lib.itermvs_fuse_points_workspace_bytes(0, 4) == -2
    assert lib.itermvs_fuse_points_workspace_bytes(46341, 46341) == -2           # H * W beyond the 32-bit pixel index
    assert lib.itermvs_fuse_points_workspace_bytes(1, 0x7fffff00) > 0
    assert lib.itermvs_fuse_points_workspace_bytes(1152, 1600) == 3 * 4 * 7200   # three uint32 counts per 256-pixel workgroup
    assert lib.itermvs_fuse_points_workspace_bytes(1, 1) == 12 and lib.itermvs_fuse_points_workspace_bytes(1, 257) == 24


def test_ops_fuse_points_refuses_cpu_tensors():
    import torch
    from itermvs_amd import ops
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)                      # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fuse_points(z(4, 4, dt=torch.float64), z(4, 4), z(21, dt=torch.float32), z(4, 4, 3), z(240), z(1, dt=torch.int64),
                        z(1, 4, dt=torch.int64), 0)


def test_group_views_partitions_in_order_within_the_budget():
    from itermvs_amd import fusion
    h, w = 1152, 1600
    per = h * w * 15
    assert fusion.group_views(49, h, w, 2 << 30) == [(0, 49)]                    # a DTU scan fits the default budget
    for n, budget in ((49, 10 * per), (49, 10 * per + per - 1), (7, per), (5, 3 * per), (1, per), (0, per), (49, 1 << 40)):
        groups = fusion.group_views(n, h, w, budget)
        assert [i for a, b in groups for i in range(a, b)] == list(range(n))     # every view once, order kept
        assert all(a < b and (b - a) * per <= budget for a, b in groups)
        assert len(groups) == -(-n // (budget // per))                           # and no more groups than the budget asks for
    with pytest.raises(ValueError, match="below one"):
        fusion.group_views(3, h, w, per - 1)


def test_colour_conversion_is_the_identity_on_bytes():
    """eval.py:72,296: img = uint8 / 255. in float32, colour = (img * 255).astype(uint8).  The kernel copies the bytes."""
    u = np.arange(256, dtype=np.uint8)
    img = u.astype(np.float32) / 255.0                                           # fusion.read_scan_image
    assert img.dtype == np.float32 and np.array_equal((img * 255).astype(np.uint8), u)
    assert np.array_equal(((np.float32(1) * u / np.float32(255.0)) * 255).astype(np.uint8), u)


def test_ply_from_raw_records_equals_write_ply(tmp_path):
    from itermvs_amd import fusion, ops
    assert RECORD.itemsize == ops.POINT_RECORD_BYTES == 15
    xyz = np.array([[0.5, -1.25, 700.0], [np.inf, 3e-41, -0.0], [1e30, np.nan, 2.0], [7, 8, 9]], np.float32)
    rgb = np.array([[0, 127, 255], [1, 2, 3], [250, 251, 252], [9, 8, 7]], np.uint8)
    fusion.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    body = b"".join(xyz[i].astype("<f4").tobytes() + rgb[i].tobytes() for i in range(4))      # hand-made records
    assert (tmp_path / "a.ply").read_bytes() == fusion.ply_header(4) + body
    assert fusion.ply_header(0).startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\n")
    back = np.frombuffer(body, RECORD)
    assert back["x"].view(np.uint32).tolist() == xyz[:, 0].view(np.uint32).tolist() and back["blue"].tolist() == [255, 3, 252, 7]


def test_filter_depth_rejects_unknown_points_mode_before_any_work(tmp_path):
    from itermvs_amd import fusion
    with pytest.raises(ValueError, match="points must be"):                      # no pair.txt there: the check comes first
        fusion.filter_depth(str(tmp_path / "none"), str(tmp_path / "none"), str(tmp_path / "x.ply"), 1.0, 0.01, 0.3,
                            img_wh=(8, 8), points="bogus")
    assert not (tmp_path / "x.ply").exists()


def test_save_mask_roundtrip(tmp_path):
    from PIL import Image
    from itermvs_amd import fusion
    rng = np.random.default_rng(0)
    m = rng.uniform(size=(13, 17)) < 0.45
    fusion.save_mask(str(tmp_path / "m.png"), m)
    fusion.save_mask(str(tmp_path / "u.png"), m.astype(np.uint8))                # the kernels' uint8 0 / 1 masks
    for name in ("m.png", "u.png"):
        with Image.open(str(tmp_path / name)) as im:
            assert im.mode == "L" and im.size == (17, 13)
            a = np.array(im)
        assert set(np.unique(a)) <= {0, 255} and np.array_equal(a == 255, m)


def test_eval_parser_has_the_fusion_switches():
    import sys
    sys.path.insert(0, ROOT)
    import eval as E
    a = E.build_parser().parse_args([])
    assert a.fuse_points == "host" and a.save_masks is False
    a = E.build_parser().parse_args(["--filter", "--fuse_points", "device", "--save_masks"])
    assert a.fuse_points == "device" and a.save_masks is True
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--fuse_points", "somewhere"])

"""itermvs_resize_rgb8 and eval.py --fuse_source memory, the parts that need no GPU: Pillow's coefficient tables as the package
computes them, the C ABI of the new entry point, the new flags and the whole-scan sharding."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from resize_reference import IMAGES, SHAPES, integer_resize, make_image, pillow_resize


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("src_hw,dst_hw", SHAPES)
def test_package_tables_through_integer_passes_equal_pillow(src_hw, dst_hw, kind):
    from itermvs_amd.resize import resize_tables
    raw = make_image(kind, *src_hw)
    got = integer_resize(raw, dst_hw[0], dst_hw[1], resize_tables(src_hw[0], src_hw[1], dst_hw[0], dst_hw[1]))
    want = pillow_resize(raw, *dst_hw)
    assert got.dtype == np.uint8 and got.shape == want.shape == (dst_hw[0], dst_hw[1], 3)
    assert np.array_equal(got, want)


def test_tables_have_the_documented_form():
    from itermvs_amd.resize import bilinear_coefficients
    bounds, kk = bilinear_coefficients(150, 32)                # 4.7x: 11 taps, more than any fixed small footprint
    assert bounds.dtype == kk.dtype == np.int32 and bounds.shape == (32, 2) and kk.shape[0] == 32
    assert kk.shape[1] == 11                                   # Pillow's ksize = ceil(support) * 2 + 1, support = 150 / 32
    assert 9 <= int(bounds[:, 1].max()) <= 11                  # a window of 2 * 4.6875 samples holds 9 or 10 of them
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 150).all()     # no tap leaves the image
    assert (kk >= 0).all() and (np.abs(kk.sum(1).astype(np.int64) - (1 << 22)) <= 11).all()
    for i, (_, count) in enumerate(bounds):
        assert not kk[i, count:].any()
    bounds, kk = bilinear_coefficients(64, 64)                 # an axis that keeps its size: the identity
    assert np.array_equal(bounds[:, 0], np.arange(64)) and (bounds[:, 1] == 1).all() and (kk == 1 << 22).all()
    with pytest.raises(ValueError):
        bilinear_coefficients(0, 4)


def test_resize_rgb8_is_declared_bound_and_exported():
    from itermvs_amd import _lib
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(itermvs_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    assert "itermvs_resize_rgb8" in declared and "itermvs_resize_rgb8" in _lib.PROTOTYPES and hasattr(lib, "itermvs_resize_rgb8")
    assert len(_lib.PROTOTYPES["itermvs_resize_rgb8"][1]) == 14
    exports = open(os.path.join(ROOT, "itermvs_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*itermvs_\*;", exports)        # the version script exports the itermvs_ prefix
    makefile = open(os.path.join(ROOT, "itermvs_amd", "csrc", "Makefile")).read()
    assert makefile.count("resize_rgb8.hip") == 2               # SRCS and the resource-usage list


def test_resize_rgb8_argument_validation_without_a_launch():
    """every check precedes the launch, so these calls are safe without a GPU"""
    from itermvs_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint8 * 256)()
    a = C.addressof(buf)
    ok = dict(src=a, V=1, Hs=4, Ws=4, H=2, W=2, xbounds=a, xk=a, KX=5, ybounds=a, yk=a, KY=5, out=a, stream=None)
    call = lambda **kw: lib.itermvs_resize_rgb8(*{**ok, **kw}.values())          # noqa: E731
    for name in ("src", "xbounds", "xk", "ybounds", "yk", "out"):
        assert call(**{name: None}) == -1, name                                  # ERR_NULL
    for bad in (dict(V=0), dict(Hs=0), dict(Ws=-1), dict(H=0), dict(W=0), dict(KX=0), dict(KY=-2)):
        assert call(**bad) == -2, bad                                            # ERR_DIMS


def test_ops_resize_rgb8_refuses_cpu_tensors():
    import torch
    from itermvs_amd import ops
    with pytest.raises(RuntimeError, match="CUDA uint8"):
        ops.resize_rgb8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4)


def _parse(argv):
    sys.path.insert(0, ROOT)
    import eval as E
    return E, E.build_parser().parse_args(argv)


def test_fuse_source_defaults_keep_todays_behaviour():
    E, a = _parse([])
    assert a.fuse_source == "files" and a.no_pfm is False and E.check_fuse_source(a) == "files"
    E, a = _parse(["--dataset", "folder", "--filter", "--fuse_source", "memory", "--no_pfm"])
    assert E.check_fuse_source(a) == "memory" and a.no_pfm is True
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--fuse_source", "somewhere"])
    assert "memory" in E.build_parser().format_help().split("--fuse_points")[2]      # the flag's help says what memory does


@pytest.mark.parametrize("argv,names", [
    (["--dataset", "folder", "--fuse_source", "memory"], ["--filter"]),
    (["--dataset", "synthetic", "--filter", "--fuse_source", "memory"], ["--dataset folder", "synthetic"]),
    (["--fuse_source", "memory"], ["--dataset folder", "--filter"]),
    (["--dataset", "folder", "--filter", "--no_pfm"], ["--no_pfm", "--fuse_source memory"]),
    (["--dataset", "folder", "--filter", "--fuse_source", "files", "--no_pfm"], ["--no_pfm", "--fuse_source memory"]),
])
def test_fuse_source_argument_validation_names_the_cause(argv, names):
    E, a = _parse(argv)
    with pytest.raises(SystemExit) as e:
        E.check_fuse_source(a)
    for name in names:
        assert name in str(e.value), (name, str(e.value))
    with pytest.raises(SystemExit) as e2:              # the driver entry refuses before it touches a device
        E.fuse_memory(a)
    assert str(e2.value) == str(e.value)


def test_ranks_take_whole_scans():
    """3 scans over 2 ranks: every scan goes to exactly one rank, with all of its depth maps"""
    from itermvs_amd import shard
    from itermvs_amd.scan_fuse import scan_indices

    class Metas:
        metas = [(f"scan{s}", v, [(v + 1) % 4]) for s in (1, 2, 3) for v in range(4)]

    scans = list(dict.fromkeys(m[0] for m in Metas.metas))
    assert scans == ["scan1", "scan2", "scan3"]
    mine = [[scans[i] for i in shard.shard_indices(len(scans), rank, 2)] for rank in range(2)]
    assert sorted(mine[0] + mine[1]) == scans and not set(mine[0]) & set(mine[1])
    maps = [[i for s in part for i in scan_indices(Metas, s)] for part in mine]
    assert sorted(maps[0] + maps[1]) == list(range(12))
    for part, idx in zip(mine, maps):
        assert {Metas.metas[i][0] for i in idx} == set(part) and len(idx) == 4 * len(part)


def test_a_source_view_without_a_depth_map_is_refused():
    from itermvs_amd.scan_fuse import check_views

    class Metas:
        metas = [("scan1", v, [v + 1]) for v in range(3)]          # view 3 is a source only

    check_views(Metas, "scan1", [(0, [1, 2]), (1, [2])])
    with pytest.raises(FileNotFoundError, match=r"scan1.*view 3"):
        check_views(Metas, "scan1", [(0, [1]), (2, [3])])

"""eval.py --fuse_source memory on the MI355X: itermvs_resize_rgb8 against Pillow, and the one-pass driver against today's two
passes (save_depth, then fuse_scans with --fuse_points device) -- the same PLY, PFM and mask bytes, no file touched twice."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from resize_reference import IMAGES, SHAPES, make_image, pillow_resize

pytestmark = pytest.mark.gpu
DEV = "cuda"


# -- 1. the kernel ------------------------------------------------------------------------------------------------------
# the acceptance shapes all have W % 4 == 0 (four pixels per thread); two more take the one-pixel-per-thread launch
ODD_SHAPES = [((30, 45), (21, 34)), ((9, 7), (13, 5))]


def _stack(src_hw):
    """V = 3: the random, the all-255 and the all-0 image of one shape"""
    return np.stack([make_image(kind, *src_hw) for kind in IMAGES])


@pytest.mark.parametrize("src_hw,dst_hw", SHAPES + ODD_SHAPES)
def test_resize_rgb8_equals_pillow(src_hw, dst_hw):
    from itermvs_amd import ops
    raw = _stack(src_hw)
    got = ops.resize_rgb8(torch.from_numpy(raw).to(DEV), dst_hw[0], dst_hw[1])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, dst_hw[0], dst_hw[1], 3) and got.is_contiguous()
    got = got.cpu().numpy()
    for v in range(3):
        assert np.array_equal(got[v], pillow_resize(raw[v], *dst_hw)), v


@pytest.mark.parametrize("src_hw,dst_hw", [((50, 64), (48, 64)), ((75, 100), (64, 96))])
def test_resize_rgb8_from_an_unaligned_source(src_hw, dst_hw):
    """a source that does not start on a 4-byte boundary cannot be read as dwords: the byte-wise launch gives the same bytes"""
    from itermvs_amd import ops
    raw = _stack(src_hw)
    flat = torch.zeros(raw.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(raw).to(DEV).reshape(-1)
    view = flat[1:].view(raw.shape)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    got = ops.resize_rgb8(view, *dst_hw).cpu().numpy()
    for v in range(3):
        assert np.array_equal(got[v], pillow_resize(raw[v], *dst_hw)), v


def test_resize_rgb8_same_size_returns_the_input_bytes():
    from itermvs_amd import ops
    raw = torch.from_numpy(_stack((36, 40))).to(DEV)
    got = ops.resize_rgb8(raw, 36, 40)
    assert got.dtype == torch.uint8 and torch.equal(got, raw)


def test_resize_rgb8_refuses_bad_arguments():
    from itermvs_amd import ops
    good = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    for bad in (good.cpu(), good.float(), torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=DEV), good[0]):
        with pytest.raises(RuntimeError, match="resize_rgb8"):
            ops.resize_rgb8(bad, 4, 4)
    with pytest.raises(RuntimeError, match="positive"):
        ops.resize_rgb8(good, 0, 4)


# -- 2. the driver ------------------------------------------------------------------------------------------------------
N_VIEWS = 6
IMG_WH = (96, 64)                  # inference size; the files are 100 x 75, so colours and intrinsics rescale on both axes
LOOSE = ["--photo_thres", "0", "--geo_pixel_thres", "1e6", "--geo_depth_thres", "1e6", "--geo_mask_thres", "1"]


def write_scans(root, source_only_view=False):
    """two scans of six views stored at 75 x 100; every view is a reference view with four source views.
    ``source_only_view``: view 5 of both scans is named as a source but is no reference view."""
    from PIL import Image
    from itermvs_amd import synthetic
    w, h = IMG_WH
    names = []
    for si in range(2):
        s = synthetic.make_scene_sample(num_views=N_VIEWS, height=h, width=w, seed=40 + si)
        k0, exts = synthetic.camera_parameters(N_VIEWS, h, w, ref_shift=si)
        k = np.array(k0, dtype=np.float64)
        k[0] *= 100 / w                                       # the intrinsics of the 100 x 75 file
        k[1] *= 75 / h
        scan = os.path.join(root, f"scan{si + 1}")
        os.makedirs(os.path.join(scan, "cams_1"))
        os.makedirs(os.path.join(scan, "images"))
        for v in range(N_VIEWS):
            img = ((s["imgs"]["level_0"][0, v].permute(1, 2, 0).numpy() + 1) * 127.5).round().clip(0, 255).astype(np.uint8)
            Image.fromarray(img).resize((100, 75), Image.BICUBIC).save(os.path.join(scan, "images", "{:0>8}.png".format(v)))
            rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)      # noqa: E731
            with open(os.path.join(scan, "cams_1", "{:0>8}_cam.txt".format(v)), "w") as f:
                f.write(f"extrinsic\n{rows(np.array(exts[v], dtype=np.float64))}\n\nintrinsic\n{rows(k)}\n\n425.0 2.5 192 935.0\n")
        refs = range(N_VIEWS - 1) if source_only_view else range(N_VIEWS)
        lines = [str(len(refs))]
        for v in refs:
            srcs = [(v + 1) % N_VIEWS, (v + 5) % N_VIEWS, (v + 2) % N_VIEWS, (v + 3) % N_VIEWS]
            lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} 1.0" for u in srcs)]
        with open(os.path.join(scan, "pair.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        names.append(f"scan{si + 1}")
    return names


def _eval_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


def _args(data, out, extra):
    return _eval_module().build_parser().parse_args(
        ["--dataset", "folder", "--testpath", str(data), "--n_views", "4", "--img_wh", str(IMG_WH[0]), str(IMG_WH[1]),
         "--iteration", "2", "--outdir", str(out), "--filter"] + LOOSE + list(extra))


STAT_LINE = re.compile(r"^processing \S+, ref-view\d+, geo_mask:")


def _stat_lines(capsys):
    return [line for line in capsys.readouterr().out.splitlines() if STAT_LINE.match(line)]


def two_pass(data, out, extra, capsys):
    """today's path -> ({scan: stats as filter_depth returns them}, the printed mask-share lines)"""
    from itermvs_amd import fusion
    E = _eval_module()
    args = _args(data, out, ["--fuse_points", "device"] + list(extra))
    capsys.readouterr()
    E.save_depth(args)
    returned = {}
    inner = fusion.filter_depth

    def recording(scan_folder, *a, **kw):
        returned[os.path.basename(scan_folder)] = inner(scan_folder, *a, **kw)
        return returned[os.path.basename(scan_folder)]

    fusion.filter_depth = recording
    try:
        assert E.fuse_scans(args) == 2
    finally:
        fusion.filter_depth = inner
    return returned, _stat_lines(capsys)


def from_memory(data, out, extra, capsys):
    E = _eval_module()
    capsys.readouterr()
    returned = E.fuse_memory(_args(data, out, ["--fuse_source", "memory"] + list(extra)))
    return returned, _stat_lines(capsys)


def _files(out, suffix=None):
    got = {}
    for dp, _, files in os.walk(out):
        for f in files:
            if suffix is None or f.endswith(suffix):
                with open(os.path.join(dp, f), "rb") as fh:
                    got[os.path.relpath(os.path.join(dp, f), out)] = fh.read()
    return got


def _vertices(ply: bytes) -> int:
    return int(re.search(rb"element vertex (\d+)", ply).group(1))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("scans")
    write_scans(str(root))
    return root


def _compare(data, tmp_path, extra, capsys):
    a_stats, a_lines = two_pass(data, tmp_path / "a", extra, capsys)
    b_stats, b_lines = from_memory(data, tmp_path / "b", extra, capsys)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    plys = sorted(n for n in a if n.endswith(".ply"))
    assert plys == ["scan1.ply", "scan2.ply"]
    for n in plys:
        print(n, "vertices (two passes):", _vertices(a[n]))
        assert _vertices(a[n]) >= 1000, n                              # an empty cloud would compare nothing
        assert len(a[n]) > 1000 * 15
    for n in plys:
        assert b[n] == a[n], n
    pfms = sorted(n for n in a if n.endswith(".pfm"))
    assert len(pfms) == 2 * 2 * N_VIEWS and sorted(n for n in b if n.endswith(".pfm")) == pfms
    for n in pfms:
        assert b[n] == a[n], n
    assert sorted(a) == sorted(b)                                      # and nothing else on either side
    assert b_stats == a_stats and set(b_stats) == {"scan1", "scan2"} and all(len(s) == N_VIEWS for s in b_stats.values())
    assert b_lines == a_lines and len(b_lines) == 2 * N_VIEWS
    return a, b


def test_fuse_from_memory_equals_the_two_passes(data, tmp_path, capsys):
    _compare(data, tmp_path, [], capsys)


@pytest.mark.parametrize("extra", [["--feature_cache", "4"], ["--feature_cache", "12"],
                                   ["--projection", "host_fp32", "--feature_dtype", "fp16"], ["--no_graphs"]],
                         ids=["cache4_evicts", "cache12_whole_scan", "host_fp32_fp16", "no_graphs"])
def test_fuse_from_memory_equals_the_two_passes_with_options(data, tmp_path, capsys, extra):
    _compare(data, tmp_path, extra, capsys)


@pytest.mark.parametrize("extra", [[], ["--feature_cache", "12"]], ids=["plain", "cache12"])
def test_no_pfm_leaves_only_the_point_clouds(data, tmp_path, capsys, extra):
    from_memory(data, tmp_path / "b", extra, capsys)
    from_memory(data, tmp_path / "c", extra + ["--no_pfm"], capsys)
    b, c = _files(tmp_path / "b"), _files(tmp_path / "c")
    assert sorted(c) == ["scan1.ply", "scan2.ply"]                     # no .pfm, no folder content at all
    for n in c:
        assert c[n] == b[n] and _vertices(c[n]) >= 1000, n


def test_save_masks_equal_the_two_passes(data, tmp_path, capsys):
    two_pass(data, tmp_path / "a", ["--save_masks"], capsys)
    from_memory(data, tmp_path / "b", ["--save_masks", "--no_pfm"], capsys)
    a, b = _files(tmp_path / "a", ".png"), _files(tmp_path / "b", ".png")
    assert len(a) == 2 * N_VIEWS * 3 and sorted(a) == sorted(b)
    for n in a:
        assert b[n] == a[n], n
    assert _files(tmp_path / "b", ".ply") == _files(tmp_path / "a", ".ply")
    assert not _files(tmp_path / "b", ".pfm")


def test_no_file_is_touched_twice(data, tmp_path, capsys, monkeypatch):
    """--feature_cache 12 holds a whole scan: every image is opened once, for its decode, and no PFM is read"""
    from PIL import Image
    from itermvs_amd import data_io, fusion
    opened, pfm_reads = [], []
    real_open = Image.open

    def counting_open(fp, *a, **kw):
        opened.append(os.path.realpath(str(fp)))
        return real_open(fp, *a, **kw)

    def counting_read_pfm(filename, *a, **kw):
        pfm_reads.append(filename)
        raise AssertionError(f"read_pfm({filename}) in --fuse_source memory")

    monkeypatch.setattr(Image, "open", counting_open)
    monkeypatch.setattr(data_io, "read_pfm", counting_read_pfm)
    monkeypatch.setattr(fusion, "read_pfm", counting_read_pfm)
    stats, _ = from_memory(data, tmp_path / "b", ["--feature_cache", "12"], capsys)
    monkeypatch.undo()
    assert len(stats) == 2 and not pfm_reads
    want = sorted(os.path.realpath(os.path.join(str(data), f"scan{s}", "images", "{:0>8}.png".format(v)))
                  for s in (1, 2) for v in range(N_VIEWS))
    assert sorted(opened) == want                                      # each of the 12 images exactly once
    assert all(_vertices(p) >= 1000 for p in _files(tmp_path / "b", ".ply").values())


@pytest.mark.parametrize("extra", [[], ["--feature_cache", "6"]], ids=["plain", "cache6"])
def test_a_source_view_that_is_never_a_reference_view_is_refused(tmp_path, capsys, extra):
    write_scans(str(tmp_path / "data"), source_only_view=True)
    with pytest.raises(FileNotFoundError, match=r"scan1.*view 5"):
        from_memory(tmp_path / "data", tmp_path / "b", extra, capsys)
    assert not _files(tmp_path / "b", ".ply")

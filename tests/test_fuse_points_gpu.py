"""itermvs_fuse_points / fusion.fuse_scan on the MI355X: the vertex records against oracle/fusion_oracle.py:unproject_points
bit for bit (no tolerance), several views back to back without a synchronisation, determinism, the capacity predicate, and
the scan-folder driver with ``points="device"`` against ``points="host"``."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import fusion_oracle as FO
from test_fusion import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = np.dtype([("xyz", "<u4", (3,)), ("rgb", "u1", (3,))])           # coordinates as bit patterns
assert RECORD.itemsize == 15


def _expected(avg, mask, k, e, rgb):
    """the records the reference would write for one view: float32(unproject_points) bits, rgb[mask]"""
    with np.errstate(all="ignore"):
        xyz = FO.unproject_points(avg, mask, k, e).astype(np.float32)
    out = np.zeros(int(mask.sum()), RECORD)
    out["xyz"], out["rgb"] = xyz.view(np.uint32).reshape(-1, 3), rgb[mask]
    return out


def _same_records(got, want):
    """bit patterns equal; a NaN equals a NaN whatever its payload"""
    assert got.shape == want.shape
    g, w = got["xyz"].view(np.float32), want["xyz"].view(np.float32)
    same = (got["xyz"] == want["xyz"]) | (np.isnan(g) & np.isnan(w))
    assert same.all(), f"{int((~same).sum())} of {same.size} coordinates differ, first at vertex {int(np.argwhere(~same)[0][0])}"
    assert np.array_equal(got["rgb"], want["rgb"])


def _cam(k, e):
    return torch.from_numpy(np.concatenate([np.linalg.inv(k).reshape(-1), np.linalg.inv(e)[:3].reshape(-1)]).astype(np.float32)).to(DEV)


def _emit(items, capacity=None, guard=0):
    """items: (avg float64 [H,W], final bool [H,W], k, e, rgb uint8 [H,W,3], photo or None, geo or None) emitted back to back
    into one buffer with NO synchronisation in between -> (record bytes below capacity, guard bytes, cursor, view_counts)"""
    from itermvs_amd import ops
    total = sum(int(it[1].sum()) for it in items)
    cap = total if capacity is None else capacity
    buf = torch.full((cap * 15 + guard,), 0xA5, device=DEV, dtype=torch.uint8)
    cursor = torch.zeros(1, device=DEV, dtype=torch.int64)
    counts = torch.full((len(items), 4), -7, device=DEV, dtype=torch.int64)
    u8 = lambda m: None if m is None else torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8)).to(DEV)      # noqa: E731
    dev_items = [(torch.from_numpy(avg).to(DEV), u8(final), _cam(k, e), torch.from_numpy(rgb).to(DEV), u8(photo), u8(geo))
                 for avg, final, k, e, rgb, photo, geo in items]
    torch.cuda.synchronize()
    for i, (avg, final, cam, rgb, photo, geo) in enumerate(dev_items):
        ops.fuse_points(avg, final, cam, rgb, buf, cursor, counts, i, photo, geo, capacity=cap)
    host = buf.cpu().numpy()                                              # the one download
    return host[:cap * 15], host[cap * 15:], int(cursor.item()), counts.cpu().numpy()


def _fused(views, ref, **kw):
    """fuse_reference_view of views[ref] against all the others on the GPU -> numpy (avg, photo, geo, final)"""
    from itermvs_amd import fusion
    k, e, d, conf = views[ref]
    others = [v for i, v in enumerate(views) if i != ref]
    got = fusion.fuse_reference_view(d, conf, k, e, [o[2] for o in others], [o[0] for o in others], [o[1] for o in others],
                                     device=DEV, **kw)
    avg, photo, geo, final = [t.cpu().numpy() for t in got[:4]]
    return avg, photo.astype(bool), geo.astype(bool), final.astype(bool)


@pytest.mark.parametrize("h,w,n_views", [(96, 128, 5), (70, 90, 5), (1, 1, 3), (3, 257, 3), (1152, 1600, 3)])
def test_fuse_points_matches_oracle_bit_for_bit(h, w, n_views):
    views = _scene(h, w, n_views, seed=h % 7, noise=0.002)
    ref = n_views // 2
    k, e = views[ref][0], views[ref][1]
    avg, photo, geo, final = _fused(views, ref, geo_mask_thres=2)
    rng = np.random.default_rng(h + w)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    last = np.zeros((h, w), bool)
    last[-1, -1] = True
    masks = {"final": final, "zeros": np.zeros((h, w), bool), "ones": np.ones((h, w), bool), "last": last,
             "random45": rng.uniform(size=(h, w)) < 0.45}
    if h * w > 1000:
        assert 0.1 < final.mean() < 1.0                                   # the real mask is neither empty nor full
    for name, m in masks.items():
        body, _, cursor, counts = _emit([(avg, m, k, e, rgb, photo, geo)])
        assert cursor == int(m.sum()), name
        assert counts.tolist() == [[int(photo.sum()), int(geo.sum()), int(m.sum()), 0]], name
        _same_records(np.frombuffer(body.tobytes(), RECORD), _expected(avg, m, k, e, rgb))
    # the masks are optional: -1 marks a count that was not asked for
    _, _, _, counts = _emit([(avg, final, k, e, rgb, None, None)])
    assert counts.tolist() == [[-1, -1, int(final.sum()), 0]]


def test_fuse_points_passes_non_finite_depths_through():
    """0, NaN and Inf in the maps with geo_mask_thres = 0: the vertices of those pixels are emitted, as numpy emits them"""
    h, w = 70, 90
    views = _scene(h, w, 5, 2, 0.02)
    views[1][2][10:20, 30:50] = 0.0
    views[2][2][5, 5] = np.nan
    views[2][2][6, 6] = np.inf
    views[2][2][7, 7] = 0.0
    views[2][3][5:8, 5:8] = 0.9                                           # those pixels pass the photometric mask
    k, e = views[2][0], views[2][1]
    avg, photo, geo, final = _fused(views, 2, geo_mask_thres=0)
    assert geo.all() and final[5, 5] and final[6, 6] and final[7, 7]
    rgb = np.random.default_rng(3).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = _expected(avg, final, k, e, rgb)
    assert (~np.isfinite(want["xyz"].view(np.float32))).any()             # the case does hold non-finite vertices
    body, _, cursor, counts = _emit([(avg, final, k, e, rgb, photo, geo)])
    assert cursor == int(final.sum()) and counts[0].tolist() == [int(photo.sum()), h * w, int(final.sum()), 0]
    _same_records(np.frombuffer(body.tobytes(), RECORD), want)


def _five_views(h=96, w=128):
    views = _scene(h, w, 5, 4, 0.003)
    rng = np.random.default_rng(11)
    items = []
    for ref in range(5):
        avg, photo, geo, final = _fused(views, ref)
        items.append((avg, final, views[ref][0], views[ref][1], rng.integers(0, 256, (h, w, 3), dtype=np.uint8), photo, geo))
    return items


def test_five_views_back_to_back_and_deterministic():
    items = _five_views()
    want = np.concatenate([_expected(avg, final, k, e, rgb) for avg, final, k, e, rgb, _, _ in items])
    body, _, cursor, counts = _emit(items)
    assert cursor == len(want) > 5000
    firsts = np.cumsum([0] + [int(it[1].sum()) for it in items])
    assert counts.tolist() == [[int(it[5].sum()), int(it[6].sum()), int(it[1].sum()), int(firsts[i])] for i, it in enumerate(items)]
    _same_records(np.frombuffer(body.tobytes(), RECORD), want)
    again, _, cursor2, counts2 = _emit(items)
    assert cursor2 == cursor and np.array_equal(counts2, counts) and again.tobytes() == body.tobytes()


def test_capacity_is_a_store_predicate_and_totals_stay_true(tmp_path):
    """a bounds test of the predicate ``vertex index < capacity``: the buffer is allocated WITH its guard bytes, nothing is
    written out of range at any point"""
    from itermvs_amd import fusion
    items = _five_views()
    want = np.concatenate([_expected(avg, final, k, e, rgb) for avg, final, k, e, rgb, _, _ in items])
    total = len(want)
    for short in (7, total - 3, total):                                   # the last view cut, almost everything cut, capacity 0
        cap = total - short
        body, guard, cursor, counts = _emit(items, capacity=cap, guard=4096)
        assert len(guard) == 4096 and (guard == 0xA5).all()
        assert cursor == total and counts[:, 2].sum() == total and counts[-1, 3] == total - int(items[-1][1].sum())
        _same_records(np.frombuffer(body.tobytes(), RECORD), want[:cap])
    # fuse_scan with that capacity forced: a clear error instead of a truncated cloud, and no file left behind
    views = _scene(96, 128, 5, 4, 0.003)
    pairs = [(r, [v for v in range(5) if v != r]) for r in range(5)]
    args = (pairs, {v: (views[v][0], views[v][1]) for v in range(5)}, {v: views[v][2] for v in range(5)},
            {v: views[v][3] for v in range(5)}, {i: it[4] for i, it in enumerate(items)})
    with pytest.raises(RuntimeError, match=f"emit {total} vertices, the records buffer holds {total - 7}"):
        fusion.fuse_scan(*args, str(tmp_path / "short.ply"), 1.0, 0.01, 0.3, device=DEV, group_capacity=total - 7)
    assert not (tmp_path / "short.ply").exists()
    info = {}
    stats = fusion.fuse_scan(*args, str(tmp_path / "full.ply"), 1.0, 0.01, 0.3, device=DEV, info=info)
    assert (tmp_path / "full.ply").read_bytes() == fusion.ply_header(total) + want.tobytes()
    assert info["vertices"] == total and info["synchronisations"] == info["downloads"] == len(info["groups"]) == 1
    assert stats[3] == (items[3][6].mean(), items[3][5].mean(), items[3][1].mean())
    # torch tensors on the device are accepted as they are
    on_dev = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()} for d in args[2:]]
    fusion.fuse_scan(args[0], args[1], *on_dev, str(tmp_path / "dev.ply"), 1.0, 0.01, 0.3, device=DEV)
    assert (tmp_path / "dev.ply").read_bytes() == (tmp_path / "full.ply").read_bytes()


def _scan_folder(root, orig_scale, h=64, w=96):
    """the synthetic scan folder of tests/test_fusion.py:test_filter_depth_scene_folder -> (scan folder, output folder)"""
    from PIL import Image
    from itermvs_amd.data_io import save_pfm
    views = _scene(h, w, 5, 5, 0.001)
    scan, out = root / "data" / "scan1", root / "outputs" / "scan1"
    (scan / "cams_1").mkdir(parents=True)
    (scan / "images").mkdir(parents=True)
    (out / "depth_est").mkdir(parents=True)
    (out / "confidence").mkdir(parents=True)
    lines = ["5"]
    for v, (k, e, d, conf) in enumerate(views):
        rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)      # noqa: E731
        k_disk = k.copy()
        k_disk[:2] *= orig_scale
        (scan / "cams_1" / "{:0>8}_cam.txt".format(v)).write_text(f"extrinsic\n{rows(e)}\n\nintrinsic\n{rows(k_disk)}\n\n425 2.5\n")
        img = np.zeros((int(h * orig_scale), int(w * orig_scale), 3), np.uint8)
        img[..., 0], img[..., 1], img[..., 2] = 10 + 40 * v, 200, 7
        Image.fromarray(img).save(str(scan / "images" / "{:0>8}.jpg".format(v)), quality=100)
        save_pfm(str(out / "depth_est" / "{:0>8}.pfm".format(v)), d)
        save_pfm(str(out / "confidence" / "{:0>8}.pfm".format(v)), np.full_like(conf, 0.9))
        srcs = [u for u in range(5) if u != v]
        lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} 1.0" for u in srcs)]
    (scan / "pair.txt").write_text("\n".join(lines) + "\n")
    return scan, out


def _read_ply(path):
    head, body = path.read_bytes().split(b"end_header\n", 1)
    return head, np.frombuffer(body, RECORD)


def _ulp_distance(a_bits, b_bits):
    """distance in float32 units in the last place between two arrays of finite float32 bit patterns"""
    key = lambda u: np.where(u >> 31 == 1, np.int64(0x80000000) - u.astype(np.int64), u.astype(np.int64))      # noqa: E731
    return np.abs(key(a_bits) - key(b_bits))


@pytest.mark.parametrize("orig_scale", [1.0, 2.0])
def test_filter_depth_device_against_host(tmp_path, orig_scale):
    """np.matmul (BLAS, free to fuse or reorder) against the oracle's fixed order: the float64 coordinates differ in the last
    bit, and a float32 result may then flip by one unit in the last place.  Bound: at most 1 float32 ulp per coordinate, and at
    most 1e-4 of the coordinates differ at all (the numpy host path against FO.unproject_points is at 0 on these inputs)."""
    from PIL import Image
    from itermvs_amd import fusion
    h, w = 64, 96
    scan, out = _scan_folder(tmp_path, orig_scale, h, w)
    run = lambda name, **kw: fusion.filter_depth(str(scan), str(out), str(tmp_path / name), 1.0, 0.01, 0.3, device=DEV,      # noqa: E731
                                                 img_wh=(w, h), **kw)
    st_host = run("host.ply")
    st_host2 = run("host_kw.ply", points="host", save_masks=False)
    assert st_host2 == st_host and (tmp_path / "host_kw.ply").read_bytes() == (tmp_path / "host.ply").read_bytes()
    assert not (out / "mask").exists()
    info = {}
    st_dev = run("device.ply", points="device", save_masks=True, info=info)
    assert info["synchronisations"] == info["downloads"] == len(info["groups"]) == 1 and info["groups"] == [(0, 5)]
    head_h, pts_h = _read_ply(tmp_path / "host.ply")
    head_d, pts_d = _read_ply(tmp_path / "device.ply")
    assert head_d == head_h and len(pts_d) == len(pts_h) == info["vertices"] > 1000
    assert np.array_equal(pts_d["rgb"], pts_h["rgb"])
    assert np.isfinite(pts_h["xyz"].view(np.float32)).all() and np.isfinite(pts_d["xyz"].view(np.float32)).all()
    ulp = _ulp_distance(pts_d["xyz"], pts_h["xyz"])
    share = float((ulp != 0).mean())
    print(f"orig_scale {orig_scale}: {int((ulp != 0).sum())} of {ulp.size} float32 coordinates differ (share {share:.3e}), max {int(ulp.max())} ulp")
    assert ulp.max() <= 1 and share <= 1e-4
    assert list(st_dev) == list(st_host)
    for v in st_host:
        assert np.abs(np.array(st_dev[v]) - np.array(st_host[v])).max() <= 1e-6, v
    # the reference's mask images, equal to what fuse_reference_view returns for the rescaled cameras
    cams = {}
    for v in range(5):
        k, e = fusion.read_camera_parameters(str(scan / "cams_1" / "{:0>8}_cam.txt".format(v)))
        k = k.copy()
        k[0] *= 1.0 / orig_scale
        k[1] *= 1.0 / orig_scale
        cams[v] = (k, e)
    from itermvs_amd.data_io import read_pfm
    depth = {v: np.squeeze(read_pfm(str(out / "depth_est" / "{:0>8}.pfm".format(v)))[0]) for v in range(5)}
    for v in range(5):
        srcs = [u for u in range(5) if u != v]
        conf = np.squeeze(read_pfm(str(out / "confidence" / "{:0>8}.pfm".format(v)))[0])
        _, photo, geo, final, _ = fusion.fuse_reference_view(depth[v], conf, *cams[v], [depth[u] for u in srcs],
                                                             [cams[u][0] for u in srcs], [cams[u][1] for u in srcs], device=DEV)
        for name, m in (("photo", photo), ("geo", geo), ("final", final)):
            with Image.open(str(out / "mask" / "{:0>8}_{}.png".format(v, name))) as im:
                assert im.mode == "L"
                assert np.array_equal(np.array(im), m.cpu().numpy() * 255), (v, name)
        assert abs(st_dev[v][2] - float(final.float().mean())) <= 1e-6
    # one reference view per flush group: five synchronisations and downloads, the same file
    info1 = {}
    st_one = run("device_1.ply", points="device", records_budget=h * w * 15, info=info1)
    assert info1["groups"] == [(i, i + 1) for i in range(5)] and info1["synchronisations"] == info1["downloads"] == 5
    assert st_one == st_dev and (tmp_path / "device_1.ply").read_bytes() == (tmp_path / "device.ply").read_bytes()
    with pytest.raises(ValueError, match="below one"):
        run("never.ply", points="device", records_budget=h * w * 15 - 1)
    # the host path writes the same masks and, with them, the same cloud
    import shutil
    shutil.move(str(out / "mask"), str(out / "mask_device"))
    assert run("host_masks.ply", save_masks=True) == st_host
    assert (tmp_path / "host_masks.ply").read_bytes() == (tmp_path / "host.ply").read_bytes()
    for f in sorted(os.listdir(str(out / "mask_device"))):
        assert (out / "mask" / f).read_bytes() == (out / "mask_device" / f).read_bytes(), f
    assert len(os.listdir(str(out / "mask"))) == 15
    # images handed over as float arrays (the ``images=`` form): converted on the host with the reference's expression
    imgs = {v: np.full((h, w, 3), (10 + 40 * v) / 255.0, np.float32) for v in range(5)}
    sc = (1.0 / orig_scale, 1.0 / orig_scale)
    a = fusion.filter_depth(str(scan), str(out), str(tmp_path / "img_h.ply"), 1.0, 0.01, 0.3, images=imgs, intrinsics_scale=sc, device=DEV)
    b = fusion.filter_depth(str(scan), str(out), str(tmp_path / "img_d.ply"), 1.0, 0.01, 0.3, images=imgs, intrinsics_scale=sc, device=DEV,
                            points="device")
    assert list(a) == list(b)
    assert np.array_equal(_read_ply(tmp_path / "img_h.ply")[1]["rgb"], _read_ply(tmp_path / "img_d.ply")[1]["rgb"])


def test_eval_driver_fuses_on_the_device(tmp_path):
    """eval.py --dataset folder --filter --fuse_points device --save_masks: the filter stage of the driver on a scan folder
    whose depth maps are already there writes the PLY of the library call"""
    sys.path.insert(0, ROOT)
    import eval as E
    from itermvs_amd import fusion
    h, w = 64, 96
    scan, out = _scan_folder(tmp_path, 2.0, h, w)
    args = E.build_parser().parse_args(["--dataset", "folder", "--testpath", str(tmp_path / "data"), "--outdir", str(tmp_path / "outputs"),
                                        "--img_wh", str(w), str(h), "--filter", "--fuse_points", "device", "--save_masks"])
    assert E.fuse_scans(args) == 1
    fusion.filter_depth(str(scan), str(out), str(tmp_path / "lib.ply"), args.geo_pixel_thres, args.geo_depth_thres, args.photo_thres,
                        device=DEV, img_wh=(w, h), points="device")
    assert (tmp_path / "outputs" / "scan1.ply").read_bytes() == (tmp_path / "lib.ply").read_bytes()
    assert len(os.listdir(str(out / "mask"))) == 15
    # and without the new flags the driver takes the host path, as before
    args = E.build_parser().parse_args(["--dataset", "folder", "--testpath", str(tmp_path / "data"), "--outdir", str(tmp_path / "outputs"),
                                        "--img_wh", str(w), str(h), "--filter"])
    assert E.fuse_scans(args) == 1
    fusion.filter_depth(str(scan), str(out), str(tmp_path / "lib_host.ply"), 1.0, 0.01, 0.3, device=DEV, img_wh=(w, h))
    assert (tmp_path / "outputs" / "scan1.ply").read_bytes() == (tmp_path / "lib_host.ply").read_bytes()

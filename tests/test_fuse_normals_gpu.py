"""itermvs_fuse_points_normals / fusion.fuse_scan(normals=True) / eval.py --ply_normals on the MI355X: the 27-byte records against
oracle/fusion_oracle.py:unproject_points and tests/fuse_normals_reference.py bit for bit (no tolerance), views back to back
without a synchronisation, the capacity predicate, determinism, and the PLY with the normals taken out again against the PLY
written without them, byte for byte."""
import os
import sys

import numpy as np
import pytest
import torch

import fuse_normals_reference as NR
from conftest import ROOT
from oracle import fusion_oracle as FO
from test_fusion import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
REC = 27
RECORD = np.dtype([("xyz", "<u4", (3,)), ("nrm", "<u4", (3,)), ("rgb", "u1", (3,))])       # floats as bit patterns
assert RECORD.itemsize == REC
NORMAL_LINES = b"property float nx\nproperty float ny\nproperty float nz\n"


def _expected(avg, mask, k, e, rgb, edge=0.01):
    """the records of one view: float32(unproject_points) bits, the reference normal bits, rgb[mask]"""
    with np.errstate(all="ignore"):
        xyz = FO.unproject_points(avg, mask, k, e).astype(np.float32)
    out = np.zeros(int(mask.sum()), RECORD)
    out["xyz"], out["rgb"] = xyz.view(np.uint32).reshape(-1, 3), rgb[mask]
    out["nrm"] = NR.normals(avg, mask, k, e, edge).view(np.uint32).reshape(-1, 3)
    return out


def _same_records(got, want):
    """bit patterns equal; a NaN coordinate equals a NaN whatever its payload; a normal is never NaN"""
    assert got.shape == want.shape
    g, w = got["xyz"].view(np.float32), want["xyz"].view(np.float32)
    same = (got["xyz"] == want["xyz"]) | (np.isnan(g) & np.isnan(w))
    assert same.all(), f"{int((~same).sum())} of {same.size} coordinates differ, first at vertex {int(np.argwhere(~same)[0][0])}"
    same = got["nrm"] == want["nrm"]
    assert same.all(), (f"{int((~same).sum())} of {same.size} normal components differ, first at vertex "
                        f"{int(np.argwhere(~same)[0][0])}: {got['nrm'][~same][:3]} for {want['nrm'][~same][:3]}")
    assert np.array_equal(got["rgb"], want["rgb"])


def _cam(k, e):
    return torch.from_numpy(np.concatenate([np.linalg.inv(k).reshape(-1), np.linalg.inv(e)[:3].reshape(-1)]).astype(np.float32)).to(DEV)


def _emit(items, capacity=None, guard=0, edge=0.01):
    """items: (avg float64 [H,W], final bool [H,W], k, e, rgb uint8 [H,W,3], photo or None, geo or None) emitted back to back
    into one buffer with NO synchronisation in between -> (record bytes below capacity, guard bytes, cursor, view_counts)"""
    from itermvs_amd import ops
    total = sum(int(it[1].sum()) for it in items)
    cap = total if capacity is None else capacity
    buf = torch.full((cap * REC + guard,), 0xA5, device=DEV, dtype=torch.uint8)
    cursor = torch.zeros(1, device=DEV, dtype=torch.int64)
    counts = torch.full((len(items), 4), -7, device=DEV, dtype=torch.int64)
    u8 = lambda m: None if m is None else torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8)).to(DEV)      # noqa: E731
    dev_items = [(torch.from_numpy(avg).to(DEV), u8(final), _cam(k, e), torch.from_numpy(rgb).to(DEV), u8(photo), u8(geo))
                 for avg, final, k, e, rgb, photo, geo in items]
    torch.cuda.synchronize()
    for i, (avg, final, cam, rgb, photo, geo) in enumerate(dev_items):
        ops.fuse_points_normals(avg, final, cam, rgb, buf, cursor, counts, i, photo, geo, capacity=cap, edge_thres=edge)
    host = buf.cpu().numpy()                                              # the one download
    return host[:cap * REC], host[cap * REC:], int(cursor.item()), counts.cpu().numpy()


def _fused(views, ref, **kw):
    """fuse_reference_view of views[ref] against all the others on the GPU -> numpy (avg, photo, geo, final)"""
    from itermvs_amd import fusion
    k, e, d, conf = views[ref]
    others = [v for i, v in enumerate(views) if i != ref]
    got = fusion.fuse_reference_view(d, conf, k, e, [o[2] for o in others], [o[0] for o in others], [o[1] for o in others],
                                     device=DEV, **kw)
    avg, photo, geo, final = [t.cpu().numpy() for t in got[:4]]
    return avg, photo.astype(bool), geo.astype(bool), final.astype(bool)


# noise 0.008: neighbouring depths differ by about 1 % of the depth, so with edge_thres 0.01 central, one-sided and missing
# tangents all occur (about 84 % of the reference's normals are non-zero at 70 x 90 and 96 x 128, 62 % at 3 x 257)
@pytest.mark.parametrize("h,w,n_views", [(1, 1, 3), (1, 5, 3), (5, 1, 3), (3, 257, 3), (70, 90, 5), (96, 128, 5)])
def test_records_match_the_references_bit_for_bit(h, w, n_views):
    views = _scene(h, w, n_views, seed=h % 7, noise=0.008)
    ref = n_views // 2
    k, e = views[ref][0], views[ref][1]
    avg, photo, geo, final = _fused(views, ref, geo_mask_thres=2)
    rng = np.random.default_rng(h + w)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    last = np.zeros((h, w), bool)
    last[-1, -1] = True
    masks = {"final": final, "ones": np.ones((h, w), bool), "zeros": np.zeros((h, w), bool), "last": last,
             "random45": rng.uniform(size=(h, w)) < 0.45}
    if h * w > 1000:
        assert 0.1 < final.mean() < 1.0                                   # the real mask is neither empty nor full
    for name, m in masks.items():
        want = _expected(avg, m, k, e, rgb)
        body, _, cursor, counts = _emit([(avg, m, k, e, rgb, photo, geo)])
        assert cursor == int(m.sum()), name
        assert counts.tolist() == [[int(photo.sum()), int(geo.sum()), int(m.sum()), 0]], name
        _same_records(np.frombuffer(body.tobytes(), RECORD), want)
        if h * w > 1000 and name in ("final", "ones", "random45"):
            share = float((want["nrm"] != 0).any(axis=1).mean())
            print(f"{h}x{w} {name}: {share:.3f} of {len(want)} normals are non-zero")
            assert 0.5 < share < 1.0, name                                # neither zeros against zeros nor one branch only
        if min(h, w) == 1:
            assert not want["nrm"].any(), name                            # one tangent is missing in a single row or column


def test_non_finite_depths_get_zero_normals_and_their_neighbours_the_references():
    """the 70x90 scene of test_fuse_points_passes_non_finite_depths_through: 0, NaN and Inf in the maps with geo_mask_thres = 0"""
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
    # edge_thres 0.05: at this noise (2 % per map) the default would leave most pixels without a usable neighbour
    want = _expected(avg, final, k, e, rgb, edge=0.05)
    assert (~np.isfinite(want["xyz"].view(np.float32))).any()             # the case does hold non-finite vertices
    body, _, cursor, counts = _emit([(avg, final, k, e, rgb, photo, geo)], edge=0.05)
    assert cursor == int(final.sum()) and counts[0].tolist() == [int(photo.sum()), h * w, int(final.sum()), 0]
    got = np.frombuffer(body.tobytes(), RECORD)
    _same_records(got, want)
    vertex = np.cumsum(final.ravel()) - 1                                 # pixel -> vertex index
    for y, x in ((5, 5), (6, 6), (7, 7)):
        assert not (np.isfinite(avg[y, x]) and avg[y, x] > 0), (y, x, avg[y, x])
        assert got["nrm"][vertex[y * w + x]].tolist() == [0, 0, 0], (y, x)
    near = [vertex[y * w + x] for y in range(4, 9) for x in range(4, 9) if final[y, x] and (y, x) not in ((5, 5), (6, 6), (7, 7))]
    assert len(near) >= 4 and (got["nrm"][near] != 0).any(axis=1).sum() >= len(near) // 2      # finite neighbours keep theirs


def _three_views(h=70, w=90):
    views = _scene(h, w, 3, 4, 0.008)
    rng = np.random.default_rng(11)
    items = []
    for ref in range(3):
        avg, photo, geo, final = _fused(views, ref, geo_mask_thres=1)
        items.append((avg, final, views[ref][0], views[ref][1], rng.integers(0, 256, (h, w, 3), dtype=np.uint8), photo, geo))
    return items


def test_three_views_back_to_back_capacity_and_determinism():
    """the capacity predicate ``vertex index < capacity``: the buffer is allocated WITH its guard bytes, nothing is written out
    of range at any point"""
    items = _three_views()
    want = np.concatenate([_expected(avg, final, k, e, rgb) for avg, final, k, e, rgb, _, _ in items])
    total = len(want)
    body, _, cursor, counts = _emit(items)
    assert cursor == total > 3000
    firsts = np.cumsum([0] + [int(it[1].sum()) for it in items])
    assert counts.tolist() == [[int(it[5].sum()), int(it[6].sum()), int(it[1].sum()), int(firsts[i])] for i, it in enumerate(items)]
    _same_records(np.frombuffer(body.tobytes(), RECORD), want)
    again, _, cursor2, counts2 = _emit(items)
    assert cursor2 == cursor and np.array_equal(counts2, counts) and again.tobytes() == body.tobytes()
    cap = total - 7
    short, guard, cursor3, counts3 = _emit(items, capacity=cap, guard=4096)
    assert len(guard) == 4096 and (guard == 0xA5).all()
    assert cursor3 == total and np.array_equal(counts3, counts)           # the true totals all the same
    assert short.tobytes() == body.tobytes()[:cap * REC]


# -- fuse_scan --------------------------------------------------------------------------------------------------------------
def _strip_normals(ply: bytes) -> bytes:
    """the PLY without the three header lines and without bytes 12..23 of every record"""
    head, body = ply.split(b"end_header\n", 1)
    assert head.count(NORMAL_LINES) == 1 and len(body) % REC == 0
    rec = np.frombuffer(body, np.uint8).reshape(-1, REC)
    return head.replace(NORMAL_LINES, b"") + b"end_header\n" + np.delete(rec, np.s_[12:24], axis=1).tobytes()


@pytest.fixture(scope="module")
def scan_plys(tmp_path_factory):
    """fuse_scan of one 70x90, 5-view scan with normals x dedupe -> {(normals, dedupe): (PLY bytes, info, path)}"""
    from itermvs_amd import fusion
    h, w = 70, 90
    root = tmp_path_factory.mktemp("normals_scan")
    views = _scene(h, w, 5, 4, 0.004)
    rng = np.random.default_rng(5)
    pairs = [(r, [v for v in range(5) if v != r]) for r in range(5)]
    args = (pairs, {v: (views[v][0], views[v][1]) for v in range(5)}, {v: views[v][2] for v in range(5)},
            {v: views[v][3] for v in range(5)}, {v: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for v in range(5)})
    out = {}
    for normals in (False, True):
        for dedupe in (False, True):
            info = {}
            path = root / f"n{int(normals)}_d{int(dedupe)}.ply"
            fusion.fuse_scan(*args, str(path), 1.0, 0.01, 0.3, geo_mask_thres=2, device=DEV, records_budget=3 * h * w * REC,
                             info=info, dedupe=dedupe, normals=normals)
            out[normals, dedupe] = (path.read_bytes(), info, str(path))
    return out


@pytest.mark.parametrize("dedupe", [False, True], ids=["plain", "dedupe"])
def test_normals_only_add(scan_plys, dedupe):
    from itermvs_amd import fusion
    with_n, info_n, _ = scan_plys[True, dedupe]
    without, info, _ = scan_plys[False, dedupe]
    assert info_n["normals"] is True and info_n["record_bytes"] == REC and info_n["groups"] == [(0, 3), (3, 5)]      # two flushes
    assert info["normals"] is False and info["record_bytes"] == 15 and info["dedupe"] is info_n["dedupe"] is dedupe
    assert info_n["vertices"] == info["vertices"] > 5000
    assert with_n.startswith(fusion.ply_header(info_n["vertices"], normals=True))
    assert len(with_n) == len(fusion.ply_header(info_n["vertices"], normals=True)) + REC * info_n["vertices"]
    assert _strip_normals(with_n) == without
    nrm = np.frombuffer(with_n.split(b"end_header\n", 1)[1], RECORD)["nrm"].view(np.float32).astype(np.float64)
    lengths = np.linalg.norm(nrm, axis=1)
    assert ((lengths == 0) | (np.abs(lengths - 1) <= 1e-6)).all() and (lengths > 0).mean() > 0.5
    if dedupe:
        assert info["vertices"] < scan_plys[False, False][1]["vertices"]


def test_other_readers_see_the_same_points(scan_plys):
    from itermvs_amd import data_io
    a, b = data_io.read_ply_xyz(scan_plys[True, False][2]), data_io.read_ply_xyz(scan_plys[False, False][2])
    assert a.dtype == b.dtype and a.shape == b.shape and a.shape[0] > 5000
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# -- the driver -------------------------------------------------------------------------------------------------------------
N_VIEWS = 6
IMG_WH = (96, 64)                  # inference size; the files are 100 x 75, so colours and intrinsics rescale on both axes
LOOSE = ["--photo_thres", "0", "--geo_pixel_thres", "1e6", "--geo_depth_thres", "1e6", "--geo_mask_thres", "1"]


def write_scan(root):
    """one scan of six views stored at 75 x 100, every view a reference view with four source views (the folder of
    tests/test_fuse_memory_gpu.py:write_scans, one scan of it)"""
    from PIL import Image
    from itermvs_amd import synthetic
    w, h = IMG_WH
    s = synthetic.make_scene_sample(num_views=N_VIEWS, height=h, width=w, seed=40)
    k0, exts = synthetic.camera_parameters(N_VIEWS, h, w, ref_shift=0)
    k = np.array(k0, dtype=np.float64)
    k[0] *= 100 / w                                           # the intrinsics of the 100 x 75 file
    k[1] *= 75 / h
    scan = os.path.join(root, "scan1")
    os.makedirs(os.path.join(scan, "cams_1"))
    os.makedirs(os.path.join(scan, "images"))
    for v in range(N_VIEWS):
        img = ((s["imgs"]["level_0"][0, v].permute(1, 2, 0).numpy() + 1) * 127.5).round().clip(0, 255).astype(np.uint8)
        Image.fromarray(img).resize((100, 75), Image.BICUBIC).save(os.path.join(scan, "images", "{:0>8}.png".format(v)))
        rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)      # noqa: E731
        with open(os.path.join(scan, "cams_1", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write(f"extrinsic\n{rows(np.array(exts[v], dtype=np.float64))}\n\nintrinsic\n{rows(k)}\n\n425.0 2.5 192 935.0\n")
    lines = [str(N_VIEWS)]
    for v in range(N_VIEWS):
        srcs = [(v + 1) % N_VIEWS, (v + 5) % N_VIEWS, (v + 2) % N_VIEWS, (v + 3) % N_VIEWS]
        lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} 1.0" for u in srcs)]
    with open(os.path.join(scan, "pair.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_eval_driver_writes_the_nine_property_ply(tmp_path):
    """eval.py --dataset folder --filter --fuse_source memory --ply_normals, in this process like tests/test_fuse_memory_gpu.py"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    data = tmp_path / "data"
    write_scan(str(data))
    plys = {}
    for name, extra in (("plain", []), ("normals", ["--ply_normals", "--normal_edge_thres", "0.05"])):
        args = E.build_parser().parse_args(
            ["--dataset", "folder", "--testpath", str(data), "--n_views", "4", "--img_wh", str(IMG_WH[0]), str(IMG_WH[1]),
             "--iteration", "2", "--outdir", str(tmp_path / name), "--filter", "--fuse_source", "memory", "--no_pfm"] + LOOSE + extra)
        assert E.check_ply_normals(args) is bool(extra)
        stats = E.fuse_memory(args)
        assert set(stats) == {"scan1"} and len(stats["scan1"]) == N_VIEWS
        plys[name] = (tmp_path / name / "scan1.ply").read_bytes()
    head = plys["normals"].split(b"end_header\n", 1)[0].decode("ascii").splitlines()
    assert [line.split()[-1] for line in head if line.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    n = int([line for line in head if line.startswith("element vertex")][0].split()[-1])
    assert n >= 1000 and len(plys["normals"]) - len(plys["plain"]) == 12 * n + len(NORMAL_LINES)
    assert _strip_normals(plys["normals"]) == plys["plain"]
    nrm = np.frombuffer(plys["normals"].split(b"end_header\n", 1)[1], RECORD)["nrm"].view(np.float32)
    assert np.isfinite(nrm).all() and (nrm != 0).any(axis=1).any()

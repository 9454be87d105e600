"""itermvs_fuse_depth_claim / fusion.fuse_scan(dedupe=True) / eval.py --fuse_dedupe on the MI355X: the kernel against
tests/fuse_claim_reference.py bit for bit (outputs and every claim map), its unchanged outputs against ops.fuse_depth, non-finite
depths with guard words around the claim maps, determinism, whole scans over several flush groups, and the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fuse_claim_reference as R
from conftest import ROOT
from test_fuse_claim_cpu import _scan
from test_fusion import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
THRES = dict(geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=2)
GUARD = 64                                             # guard bytes before, between and after the claim maps
CASES = [(96, 128, 4), (37, 45, 1), (40, 64, 16)]      # the last two: ragged in both dimensions of the 32 x 8 tile; S = 1 and 16


def _case(h, w, s, seed):
    """reference view in the middle of s + 1 views, noisy enough that pairs fail; claimed_ref from a seeded random mask, the
    source maps partly pre-filled.  -> (numpy arguments of R.fuse_view_claim, claimed_ref, claimed_src)"""
    from itermvs_amd import fusion
    views = _scene(h, w, s + 1, seed, 0.004)
    ref = (s + 1) // 2
    k, e, d, conf = views[ref]
    others = [v for i, v in enumerate(views) if i != ref]
    rng = np.random.default_rng(100 + seed)
    claimed_ref = (rng.uniform(size=(h, w)) < 0.3).astype(np.uint8)
    claimed_src = [(rng.uniform(size=(h, w)) < 0.1).astype(np.uint8) for _ in others]
    args = (d, conf, k, e, [o[2] for o in others], [o[0] for o in others], [o[1] for o in others])
    mats = np.stack([fusion.pair_matrices(k, e, o[0], o[1]) for o in others])
    return args, mats, claimed_ref, claimed_src


def _guarded(maps):
    """the maps inside ONE allocation with guard bytes before and after each -> (whole buffer, [H,W] views into it)"""
    h, w = maps[0].shape
    stride = GUARD + h * w
    buf = torch.full((len(maps) * stride + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    views = []
    for i, m in enumerate(maps):
        v = buf[i * stride + GUARD:(i + 1) * stride].view(h, w)
        v.copy_(torch.from_numpy(m))
        views.append(v)
    return buf, views


def _guards_intact(buf, n, hw):
    host = buf.cpu().numpy()
    stride = GUARD + hw
    return all((host[i * stride:i * stride + GUARD] == 0xA5).all() for i in range(n + 1))


def _run(args, mats, claimed_ref, claimed_src, thres=THRES):
    """-> (numpy outputs of ops.fuse_depth_claim, claim maps after the call, guards intact, inputs unchanged)"""
    from itermvs_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                # noqa: E731
    d, conf, srcs, m = t(args[0]), t(args[1]), [t(x) for x in args[4]], t(mats)
    maps = ([] if claimed_ref is None else [claimed_ref]) + list(claimed_src or [])
    buf, views = _guarded(maps) if maps else (None, [])
    c_ref = None if claimed_ref is None else views[0]
    c_src = None if claimed_src is None else views[len(views) - len(claimed_src):]
    got = ops.fuse_depth_claim(d, conf, srcs, m, c_ref, c_src, **thres)
    torch.cuda.synchronize()
    same_inputs = (np.array_equal(d.cpu().numpy(), args[0], equal_nan=True) and np.array_equal(conf.cpu().numpy(), args[1])
                   and all(np.array_equal(x.cpu().numpy(), y, equal_nan=True) for x, y in zip(srcs, args[4])))
    return ([x.cpu().numpy() for x in got], [v.cpu().numpy() for v in views],
            buf is None or _guards_intact(buf, len(maps), args[0].size), same_inputs)


def _same(got, want):
    """outputs of the kernel against the reference's: integer work exact, the float64 average bit for bit where finite"""
    avg, photo, geo, final, cnt = got
    assert np.array_equal(cnt, want[4]) and cnt.dtype == np.int32
    assert np.array_equal(photo.astype(bool), want[1]) and np.array_equal(geo.astype(bool), want[2])
    assert np.array_equal(final.astype(bool), want[3])
    assert set(np.unique(final)) <= {0, 1}
    both = np.isfinite(want[0])
    assert np.array_equal(np.isfinite(avg), both) and np.array_equal(avg[both], want[0][both])


@pytest.mark.parametrize("h,w,s", CASES)
def test_claim_kernel_matches_the_reference_bit_for_bit(h, w, s):
    from itermvs_amd import ops
    args, mats, claimed_ref, claimed_src = _case(h, w, s, seed=s)
    thres = dict(THRES, geo_mask_thres=min(2, s))                                 # one source view cannot agree twice
    want, want_maps, claims = R.fuse_view_claim(*args, claimed_ref, claimed_src, **thres)
    got, maps, guards, same_inputs = _run(args, mats, claimed_ref, claimed_src, thres)
    assert guards and same_inputs
    _same(got, want)
    assert np.array_equal(maps[0], claimed_ref)                                   # the reference view's own map is only read
    for i, (m, wm, before) in enumerate(zip(maps[1:], want_maps, claimed_src)):
        assert np.array_equal(m, wm), (i, int((m != wm).sum()))
        assert (m[before == 1] == 1).all()                                        # earlier marks survive
    new = sum(int(wm.sum()) - int(b.sum()) for wm, b in zip(want_maps, claimed_src))
    failed = int((want[4] < s).sum())
    print(f"{h}x{w} S={s}: {int(want[3].sum())} emit, {new} new marks, {failed} pixels with a failed pair")
    assert want[3].sum() > 0 and new > 0 and failed > 0 and (want[1] & want[2] & ~want[3]).any()
    # the outputs the claim maps do not touch equal ops.fuse_depth's byte for byte
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                # noqa: E731
    plain = [x.cpu().numpy() for x in ops.fuse_depth(t(args[0]), t(args[1]), [t(x) for x in args[4]], t(mats), **thres)]
    for i in (0, 1, 2, 4):
        assert got[i].tobytes() == plain[i].tobytes(), i
    assert np.array_equal(got[3], plain[3] & (claimed_ref == 0))
    # nothing claimed and nothing to claim: the whole tuple is ops.fuse_depth's
    for c_ref, c_src in ((np.zeros((h, w), np.uint8), None), (None, None)):
        bare, _, guards, _ = _run(args, mats, c_ref, c_src, thres)
        assert guards and all(a.tobytes() == b.tobytes() for a, b in zip(bare, plain))
    # claimed_ref = None with maps to mark: final is the plain one, the marks are the reference's
    want0, want_maps0, _ = R.fuse_view_claim(*args, None, claimed_src, **thres)
    got0, maps0, guards, _ = _run(args, mats, None, claimed_src, thres)
    assert guards and got0[3].tobytes() == plain[3].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(maps0, want_maps0))


def test_non_finite_depths_equal_the_reference_and_touch_nothing_else():
    h, w, s = 70, 90, 4
    args, mats, claimed_ref, claimed_src = _case(h, w, s, seed=2)
    d, srcs = args[0], args[4]
    srcs[1][10:20, 30:50] = 0.0
    srcs[0][40, 40:60], srcs[2][41, 40:60], srcs[3][42:44, 40:60] = np.nan, np.inf, -np.inf
    d[5, 5], d[6, 6], d[7, 7], d[8, 8] = np.nan, np.inf, 0.0, -np.inf
    d[30:34, 10:30] = 0.0
    args[1][5:9, 5:9] = 0.9                                                       # those pixels pass the photometric mask
    claimed_ref[5:9, 5:9] = 0
    for thres in (THRES, dict(THRES, geo_mask_thres=0), dict(THRES, geo_pixel_thres=np.inf, geo_depth_thres=np.inf)):
        with np.errstate(all="ignore"):
            want, want_maps, _ = R.fuse_view_claim(*args, claimed_ref, claimed_src, **thres)
        got, maps, guards, same_inputs = _run(args, mats, claimed_ref, claimed_src, thres)
        assert guards and same_inputs
        _same(got, want)
        assert np.array_equal(maps[0], claimed_ref)
        for i, (m, wm) in enumerate(zip(maps[1:], want_maps)):
            assert np.array_equal(m, wm), (thres, i, int((m != wm).sum()))
        if thres["geo_mask_thres"] == 0:                                          # there the non-finite pixels do emit
            assert want[3][5, 5] and want[3][6, 6] and want[3][7, 7] and want[3][8, 8]


def _device_scan(scan_args, thres, rounds=1):
    """the scan through ops.fuse_depth_claim + ops.fuse_points, views back to back -> [(record bytes, claim maps)] per round"""
    from itermvs_amd import fusion, ops
    pairs, cams, depths, confs, images = scan_args
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)        # noqa: E731
    h, w = depths[0].shape
    dep = {v: t(d, torch.float32) for v, d in depths.items()}
    out = []
    for _ in range(rounds):
        claimed = {v: torch.zeros((h, w), device=DEV, dtype=torch.uint8) for v in dep}
        records = torch.full((len(pairs) * h * w * 15,), 0xA5, device=DEV, dtype=torch.uint8)
        cursor = torch.zeros(1, device=DEV, dtype=torch.int64)
        counts = torch.zeros((len(pairs), 4), device=DEV, dtype=torch.int64)
        for i, (ref, srcs) in enumerate(pairs):
            k, e = cams[ref]
            mats = t(np.stack([fusion.pair_matrices(k, e, *cams[v]) for v in srcs]), torch.float32)
            cam = t(np.concatenate([np.linalg.inv(k).reshape(-1), np.linalg.inv(e)[:3].reshape(-1)]), torch.float32)
            avg, photo, geo, final, _ = ops.fuse_depth_claim(dep[ref], t(confs[ref], torch.float32), [dep[v] for v in srcs], mats,
                                                             claimed[ref], [claimed[v] for v in srcs], **thres)
            ops.fuse_points(avg, final, cam, t(images[ref], torch.uint8), records, cursor, counts, i, photo, geo)
        n = int(cursor.item())
        out.append((records[:n * 15].cpu().numpy().tobytes(), {v: c.cpu().numpy() for v, c in claimed.items()}))
    return out


@pytest.fixture(scope="module")
def scan():
    args = _scan(_scene(96, 128, 5, 4, 0.003))
    return args, R.fuse_scan_claim(*args, **THRES), R.fuse_scan_claim(*args, **THRES, dedupe=False)


def test_scan_is_deterministic_and_equals_the_reference(scan):
    args, (ply, _, _, claimed), _ = scan
    (rec_a, maps_a), (rec_b, maps_b) = _device_scan(args, THRES, rounds=2)
    assert rec_a == rec_b and all(maps_a[v].tobytes() == maps_b[v].tobytes() for v in maps_a)
    assert R.ply_header(len(rec_a) // 15) + rec_a == ply
    assert all(np.array_equal(maps_a[v], claimed[v]) for v in claimed)


def test_fuse_scan_dedupe_over_several_groups(scan, tmp_path):
    from itermvs_amd import fusion
    args, (ply, claimer, _, _), (ply_plain, _, _, _) = scan
    h, w = args[2][0].shape
    n, n_plain = (int(re.search(rb"element vertex (\d+)", p).group(1)) for p in (ply, ply_plain))
    print(f"plain {n_plain} vertices, dedupe {n}, {len(claimer)} suppressed")
    assert 1000 < n < n_plain and n_plain - n == len(claimer)
    call = lambda name, **kw: fusion.fuse_scan(*args, str(tmp_path / name), 1.0, 0.01, 0.3, 2, device=DEV, **kw)      # noqa: E731
    info = {}
    stats = call("dedupe.ply", records_budget=2 * h * w * 15, dedupe=True, info=info)
    assert info["groups"] == [(0, 2), (2, 4), (4, 5)] and info["synchronisations"] == 3 and info["dedupe"] is True
    assert (tmp_path / "dedupe.ply").read_bytes() == ply and info["vertices"] == n
    info1 = {}
    assert call("dedupe_1.ply", dedupe=True, info=info1) == stats and len(info1["groups"]) == 1
    assert (tmp_path / "dedupe_1.ply").read_bytes() == ply                        # the state does not depend on the grouping
    info0 = {}
    call("off.ply", dedupe=False, info=info0)
    call("default.ply")
    assert info0["dedupe"] is False and info0["vertices"] == n_plain
    assert (tmp_path / "off.ply").read_bytes() == ply_plain == (tmp_path / "default.ply").read_bytes()


def _vertices(path):
    with open(path, "rb") as f:
        return int(re.search(rb"element vertex (\d+)", f.read(400)).group(1))


def test_driver_dedupe_from_files_and_from_memory(tmp_path):
    """eval.py as child processes on one small folder scan: --fuse_points device and --fuse_source memory write the same
    deduplicated PLY, smaller than the plain one, and the run without the flag writes what the library call without it writes"""
    from itermvs_amd import fusion
    from test_fuse_memory_gpu import IMG_WH, LOOSE, write_scans
    data = tmp_path / "data"
    write_scans(str(data))
    (tmp_path / "list.txt").write_text("scan1\n")
    base = [sys.executable, os.path.join(ROOT, "eval.py"), "--dataset", "folder", "--testpath", str(data), "--testlist",
            str(tmp_path / "list.txt"), "--n_views", "4", "--img_wh", str(IMG_WH[0]), str(IMG_WH[1]), "--iteration", "2", "--filter"] + LOOSE
    runs = {"files": ["--fuse_points", "device", "--fuse_dedupe"], "memory": ["--fuse_source", "memory", "--fuse_dedupe"],
            "plain": ["--fuse_points", "device"]}
    procs = {name: subprocess.Popen(base + ["--outdir", str(tmp_path / name)] + extra, cwd=str(tmp_path), stdout=subprocess.PIPE,
                                    stderr=subprocess.STDOUT, text=True) for name, extra in runs.items()}
    for name, p in procs.items():
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (name, out[-1500:])
    ply = {name: tmp_path / name / "scan1.ply" for name in runs}
    assert ply["files"].read_bytes() == ply["memory"].read_bytes()
    n, n_plain = _vertices(ply["files"]), _vertices(ply["plain"])
    print(f"driver: plain {n_plain} vertices, --fuse_dedupe {n}")
    assert 100 < n < n_plain
    # without the flag: the bytes of the library call that knows nothing of it, on the PFMs that run wrote
    loose = dict(zip((x.lstrip("-") for x in LOOSE[0::2]), (float(x) for x in LOOSE[1::2])))
    fusion.filter_depth(str(data / "scan1"), str(tmp_path / "plain" / "scan1"), str(tmp_path / "lib.ply"), loose["geo_pixel_thres"],
                        loose["geo_depth_thres"], loose["photo_thres"], geo_mask_thres=int(loose["geo_mask_thres"]), device=DEV,
                        img_wh=IMG_WH, points="device")
    assert ply["plain"].read_bytes() == (tmp_path / "lib.ply").read_bytes()
    # and the deduplicated cloud is the library's on the same PFMs
    fusion.filter_depth(str(data / "scan1"), str(tmp_path / "files" / "scan1"), str(tmp_path / "lib_dedupe.ply"),
                        loose["geo_pixel_thres"], loose["geo_depth_thres"], loose["photo_thres"],
                        geo_mask_thres=int(loose["geo_mask_thres"]), device=DEV, img_wh=IMG_WH, points="device", dedupe=True)
    assert ply["files"].read_bytes() == (tmp_path / "lib_dedupe.ply").read_bytes()

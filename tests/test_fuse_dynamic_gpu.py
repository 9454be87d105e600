"""itermvs_fuse_depth_dynamic / fusion.fuse_scan(consistency="dynamic") / eval.py --geo_consistency dynamic on the MI355X: the
kernel against tests/fuse_dynamic_reference.py (masks and levels equal, the untouched outputs byte for byte ops.fuse_depth's), the
collapse to the static rule, true ties, monotone levels, non-finite inputs between guard bytes, the claim maps, whole scans and
the driver.  The inputs are those whose census tests/test_fuse_dynamic_cpu.py:test_input_census takes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import fuse_dynamic_reference as D
import fusion_scenes as G
import test_fuse_points_gpu as TP
from test_fuse_claim_cpu import _scan
from test_fuse_dynamic_cpu import BASE, CENSUS, build_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SHAPES = [(21, 37), (64, 96), (1, 1)]                  # ragged against the 8 x 32 tile in both directions; whole tiles; one pixel
SOURCES = [1, 2, 3, 5, 16]


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                   # a copy: the shared inputs are read-only


def _mats(args, others):
    from itermvs_amd import fusion
    return np.stack([fusion.pair_matrices(args[2], args[3], o[0], o[1]) for o in others])


@functools.lru_cache(maxsize=None)
def _inputs(h, w, s):
    """the inputs of a case, built once and shared; nothing changes them afterwards"""
    args, others, planted = build_inputs(h, w, s)
    for a in (args[0], args[1], *args[4]):
        a.flags.writeable = False
    return args, _mats(args, others), planted


@functools.lru_cache(maxsize=None)
def _want(h, w, s, n_min=D.DEFAULTS["n_min"], n_max=D.DEFAULTS["n_max"]):
    args, _, _ = _inputs(h, w, s)
    with np.errstate(all="ignore"):
        want = D.fuse_view_dynamic(*args, **BASE, **dict(D.DEFAULTS, n_min=n_min, n_max=n_max))[0]
    for a in want:
        a.flags.writeable = False
    return want


def _rule(**kw):
    r = dict(D.DEFAULTS, **kw)
    return dict(dyn_pixel_step=r["a"], dyn_depth_step=r["b"], dyn_n_min=r["n_min"], dyn_n_max=r["n_max"])


def _dynamic(args, mats, claimed_ref=None, claimed_src=None, base=BASE, **rule):
    from itermvs_amd import ops
    got = ops.fuse_depth_dynamic(_t(args[0]), _t(args[1]), [_t(x) for x in args[4]], _t(mats), claimed_ref, claimed_src, **base,
                                 **_rule(**rule))
    return [x.cpu().numpy() for x in got]


def _plain(args, mats, **thres):
    from itermvs_amd import ops
    return [x.cpu().numpy() for x in ops.fuse_depth(_t(args[0]), _t(args[1]), [_t(x) for x in args[4]], _t(mats), **thres)]


def _same_masks(got, want):
    """geo, final and level against the restatement's; the kernel's masks hold 0 and 1 only"""
    assert got[5].dtype == np.uint8 and np.array_equal(got[5], want[5]), int((got[5] != want[5]).sum())
    assert np.array_equal(got[2].astype(bool), want[2]) and np.array_equal(got[3].astype(bool), want[3])
    assert np.array_equal(got[1].astype(bool), want[1]) and np.array_equal(got[4], want[4])
    assert all(set(np.unique(got[i])) <= {0, 1} for i in (1, 2, 3))
    assert np.array_equal(got[2], (got[5] != 0).astype(np.uint8))


# -- 1. bit for bit against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SOURCES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_dynamic_kernel_equals_the_restatement(h, w, s):
    args, mats, _ = _inputs(h, w, s)
    want = _want(h, w, s)
    got = _dynamic(args, mats)
    _same_masks(got, want)
    plain = _plain(args, mats, **BASE, geo_mask_thres=3)
    assert got[0].view(np.uint64).tobytes() == plain[0].view(np.uint64).tobytes()         # depth_avg, bit patterns
    assert got[1].tobytes() == plain[1].tobytes() and got[4].tobytes() == plain[4].tobytes() and got[4].dtype == np.int32
    if s == 1:
        assert not got[2].any() and not got[5].any()                                   # one source cannot pass level 2
    elif h * w > 64:
        assert 0 < got[2].mean() < 1 and len(np.unique(got[5])) >= min(s, 4), np.unique(got[5])
    if s == 3:                                                                         # levels above S cannot accept
        three, sixteen = _dynamic(args, mats, n_max=3), _dynamic(args, mats, n_max=16)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(three, sixteen)) and three[5].tobytes() == got[5].tobytes()
    if s == 16 and h * w > 64:                                                         # every level the entry point takes
        for rule in (dict(D.DEFAULTS, n_min=1, n_max=16), dict(a=0.05, b=0.00016, n_min=1, n_max=16)):
            with np.errstate(all="ignore"):
                want16 = D.fuse_view_dynamic(*args, **BASE, **rule)[0]
            _same_masks(_dynamic(args, mats, **rule), want16)
            assert want16[5].max() >= 9                                                # levels counted in the second word too
        if (h, w) == (64, 96):
            assert want16[5].max() == 16 and len(np.unique(want16[5])) >= 15


# -- 2. collapse to the static rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [0.0021, 1.0 / 1300.0, 0.00077, 0.0025000001], ids=str)
def test_one_level_is_the_static_rule(b):
    h, w, s = CENSUS["h"], CENSUS["w"], CENSUS["s"]
    args, mats, _ = _inputs(h, w, s)
    b32 = np.float32(b)
    thres = dict(geo_pixel_thres=1.0, geo_depth_thres=float(np.float32(4) * b32), photo_thres=0.3)
    assert np.float32(thres["geo_depth_thres"]) == np.float32(4) * b32
    static = _plain(args, mats, **thres, geo_mask_thres=4)
    got = _dynamic(args, mats, base=thres, a=0.25, b=float(b32), n_min=4, n_max=4)
    for i in range(5):                                                                 # average, photo, geo, final, count
        assert got[i].tobytes() == static[i].tobytes(), i
    assert np.array_equal(got[5], 4 * static[2]) and 0 < static[2].mean() < 1


# -- 3. strictness ----------------------------------------------------------------------------------------------------------
def test_a_tie_rejects():
    """four copies of one source view: every copy has the same errors, so level n is c_n = 4 or 0.  With the step at half a
    pixel's own error (halving is exact) level 2's threshold IS that error and must reject it, level 4 accepts it; one float up
    and level 2 accepts it too."""
    h, w, s = CENSUS["h"], CENSUS["w"], CENSUS["s"]
    args, mats, _ = _inputs(h, w, s)
    d, conf, k, e, srcs, ks, es = args
    p = G.pair_detail(d, k, e, srcs[0], ks[0], es[0])
    assert p["dist"].dtype == np.float64 and p["rel"].dtype == np.float32
    with np.errstate(invalid="ignore"):
        good = (p["dist"] > 0.05) & (p["dist"] < 1) & (p["rel"] > np.float32(1e-5)) & (p["rel"] < np.float32(0.01))
    y, x = (int(v[0]) for v in np.nonzero(good))
    dist_p, rel_p = p["dist"][y, x], p["rel"][y, x]
    four = (d, conf, k, e, [srcs[0]] * 4, [ks[0]] * 4, [es[0]] * 4)
    mats4 = np.stack([mats[0]] * 4)
    run = lambda **rule: _dynamic(four, mats4, **rule)[5][y, x]                        # noqa: E731
    half_a, half_b = float(dist_p / 2), float(rel_p / np.float32(2))
    assert np.float64(2) * np.float64(half_a) == dist_p and np.float32(2) * np.float32(half_b) == rel_p
    assert run(a=half_a, b=1.0, n_min=2, n_max=2) == 0 and run(a=half_a, b=1.0, n_min=4, n_max=4) == 4
    assert run(a=half_a, b=1.0, n_min=2, n_max=4) == 3                                 # 1.5 times the error is the first above it
    assert run(a=float(np.nextafter(half_a, np.inf)), b=1.0, n_min=2, n_max=2) == 2
    assert run(a=1e6, b=half_b, n_min=2, n_max=2) == 0 and run(a=1e6, b=half_b, n_min=4, n_max=4) == 4
    assert run(a=1e6, b=float(np.nextafter(np.float32(half_b), np.float32(np.inf))), n_min=2, n_max=2) == 2
    for rule in (dict(a=half_a, b=1.0, n_min=2, n_max=4), dict(a=1e6, b=half_b, n_min=2, n_max=4)):
        with np.errstate(all="ignore"):
            want = D.fuse_view_dynamic(*four, **BASE, **rule)[0]
        _same_masks(_dynamic(four, mats4, **rule), want)


# -- 4. monotone levels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,n_max", [(5, 5), (16, 16)])
def test_fewer_levels_accept_what_their_levels_hold(s, n_max):
    h, w = CENSUS["h"], CENSUS["w"]
    args, mats, _ = _inputs(h, w, s)
    full = _dynamic(args, mats, n_max=n_max)
    _same_masks(full, _want(h, w, s, 2, n_max))
    for m in range(2, n_max):
        part = _dynamic(args, mats, n_max=m)
        assert np.array_equal(part[2] != 0, (full[5] != 0) & (full[5] <= m)), m
        assert np.array_equal(part[5], np.where(full[5] <= m, full[5], 0)), m


# -- 5. extremes, with guard bytes around every output ------------------------------------------------------------------------
def _raw(args, mats, base, rule, claimed=None):
    """the entry point itself, every output inside ONE allocation with guard bytes around it -> (outputs, guards intact)"""
    from itermvs_amd import _lib
    h, w = args[0].shape
    sizes = dict(avg=8 * h * w, photo=h * w, geo=h * w, final=h * w, cnt=4 * h * w, level=h * w)
    slot = {n: (b + GUARD - 1) // GUARD * GUARD + GUARD for n, b in sizes.items()}
    buf = torch.full((GUARD + sum(slot.values()),), 0xA5, device=DEV, dtype=torch.uint8)
    at, off = {}, GUARD
    for n in sizes:
        at[n], off = off, off + slot[n]
    d, conf, srcs, m = _t(args[0]), _t(args[1]), [_t(x) for x in args[4]], _t(mats)
    ptrs = (C.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
    base_ptr = buf.data_ptr()
    status = _lib.load().itermvs_fuse_depth_dynamic(
        d.data_ptr(), conf.data_ptr(), ptrs, m.data_ptr(), len(srcs), h, w, base["geo_pixel_thres"], base["geo_depth_thres"],
        base["photo_thres"], base_ptr + at["avg"], base_ptr + at["photo"], base_ptr + at["geo"], base_ptr + at["final"],
        base_ptr + at["cnt"], None, None, rule["a"], rule["b"], rule["n_min"], rule["n_max"], base_ptr + at["level"],
        torch.cuda.current_stream().cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    inside = np.zeros(host.size, bool)
    for n in sizes:
        inside[at[n]:at[n] + sizes[n]] = True
    dt = dict(avg=np.float64, photo=np.uint8, geo=np.uint8, final=np.uint8, cnt=np.int32, level=np.uint8)
    out = [host[at[n]:at[n] + sizes[n]].view(dt[n]).reshape(h, w) for n in ("avg", "photo", "geo", "final", "cnt", "level")]
    return out, bool((host[~inside] == 0xA5).all())


@pytest.mark.parametrize("rule", [D.DEFAULTS, dict(a=1e300, b=3e38, n_min=1, n_max=16), dict(a=1e-300, b=1e-30, n_min=1, n_max=2)],
                         ids=["defaults", "huge_steps", "tiny_steps"])
def test_non_finite_inputs_equal_the_restatement_and_nothing_else_is_written(rule):
    h, w, s = 21, 37, 5
    args, mats, planted = _inputs(h, w, s)
    args = (args[0].copy(), args[1].copy(), *args[2:4], [x.copy() for x in args[4]], *args[5:])
    d, conf, srcs = args[0], args[1], args[4]
    d[3, 4:9], d[4, 4:9], d[5, 4:9], d[6, 4:9], d[7, 4:9] = 0.0, -250.0, np.nan, np.inf, -np.inf
    conf[3:8, 4:9] = 0.9                                                               # those pixels pass the photometric mask
    srcs[0][10, 5:30], srcs[1][11, 5:30], srcs[2][12, 5:30], srcs[3][13:15, 5:30] = np.nan, np.inf, -np.inf, 0.0
    detail = G.pair_detail(d, args[2], args[3], srcs[4], args[5][4], args[6][4])
    assert (detail["kz"] <= 0).sum() >= 5                                              # projections behind the last source's camera
    assert all(planted[key] is not None for key in ("nan", "inf", "zero", "negative", "clamp"))
    with np.errstate(all="ignore"):
        want = D.fuse_view_dynamic(*args, **BASE, **rule)[0]
    got, guards = _raw(args, mats, BASE, rule)
    assert guards
    _same_masks(got, want)
    both = np.isfinite(want[0])
    assert np.array_equal(np.isfinite(got[0]), both) and np.array_equal(got[0][both], want[0][both])
    assert not got[5][3, 4:9].any() and not got[5][5:8, 4:9].any() and not got[5][planted["nan"]]     # zero, NaN, inf: no level
    if rule["a"] == 1e300:
        assert (got[5] == 1).mean() > 0.5 and (got[5] == 0).sum() >= 20
    if rule["a"] == 1e-300:
        assert not got[5].any()


# -- 6. with claim maps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,s", [(21, 37, 5), (64, 96, 3)])
def test_claim_maps_equal_the_restatement(h, w, s):
    from itermvs_amd import ops
    args, mats, planted = _inputs(h, w, s)
    claimed_ref, claimed_src = G.claim_maps(h, w, s, s, planted)
    with np.errstate(all="ignore"):
        want, want_maps, _ = D.fuse_view_dynamic(*args, claimed_ref, claimed_src, **BASE, **D.DEFAULTS)
    c_ref, c_src = _t(claimed_ref), [_t(c) for c in claimed_src]
    got = _dynamic(args, mats, c_ref, c_src)
    _same_masks(got, want)
    assert np.array_equal(c_ref.cpu().numpy(), claimed_ref)                            # the reference view's own map is only read
    new = 0
    for i, (m, wm, before) in enumerate(zip(c_src, want_maps, claimed_src)):
        m = m.cpu().numpy()
        assert np.array_equal(m, wm), (i, int((m != wm).sum()))
        assert (m[before == 1] == 1).all()
        new += int(wm.sum()) - int(before.sum())
    assert new > 0 and want[3].any() and (want[1] & want[2] & ~want[3]).any()
    free = _dynamic(args, mats)                                                        # what the claim maps do not touch
    for i in (0, 1, 2, 4, 5):
        assert got[i].tobytes() == free[i].tobytes(), i
    assert np.array_equal(got[3], free[3] & (claimed_ref == 0))
    # claimed_ref alone gates, claimed_src alone marks
    only_ref = _dynamic(args, mats, _t(claimed_ref), None)
    assert only_ref[3].tobytes() == got[3].tobytes()
    with np.errstate(all="ignore"):
        want0, want_maps0, _ = D.fuse_view_dynamic(*args, None, claimed_src, **BASE, **D.DEFAULTS)
    c_src0 = [_t(c) for c in claimed_src]
    only_src = _dynamic(args, mats, None, c_src0)
    assert only_src[3].tobytes() == free[3].tobytes()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(c_src0, want_maps0))
    # a map that is read and written in one launch
    alias = [_t(c) for c in claimed_src]
    with pytest.raises(RuntimeError, match=r"itermvs_fuse_depth_dynamic failed.*status -2"):
        ops.fuse_depth_dynamic(_t(args[0]), _t(args[1]), [_t(x) for x in args[4]], _t(mats), alias[s - 1], alias)


# -- 7. fuse_scan -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan():
    views = G.general_scene(32, 64, 6, CENSUS["seed"], CENSUS["noise"])
    args = _scan(views)
    with np.errstate(all="ignore"):
        return args, D.fuse_scan_dynamic(*args, **BASE, **D.DEFAULTS), D.fuse_scan_dynamic(*args, **BASE, dedupe=True, **D.DEFAULTS)


def test_fuse_scan_dynamic_equals_the_restatement(scan, tmp_path, monkeypatch):
    from itermvs_amd import fusion
    args, (ply, views, _), (ply_dedupe, views_dedupe, _) = scan
    n, n_dedupe = (len(p.split(b"end_header\n", 1)[1]) // 15 for p in (ply, ply_dedupe))
    print(f"dynamic: {n} vertices, with dedupe {n_dedupe}")
    assert 500 < n_dedupe < n
    call = lambda name, **kw: fusion.fuse_scan(*args, str(tmp_path / name), 1.0, 0.01, 0.3, device=DEV, **kw)      # noqa: E731
    info = {}
    stats = call("dynamic.ply", consistency="dynamic", info=info, mask_folder=str(tmp_path / "mask"))
    assert (tmp_path / "dynamic.ply").read_bytes() == ply and info["consistency"] == "dynamic" and info["vertices"] == n
    for ref, (g, ph, fin) in stats.items():
        v = views[ref]
        assert abs(g - v["geo"].mean()) < 1e-9 and abs(ph - v["photo"].mean()) < 1e-9 and abs(fin - v["final"].mean()) < 1e-9
    from PIL import Image
    for ref in views:
        for name in ("geo", "final", "photo"):
            with Image.open(str(tmp_path / "mask" / "{:0>8}_{}.png".format(ref, name))) as im:
                assert np.array_equal(np.array(im) != 0, views[ref][name]), (ref, name)
    # geo_mask_thres is not an argument of the rule
    call("dynamic_9.ply", consistency="dynamic", geo_mask_thres=9)
    assert (tmp_path / "dynamic_9.ply").read_bytes() == ply
    call("dedupe.ply", consistency="dynamic", dedupe=True, records_budget=2 * 32 * 64 * 15)
    assert (tmp_path / "dedupe.ply").read_bytes() == ply_dedupe
    # normals: the vertices and their order are those without them
    call("normals.ply", consistency="dynamic", normals=True)
    head, body = (tmp_path / "normals.ply").read_bytes().split(b"end_header\n", 1)
    rec = np.frombuffer(body, np.dtype([("xyz", "<u4", (3,)), ("nrm", "<u4", (3,)), ("rgb", "u1", (3,))]))
    plain = np.frombuffer(ply.split(b"end_header\n", 1)[1], D.R.RECORD)
    assert len(rec) == n and rec["xyz"].tobytes() == plain["xyz"].tobytes() and rec["rgb"].tobytes() == plain["rgb"].tobytes()
    assert (rec["nrm"] != 0).any()
    # mesh: it runs, and the views it keeps are photo & geo with the dynamic geo
    kept = {}
    inner = fusion.write_scan_mesh
    monkeypatch.setattr(fusion, "write_scan_mesh", lambda mesh, bounds, depth, mask, *a, **kw: (kept.update(mask=mask.cpu().numpy()),
                                                                                              inner(mesh, bounds, depth, mask, *a, **kw))[1])
    mesh_info = {}
    call("with_mesh.ply", consistency="dynamic", mesh=dict(path=str(tmp_path / "mesh.ply"), resolution=48), info=mesh_info)
    assert (tmp_path / "with_mesh.ply").read_bytes() == ply and (tmp_path / "mesh.ply").read_bytes().startswith(b"ply\n")
    print("mesh:", mesh_info["mesh"]["vertices"], "vertices,", mesh_info["mesh"]["faces"], "faces")
    for i, (ref, _) in enumerate(args[0]):
        assert np.array_equal(kept["mask"][i] != 0, views[ref]["kept"]), ref
    # static, given explicitly, is the default call
    call("default.ply")
    call("static.ply", consistency="static", dyn_pixel_step=7.0, dyn_n_min=1, dyn_n_max=1)
    assert (tmp_path / "static.ply").read_bytes() == (tmp_path / "default.ply").read_bytes() != ply


# -- 8. the driver ----------------------------------------------------------------------------------------------------------
RULES = {"defaults": ([], D.DEFAULTS),
         "flags": (["--dyn_pixel_step", "0.4", "--dyn_depth_step", "0.0015", "--dyn_levels", "1", "3"], dict(a=0.4, b=0.0015, n_min=1, n_max=3))}
PLANE = dict(h=48, w=80, views=5, seed=5, noise=0.002)     # tests/test_fusion.py's folder, noisy enough for a partial mask


def _plane_folder(root):
    """the synthetic scan folder of tests/test_fusion.py:test_filter_depth_scene_folder with each view's own confidence map and
    random colours stored losslessly at the depth maps' size -> (testpath, outdir, the arguments of D.fuse_scan_dynamic as the
    filter reads them back from the files)"""
    from PIL import Image
    from itermvs_amd import fusion
    from itermvs_amd.data_io import save_pfm
    from test_fusion import _scene
    h, w, n = PLANE["h"], PLANE["w"], PLANE["views"]
    views = _scene(h, w, n, PLANE["seed"], PLANE["noise"])
    scan, out = root / "data" / "scan1", root / "outputs" / "scan1"
    for folder in (scan / "cams_1", scan / "images", out / "depth_est", out / "confidence"):
        folder.mkdir(parents=True)
    rng = np.random.default_rng(3)
    lines, cams, images = [str(n)], {}, {}
    rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)      # noqa: E731
    for v, (k, e, d, conf) in enumerate(views):
        name = "{:0>8}".format(v)
        (scan / "cams_1" / (name + "_cam.txt")).write_text(f"extrinsic\n{rows(e)}\n\nintrinsic\n{rows(k)}\n\n425 2.5\n")
        images[v] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(images[v]).save(str(scan / "images" / (name + ".png")))
        save_pfm(str(out / "depth_est" / (name + ".pfm")), d)
        save_pfm(str(out / "confidence" / (name + ".pfm")), conf)
        srcs = [u for u in range(n) if u != v]
        lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} 1.0" for u in srcs)]
        cams[v] = fusion.read_camera_parameters(str(scan / "cams_1" / (name + "_cam.txt")))
        assert cams[v][0].tobytes() == k.tobytes() and cams[v][1].tobytes() == e.tobytes()
    (scan / "pair.txt").write_text("\n".join(lines) + "\n")
    pairs = fusion.read_pair_file(str(scan / "pair.txt"))
    return root / "data", root / "outputs", (pairs, cams, {v: views[v][2] for v in range(n)}, {v: views[v][3] for v in range(n)}, images)


def _masks(folder, views):
    from PIL import Image
    out = {}
    for ref in views:
        for kind in ("photo", "geo", "final"):
            with Image.open(str(folder / "{:0>8}_{}.png".format(ref, kind))) as im:
                assert im.mode == "L" and set(np.unique(np.array(im))) <= {0, 255}
                out[(ref, kind)] = np.array(im) != 0
    return out


@pytest.mark.parametrize("rule", list(RULES))
def test_driver_filter_stage_host_and_device_write_the_dynamic_masks(rule, tmp_path, capsys):
    """eval.py's filter stage with --fuse_points host and device on the plane folder: the mask PNGs of both are the restatement's
    photo, dynamic geo and final; the device cloud is the restatement's byte for byte and the host cloud agrees with it as
    tests/test_fuse_points_gpu.py:test_filter_depth_device_against_host demands; the static rule on the same folder writes other
    masks and another cloud"""
    import test_fuse_memory_gpu as TM
    flags, params = RULES[rule]
    data, outdir, scan_args = _plane_folder(tmp_path)
    with np.errstate(all="ignore"):
        ply, views, _ = D.fuse_scan_dynamic(*scan_args, **BASE, **params)
    shares = {ref: float(v["geo"].mean()) for ref, v in views.items()}
    print(rule, "dynamic geo shares", shares)
    assert all(0.05 < g < 0.95 for g in shares.values())
    E = TM._eval_module()
    base = ["--testpath", str(data), "--outdir", str(outdir), "--img_wh", str(PLANE["w"]), str(PLANE["h"]), "--filter", "--save_masks"]
    clouds, masks = {}, {}
    for mode in ("host", "device", "static_host", "static_device"):
        extra = [] if mode.startswith("static") else ["--geo_consistency", "dynamic"] + flags
        a = E.build_parser().parse_args(base + extra + ["--fuse_points", mode.split("_")[-1]])
        capsys.readouterr()
        assert E.fuse_scans(a) == 1
        lines = TM._stat_lines(capsys)
        clouds[mode] = (outdir / "scan1.ply").read_bytes()
        masks[mode] = _masks(outdir / "scan1" / "mask", views)
        if mode == "device":                                                           # the host path averages in float32
            want = ["processing scan1, ref-view{:0>2}, geo_mask:{:3f} photo_mask:{:3f} final_mask: {:3f}".format(
                ref, v["geo"].mean(), v["photo"].mean(), v["final"].mean()) for ref, v in views.items()]
            assert lines == want, mode
    for mode in ("host", "device"):
        for (ref, kind), m in masks[mode].items():
            assert np.array_equal(m, views[ref][kind]), (mode, ref, kind)
    assert clouds["device"] == ply
    (tmp_path / "host.ply").write_bytes(clouds["host"])
    (tmp_path / "device.ply").write_bytes(clouds["device"])
    head_h, pts_h = TP._read_ply(tmp_path / "host.ply")
    head_d, pts_d = TP._read_ply(tmp_path / "device.ply")
    assert head_d == head_h and len(pts_d) == len(pts_h) > 1000 and np.array_equal(pts_d["rgb"], pts_h["rgb"])
    assert np.isfinite(pts_h["xyz"].view(np.float32)).all() and np.isfinite(pts_d["xyz"].view(np.float32)).all()
    ulp = TP._ulp_distance(pts_d["xyz"], pts_h["xyz"])
    assert ulp.max() <= 1 and float((ulp != 0).mean()) <= 1e-4
    # the static rule (--geo_mask_thres 3) on the same files: the same photo masks, other geo masks, other clouds
    for mode in ("host", "device"):
        static = masks["static_" + mode]
        assert all(np.array_equal(static[(ref, "photo")], views[ref]["photo"]) for ref in views)
        assert all(not np.array_equal(static[(ref, "geo")], views[ref]["geo"]) for ref in views), mode
        assert clouds["static_" + mode] != clouds[mode]
    assert masks["static_host"].keys() == masks["static_device"].keys()
    assert all(np.array_equal(masks["static_host"][key], masks["static_device"][key]) for key in masks["static_host"])


def test_driver_dynamic_from_memory_equals_the_two_passes(tmp_path, capsys):
    """the whole driver on the two-scan folder of tests/test_fuse_memory_gpu.py (the depth maps come from the network with seeded
    random weights: half of the pairs reproject further than 9 px and 11 % of the depth, so the base thresholds are that file's
    loose ones and the steps 5 px and 5 %, which keep between a fifth and nine tenths of every view): --fuse_points host and device
    fuse the PFMs of one inference run, --fuse_source memory infers and fuses in one pass"""
    import test_fuse_memory_gpu as TM
    from itermvs_amd import fusion
    from itermvs_amd.data_io import read_pfm
    data = tmp_path / "data"
    TM.write_scans(str(data))
    E = TM._eval_module()
    rule = dict(a=5.0, b=0.05, n_min=2, n_max=4)
    dyn = ["--geo_consistency", "dynamic", "--dyn_pixel_step", "5", "--dyn_depth_step", "0.05", "--dyn_levels", "2", "4", "--save_masks"]
    common = ["--dataset", "folder", "--testpath", str(data), "--n_views", "4", "--img_wh", str(TM.IMG_WH[0]), str(TM.IMG_WH[1]),
              "--iteration", "2", "--filter"] + TM.LOOSE[:6] + dyn                    # LOOSE without its --geo_mask_thres
    parse = lambda out, extra: E.build_parser().parse_args(common + ["--outdir", str(out)] + extra)      # noqa: E731
    a_host, a_dev = parse(tmp_path / "a", ["--fuse_points", "host"]), parse(tmp_path / "a", ["--fuse_points", "device"])
    a_mem = parse(tmp_path / "b", ["--fuse_source", "memory"])
    assert all(E.check_geo_consistency(a) == "dynamic" for a in (a_host, a_dev, a_mem))
    E.save_depth(a_host)
    capsys.readouterr()
    assert E.fuse_scans(a_host) == 2
    host = TM._files(tmp_path / "a")
    capsys.readouterr()
    assert E.fuse_scans(a_dev) == 2
    lines_dev = TM._stat_lines(capsys)
    dev = TM._files(tmp_path / "a")
    mem_stats = E.fuse_memory(a_mem)
    lines_mem = TM._stat_lines(capsys)
    mem = TM._files(tmp_path / "b")
    assert lines_dev == lines_mem and len(lines_dev) == 2 * TM.N_VIEWS
    assert len([n for n in dev if n.endswith(".png")]) == 2 * TM.N_VIEWS * 3
    for scan in ("scan1", "scan2"):
        name = scan + ".ply"
        assert dev[name] == mem[name]                                                  # device and memory: byte for byte
        (tmp_path / "host.ply").write_bytes(host[name])
        (tmp_path / "dev.ply").write_bytes(dev[name])
        head_h, pts_h = TP._read_ply(tmp_path / "host.ply")
        head_d, pts_d = TP._read_ply(tmp_path / "dev.ply")
        assert head_d == head_h and len(pts_d) == len(pts_h) >= 1000 and np.array_equal(pts_d["rgb"], pts_h["rgb"])
        assert np.isfinite(pts_h["xyz"].view(np.float32)).all() and np.isfinite(pts_d["xyz"].view(np.float32)).all()
        ulp = TP._ulp_distance(pts_d["xyz"], pts_h["xyz"])
        assert ulp.max() <= 1 and float((ulp != 0).mean()) <= 1e-4                     # as the host/device test demands
        # the geo PNG of every run is the restatement's level map of the PFMs that the first pass wrote
        cams, depth = {}, {}
        for v in range(TM.N_VIEWS):
            k, e = fusion.read_camera_parameters(str(data / scan / "cams_1" / "{:0>8}_cam.txt".format(v)))
            k = k.copy()
            k[0] *= TM.IMG_WH[0] / 100
            k[1] *= TM.IMG_WH[1] / 75
            cams[v] = (k, e)
            depth[v] = np.squeeze(read_pfm(str(tmp_path / "a" / scan / "depth_est" / "{:0>8}.pfm".format(v)))[0])
        got = {run: _masks(folder / scan / "mask", range(TM.N_VIEWS)) for run, folder in (("device", tmp_path / "a"), ("memory", tmp_path / "b"))}
        for ref, srcs in fusion.read_pair_file(str(data / scan / "pair.txt")):
            errors = [D.pair_errors(depth[ref], *cams[ref], depth[s], *cams[s]) for s in srcs]
            geo = D.level_map([x[0] for x in errors], [x[1] for x in errors], **rule) != 0
            assert 0.2 < geo.mean() < 0.9, (scan, ref, float(geo.mean()))
            for kind in ("photo", "geo", "final"):
                png = os.path.join(scan, "mask", "{:0>8}_{}.png".format(ref, kind))
                assert dev[png] == mem[png] == host[png], png
            for run in got:
                assert np.array_equal(got[run][(ref, "geo")], geo), (run, scan, ref)
                assert np.array_equal(got[run][(ref, "final")], geo & got[run][(ref, "photo")]), (run, scan, ref)
            g, ph, fin = mem_stats[scan][ref]
            assert abs(g - geo.mean()) < 1e-9 and ph == 1.0 and abs(fin - g) < 1e-9

"""``--fuse_dedupe`` (itermvs_fuse_depth_claim), the parts that need no GPU: the numpy statement of the contract
(tests/fuse_claim_reference.py) on whole scans and at a depth edge, the status codes of the C entry point, and the Python /
driver surface."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_claim_reference as R
from conftest import ROOT
from oracle import fusion_oracle as FO
from test_fusion import _scene


def _scan(views):
    """every view a reference view with every other view as a source -> the arguments of R.fuse_scan_claim"""
    n = len(views)
    h, w = views[0][2].shape
    rng = np.random.default_rng(11)
    pairs = [(r, [v for v in range(n) if v != r]) for r in range(n)]
    return (pairs, {v: (views[v][0], views[v][1]) for v in range(n)}, {v: views[v][2] for v in range(n)},
            {v: views[v][3] for v in range(n)}, {v: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for v in range(n)})


@pytest.fixture(scope="module")
def scans():
    args = _scan(_scene())
    return args, R.fuse_scan_claim(*args, geo_mask_thres=2, dedupe=False), R.fuse_scan_claim(*args, geo_mask_thres=2)


def _records(ply):
    return np.frombuffer(ply.split(b"end_header\n", 1)[1], R.RECORD)


def test_first_view_is_untouched_and_the_cloud_is_a_strictly_smaller_subsequence(scans):
    _, (ply_plain, no_claimer, views_plain, _), (ply, claimer, views, _) = scans
    assert not no_claimer and ply_plain.startswith(R.ply_header(sum(len(v["records"]) for v in views_plain.values())))
    assert np.array_equal(views[0]["final"], views_plain[0]["final"]) and views[0]["final"].sum() > 1000
    assert views[0]["records"].tobytes() == views_plain[0]["records"].tobytes()
    plain, dedupe = _records(ply_plain), _records(ply)
    assert 0 < len(dedupe) < len(plain)
    print(f"plain {len(plain)} vertices, dedupe {len(dedupe)}")
    rows = [r.tobytes() for r in plain]
    at = 0
    for r in dedupe:                                   # every vertex is found, in order, in the plain cloud
        r = r.tobytes()
        while at < len(rows) and rows[at] != r:
            at += 1
        assert at < len(rows)
        at += 1
    for v in views:                                    # which is per view: the plain records of the pixels that still emit
        assert not (views[v]["final"] & ~views_plain[v]["final"]).any()
        keep = views[v]["final"][views_plain[v]["final"]]
        assert views[v]["records"].tobytes() == views_plain[v]["records"][keep].tobytes()


def test_every_suppressed_pixel_was_claimed_by_an_emitted_pixel_of_an_earlier_view(scans):
    (pairs, cams, depths, _, _), _, (_, claimer, views, claimed) = scans
    order = [ref for ref, _ in pairs]
    suppressed = {(v, int(p)) for v in views for p in np.flatnonzero((views[v]["plain"] & ~views[v]["final"]).reshape(-1))}
    assert suppressed and suppressed == set(claimer)
    h, w = depths[0].shape
    ok = {}
    for (v, p), (cv, cp) in claimer.items():
        assert cv >= 0 and order.index(cv) < order.index(v), (v, p, cv)
        assert views[cv]["final"].reshape(-1)[cp], (v, p, cv, cp)                   # the claimer was emitted
        assert claimed[v].reshape(-1)[p] == 1
        if (cv, v) not in ok:                          # v is a consistent source of the claimer, and p is the pixel it reached
            ok[(cv, v)] = R.claim_targets(depths[cv], *cams[cv], depths[v], *cams[v], 1.0, 0.01)
        good, may, qy, qx = ok[(cv, v)]
        assert good.reshape(-1)[cp] and may.reshape(-1)[cp] and qy.reshape(-1)[cp] * w + qx.reshape(-1)[cp] == p


def test_single_view_function_matches_the_plain_filter_when_nothing_is_claimed():
    views = _scene(40, 64, 3, 1, 0.004)
    k, e, d, conf = views[1]
    others = [views[0], views[2]]
    args = (d, conf, k, e, [o[2] for o in others], [o[0] for o in others], [o[1] for o in others])
    want = FO.fuse_reference_view(*args, geo_mask_thres=1)
    got, maps, _ = R.fuse_view_claim(*args, None, None, geo_mask_thres=1)
    assert maps is None and all(np.array_equal(a, b) for a, b in zip(got, want))
    mark = np.random.default_rng(0).uniform(size=d.shape) < 0.3
    before = [np.zeros(d.shape, np.uint8), np.zeros(d.shape, np.uint8)]
    before[0][3, 5] = 1
    got, maps, claims = R.fuse_view_claim(*args, mark.astype(np.uint8), before, geo_mask_thres=1)
    assert np.array_equal(got[3], want[3] & ~mark) and all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    assert maps[0][3, 5] == 1 and before[0].sum() == 1                                # marks survive, the inputs are not written
    assert all(m.sum() > 100 for m in maps) and all(len(p) == len(q) for p, q in claims)


def test_depth_edge_keeps_the_nearest_pixel_across_the_step_unclaimed():
    """The source map is shifted by 5 % on the lower-right triangle.  A reprojection whose four bilinear taps hold three values
    of the plane (a) and one of the shifted surface (1.05 a) with weight t samples a (1 + 0.05 t): it is consistent when
    0.05 t < geo_depth_thres, and the shifted tap is the nearest pixel when both fractions exceed 1/2, i.e. t in (0.25, 1).
    geo_depth_thres = 0.02 sits between 0.05 * 0.25 and 0.05 * 0.5: such pixels are consistent for t < 0.4, and the nearest pixel
    differs from the sample by 0.05 (1 - t) / (1 + 0.05 t) > 0.029 > 0.02, so the depth-edge condition refuses every one of them.
    Without the condition they would be claimed by points of a surface 5 % away.  geo_pixel_thres = 2 leaves the decision to the
    depths."""
    h, w = 64, 96
    views = _scene(h, w, 2, 0, 0.0)
    (k0, e0, d0, _), (k1, e1, d1, _) = views
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    shifted = xs * h + ys * w > h * w
    d1 = np.where(shifted, d1 * np.float32(1.05), d1).astype(np.float32)
    ok, may, qy, qx = R.claim_targets(d0, k0, e0, d1, k1, e1, 2.0, 0.02)
    _, loose, ly, lx = R.claim_targets(d0, k0, e0, d1, k1, e1, 2.0, 0.02, depth_condition=False)
    across = loose & shifted[ly, lx]                   # consistent, and the nearest source pixel is on the shifted surface
    assert across.sum() >= 1 and not (may & across).any()
    assert ok[across].all() and not shifted[qy[may], qx[may]].any() and may.sum() > 1000
    conf = np.ones((h, w), np.float32)
    zero = np.zeros((h, w), np.uint8)
    (_, _, _, final, _), (with_edge,), _ = R.fuse_view_claim(d0, conf, k0, e0, [d1], [k1], [e1], None, [zero], 2.0, 0.02, 0.3, 1)
    _, (without,), _ = R.fuse_view_claim(d0, conf, k0, e0, [d1], [k1], [e1], None, [zero], 2.0, 0.02, 0.3, 1, depth_condition=False)
    assert final[across].all()
    assert with_edge[shifted].sum() == 0 and without[shifted].sum() >= 1              # the reference alone shows it
    assert np.array_equal(with_edge[~shifted], without[~shifted]) and with_edge.sum() > 1000
    print(f"{int(across.sum())} emitted pixels have their nearest source pixel across the step; none of them claims it")


def test_claim_entry_point_is_declared_bound_and_documented():
    from itermvs_amd import _lib
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    lib = _lib.load()
    assert hasattr(lib, "itermvs_fuse_depth_claim") and lib.itermvs_version() == _lib.ABI_VERSION == 20
    plain, claim = _lib.PROTOTYPES["itermvs_fuse_depth"], _lib.PROTOTYPES["itermvs_fuse_depth_claim"]
    assert claim[1][:16] == plain[1][:16] and len(claim[1]) == len(plain[1]) + 2      # the same arguments plus the two map arguments
    doc = header.split("itermvs_fuse_depth_claim --")[1].split("*/")[0]
    assert "eval.py:238-269" in doc and "no counterpart in the reference" in doc


def test_claim_status_codes_without_a_launch():
    """every check precedes the launch, so these calls are safe without a GPU"""
    from itermvs_amd import _lib
    lib = _lib.load()
    buf, other = (C.c_uint8 * 256)(), (C.c_uint8 * 256)()
    a, b = C.addressof(buf), C.addressof(other)
    ptrs = lambda n, v=a: (C.c_void_p * n)(*[v] * n)                              # noqa: E731
    ok = dict(depth_ref=a, conf_ref=a, depth_src=ptrs(2), mats=a, S=2, H=4, W=4, pix=1.0, dep=0.01, photo=0.3, thres=1,
              depth_avg=a, photo_mask=None, geo_mask=None, final_mask=None, geo_sum=None, claimed_ref=b, claimed_src=ptrs(2),
              stream=None)
    call = lambda **kw: lib.itermvs_fuse_depth_claim(*{**ok, **kw}.values())      # noqa: E731
    for name in ("depth_ref", "conf_ref", "depth_src", "mats", "depth_avg"):
        assert call(**{name: None}) == -1, name                                   # ERR_NULL
    assert call(H=0) == -2 and call(W=0) == -2                                    # ERR_DIMS
    assert call(S=0) == -4                                                        # ERR_VIEWS
    assert call(S=17, depth_src=ptrs(17), claimed_src=ptrs(17)) == -4
    hole = ptrs(2)
    hole[1] = None
    assert call(depth_src=hole) == -1
    assert call(claimed_src=hole) == -1                                           # a NULL entry inside claimed_src
    alias = ptrs(2)
    alias[1] = b
    assert call(claimed_src=alias) == -2                                          # claimed_src[1] == claimed_ref
    assert call(claimed_ref=a) == -2
    assert call(S=17, depth_src=ptrs(17), claimed_src=alias) == -4                # the existing checks come first
    hole[0], hole[1] = None, b
    assert call(claimed_src=hole) == -1


def test_ops_and_filter_depth_refuse_what_cannot_work(tmp_path):
    import torch
    from itermvs_amd import fusion, ops
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)                     # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fuse_depth_claim(z(4, 4), z(4, 4), [z(4, 4)], z(1, 60), z(4, 4, dt=torch.uint8), [z(4, 4, dt=torch.uint8)])
    with pytest.raises(ValueError, match="dedupe=True needs points='device'") as e:
        fusion.filter_depth(str(tmp_path / "none"), str(tmp_path / "none"), str(tmp_path / "x.ply"), 1.0, 0.01, 0.3,
                            img_wh=(8, 8), points="host", dedupe=True)             # no pair.txt there: the check comes first
    assert "points='host'" in str(e.value) and not (tmp_path / "x.ply").exists()


def _eval():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


def test_eval_help_lists_the_flag():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    text = " ".join(p.stdout.split("--fuse_dedupe")[2].split())
    assert "sub-sequence of the default cloud" in text and "every byte as before" in text
    a = _eval().build_parser().parse_args([])
    assert a.fuse_dedupe is False and _eval().check_fuse_dedupe(a) is False


@pytest.mark.parametrize("argv,names", [
    (["--fuse_points", "device", "--fuse_dedupe"], ["--fuse_dedupe", "--filter"]),
    (["--filter", "--fuse_dedupe"], ["--fuse_dedupe", "--fuse_points device", "--fuse_source memory"]),
    (["--fuse_dedupe"], ["--fuse_dedupe", "--filter", "--fuse_points device", "--fuse_source memory"]),
])
def test_eval_refuses_dedupe_without_its_flags(argv, names):
    E = _eval()
    a = E.build_parser().parse_args(argv)
    with pytest.raises(SystemExit) as e:
        E.check_fuse_dedupe(a)
    for name in names:
        assert name in str(e.value), (name, str(e.value))
    with pytest.raises(SystemExit) as e2:              # the filter stage refuses before it touches a device
        E.fuse_scans(a)
    assert str(e2.value) == str(e.value)


def test_eval_accepts_dedupe_with_either_gpu_assembly():
    E = _eval()
    for argv in (["--filter", "--fuse_points", "device"], ["--dataset", "folder", "--filter", "--fuse_source", "memory"]):
        a = E.build_parser().parse_args(argv + ["--fuse_dedupe"])
        assert a.fuse_dedupe is True and E.check_fuse_dedupe(a) is True

"""``--geo_consistency dynamic`` (itermvs_fuse_depth_dynamic), the parts that need no GPU: the numpy statement of the level rule
(tests/fuse_dynamic_reference.py) against a per-pixel Python loop, the status codes and the validation order of the C entry point,
the driver's argparse rules, and the census of the inputs that tests/test_fuse_dynamic_gpu.py runs the kernel on."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_dynamic_reference as D
import fusion_scenes as G
from conftest import ROOT
from oracle import fusion_oracle as FO

# The inputs of the GPU file: tests/fusion_scenes.py:general_scene at this seed and noise with the pixels of ``plant_edges``, the
# reference view ``ref`` against all the others.  Seed, noise and reference view were searched on the restatement alone (noise
# 0.0017 to 0.0026, seeds 1 to 30, reference views 1 to 4) for the census of ``test_input_census``: with five sources the last
# level needs all five to agree at 1.25 px / 0.38 % while no two agree at 0.5 px / 0.15 %, which about one draw in twenty holds
# at 1 % of 777 pixels.  A GPU test on inputs where every pixel lands in one class would hide a wrong level loop.
CENSUS = dict(h=21, w=37, s=5, ref=2, seed=19, noise=0.0017)
BASE = dict(geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3)


def build_inputs(h, w, s, plant=True):
    """-> (the positional arguments of ``D.fuse_view_dynamic`` for the census reference view against the s others, others, planted)
    at any size and number of sources; the reference view is the census one where the scene has that many views"""
    views = G.general_scene(h, w, s + 1, CENSUS["seed"], CENSUS["noise"])
    ref = min(CENSUS["ref"], s - 1)
    planted = {}
    if plant and h * w > 64:
        views, planted = G.plant_edges(views, ref)
    args, others = G.split(views, ref)
    return args, others, planted


def _loop(args, a, b, n_min, n_max, geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3):
    """the rule as include/itermvs_hip.h words it, one pixel and one source at a time, on numpy scalars of the stated types"""
    d, conf, k, e, srcs, ks, es = args
    h, w = d.shape
    s_n = len(srcs)
    errors = [D.pair_errors(d, k, e, ds, k2, e2) for ds, k2, e2 in zip(srcs, ks, es)]
    level = np.zeros((h, w), np.uint8)
    count = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            for dist, rel in errors:
                count[y, x] += bool(dist[y, x] < np.float64(geo_pixel_thres) and rel[y, x] < np.float32(geo_depth_thres))
            for n in range(n_min, min(n_max, s_n) + 1):
                c_n = 0
                for dist, rel in errors:
                    assert type(dist[y, x]) is np.float64 and type(rel[y, x]) is np.float32
                    c_n += bool(dist[y, x] < np.float64(n) * np.float64(a) and rel[y, x] < np.float32(n) * np.float32(b))
                if c_n >= n:
                    level[y, x] = n
                    break
    photo = conf > photo_thres
    return level, count, photo


@pytest.mark.parametrize("rule", [D.DEFAULTS, dict(a=0.4, b=0.0015, n_min=1, n_max=3), dict(a=0.25, b=0.0025, n_min=3, n_max=3),
                                  dict(a=0.3, b=0.001, n_min=2, n_max=16)], ids=["defaults", "from_1", "one_level", "n_max_above_S"])
def test_restatement_equals_a_plain_loop(rule):
    views = G.general_scene(5, 7, 4, CENSUS["seed"], CENSUS["noise"])
    views[1][2][2, 3], views[0][2][1, 1], views[0][2][4, 6], views[2][2][0, 0] = np.nan, np.nan, 0.0, np.inf
    args, _ = G.split(views, 0)
    with np.errstate(all="ignore"):
        level, count, photo = _loop(args, **rule)
        (avg, ph, geo, final, cnt, lvl), maps, claims = D.fuse_view_dynamic(*args, **BASE, **rule)
        plain = FO.fuse_reference_view(*args, **BASE, geo_mask_thres=3)
    assert maps is None and claims == [] and lvl.dtype == np.uint8
    assert np.array_equal(lvl, level) and np.array_equal(cnt, count) and np.array_equal(ph, photo)
    assert np.array_equal(geo, level != 0) and np.array_equal(final, photo & (level != 0))
    assert avg.tobytes() == plain[0].tobytes() and np.array_equal(cnt, plain[4])          # the average is the static filter's
    assert lvl[1, 1] == 0 and lvl[4, 6] == 0                                               # NaN and zero reference depths fail
    assert len(set(lvl.ravel().tolist())) >= 2, lvl
    claimed = np.zeros((5, 7), np.uint8)
    claimed[2] = 1
    got, maps, _ = D.fuse_view_dynamic(*args, claimed, [np.zeros((5, 7), np.uint8)] * 3, **BASE, **rule)
    assert np.array_equal(got[3], final & (claimed == 0)) and np.array_equal(got[5], lvl) and len(maps) == 3


def test_levels_are_monotone_and_collapse_to_the_static_rule():
    """on the restatement: thresholds grow with n, so a run with fewer levels accepts the pixels whose level it still holds; and
    one level n with a = geo_pixel_thres / n, b = geo_depth_thres / n in float32 is the static rule with geo_mask_thres = n"""
    args, _, _ = build_inputs(21, 37, 5)
    with np.errstate(all="ignore"):
        full = D.fuse_view_dynamic(*args, **BASE, **dict(D.DEFAULTS, n_max=5))[0]
        for m in (2, 3, 4):
            part = D.fuse_view_dynamic(*args, **BASE, **dict(D.DEFAULTS, n_max=m))[0]
            assert np.array_equal(part[2], (full[5] != 0) & (full[5] <= m)), m
        b = np.float32(0.0021)
        one = D.fuse_view_dynamic(*args, **BASE, a=0.25, b=float(b), n_min=4, n_max=4)[0]
        static = FO.fuse_reference_view(*args, geo_pixel_thres=1.0, geo_depth_thres=np.float32(4) * b, photo_thres=0.3, geo_mask_thres=4)
    assert np.array_equal(one[2], static[2]) and np.array_equal(one[3], static[3]) and 0 < static[2].mean() < 1


def test_input_census():
    """the inputs the GPU tests use, on the restatement alone"""
    c = CENSUS
    assert (c["h"], c["w"], c["s"]) == (21, 37, 5)
    args, _, planted = build_inputs(c["h"], c["w"], c["s"])
    assert all(planted[key] is not None for key in ("nan", "inf", "zero", "negative", "clamp"))
    (_, _, geo, _, cnt, level), _, _ = D.fuse_view_dynamic(*args, **BASE, **D.DEFAULTS)
    shares = {n: float((level == n).mean()) for n in range(0, 6)}
    static = cnt >= 3
    only_dynamic, only_static = float((geo & ~static).mean()), float((~geo & static).mean())
    print("level shares", shares, "dynamic only", only_dynamic, "static only", only_static)
    assert set(np.unique(level)) <= {0, 2, 3, 4, 5}
    for n in (2, 3, 4, 5):
        assert shares[n] >= 0.01, (n, shares)
    assert shares[0] >= 0.05 and only_dynamic >= 0.01 and only_static >= 0.01


def test_dynamic_entry_point_is_declared_bound_and_documented():
    from itermvs_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "itermvs_hip.h")).read()
    lib = _lib.load()
    assert hasattr(lib, "itermvs_fuse_depth_dynamic") and lib.itermvs_version() == _lib.ABI_VERSION == 20
    claim, dyn = _lib.PROTOTYPES["itermvs_fuse_depth_claim"][1], _lib.PROTOTYPES["itermvs_fuse_depth_dynamic"][1]
    # the arguments of the claim entry point without geo_mask_thres (its 11th), then a, b, n_min, n_max, geo_level before the stream
    assert dyn == claim[:10] + claim[11:18] + [C.c_double, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    doc = header.split("itermvs_fuse_depth_dynamic --")[1].split("*/")[0]
    for words in ("UNVERIFIED", "rounded once", "NaN fails", "n_max > S is allowed", "no counterpart"):
        assert words in doc, words
    assert "geo_mask_thres" not in header.split("int itermvs_fuse_depth_dynamic(")[1].split(";")[0]
    assert (ops.DYN_PIXEL_STEP, ops.DYN_N_MIN, ops.DYN_N_MAX) == (0.25, 2, 10) and ops.DYN_DEPTH_STEP == 1.0 / 1300.0
    assert D.DEFAULTS["b"] == float(np.float32(ops.DYN_DEPTH_STEP))                        # what the float argument becomes
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--geo_consistency dynamic" in design and "unverified" in design.split("--geo_consistency dynamic")[1][:6000]


def test_dynamic_status_codes_and_their_order_without_a_launch():
    """every check precedes the launch, so these calls are safe without a GPU; a fully valid call is never made"""
    from itermvs_amd import _lib
    lib = _lib.load()
    buf, other = (C.c_uint8 * 256)(), (C.c_uint8 * 256)()
    a, b = C.addressof(buf), C.addressof(other)
    ptrs = lambda n, v=a: (C.c_void_p * n)(*[v] * n)                              # noqa: E731
    ok = dict(depth_ref=a, conf_ref=a, depth_src=ptrs(2), mats=a, S=2, H=4, W=4, pix=1.0, dep=0.01, photo=0.3, depth_avg=a,
              photo_mask=None, geo_mask=None, final_mask=None, geo_sum=None, claimed_ref=b, claimed_src=ptrs(2), step_a=0.25,
              step_b=0.001, n_min=2, n_max=10, geo_level=None, stream=None)
    call = lambda **kw: lib.itermvs_fuse_depth_dynamic(*{**ok, **kw}.values())    # noqa: E731
    bad_rule = dict(step_a=-1.0)                                                  # goes with a case to show which check is first
    # 1. the checks of itermvs_fuse_depth_claim, in its order
    for name in ("depth_ref", "conf_ref", "depth_src", "mats", "depth_avg"):
        assert call(**{name: None}) == -1 == call(**{name: None}, **bad_rule), name   # ERR_NULL
    assert call(H=0) == -2 and call(W=0) == -2                                    # ERR_DIMS
    assert call(S=0) == -4 == call(S=0, **bad_rule)                               # ERR_VIEWS
    assert call(S=17, depth_src=ptrs(17), claimed_src=ptrs(17)) == -4
    assert call(H=0, S=0) == -2 and call(depth_ref=None, H=0) == -1
    hole = ptrs(2)
    hole[1] = None
    assert call(depth_src=hole) == -1 == call(depth_src=hole, **bad_rule)
    assert call(claimed_src=hole) == -1 == call(claimed_src=hole, **bad_rule)     # a NULL entry inside claimed_src
    alias = ptrs(2)
    alias[1] = b
    assert call(claimed_src=alias) == -2 and call(claimed_ref=a) == -2            # claimed_src[s] == claimed_ref
    assert call(S=17, depth_src=ptrs(17), claimed_src=alias) == -4                # the existing checks come first
    assert call(S=0, claimed_src=hole) == -4
    # 2. the rule's parameters: ERR_DIMS, with or without claim maps
    for maps in ({}, dict(claimed_ref=None, claimed_src=None), dict(claimed_ref=None), dict(claimed_src=None)):
        for value in (0.0, -0.25, float("nan"), float("inf"), -float("inf")):
            assert call(step_a=value, **maps) == -2, value
            assert call(step_b=value, **maps) == -2, value
        assert call(step_b=1e-60, **maps) == -2                                   # rounds to 0 as a float
        assert call(n_min=0, **maps) == -2 and call(n_min=-1, **maps) == -2
        assert call(n_min=5, n_max=4, **maps) == -2
        assert call(n_max=17, **maps) == -2 and call(n_min=17, n_max=17, **maps) == -2
    assert call(claimed_src=hole, n_max=17) == -1                                 # a NULL claim map is reported before the levels


def test_ops_and_fusion_refuse_what_cannot_work(tmp_path):
    import torch
    from itermvs_amd import fusion, ops
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)                     # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fuse_depth_dynamic(z(4, 4), z(4, 4), [z(4, 4)], z(1, 60), z(4, 4, dt=torch.uint8), [z(4, 4, dt=torch.uint8)])
    assert fusion.dynamic_options() is None and fusion.dynamic_options("static", dyn_pixel_step=-1) is None
    assert fusion.dynamic_options("dynamic") == dict(dyn_pixel_step=0.25, dyn_depth_step=1.0 / 1300.0, dyn_n_min=2, dyn_n_max=10)
    for bad in (dict(consistency="both"), dict(consistency="dynamic", dyn_pixel_step=0.0), dict(consistency="dynamic", dyn_depth_step=float("nan")),
                dict(consistency="dynamic", dyn_depth_step=1e-60), dict(consistency="dynamic", dyn_depth_step=1e60),
                dict(consistency="dynamic", dyn_n_min=0), dict(consistency="dynamic", dyn_n_min=4, dyn_n_max=3),
                dict(consistency="dynamic", dyn_n_max=17)):
        with pytest.raises(ValueError):
            fusion.dynamic_options(**bad)
        for points in ("host", "device"):                                         # no pair.txt there: the check comes first
            with pytest.raises(ValueError, match="consistency|dyn_"):
                fusion.filter_depth(str(tmp_path / "none"), str(tmp_path / "none"), str(tmp_path / "x.ply"), 1.0, 0.01, 0.3,
                                    img_wh=(8, 8), points=points, **bad)
    assert not (tmp_path / "x.ply").exists()


def _eval():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval as E
    return E


def test_eval_help_lists_the_flags():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    text = " ".join(p.stdout.split())
    for flag in ("--geo_consistency {static,dynamic}", "--dyn_pixel_step", "--dyn_depth_step", "--dyn_levels MIN MAX"):
        assert flag in text, flag
    assert "every byte as before" in " ".join(p.stdout.split("--geo_consistency")[2].split()) and "unverified" in text
    E = _eval()
    a = E.build_parser().parse_args([])
    assert a.geo_consistency == "static" and a.geo_mask_thres == 3 and E.check_geo_consistency(a) == "static"
    a = E.build_parser().parse_args(["--filter", "--geo_mask_thres", "4"])
    assert a.geo_mask_thres == 4 and E.check_geo_consistency(a) == "static"


@pytest.mark.parametrize("argv", [["--filter"], ["--filter", "--fuse_points", "device", "--fuse_dedupe", "--ply_normals", "--mesh"],
                                  ["--dataset", "folder", "--filter", "--fuse_source", "memory", "--dyn_levels", "1", "16"],
                                  ["--filter", "--dyn_pixel_step", "0.5", "--dyn_depth_step", "0.002", "--dyn_levels", "3", "3"]])
def test_eval_accepts_dynamic_with_every_assembly(argv):
    from itermvs_amd import fusion
    E = _eval()
    a = E.build_parser().parse_args(argv + ["--geo_consistency", "dynamic"])
    assert E.check_geo_consistency(a) == "dynamic"
    kw = fusion.consistency_from_args(a)
    assert kw["consistency"] == "dynamic" and fusion.dynamic_options(**kw) is not None
    if "--dyn_pixel_step" in argv:
        assert kw == dict(consistency="dynamic", dyn_pixel_step=0.5, dyn_depth_step=0.002, dyn_n_min=3, dyn_n_max=3)
    elif "--dyn_levels" not in argv:
        assert kw == dict(consistency="dynamic", dyn_pixel_step=0.25, dyn_depth_step=1.0 / 1300.0, dyn_n_min=2, dyn_n_max=10)


@pytest.mark.parametrize("argv,names", [
    (["--filter", "--geo_consistency", "dynamic", "--geo_mask_thres", "3"], ["--geo_mask_thres 3", "--geo_consistency dynamic"]),
    (["--filter", "--geo_mask_thres", "5", "--geo_consistency", "dynamic"], ["--geo_mask_thres 5", "--dyn_levels"]),
    (["--geo_consistency", "dynamic"], ["--geo_consistency dynamic", "--filter"]),
    (["--filter", "--dyn_pixel_step", "0.5"], ["--dyn_pixel_step", "--geo_consistency dynamic"]),
    (["--filter", "--dyn_depth_step", "0.001"], ["--dyn_depth_step", "--geo_consistency dynamic"]),
    (["--filter", "--geo_consistency", "static", "--dyn_levels", "2", "5"], ["--dyn_levels", "--geo_consistency dynamic"]),
    (["--filter", "--geo_consistency", "dynamic", "--dyn_levels", "0", "5"], ["--dyn_levels MIN", "0..5"]),
    (["--filter", "--geo_consistency", "dynamic", "--dyn_levels", "6", "5"], ["--dyn_levels MIN", "6..5"]),
    (["--filter", "--geo_consistency", "dynamic", "--dyn_levels", "2", "17"], ["--dyn_levels MIN", "2..17"]),
    (["--filter", "--geo_consistency", "dynamic", "--dyn_pixel_step", "0"], ["--dyn_pixel_step"]),
    (["--filter", "--geo_consistency", "dynamic", "--dyn_depth_step", "nan"], ["--dyn_depth_step"]),
    (["--filter", "--geo_consistency", "dynamic", "--dyn_depth_step", "1e-60"], ["--dyn_depth_step", "float32", "1e-60"]),   # 0 as a float
    (["--filter", "--geo_consistency", "dynamic", "--dyn_depth_step", "1e60"], ["--dyn_depth_step", "float32", "1e+60"]),    # inf as a float
])
def test_eval_refuses_with_an_argparse_error(argv, names, capsys):
    E = _eval()
    a = E.build_parser().parse_args(argv)
    for stage in (E.check_geo_consistency, E.fuse_scans):                           # the filter stage refuses before it touches a device
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            stage(a)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "usage:" in err                              # what argparse does with an error
        for name in names:
            assert name in err, (name, err)


def test_eval_refuses_dynamic_in_a_child_process_too():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--filter", "--geo_consistency", "dynamic", "--geo_mask_thres", "2"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--geo_mask_thres 2 cannot be given with --geo_consistency dynamic" in p.stderr
    p = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--geo_consistency", "sometimes"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 2 and "invalid choice" in p.stderr

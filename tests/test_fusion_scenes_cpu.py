"""tests/fusion_scenes.py before any kernel sees it, without a GPU: the scene has the properties it is there for, the census shows
that every case of tests/test_fusion_general_gpu.py holds every branch the kernels have, the restatements on it are sensitive to
the slot errors that tests/test_fusion.py:_scene cannot see, and the host packer lays a pair block out as the header says.

What the census does NOT demand, and why:
  * every value 0..S of the consistency count is demanded at 37 x 61 and 72 x 104; at 9 x 33 (297 pixels) the bins 0..S are demanded
    for S <= 5 only;
  * the sizes (1,1), (1,33), (9,1) and (8,32) of the GPU file are there for the launch geometry (one pixel, one row, one column, one
    full tile); a single row or column cannot hold a silhouette in both axes, so the census is taken at 9 x 33 and above;
  * under the third threshold set (geo_mask_thres = S + 1) nothing emits by construction: the final-mask share must be 0 there and
    the claim and normals conditions, which speak of emitting pixels, do not apply;
  * with the view behind the surface as the reference every source stands in front of the wall it sees, so the pairs with kz <= 0
    are those of the planted negative depth; with any other reference they are the sphere's pixels in the view behind it.
The 21-float ``cam`` block of ``fusion.fuse_scan`` is built after the first upload, so it is held on the GPU
(tests/test_fusion_general_gpu.py:test_fuse_scan_packs_the_reference_views_cam_block)."""
import numpy as np
import pytest

import fuse_normals_reference as NR
import fusion_scenes as G
from oracle import fusion_oracle as FO
from test_fusion import _scene

DEFAULTS = dict(geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=3)
STRICT = dict(geo_pixel_thres=0.5, geo_depth_thres=0.005, photo_thres=0.0, geo_mask_thres=1)
SEED, NOISE = 3, 0.002


def thresholds(name, s):
    """the three threshold sets by name; "nothing" needs the number of source views"""
    return {"defaults": DEFAULTS, "strict": STRICT,
            "nothing": dict(geo_pixel_thres=2.0, geo_depth_thres=0.01, photo_thres=0.8, geo_mask_thres=s + 1)}[name]


def ref_index(which, s):
    """"first", "last" (the last view in front of the sphere) or "behind" among the s + 1 views of a case"""
    return {"first": 0, "last": s - 1, "behind": s}[which]


# (h, w, S, reference view, threshold set): the cases of the GPU file that the census is taken on.  The view behind the surface and
# 9 x 33 from the first view go with the strict set: under the defaults none of their emitting pixels is refused at a depth edge.
CENSUS_CASES = [(72, 104, 5, "first", "defaults"), (72, 104, 5, "last", "defaults"), (72, 104, 5, "behind", "strict"),
                (72, 104, 16, "first", "defaults"), (72, 104, 2, "last", "nothing"),
                (37, 61, 5, "first", "strict"), (37, 61, 5, "last", "defaults"), (37, 61, 5, "behind", "strict"),
                (37, 61, 2, "first", "strict"), (37, 61, 1, "first", "strict"), (37, 61, 5, "first", "nothing"),
                (9, 33, 5, "last", "defaults"), (9, 33, 5, "first", "strict"), (9, 33, 5, "first", "nothing")]
# launch geometry only (see the module docstring)
TINY_CASES = [(1, 1, 1, "first", "strict"), (1, 33, 2, "first", "strict"), (9, 1, 5, "last", "strict"), (8, 32, 16, "first", "defaults")]


def build_case(h, w, s, which, plant=True):
    """-> (views, reference index, planted): the inputs of one case, shared with the GPU file"""
    views = G.general_scene(h, w, s + 1, SEED, NOISE)
    ref = ref_index(which, s)
    if plant and h * w > 64:
        views, planted = G.plant_edges(views, ref)
    else:
        planted = {}
    return views, ref, planted


def test_scene_has_the_properties_it_is_there_for():
    for h, w, n in ((72, 104, 6), (9, 33, 6), (37, 61, 17)):
        views = G.general_scene(h, w, n, SEED, 0.0)
        ks, es = [v[0] for v in views], [v[1] for v in views]
        assert all(k.dtype == np.float32 and e.dtype == np.float32 and e.shape == (4, 4) for k, e in zip(ks, es))
        assert all(v[2].dtype == np.float32 and v[2].shape == (h, w) and v[3].dtype == np.float32 for v in views)
        assert all(k[0, 0] != k[1, 1] for k in ks) and sum(k[0, 1] != 0 for k in ks) >= 2
        assert len({k.tobytes() for k in ks}) == n and len({(float(k[0, 2]), float(k[1, 2])) for k in ks}) == n
        assert len({float(k[0, 0]) for k in ks}) == n
        for i, e in enumerate(es):
            assert (e[:3] != 0).all(), (i, e)
            for j, e2 in enumerate(es):
                if i != j:
                    assert (np.matmul(e2, np.linalg.inv(e))[:3] != 0).all(), (i, j)
        # the pair block: the only exact zeros are the structural ones of K and inv(K); _scene has 24 in 60
        m = FO.pair_matrices(ks[0], es[0], ks[1], es[1])
        assert (m["t_rs"][:3] != 0).all() and (m["t_sr"][:3] != 0).all()
        assert sum(int((m[p] == 0).sum()) for p in ("a_ref", "k_src", "a_src", "k_ref")) <= 14
        for k, e, d, _ in views[:-1]:                      # every front view: sphere and wall, so a silhouette
            assert (d < 500).sum() >= 4 and (d > 800).sum() >= 4 and np.isfinite(d).all() and (d > 0).all()
        assert (views[-1][2] > 300).all()                  # the view behind sees the wall only
        k, e, d, _ = views[0]
        p = G.pair_detail(d, k, e, views[-1][2], views[-1][0], views[-1][1])
        assert (p["kz"][d < 500] <= 0).all()               # and every sphere point of view 0 lies behind it
    old = _scene(37, 61, 6, 1, 0.0)
    m = FO.pair_matrices(old[0][0], old[0][1], old[1][0], old[1][1])
    assert sum(int((m[p][:3] == 0).sum()) for p in m) == 24


def _check(c, h, w, s, name):
    """the conditions of the module docstring on one census"""
    hist = c["histogram"]
    if h * w >= 37 * 61 or s <= 5:
        assert all(n > 0 for n in hist), hist
    for key in ("behind", "outside_window", "clamp", "nonfinite", "only_distance", "only_depth"):
        assert c[key] > 0, (key, c)
    if name == "nothing":
        assert c["final_share"] == 0 and c["claims"] == 0
        return
    assert c["final_share"] >= 0.15, c
    for key in ("edge_refused", "first_row_or_column", "last_row_or_column", "target_outside", "claims"):
        assert c[key] > 0, (key, c)
    for axis in "xy":                                       # both sides of a silhouette: one-sided differences are taken
        assert c[f"normal_{axis}_one_sided"] > 0 and c[f"normal_{axis}_central"] > 0, c


@pytest.mark.parametrize("h,w,s,which,name", CENSUS_CASES)
def test_census(h, w, s, which, name):
    views, ref, planted = build_case(h, w, s, which)
    assert all(planted[key] is not None for key in ("nan", "inf", "zero", "negative_zero", "negative", "tiny", "clamp", "outside"))
    assert all(f"{key}_{i}" in planted for key in ("src_nan", "src_zero", "src_negative", "src_inf") for i in range(min(2, s)))
    claimed_ref, _ = G.claim_maps(h, w, s, s, planted)
    c = G.census(views, ref, thresholds(name, s), claimed_ref)
    print(h, w, s, which, name, c)
    _check(c, h, w, s, name)
    d = views[ref][2]
    assert np.isnan(d[planted["nan"]]) and np.isinf(d[planted["inf"]]) and d[planted["tiny"]] == np.float32(1e-30)
    assert d[planted["zero"]] == 0 and not np.signbit(d[planted["zero"]]) and np.signbit(d[planted["negative_zero"]])
    # the clamp pixel: its float64 source coordinate in source 0 is finite and beyond 2^26 pixels
    (dr, _, k, e, srcs, ks, es), _ = G.split(views, ref)
    p = G.pair_detail(dr, k, e, srcs[0], ks[0], es[0])
    xy = np.array([p["x_src"][planted["clamp"]], p["y_src"][planted["clamp"]]], np.float64)
    assert np.isfinite(xy).all() and np.abs(xy).max() > 2.0 ** 26
    # without the planted pixels the scene itself holds the points behind a camera, unless the reference is the view behind
    if which != "behind":
        plain, _, _ = build_case(h, w, s, which, plant=False)
        assert G.census(plain, ref, thresholds(name, s))["behind"] >= 20


def _outputs(views, ref, thres=DEFAULTS):
    args, _ = G.split(views, ref)
    with np.errstate(all="ignore"):
        return FO.fuse_reference_view(*args, **thres)


def _changed(a, b):
    """share of pixels at which the count or the float64 average differs (a NaN equals a NaN)"""
    return float((~((a[4] == b[4]) & ((a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0]))))).mean())


def _swap(*pairs):
    def mutate(m):
        m = dict(m)
        for a, b in pairs:
            m[a], m[b] = m[b], m[a]
        return m
    return mutate


MUTATIONS = {
    "K_src <-> K_ref with their inverses": _swap(("k_src", "k_ref"), ("a_src", "a_ref")),
    "inv(K_ref) <-> inv(K_src) alone": _swap(("a_ref", "a_src")),
    "t_rs <-> t_sr": _swap(("t_rs", "t_sr")),
    "K_src transposed": lambda m: dict(m, k_src=np.ascontiguousarray(m["k_src"].T)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_slot_errors_change_the_general_scene_and_the_first_one_not_the_old_scene(name, monkeypatch):
    general = G.general_scene(37, 61, 6, SEED, NOISE)
    old = _scene(96, 128, 5, 1, 0.004)
    want, want_old = _outputs(general, 0, STRICT), _outputs(old, 2)
    true = FO.pair_matrices
    monkeypatch.setattr(FO, "pair_matrices", lambda *a: MUTATIONS[name](true(*a)))
    got, got_old = _outputs(general, 0, STRICT), _outputs(old, 2)
    share, share_old = _changed(got, want), _changed(got_old, want_old)
    print(f"{name}: {share:.3f} of the general scene's pixels change, {share_old:.3f} of _scene's")
    assert share > 0.10
    if name.startswith("K_src <-> K_ref"):                  # the recorded blind spot: one K for every view
        assert share_old == 0.0 and np.array_equal(got_old[4], want_old[4]) and got_old[0].tobytes() == want_old[0].tobytes()


def test_reassociated_products_change_bits(monkeypatch):
    """m0 x + (m1 y + m2 z) in place of (m0 x + m1 y) + m2 z: the contract is k ascending.  With general cameras the float64 values
    do change: the source-space z of the projection and the float64 world points differ in their last bits at most pixels (on
    _scene's rows [c, 0, s] one product is an exact zero and the order cannot matter).  What the kernels WRITE is a different
    matter: every float64 chain of the filter ends in a float32 rounding (the source coordinates, the reprojected depth, the vertex),
    and a last-bit float64 difference crosses a float32 rounding boundary about once in 2^29 values, so the count map and the
    average are expected to stay as they are.  Both are recorded here; only the first is asserted."""
    general = G.general_scene(37, 61, 6, SEED, NOISE)
    want = _outputs(general, 0, STRICT)
    (d, _, k, e, srcs, ks, es), _ = G.split(general, 0)
    kz = G.pair_detail(d, k, e, srcs[0], ks[0], es[0])["kz"]
    xyz = FO.unproject_points(want[0], want[3], k, e)
    up = lambda m: m.astype(np.float64)                      # noqa: E731
    monkeypatch.setattr(FO, "_mat3", lambda m, p: np.stack([up(m)[i, 0] * p[0] + (up(m)[i, 1] * p[1] + up(m)[i, 2] * p[2]) for i in range(3)]))
    monkeypatch.setattr(FO, "_mat4", lambda m, p: np.stack([up(m)[i, 0] * p[0] + (up(m)[i, 1] * p[1] + (up(m)[i, 2] * p[2] + up(m)[i, 3] * 1.0))
                                                              for i in range(3)]))
    got = _outputs(general, 0, STRICT)
    bits = int((got[0].view(np.uint64) != want[0].view(np.uint64)).sum())
    print(f"re-associated products: {bits} of {want[0].size} averages change, {int((got[4] != want[4]).sum())} counts")
    kz_share = float((G.pair_detail(d, k, e, srcs[0], ks[0], es[0])["kz"] != kz).mean())
    xyz_share = float((FO.unproject_points(want[0], want[3], k, e) != xyz).any(axis=1).mean())
    print(f"float64: {kz_share:.3f} of the source-space z and {xyz_share:.3f} of the world points change")
    assert kz_share > 0.10 and xyz_share > 0.10


def test_wrong_views_k_in_the_cam_block_changes_points_and_normals():
    general = G.general_scene(37, 61, 6, SEED, NOISE)
    avg, _, _, final, _ = _outputs(general, 0, STRICT)
    (k, e), k_wrong = general[0][:2], general[1][0]
    xyz, bad = (FO.unproject_points(avg, final, kk, e).astype(np.float32) for kk in (k, k_wrong))
    assert final.sum() > 1000 and float((xyz != bad).any(axis=1).mean()) > 0.10
    n, n_bad = NR.normals(avg, final, k, e), NR.normals(avg, final, k_wrong, e)
    assert float((n != n_bad).any(axis=1).mean()) > 0.10
    old = _scene(37, 61, 6, 1, 0.002)                      # and on _scene every view's K is the same matrix
    assert all(v[0].tobytes() == old[0][0].tobytes() for v in old)


def test_pair_matrices_packs_the_six_parts_in_the_headers_order():
    """include/itermvs_hip.h: inv(K_ref)(9) | (E_src inv(E_ref)) rows 0..2 (12) | K_src(9) | inv(K_src)(9) | (E_ref inv(E_src)) rows
    0..2 (12) | K_ref(9), byte for byte the restatement's matrices"""
    from itermvs_amd import fusion
    views = G.general_scene(37, 61, 6, SEED, NOISE)
    (k_ref, e_ref), (k_src, e_src) = views[1][:2], views[3][:2]
    m = FO.pair_matrices(k_ref, e_ref, k_src, e_src)
    parts = [m["a_ref"], m["t_rs"][:3], m["k_src"], m["a_src"], m["t_sr"][:3], m["k_ref"]]
    assert len({p.tobytes() for p in parts}) == 6 and all(p.dtype == np.float32 for p in parts)
    got = fusion.pair_matrices(k_ref, e_ref, k_src, e_src)
    assert got.dtype == np.float32 and got.shape == (60,)
    assert got.tobytes() == b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
    for at, p in zip((0, 9, 21, 30, 39, 51), parts):          # the offsets csrc/fusion.hip reads them at
        assert got[at:at + p.size].tobytes() == np.ascontiguousarray(p).tobytes(), at

"""Error statuses of the entry points of the one-thread-per-item ("flat") kernels, whose grids csrc/flat_launch.hpp now counts: every
case starts from a valid argument list in HOST memory and breaks exactly one thing -- each null pointer, each dimension at 0, the
alignment rules of the convex pair, the smallest in-range int32 dimensions whose item count crosses the launch's limit, a grid.y
one above its limit, and for the two two-piece launches a case where each piece is in range and only their sum is not.  Every
expected status is a rejection that precedes any launch; a fully valid list is never passed.

The limits (flat_launch.hpp): gridDim.x * blockDim.x < 2^32, that is MAX256 = 2^32 - 256 items of a 256-thread launch; grid.y <=
65535; INT32 = 2^31 - 1 items where the kernel forms the index or a product of its dimensions in an int.

Against the library BEFORE flat_launch.hpp every case passes unchanged except the ones marked CHANGED: that library checked no item
count (itermvs_tap_indices, itermvs_resize_rgb8 and itermvs_undistort_rgb8: only 2^31 blocks) and narrowed the block count with a
cast.  Without a device it answered ITERMVS_ERR_LAUNCH (-7) to each of the 40 CHANGED cases; with a device the same calls either
failed in the runtime (-7) or launched a wrapped grid and answered ITERMVS_OK with part of the output unwritten.  All of them now
answer ITERMVS_ERR_DIMS.  Three CHANGED cases are limits outside the item count that the kernels' 32-bit arithmetic needs:
H1 * W1 of itermvs_warp_backward, 3 * Ws of the two image pyramids, 2 * H of itermvs_resize_rgb8."""
import ctypes as C

import pytest

NULL, DIMS, VIEWS, ALIGN, LAYOUT, DTYPE = -1, -2, -4, -5, -6, -8
_BUF = (C.c_float * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16          # a 16-byte aligned host address
A4 = A + 4                                       # aligned to 4 bytes only
N3 = (C.c_int32 * 3)(1, 1, 1)
N3_BIG = (C.c_int32 * 3)(2 ** 31 - 1, 1, 1)
PARAMS = (C.c_double * 4)(100.0, 100.0, 4.0, 4.0)
T = 2 ** 31 - 127                                # 2 * T = MAX256 + 2, the first even count past the limit of a 256-thread launch
CH = " CHANGED"

# entry point -> its valid argument list, in call order (struct arguments: the struct's fields under "p." / "src.")
VALID = {
    "itermvs_bilinear_up": dict(x=A, M=1, H=3, W=5, scale=2, act=0, out=A, stream=None),
    "itermvs_bilinear_up2": dict(x=A, B=1, C=1, H=3, W=5, scale=2, act=0, out=A, out_sb=60, out2=None, out2_sb=0, stream=None),
    "itermvs_prob_regress": dict(logits=A, sb=3840, sc=15, sp=1, B=1, P=15, nd_out0=A, nd_sb0=15, nd_out1=None, nd_sb1=0, prob=None, best=None, stream=None),
    "itermvs_gru_rh": dict(zr=A, h=A, h_sb=480, rh=A, rh_sb=480, B=1, hid=32, P=15, stream=None),
    "itermvs_gru_out": dict(zr=A, q=A, h=A, h_sb=480, h_copy=None, B=1, hid=32, P=15, stream=None),
    "itermvs_pack_scores": dict(s0=A, s1=A, s2=A, N=N3, B=1, P=15, dst0=A, dst1=None, dst_sb=45, ch0=0, stream=None),
    "itermvs_convex_upsample": dict(logits=A, sb=2160, sc=15, sy=5, sx=1, nd=A, nd_sb=15, inv_depth_min=A, inv_depth_max=A, B=1, H=3, W=5, depth=A,
                                    norm_out=None, stream=None),
    "itermvs_final_upsample": dict(logits=A, sb=2160, sc=15, sy=5, sx=1, nd=A, nd_sb=15, inv_depth_min=A, inv_depth_max=A, B=1, H=3, W=5, depth=A,
                                   conf=A, M=1, conf_up=A, stream=None),
    "itermvs_tap_indices": {"p.B": 1, "p.S": 2, "p.H": 3, "p.W": 5, "p.N": 4, "p.H1": 3, "p.W1": 5, "p.init": 0, "p.proj": A, "p.depth": A, "p.norm_depth": None,
                            "p.norm_depth_sb": 0, "p.inv_depth_min": A, "p.inv_depth_max": A, "p.out": A, "p.coords": None, "stream": None},
    "itermvs_pvw_tail": dict(x=A, w=A, bias=None, M=1, N=32, C=16, P=15, out=A, stream=None),
    "itermvs_view_aggregate": dict(corr=A, w=A, S=2, B=1, N=4, P=15, out=A, stream=None),
    "itermvs_view_aggregate_up": dict(corr=A, corr_layout=0, w=A, S=2, B=1, N=4, H3=3, W3=5, out=A, w_up=A, w_up_interleaved=0, stream=None),
    "itermvs_softmax_max": dict(x=A, M=1, N=32, P=15, out=A, stream=None),
    "itermvs_warp": {"src.data": A, "src.sb": 240, "src.sc": 15, "src.sy": 5, "src.sx": 1, "src.C": 16, "src.H": 3, "src.W": 5, "src.dtype": 0,
                     "proj": A, "depth": A, "B": 1, "N": 4, "H": 3, "W": 5, "out": A, "mask": None, "stream": None},
    "itermvs_warp_backward": dict(grad_out=A, proj=A, depth=A, B=1, C=16, N=4, H=3, W=5, H1=3, W1=5, grad_src=A, stream=None),
    "itermvs_compose_proj": dict(mats=A, n_sets=1, V=3, out=A, nan_flag=None, depth_min=A, depth_max=A, B=1, inv_min=A, inv_max=A, stream=None),
    "itermvs_image_pyramid": dict(src=A, V=1, Hs=6, Ws=10, H=8, W=8, level0=A, level1=A, level2=A, level3=A, stream=None),
    "itermvs_image_pyramid_jitter": dict(src=A, V=1, Hs=6, Ws=10, H=8, W=8, jitter=A, lsum=A, level0=A, level1=A, level2=A, level3=A, stream=None),
    "itermvs_gt_pyramid": dict(depth_rows=A, mask_src=None, params=A, B=1, Hs=6, Ws=10, H=8, W=8, recipe=1, depth0=A, depth1=A, depth2=A, depth3=A,
                               mask0=A, mask1=A, mask2=A, mask3=A, stream=None),
    "itermvs_resize_rgb8": dict(src=A, V=1, Hs=6, Ws=10, H=3, W=5, xbounds=A, xk=A, KX=2, ybounds=A, yk=A, KY=2, out=A, stream=None),
    "itermvs_undistort_rgb8": dict(src=A, Hs=6, Ws=10, model=1, params=PARAMS, n_params=4, fx_o=100.0, fy_o=100.0, cx_o=2.5, cy_o=1.5, Ho=3, Wo=5, out=A,
                                   map=None, stream=None),
}


def nulls(*names, status=NULL):
    return [(f"{n} null", {n: None}, status) for n in names]


def zeros(*names, status=DIMS):
    return [(f"{n} 0", {n: 0}, status) for n in names]


CONVEX = (nulls("logits", "nd", "inv_depth_min", "inv_depth_max", "depth") + zeros("B", "H", "W") + [
    ("depth pointer", dict(depth=A4), ALIGN),
    ("4 B H W = 2^31" + CH, dict(H=1, W=2 ** 29), DIMS),                        # INT32: the kernel forms the output row 4 * y + i in an int
    ("4 B H W leaves 64 bits" + CH, dict(B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1), DIMS)])

CASES = {
    "itermvs_bilinear_up": nulls("x", "out") + zeros("M", "H", "W", "scale") + [
        ("M H W scale^2 = MAX256 + 2" + CH, dict(M=2, H=1, W=T, scale=1), DIMS),
        ("M H W scale^2 leaves 64 bits" + CH, dict(M=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, scale=2 ** 31 - 1), DIMS)],
    "itermvs_bilinear_up2": nulls("x", "out") + zeros("B", "C", "H", "W", "scale") + [
        ("B C H W scale^2 = MAX256 + 2" + CH, dict(B=2, H=1, W=T, scale=1), DIMS),
        ("B C H W scale^2 leaves 64 bits" + CH, dict(B=2 ** 31 - 1, C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, scale=2 ** 31 - 1), DIMS)],
    "itermvs_prob_regress": nulls("logits") + zeros("B", "P") + [
        ("8 P = MAX256 + 8" + CH, dict(P=2 ** 29 - 31), DIMS), ("grid.y 65536" + CH, dict(B=65536), DIMS)],
    "itermvs_gru_rh": nulls("zr", "h", "rh") + zeros("B", "hid", "P") + [("B hid P = MAX256 + 2" + CH, dict(B=2, hid=1, P=T), DIMS)],
    "itermvs_gru_out": nulls("zr", "q", "h") + zeros("B", "hid", "P") + [("B hid P = MAX256 + 2" + CH, dict(B=2, hid=1, P=T), DIMS)],
    "itermvs_pack_scores": nulls("s0", "s1", "s2", "N", "dst0") + zeros("B", "P") + [
        ("B (N0 + N1 + N2) P = 2^31 + 1" + CH, dict(P=715827883), DIMS),         # INT32: the kernel adds N0 + N1 + N2 in an int
        ("N sum leaves int32" + CH, dict(N=N3_BIG), DIMS)],
    "itermvs_convex_upsample": CONVEX + [("norm_out pointer", dict(norm_out=A4), ALIGN)],
    "itermvs_final_upsample": CONVEX + nulls("conf", "conf_up") + zeros("M") + [
        ("16 M H W = MAX256 + 16" + CH, dict(H=1, W=2 ** 28 - 15), DIMS),
        ("only the sum: 2^16 + (2^24 - 2^16) blocks" + CH, dict(B=4, H=1, W=2 ** 20, M=255), DIMS)],
    "itermvs_tap_indices": zeros("p.B", "p.H", "p.W", "p.H1", "p.W1", "p.N") + zeros("p.S", status=VIEWS) + [("p.S 17", {"p.S": 17}, VIEWS)] +
        nulls("p.proj", "p.inv_depth_min", "p.inv_depth_max", "p.out") + [
        ("no hypothesis source", {"p.depth": None}, NULL), ("init with N 1", {"p.init": 1, "p.N": 1}, DIMS),
        ("B S N H W = 2^31" + CH, {"p.S": 1, "p.N": 2, "p.H": 1, "p.W": 2 ** 30}, DIMS)],              # INT32: the kernel keeps H * W in an int
    "itermvs_pvw_tail": nulls("x", "w", "out") + zeros("M", "P", "N") + [
        ("N 33", dict(N=33), DIMS), ("C 32", dict(C=32), -3),
        ("8 P = 2^32 - 504 (512 threads)" + CH, dict(P=2 ** 29 - 63), DIMS), ("grid.y 65536" + CH, dict(M=65536), DIMS)],
    "itermvs_view_aggregate": nulls("corr", "w", "out") + zeros("S", "B", "N", "P") + [                 # INT32: the kernel gets N * 8 as an int
        ("8 B N P = 2^31, four per thread" + CH, dict(N=1, P=2 ** 28), DIMS), ("8 B N P = 2^31, one per thread" + CH, dict(N=1, P=2 ** 28, w=A4), DIMS)],
    "itermvs_view_aggregate_up": nulls("corr", "w", "out", "w_up") + zeros("S", "B", "N", "H3", "W3") + [
        ("corr_layout 2", dict(corr_layout=2), LAYOUT), ("groups last: corr pointer", dict(corr_layout=1, corr=A4), ALIGN),
        ("8 B N P = 2^31" + CH, dict(N=1, H3=1, W3=2 ** 28), DIMS), ("groups last: 8 B N P = 2^31" + CH, dict(corr_layout=1, N=1, H3=1, W3=2 ** 28), DIMS),
        ("4 B S P = MAX256 + 32" + CH, dict(N=1, S=8, H3=1, W3=2 ** 27 - 7), DIMS),
        ("only the sum: 2^14 + (2^24 - 2^14) blocks" + CH, dict(N=2, S=1023, H3=1, W3=2 ** 20), DIMS)],
    "itermvs_softmax_max": nulls("x", "out") + zeros("M", "N", "P") + [
        ("M P = 2^32 - 62 (64 threads)" + CH, dict(M=2, P=2 ** 31 - 31), DIMS), ("N 33: M P = MAX256 + 2" + CH, dict(N=33, M=2, P=T), DIMS)],
    "itermvs_warp": nulls("src.data", "proj", "depth", "out") + zeros("B", "N", "H", "W", "src.C", "src.H", "src.W") + [
        ("src.dtype 1", {"src.dtype": 1}, DTYPE), ("B N H W = MAX256 + 2" + CH, dict(B=2, N=1, H=1, W=T), DIMS)],
    "itermvs_warp_backward": nulls("grad_out", "proj", "depth", "grad_src") + zeros("B", "C", "N", "H", "W", "H1", "W1") + [
        ("B N H W = MAX256 + 2" + CH, dict(B=2, N=1, H=1, W=T), DIMS),
        ("H1 W1 = 2^31" + CH, dict(H1=2, W1=2 ** 30), DIMS)],                    # the kernel forms y * W1 + x of the source map in an int
    "itermvs_compose_proj": nulls("mats", "out") + zeros("n_sets") + [
        ("V 1", dict(V=1), VIEWS), ("V 18", dict(V=18), VIEWS), ("inv_min without depth_min", dict(depth_min=None), NULL), ("inv_min with B 0", dict(B=0), NULL),
        ("n_sets (V - 1) = 2^31" + CH, dict(n_sets=2 ** 30), DIMS)],             # INT32: the kernel takes the item as an int
    "itermvs_image_pyramid": nulls("src", "level0") + zeros("V", "Hs", "Ws", "H", "W") + [
        ("levels of H 12", dict(H=12), DIMS),
        ("V H W = MAX256 + 2" + CH, dict(V=2, H=1, W=T, level1=None, level2=None, level3=None), DIMS),
        ("3 Ws > 2^31 - 1" + CH, dict(Ws=715827883), DIMS)],                      # the kernel forms x * 3 + c of a source row in an int
    "itermvs_image_pyramid_jitter": nulls("src", "jitter", "lsum", "level0") + zeros("V", "Hs", "Ws", "H", "W") + [
        ("levels of H 12", dict(H=12), DIMS), ("grid.y 65536", dict(V=65536), DIMS),
        ("H W = MAX256 + 2" + CH, dict(H=2, W=T, level1=None, level2=None, level3=None), DIMS),
        ("V H W = MAX256 + 2" + CH, dict(V=2, H=1, W=T, level1=None, level2=None, level3=None), DIMS),
        ("3 Ws > 2^31 - 1" + CH, dict(Ws=715827883), DIMS)],
    "itermvs_gt_pyramid": nulls("depth_rows", "params") + zeros("B", "Hs", "Ws", "H", "W") + [
        ("recipe 2", dict(recipe=2), DIMS), ("DTU masks without mask_src", dict(recipe=0), NULL), ("H 12", dict(H=12), DIMS), ("grid.y 65536", dict(B=65536), DIMS),
        ("Hs Ws = 2^31", dict(Hs=2 ** 16, Ws=2 ** 15), DIMS),
        ("85 H W / 64 = MAX256 + 85" + CH, dict(H=8, W=8 * 50529025), DIMS)],
    "itermvs_resize_rgb8": nulls("src", "out", "xbounds", "xk", "ybounds", "yk") + zeros("V", "Hs", "Ws", "H", "W", "KX", "KY") + [
        ("V H W = MAX256 + 4" + CH, dict(V=2, H=2, W=2 ** 30 - 63), DIMS),
        ("2 H = 2^31" + CH, dict(H=2 ** 30), DIMS)],                             # the kernel forms 2 * y in an int
    "itermvs_undistort_rgb8": nulls("src", "out", "params") + zeros("Hs", "Ws", "Ho", "Wo") + [
        ("model 7", dict(model=7), -9), ("n_params 5", dict(n_params=5), DIMS), ("Ho Wo = MAX256 + 2" + CH, dict(Ho=2, Wo=T), DIMS)],
}
ALL = [(fn, name, broken, status) for fn, cases in CASES.items() for name, broken, status in cases]


def call(lib, fn, args):
    """the call of `fn` with the argument list `args`; "p." / "src." entries are the fields of the struct passed first"""
    from itermvs_amd import _lib
    fields = {k.split(".")[1]: v for k, v in args.items() if "." in k}
    plain = [v for k, v in args.items() if "." not in k]
    if fields:
        struct = (_lib.TapParams if fn == "itermvs_tap_indices" else _lib.FMap)(**fields)
        plain.insert(0, C.byref(struct))
    assert len(_lib.PROTOTYPES[fn][1]) == len(plain), fn
    return getattr(lib, fn)(*plain)


def test_every_entry_point_and_argument_is_covered():
    assert set(CASES) == set(VALID)
    for fn, args in VALID.items():
        assert all(broken and set(broken) <= set(args) for _, broken, _ in CASES[fn]), fn
        assert any(CH in name for name, _, _ in CASES[fn]), fn          # every entry point has its limit case


@pytest.mark.parametrize("fn,name,broken,status", ALL, ids=[f"{c[0][8:]}: {c[1]}" for c in ALL])
def test_one_broken_argument(fn, name, broken, status):
    from itermvs_amd import _lib
    assert broken, "a fully valid list is never passed"
    assert call(_lib.load(), fn, dict(VALID[fn], **broken)) == status

"""Error statuses of the fused one-launch entry points (res_chain16, lateral_conv3x3, conv3x3_conv1x1, gru_conv, down_conv, the three
head entries, the two corrnet entries, stem): every case starts from a valid argument list in HOST memory and breaks exactly one
thing -- each null pointer, each size limit, each channel / layout / alignment rule, the per-image 32-bit offset limits and the
2^31 tile-count limit.  Every expected status is a rejection that precedes any launch; a fully valid list is never passed.

The expected statuses are the ones the library returned BEFORE the tile-count check and the launch tail of these entry points
were gathered into csrc/tile_walk.hpp: this file passes unchanged against that library, with the exceptions marked CHANGED below:
  * itermvs_head_fused / itermvs_head_fused_conf computed tiles_x * H * B in a plain int and never checked it; from 2^31 tiles on they
    now answer ITERMVS_ERR_DIMS like every other entry point (the one intended fix);
  * itermvs_down_conv set its kernel's LDS attribute (a HIP call) before it checked the tile count, so without a device it answered
    ITERMVS_ERR_LAUNCH at 2^31 tiles; the tile count is now checked first, as in the other entry points: ITERMVS_ERR_DIMS.
Every tile-count check now precedes every HIP call (persistent_plan_cus asks the device for its CU count only afterwards).

Not here, because no argument list reaches it: the 16 * H * W * 4 < 2^31 limit of res_chain16 (H, W <= 4095 is checked first and
is tighter)."""
import ctypes as C

import pytest

NULL, DIMS, CHANNELS, ALIGN, LAYOUT = -1, -2, -3, -5, -6
_BUF = (C.c_float * 64)()
A = (C.addressof(_BUF) + 15) // 16 * 16          # a 16-byte aligned host address
A4, A8 = A + 4, A + 8                            # aligned to 4 / 8 bytes only


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


W3, W3_NULL1, W3_ODD2 = ptrs(A, A, A), ptrs(A, None, A), ptrs(A, A, A4)
SEG = (C.c_int32 * 2)(1, 2)

# entry point -> its valid argument list, in call order
VALID = {
    "itermvs_res_chain16": dict(y1=A, y1_sn=1024, shortcut=A, shortcut_sn=1024, in_layout=0, N=1, H=8, W=8, weights=W3, bias=W3, out=A, out_sn=1024, stream=None),
    "itermvs_lateral_conv3x3": dict(fine=A, fine_sn=1024, Cf=16, coarse=A, coarse_sn=256, N=1, H=8, W=8, w_lat=A, b_lat=A, w_out=A, b_out=A, Cout=16,
                                    out=A, out_sn=1024, out_layout=0, out2=None, stream=None),
    "itermvs_conv3x3_conv1x1": dict(x=A, x_sb=2048, B=1, H=8, W=8, w0_tile=A, w1_packed=A, weight_format=0, bias1=A, NO=16, out=A, out_sb=1024, stream=None),
    "itermvs_gru_conv": dict(x=A, x_sb=2752, B=1, H=8, W=8, mode=0, w_packed=A, bias=A, h=A, h_sb=2048, z=A, z_sb=2048, out=A, out_sb=2048, out2=A,
                             out2_sb=2048, stream=None),
    "itermvs_down_conv": dict(x=A, x_sn=1024, N=1, Cin=16, H=8, W=8, w_packed=A, bias=A, C=32, y=A, y_sn=512, sc=A, sc_sn=512, stream=None),
    "itermvs_head_fused": dict(hidden=A, hidden_sb=2048, B=1, H=8, W=8, w0_tile=A, w0_format=0, w1_packed=A, w2_packed=A, w2_format=0, bias2=A,
                               nd_out0=A, nd_sb0=64, nd_out1=None, nd_sb1=0, best=None, stream=None),
    "itermvs_head_fused_conf": dict(hidden=A, hidden_sb=2048, B=1, H=8, W=8, w0_tile=A, w1_packed=A, w2_packed=A, w2_format=0, bias2=A, nd_out0=A, nd_sb0=64,
                                    nd_out1=None, nd_sb1=0, best=None, wc_tile=A, conf_dot=A, conf=A, conf_sb=64, stream=None),
    "itermvs_head_regress": dict(x=A, x_sb=2048, B=1, P=64, w1_packed=A, w2_packed=A, bias2=A, nd_out0=A, nd_sb0=64, nd_out1=None, nd_sb1=0, best=None,
                                 stream=None),
    "itermvs_corrnet": dict(x=A, x_sn=512, weights=W3, seg_end=SEG, n_seg=1, M=1, H=8, W=8, out=A, out_sn=64, out2=None, out2_sn=0, stream=None),
    "itermvs_stem": dict(x=A, x_sn=768, M=1, H=16, W=16, w0=A, w1=A, y=A, sc=A, out_sn=1024, out_layout=0, stream=None),
}
VALID["itermvs_corrnet_bf16x3"] = VALID["itermvs_corrnet"]

HEAD = [("hidden null", dict(hidden=None), NULL), ("w0 null", dict(w0_tile=None), NULL), ("w1 null", dict(w1_packed=None), NULL),
        ("w2 null", dict(w2_packed=None), NULL), ("bias2 null", dict(bias2=None), NULL),
        ("B 0", dict(B=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS),
        ("w2_format 1", dict(w2_format=1), LAYOUT), ("w0 pointer", dict(w0_tile=A4), ALIGN), ("w2 pointer", dict(w2_packed=A8), ALIGN)]
HEAD_TILES = ("2^31 tiles CHANGED", dict(B=32768, H=65536, W=16), DIMS)      # (the library before tile_walk.hpp wrapped an int here)
CORRNET = [("x null", dict(x=None), NULL), ("weights null", dict(weights=None), NULL), ("out null", dict(out=None), NULL),
           ("M 0", dict(M=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS), ("H 6", dict(H=6), DIMS), ("W 10", dict(W=10), DIMS),
           ("n_seg 0", dict(n_seg=0), DIMS), ("n_seg 4", dict(n_seg=4), DIMS),
           ("8 H W 4 = 2^31", dict(H=8192, W=8192), DIMS),
           ("second weight set null", dict(n_seg=2, weights=W3_NULL1), NULL), ("third weight set pointer", dict(n_seg=3, weights=W3_ODD2), ALIGN)]

CASES = {
    "itermvs_res_chain16": [
        ("y1 null", dict(y1=None), NULL), ("shortcut null", dict(shortcut=None), NULL), ("weights null", dict(weights=None), NULL),
        ("bias null", dict(bias=None), NULL), ("out null", dict(out=None), NULL),
        ("N 0", dict(N=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS), ("H 4096", dict(H=4096), DIMS), ("W 4096", dict(W=4096), DIMS),
        ("in_layout 2", dict(in_layout=2), LAYOUT), ("in_layout -1", dict(in_layout=-1), LAYOUT),
        ("nhwc: y1 pointer", dict(in_layout=1, y1=A4), ALIGN), ("nhwc: shortcut pointer", dict(in_layout=1, shortcut=A8), ALIGN),
        ("nhwc: y1 stride", dict(in_layout=1, y1_sn=1026), ALIGN), ("nhwc: shortcut stride", dict(in_layout=1, shortcut_sn=1026), ALIGN),
        ("second layer null", dict(weights=W3_NULL1), NULL), ("third layer pointer", dict(weights=W3_ODD2), ALIGN),
        ("2^31 tiles", dict(N=32768, H=4095, W=4095), DIMS)],
    "itermvs_lateral_conv3x3": [
        ("fine null", dict(fine=None), NULL), ("coarse null", dict(coarse=None), NULL), ("w_lat null", dict(w_lat=None), NULL),
        ("w_out null", dict(w_out=None), NULL), ("out null", dict(out=None), NULL),
        ("N 0", dict(N=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS), ("H 7", dict(H=7), DIMS), ("W 9", dict(W=9), DIMS),
        ("H 8192", dict(H=8192), DIMS), ("W 8192", dict(W=8192), DIMS),
        ("48 H W 4 >= 2^31", dict(H=4096, W=4096), DIMS),
        ("Cf 32", dict(Cf=32), CHANNELS), ("Cout 32", dict(Cout=32), CHANNELS),
        ("out_layout -1", dict(out_layout=-1), LAYOUT), ("out_layout 4", dict(out_layout=4), LAYOUT),
        ("w_out pointer", dict(w_out=A8), ALIGN), ("nhwc: out pointer", dict(out_layout=1, out=A8), ALIGN), ("nhwc: out stride", dict(out_layout=1, out_sn=1026), ALIGN),
        ("16-bit: out pointer", dict(out_layout=2, out=A4), ALIGN), ("16-bit: out stride", dict(out_layout=3, out_sn=1026), ALIGN),
        ("2^31 tiles", dict(N=65536, H=2048, W=4096), DIMS)],
    "itermvs_conv3x3_conv1x1": [
        ("x null", dict(x=None), NULL), ("w0 null", dict(w0_tile=None), NULL), ("w1 null", dict(w1_packed=None), NULL), ("out null", dict(out=None), NULL),
        ("weight_format 1", dict(weight_format=1), LAYOUT), ("B 0", dict(B=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS),
        ("NO 0", dict(NO=0), CHANNELS), ("NO 193", dict(NO=193), CHANNELS),
        ("w0 pointer", dict(w0_tile=A4), ALIGN), ("w1 pointer", dict(w1_packed=A8), ALIGN), ("bias pointer", dict(bias1=A4), ALIGN),
        ("32 H W = 2^31", dict(H=8192, W=8192), DIMS), ("2^31 tiles", dict(B=32768, H=65536, W=16), DIMS)],
    "itermvs_gru_conv": [
        ("x null", dict(x=None), NULL), ("w null", dict(w_packed=None), NULL), ("h null", dict(h=None), NULL), ("out null", dict(out=None), NULL),
        ("mode 2", dict(mode=2), DIMS), ("mode -1", dict(mode=-1), DIMS), ("mode 0 without out2", dict(out2=None), NULL), ("mode 1 without z", dict(mode=1, z=None), NULL),
        ("B 0", dict(B=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS),
        ("43 H W 4 > 2^29", dict(H=2048, W=2048), DIMS), ("w pointer", dict(w_packed=A8), ALIGN),
        ("2^31 tiles", dict(B=32768, H=65536, W=16), DIMS)],
    "itermvs_down_conv": [
        ("x null", dict(x=None), NULL), ("w null", dict(w_packed=None), NULL), ("y null", dict(y=None), NULL), ("sc null", dict(sc=None), NULL),
        ("N 0", dict(N=0), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS), ("H 4096", dict(H=4096), DIMS), ("W 4096", dict(W=4096), DIMS),
        ("Cin 48", dict(Cin=48), CHANNELS), ("16 -> 48", dict(C=48), CHANNELS), ("32 -> 32", dict(Cin=32), CHANNELS),
        ("Cin H W 4 > 2^30", dict(Cin=32, C=48, H=4095, W=4095), DIMS), ("w pointer", dict(w_packed=A4), ALIGN),
        ("2^31 tiles CHANGED", dict(N=32768, H=4095, W=4095), DIMS)],     # (before: ERR_LAUNCH without a device, the attribute came first)
    "itermvs_head_fused": HEAD + [("w0_format 1", dict(w0_format=1), LAYOUT), ("w0_format 3 with fp32 last layer", dict(w0_format=3), LAYOUT), HEAD_TILES],
    "itermvs_head_fused_conf": HEAD + [("wc null", dict(wc_tile=None), NULL), ("conf_dot null", dict(conf_dot=None), NULL), ("conf null", dict(conf=None), NULL),
                                       ("wc pointer", dict(wc_tile=A8), ALIGN), HEAD_TILES],
    "itermvs_head_regress": [("x null", dict(x=None), NULL), ("w1 null", dict(w1_packed=None), NULL), ("w2 null", dict(w2_packed=None), NULL),
                             ("bias2 null", dict(bias2=None), NULL), ("B 0", dict(B=0), DIMS), ("P 0", dict(P=0), DIMS)],
    "itermvs_corrnet": CORRNET,
    "itermvs_corrnet_bf16x3": CORRNET,
    "itermvs_stem": [
        ("x null", dict(x=None), NULL), ("w0 null", dict(w0=None), NULL), ("w1 null", dict(w1=None), NULL), ("y null", dict(y=None), NULL), ("sc null", dict(sc=None), NULL),
        ("M -1", dict(M=-1), DIMS), ("H 0", dict(H=0), DIMS), ("W 0", dict(W=0), DIMS),
        ("out_layout 2", dict(out_layout=2), LAYOUT), ("out_layout -1", dict(out_layout=-1), LAYOUT),
        ("nhwc: y pointer", dict(out_layout=1, y=A4), ALIGN), ("nhwc: sc pointer", dict(out_layout=1, sc=A8), ALIGN), ("nhwc: stride", dict(out_layout=1, out_sn=1026), ALIGN),
        ("2^31 tiles", dict(M=2 ** 30, H=18, W=16), DIMS)],
}
ALL = [(fn, name, broken, status) for fn, cases in CASES.items() for name, broken, status in cases]


def test_every_entry_point_and_argument_is_covered():
    from itermvs_amd import _lib
    assert set(CASES) == set(VALID)
    for fn, args in VALID.items():
        assert len(_lib.PROTOTYPES[fn][1]) == len(args), fn
        assert all(set(b) <= set(args) for _, b, _ in CASES[fn]), fn


@pytest.mark.parametrize("fn,name,broken,status", ALL, ids=[f"{c[0][8:]}: {c[1]}" for c in ALL])
def test_one_broken_argument(fn, name, broken, status):
    from itermvs_amd import _lib
    lib = _lib.load()
    assert broken, "a fully valid list is never passed"
    args = dict(VALID[fn], **broken)
    assert getattr(lib, fn)(*args.values()) == status

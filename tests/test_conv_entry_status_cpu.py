"""Error statuses of itermvs_conv2d: every case starts from a valid parameter block in HOST memory and breaks exactly one thing.
The calls go through itermvs_conv2d_plan (the same validation and kernel choice, no device call); because every expected status
is a rejection that precedes any launch, itermvs_conv2d itself is then called with the same block and must answer the same.  A
fully valid block is never passed to itermvs_conv2d.  The expected statuses are those itermvs_conv2d returned before its checks,
its argument fill and its kernel choice were gathered into conv_plan.hpp (98 cases: every check of the entry point and every
"not covered" answer of conv_tile, deconv and conv_tile3; the direct and conv_mfma back ends cover every shape)."""
import ctypes as C

import pytest

NULL, DIMS, ALIGN, LAYOUT = -1, -2, -5, -6
_BUF = (C.c_float * 64)()
ADDR = (C.addressof(_BUF) + 15) // 16 * 16

# valid starting blocks: scalar fields and which pointers are set
TILE = dict(n_seg=1, N=1, Cin=16, Hin=8, Win=8, Cout=16, ksize=3, stride=1, pad=1, dilation=1, transposed=0, act=1, weight_format=2,
            add_mode=0, out_layout=0, split_cout=0, act_b=0, in_layout=0, inp=1, out=1, w0=1, w1=0, out2=0, add=0, aux1=0, aux2=0, out_b=0, in_sn=1024)
TILE3 = dict(TILE, weight_format=3)
MFMA = dict(TILE, weight_format=1)
DIRECT = dict(TILE, weight_format=0)
DOT = dict(TILE, act=6, aux1=1)
SPLIT = dict(TILE, Cout=48, split_cout=16, act_b=2, out_b=1)
NHWC_IN = dict(TILE3, Cin=8, in_layout=1)                 # the tap-pair form with channels-last input
NHWC_OUT = dict(TILE, act=0, out_layout=1)
UP2 = dict(MFMA, ksize=1, pad=0, act=0, add_mode=1, add=1, Cout=48)
DECONV = dict(TILE, transposed=1, stride=2)

CASES = [
    # ---- the checks of the entry point, in their order
    ("in null", TILE, dict(inp=0), NULL), ("out null", TILE, dict(out=0), NULL), ("weight null", TILE, dict(w0=0), NULL),
    ("N 0", TILE, dict(N=0), DIMS), ("Cin 0", TILE, dict(Cin=0), DIMS), ("Cout 0", TILE, dict(Cout=0), DIMS),
    ("Hin 0", TILE, dict(Hin=0), DIMS), ("Win 0", TILE, dict(Win=0), DIMS),
    ("ksize 2", TILE, dict(ksize=2), DIMS), ("ksize 5", MFMA, dict(ksize=5), DIMS),
    ("n_seg 0", TILE, dict(n_seg=0), DIMS), ("n_seg 4", TILE, dict(n_seg=4), DIMS), ("act -1", TILE, dict(act=-1), DIMS), ("act 8", TILE, dict(act=8), DIMS),
    ("dot: no aux1", DOT, dict(aux1=0), DIMS), ("dot: add", DOT, dict(add=1), DIMS), ("dot: out2", DOT, dict(out2=1), DIMS),
    ("dot: out_layout", DOT, dict(out_layout=1), DIMS), ("dot: Cout 48", DOT, dict(Cout=48), DIMS), ("dot: format 1", DOT, dict(weight_format=1), DIMS),
    ("dot: 1x1", DOT, dict(ksize=1, pad=0), DIMS), ("dot: split", DOT, dict(Cout=32, split_cout=16, out_b=1), DIMS),
    ("dot: transposed", DOT, dict(transposed=1, stride=2), DIMS), ("dot: two segments", DOT, dict(n_seg=2, w1=1), DIMS),
    ("act 4: no aux1", TILE, dict(act=4), NULL), ("act 5: no aux1", TILE, dict(act=5, aux2=1), NULL), ("act 5: no aux2", TILE, dict(act=5, aux1=1), NULL),
    ("sigmoid + add", TILE, dict(act=2, add=1), DIMS),
    ("add_mode -1", TILE, dict(add_mode=-1), DIMS), ("add_mode 2", TILE, dict(add_mode=2), DIMS),
    ("out_layout -1", TILE, dict(out_layout=-1), DIMS), ("out_layout 4", TILE, dict(out_layout=4), DIMS),
    ("in_layout 2", TILE, dict(in_layout=2), LAYOUT), ("in_layout -1", TILE, dict(in_layout=-1), LAYOUT),
    ("nhwc in: format 2", NHWC_IN, dict(weight_format=2), LAYOUT), ("nhwc in: 1x1", NHWC_IN, dict(ksize=1, pad=0), LAYOUT),
    ("nhwc in: Cin 16", NHWC_IN, dict(Cin=16), LAYOUT), ("nhwc in: stride 2", NHWC_IN, dict(stride=2), LAYOUT),
    ("nhwc in: dilation 2", NHWC_IN, dict(dilation=2, pad=2), LAYOUT), ("nhwc in: transposed", NHWC_IN, dict(transposed=1), LAYOUT),
    ("nhwc in: pointer", NHWC_IN, dict(inp=2), ALIGN), ("nhwc in: batch stride", NHWC_IN, dict(in_sn=514), ALIGN),
    ("split: format 1", SPLIT, dict(weight_format=1), DIMS), ("split: transposed", SPLIT, dict(transposed=1, stride=2), DIMS),
    ("split: out_layout", SPLIT, dict(out_layout=1, act=0), DIMS), ("split: add", SPLIT, dict(add=1), DIMS), ("split: out2", SPLIT, dict(out2=1), DIMS),
    ("split 8", SPLIT, dict(split_cout=8), DIMS), ("split = Cout", SPLIT, dict(split_cout=48), DIMS), ("split 24", SPLIT, dict(split_cout=24), DIMS),
    ("split: no out_b", SPLIT, dict(out_b=0), DIMS), ("split: act_b -1", SPLIT, dict(act_b=-1), DIMS), ("split: act_b 5", SPLIT, dict(act_b=5), DIMS),
    ("split: act 5", SPLIT, dict(act=5, aux1=1, aux2=1), DIMS), ("split: act_b 4 without aux1", SPLIT, dict(act_b=4), NULL),
    ("nhwc out: format 0", NHWC_OUT, dict(weight_format=0), DIMS), ("nhwc out: transposed", NHWC_OUT, dict(transposed=1, stride=2), DIMS),
    ("nhwc out: relu", NHWC_OUT, dict(act=1), DIMS), ("nhwc out: add", NHWC_OUT, dict(add=1), DIMS), ("nhwc out: Cout 18", NHWC_OUT, dict(Cout=18), DIMS),
    ("up2: no add", UP2, dict(add=0), DIMS), ("up2: format 0", UP2, dict(weight_format=0), DIMS), ("up2: relu", UP2, dict(act=1), DIMS),
    ("up2: transposed", dict(UP2, weight_format=2, ksize=3, pad=1), dict(transposed=1, stride=2), DIMS),
    ("second weight set null", TILE, dict(n_seg=2), NULL),
    ("transposed: format 0", DECONV, dict(weight_format=0), DIMS), ("transposed: format 1", DECONV, dict(weight_format=1), DIMS),
    ("transposed: format 3", DECONV, dict(weight_format=3), DIMS),
    ("stride 0", TILE, dict(stride=0), DIMS), ("dilation 0", MFMA, dict(dilation=0), DIMS), ("pad -1", DIRECT, dict(pad=-1), DIMS),
    ("Hout 0", TILE, dict(Hin=1, pad=0), DIMS), ("Wout 0", MFMA, dict(Win=2, pad=0), DIMS),
    ("up2: odd Hout", UP2, dict(Hin=7), DIMS), ("up2: odd Wout", UP2, dict(Win=7), DIMS),
    # ---- "not covered" answers of the back ends
    ("deconv: 1x1", DECONV, dict(ksize=1), DIMS), ("deconv: stride 1", DECONV, dict(stride=1), DIMS), ("deconv: pad 0", DECONV, dict(pad=0), DIMS),
    ("deconv: sigmoid", DECONV, dict(act=2), DIMS), ("deconv: Cin 4", DECONV, dict(Cin=4), DIMS), ("deconv: Cin 48", DECONV, dict(Cin=48), DIMS),
    ("deconv: Cout 48", DECONV, dict(Cout=48), DIMS),
    ("tile: 1x1", TILE, dict(ksize=1, pad=0), DIMS), ("tile: stride 3", TILE, dict(stride=3), DIMS), ("tile: stride 2 + dilation 2", TILE, dict(stride=2, dilation=2), DIMS),
    ("tile: Cin 3 at stride 2", TILE, dict(Cin=3, stride=2), DIMS), ("tile: Cin 8 at dilation 2", TILE, dict(Cin=8, dilation=2, pad=2), DIMS),
    ("tile: weights exceed LDS", TILE, dict(Cin=128), DIMS), ("tile: dot block exceeds LDS", DOT, dict(Cin=64, Cout=32), DIMS),
    ("tile3: Cin 4", TILE3, dict(Cin=4), DIMS), ("tile3: 1x1", TILE3, dict(ksize=1, pad=0), DIMS), ("tile3: stride 3", TILE3, dict(stride=3), DIMS),
    ("tile3: dilation 3", TILE3, dict(dilation=3, pad=3), DIMS), ("pair: stride 2", TILE3, dict(Cin=8, stride=2), DIMS),
    ("pair: dilation 2", TILE3, dict(Cin=5, dilation=2, pad=2), DIMS), ("pair: split", dict(SPLIT, weight_format=3), dict(Cin=8), DIMS),
    ("tile3: weights exceed LDS", TILE3, dict(Cin=128, Cout=16), DIMS),
    ("tile3: dot block exceeds LDS", dict(DOT, weight_format=3), dict(Cin=64, Cout=32, stride=2), DIMS),
]


def make_params(spec):
    from itermvs_amd import _lib
    p = _lib.ConvParams()
    for k, v in spec.items():
        if k in ("inp", "out", "out2", "add", "aux1", "aux2", "out_b"):
            setattr(p, k, ADDR + 4 * (v - 1) if v else None)       # 2: set, but not 16-byte aligned
        elif k in ("w0", "w1"):
            p.weight[int(k[1])] = ADDR if v else None
        else:
            setattr(p, k, v)
    p.out_sn = spec["Cout"] * spec["Hin"] * spec["Win"]
    return p


def test_null_arguments():
    from itermvs_amd import _lib
    lib = _lib.load()
    plan = _lib.ConvPlan()
    assert lib.itermvs_conv2d_plan(None, C.byref(plan)) == NULL
    assert lib.itermvs_conv2d_plan(C.byref(make_params(TILE)), None) == NULL
    assert lib.itermvs_conv2d(None, None) == NULL


def test_the_starting_blocks_are_valid():
    from itermvs_amd import _lib
    lib = _lib.load()
    for name, spec, backend in (("TILE", TILE, "tile"), ("TILE3", TILE3, "tile3"), ("MFMA", MFMA, "mfma_splitk"), ("DIRECT", DIRECT, "direct"),
                                ("DOT", DOT, "tile"), ("SPLIT", SPLIT, "tile"), ("NHWC_IN", NHWC_IN, "tile3_pair"), ("NHWC_OUT", NHWC_OUT, "tile"),
                                ("UP2", UP2, "lateral_up2"), ("DECONV", DECONV, "deconv")):
        plan = _lib.ConvPlan()
        assert lib.itermvs_conv2d_plan(C.byref(make_params(spec)), C.byref(plan)) == 0, name
        assert _lib.ConvPlan.BACKENDS[plan.backend] == backend, (name, str(plan))


@pytest.mark.parametrize("name,start,broken,status", CASES, ids=[c[0] for c in CASES])
def test_one_broken_field(name, start, broken, status):
    from itermvs_amd import _lib
    lib = _lib.load()
    p = make_params(dict(start, **broken))
    plan = _lib.ConvPlan()
    got = lib.itermvs_conv2d_plan(C.byref(p), C.byref(plan))
    assert got == status, (name, got, str(plan) if got == 0 else "")
    assert lib.itermvs_conv2d(C.byref(p), None) == status         # rejected before any launch (the plan just said so)

"""Error statuses of the six fused correlation entry points (itermvs_corr_iter, _iter_slots, _init, _init_slots,
_iter_backward, _init_backward): every case starts from a valid parameter block in HOST memory and breaks exactly one thing.
Validation precedes any launch, so the calls are safe without a GPU; a fully valid block is never passed.  The expected
statuses are those the entry points returned before their checks were gathered into shared functions."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

NULL, DIMS, CHANNELS, VIEWS, ALIGN, LAYOUT, DTYPE = -1, -2, -3, -4, -5, -6, -8
S = 2


def valid_blocks():
    from itermvs_amd import _lib
    v = SimpleNamespace(lib=_lib.load(), F16=_lib.F16)
    v.buf = (C.c_float * 64)()
    a = v.a = (C.addressof(v.buf) + 15) // 16 * 16
    v.slots = (_lib.LevelSlots * 3)()
    q = v.q = _lib.CorrIterParams()
    q.B, q.S, q.H, q.W = 1, S, 4, 4
    q.ref_q = q.proj = q.view_w = q.inv_depth_min = q.inv_depth_max = q.norm_depth = a
    for i, c in enumerate((16, 32, 48)):
        for s in (v.slots[i], q.src[i]):
            s.C, s.H, s.W, s.dtype = c, 4, 4, _lib.F32
            s.sc, s.sx, s.sy = 1, c, 4 * c
        v.slots[i].slab, v.slots[i].slot, v.slots[i].n_slots, v.slots[i].slot_stride = a, a, 4, 16 * c
        q.src[i].sb = 16 * c
        q.src[i].view[0] = q.src[i].view[1] = a
        q.N[i], q.out[i] = (4, 4, 2)[i], a
    p = v.p = _lib.CorrInitParams()
    p.B, p.S, p.H, p.W, p.N = 1, S, 4, 4, 32
    p.src = q.src[2]
    p.ref.data, p.ref.C, p.ref.H, p.ref.W, p.ref.dtype = a, 48, 4, 4, _lib.F32
    p.ref.sc, p.ref.sx, p.ref.sy, p.ref.sb = 1, 48, 192, 768
    p.proj = p.inv_depth_min = p.inv_depth_max = p.out = a
    # gradient arguments
    v.go = (C.c_void_p * 3)(a, a, a)
    v.gsrc = [(C.c_void_p * S)(a, a) for _ in range(3)]
    v.gs = (C.POINTER(C.c_void_p) * 3)(*[C.cast(g, C.POINTER(C.c_void_p)) for g in v.gsrc])
    v.args = {"q": C.byref(q), "p": C.byref(p), "slots": v.slots, "slot3": C.byref(v.slots[2]), "go": C.byref(v.go),
              "gs": C.byref(v.gs), "gref": a, "gout3": a, "gsrc3": v.gsrc[2]}
    return v


CALLS = {
    "iter": lambda v, k: v.lib.itermvs_corr_iter(k["q"], None),
    "iter_slots": lambda v, k: v.lib.itermvs_corr_iter_slots(k["q"], k["slots"], None),
    "init": lambda v, k: v.lib.itermvs_corr_init(k["p"], None),
    "init_slots": lambda v, k: v.lib.itermvs_corr_init_slots(k["p"], k["slot3"], None),
    "iter_backward": lambda v, k: v.lib.itermvs_corr_iter_backward(k["q"], k["go"], k["gs"], k["gref"], None),
    "init_backward": lambda v, k: v.lib.itermvs_corr_init_backward(k["p"], k["gout3"], k["gsrc3"], k["gref"], None),
}
ITER, INIT = ("iter", "iter_slots", "iter_backward"), ("init", "init_slots", "init_backward")
DIRECT, SLOT = ("iter", "init", "iter_backward", "init_backward"), ("iter_slots", "init_slots")


def level(v, entry):
    """the one level description ``entry`` reads for level 3 (the only level of the initialisation branch)"""
    return v.slots[2] if entry in SLOT else (v.q.src[2] if entry in ITER else v.p.src)


def params(v, entry):
    return v.q if entry in ITER else v.p


def arg(name, value):
    return lambda v, e: v.args.__setitem__(name, value)


def stride_field(entry):
    return "slot_stride" if entry in SLOT else "sb"


def on_level(**kw):
    """set fields of the level description; ``stride`` = the batch or slot stride; a callable gets the description"""
    def f(v, e):
        L = level(v, e)
        for k, x in kw.items():
            setattr(L, stride_field(e) if k == "stride" else k, x(L) if callable(x) else x)
    return f


def on_params(**kw):
    def f(v, e):
        for k, x in kw.items():
            setattr(params(v, e), k, x)
    return f


def half(v, e):
    """a valid fp16 block (strides stay multiples of 8) whose level-3 column stride is then a multiple of 4 only"""
    for s in list(v.slots) + list(v.q.src) + [v.p.src, v.p.ref]:
        s.dtype = v.F16
    L = level(v, e)
    L.sx, L.sy = L.C + 4, 4 * (L.C + 4) + 4
    setattr(L, stride_field(e), 4 * L.sy + 8)


def too_large(v, e):
    """H * sy * 4 bytes reach 2^32 (slots still do not overlap)"""
    L = level(v, e)
    L.H = 1 << 24
    setattr(L, stride_field(e), L.H * L.sy)


CASES = []


def case(entries, name, mutate, *expected):
    """one fault for each of ``entries``; ``expected``: one status for all, or one per entry"""
    for i, e in enumerate(entries):
        CASES.append(pytest.param(e, mutate, expected[i if len(expected) > 1 else 0], id=f"{e}-{name}"))


ALL = ITER + INIT
# the rules both level forms share
case(ALL, "channels", lambda v, e: (on_level(C=20, sx=20, sy=80, stride=320)(v, e), setattr(v.p.ref, "C", 20)), CHANNELS)
case(ALL, "level-H", on_level(H=0), DIMS)
case(ALL, "level-W", on_level(W=0), DIMS)
case(ALL, "channels-last", on_level(sc=2), LAYOUT)
case(ALL, "level-dtype", on_level(dtype=3), DTYPE)
case(ALL, "sx-align", on_level(sx=lambda L: L.C + 2), ALIGN)
case(ALL, "sy-align", on_level(sy=lambda L: L.sy + 2), ALIGN)
case(ALL, "stride-align", on_level(stride=lambda L: 16 * L.C + 2), ALIGN)
case(ALL, "16bit-align", half, ALIGN)
case(ALL, "byte-offsets", too_large, DIMS)
# direct form
case(DIRECT, "view-null", lambda v, e: level(v, e).view.__setitem__(1, None), NULL)
case(DIRECT, "view-align", lambda v, e: level(v, e).view.__setitem__(1, v.a + 4), ALIGN)
case(DIRECT, "sx-zero", on_level(sx=0), DIMS)
case(DIRECT, "sy-zero", on_level(sy=0), DIMS)
# slot form
case(SLOT, "slab-null", on_level(slab=None), NULL)
case(SLOT, "table-null", on_level(slot=None), NULL)
case(SLOT, "n_slots", on_level(n_slots=0), DIMS)
case(SLOT, "slab-align", lambda v, e: setattr(level(v, e), "slab", v.a + 4), ALIGN)
case(SLOT, "overlap", on_level(slot_stride=lambda L: 4 * L.sy - 4), LAYOUT)
case(SLOT, "sx-below-C", on_level(sx=lambda L: L.C - 4), LAYOUT)
case(SLOT, "sy-below-row", on_level(sy=lambda L: 4 * L.sx - 4), LAYOUT)
# parameter blocks
case(ITER, "p-null", arg("q", None), NULL)
case(INIT, "p-null", arg("p", None), NULL)
case(("iter_slots",), "src-null", arg("slots", None), NULL)
case(("init_slots",), "src-null", arg("slot3", None), NULL)
for f in ("B", "H", "W"):
    case(ALL, f + "-zero", on_params(**{f: 0}), DIMS)
case(ALL, "S-zero", on_params(S=0), VIEWS)
case(ALL, "S-17", on_params(S=17), VIEWS)
for f in ("ref_q", "proj", "view_w", "inv_depth_min", "inv_depth_max"):
    case(ITER, f + "-null", on_params(**{f: None}), NULL)
for f in ("proj", "inv_depth_min", "inv_depth_max"):
    case(INIT, f + "-null", on_params(**{f: None}), NULL)
case(("iter", "iter_slots"), "ref_q-align", lambda v, e: setattr(v.q, "ref_q", v.a + 4), ALIGN)
case(ITER, "N-zero", lambda v, e: v.q.N.__setitem__(1, 0), DIMS)
case(ITER, "N-9", lambda v, e: v.q.N.__setitem__(2, 9), DIMS)
case(("iter", "iter_slots"), "out-null", lambda v, e: v.q.out.__setitem__(1, None), NULL)
case(ITER, "no-hypotheses", on_params(norm_depth=None), NULL)
case(ITER, "view_w-ss-zero", on_params(view_w_sb=32, view_w_ss=0, view_w_sp=1), LAYOUT)
case(ITER, "view_w-sp-zero", on_params(view_w_sb=32, view_w_ss=16, view_w_sp=0), LAYOUT)
case(ITER, "view_w-sb-negative", on_params(view_w_sb=-32, view_w_ss=16, view_w_sp=1), LAYOUT)
case(("iter_backward",), "view_w-interleaved", on_params(view_w_sb=32, view_w_ss=1, view_w_sp=2), LAYOUT)
case(("iter_backward",), "view_w-batch-stride", on_params(view_w_sb=64, view_w_ss=16, view_w_sp=1), LAYOUT)
case(("iter", "iter_slots"), "impl", on_params(impl=1), DIMS)
case(ITER, "dtype-differs", lambda v, e: [setattr(s, "dtype", v.F16) for s in (v.slots[1], v.q.src[1])], DTYPE)
case(INIT, "N-1", on_params(N=1), DIMS)
case(INIT, "ref-null", lambda v, e: setattr(v.p.ref, "data", None), NULL)
case(("init", "init_slots"), "out-null", on_params(out=None), NULL)
for f in ("C", "H", "W"):
    case(INIT, "ref-" + f, lambda v, e, f=f: setattr(v.p.ref, f, 8), DIMS, DIMS, LAYOUT)
case(INIT, "ref-dtype", lambda v, e: setattr(v.p.ref, "dtype", v.F16), DTYPE)
case(("init", "init_slots"), "out_layout-2", on_params(out_layout=2), LAYOUT)
case(("init", "init_slots"), "groups-last-align", lambda v, e: (setattr(v.p, "out_layout", 1), setattr(v.p, "out", v.a + 4)), ALIGN)
# what only the gradient entry points ask
for name in ("go", "gs", "gref"):
    case(("iter_backward",), name + "-null", arg(name, None), NULL)
case(("iter_backward",), "grad_out-level-null", lambda v, e: v.go.__setitem__(1, None), NULL)
case(("iter_backward",), "grad_src-level-null", lambda v, e: v.gs.__setitem__(1, C.POINTER(C.c_void_p)()), NULL)
case(("iter_backward",), "grad_src-view-null", lambda v, e: v.gsrc[1].__setitem__(1, None), NULL)
for name in ("gout3", "gsrc3", "gref"):
    case(("init_backward",), name + "-null", arg(name, None), NULL)
case(("init_backward",), "grad_src-view-null", lambda v, e: v.gsrc[2].__setitem__(1, None), NULL)
case(("init_backward",), "out_layout-1", on_params(out_layout=1), LAYOUT)
case(("init_backward",), "N-33", on_params(N=33), DIMS)
case(("init_backward",), "ref-channels-last", lambda v, e: setattr(v.p.ref, "sc", 2), LAYOUT)
case(("init_backward",), "ref-sx-align", lambda v, e: setattr(v.p.ref, "sx", 50), ALIGN)
case(("init_backward",), "ref-data-align", lambda v, e: setattr(v.p.ref, "data", v.a + 4), ALIGN)


@pytest.mark.parametrize("entry,mutate,expected", CASES)
def test_one_fault_status(entry, mutate, expected):
    if torch.cuda.is_available():
        pytest.skip("host pointers: only where nothing can be launched")
    v = valid_blocks()
    mutate(v, entry)
    assert CALLS[entry](v, v.args) == expected

"""The depth and confidence head kernels of itermvs_amd/csrc/head.hip (itermvs_head_regress, itermvs_head_fused in its fp32,
bf16x3 and bf16x3_all arithmetic, itermvs_head_fused_conf with either w2 form) against the float64 restatement of
tests/head_reference.py, per pixel: maps narrower than a tile and lower than the halo, last tiles of one to three pixels,
consecutive tiles in different batch items, every regime of the tile walk, the engine's strided layouts, designed weights
with a closed form.  Needs an MI355X: run with ``-m gpu``.

Every pixel is asserted (``head_reference.check_depth``).  A pixel is *undecided* when the two largest float64 logits differ
by at most 8 x floor of the logits and are not equal; there the kernel may have either bin, and its nd must be that of the
window around the bin it has.  Everywhere else the arg-max is exact.

Bounds.  floor = max |fp32 CPU restatement - fp64 reference| on the very inputs of the case (the restatement is the reference
function run in float32), bound = max(2e-6, 4 x floor) -- ``update_tail_reference.bound``; 2e-6 is the loosest bound
tests/test_kernels_gpu.py asserts on nd (test_head_regress_fused_matches_chain) and its bound on the confidence
(test_head_fused_with_confidence_head).  tests/test_head_reference_cpu.py prints the floors; those measured on an x86-64 host
(torch CPU) are listed in each test's docstring.  No number comes from a kernel's output."""
import functools

import pytest
import torch

import head_reference as H
import update_tail_reference as R
import walk_shapes

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.25
FUSED_FORMS = ["fp32", "bf16x3", "bf16x3_all", "conf_fp32", "conf_bf16x3"]
LAYOUTS = ["plain", "slice43", "every_other"]


def ops():
    from itermvs_amd import ops as _ops
    return _ops


def cu(t):
    return t.to(DEV)


def lay_hidden(x: torch.Tensor, kind: str) -> torch.Tensor:
    """the CPU tensor [B,32,H,W] on the device: stand-alone, as the first 32 channels of a 43-channel buffer (the engine's GRU
    buffer: batch stride 43 P) or as every other item of a [2B,32,H,W] buffer; what does not belong to it holds 7"""
    b, c, h, w = x.shape
    if kind == "plain":
        return cu(x).contiguous()
    if kind == "slice43":
        big = torch.full((b, 43, h, w), 7.0, device=DEV)
        big[:, :c] = cu(x)
        return big[:, :c]
    assert kind == "every_other"
    big = torch.full((2 * b, c, h, w), 7.0, device=DEV)
    big[::2] = cu(x)
    return big[::2]


def sentinel_buffer(shape):
    return torch.full(shape, SENTINEL, device=DEV)


def untouched(buf: torch.Tensor, written) -> bool:
    keep = [c for c in range(buf.shape[1]) if c not in written]
    return torch.equal(buf[:, keep], torch.full_like(buf[:, keep], SENTINEL))


class Packed:
    """the device operands of one set of weights, per form"""

    def __init__(self, w, b2_run):
        o = ops()
        self.b2 = cu(b2_run).contiguous()
        self.w0_fp32 = o.MfmaWeight(cu(w["w0"]), split3=False)
        self.w0_split = o.pack_head_w0_split3(cu(w["w0"]))
        self.a1, self.a2_fp32 = o.pack_head_weights(cu(w["w1"]), cu(w["w2"]))
        self.a2_split = o.pack_head_w2_split3(cu(w["w2"]))
        self.wc = o.MfmaWeight(cu(w["c0"]), split3=False)
        self.cdot = torch.cat([cu(w["c2w"]).reshape(-1), cu(w["c2b"]).reshape(-1)]).contiguous()

    def fused(self, hidden, form, conf=None, **kw):
        w0 = self.w0_split if form == "bf16x3_all" else self.w0_fp32
        a2 = self.a2_fp32 if form in ("fp32", "conf_fp32") else self.a2_split
        if form.startswith("conf"):
            kw["conf"] = (self.wc, self.cdot, conf)
        return ops().head_fused(hidden, w0, self.a1, a2, self.b2, **kw)

    def regress(self, x, **kw):
        return ops().head_regress(x, self.a1, self.a2_fp32, self.b2, **kw)


def judge(nd, best, ref, tag):
    """print the figures, then assert every pixel"""
    ok = ~ref["undecided"]
    err = R.maxdiff(nd.cpu()[ok], ref["nd"][ok])
    wrong = int((best.cpu() != ref["best"])[ok].sum())
    print(f"head {tag}: nd err {err:.3e} (bound, floor) {ref['nd_bound']}; arg-max differs at {wrong} decided pixels; "
          f"undecided {int((~ok).sum())} of {ok.numel()}; logit floor {ref['logit_floor']:.2e}")
    assert nd.dtype == torch.float32
    H.check_depth(nd, best, ref)


def conditions(shape, ref):
    """the input conditions tests/test_head_reference_cpu.py pins, on the shape this device gives"""
    share = float(ref["undecided"].double().mean())
    assert share == 0.0 if shape[1] * shape[2] <= 256 else share <= 0.01
    assert ref["best32_ok"]


def run_fused_form(hidden_d, pk, form, ref, tag):
    """one fused form on one device tensor: result against the reference, the rider's confidence and its bit-identical depth
    outputs, a second launch with the same bits -> (nd, best)"""
    b, _, h, w = hidden_d.shape
    if form.startswith("conf"):
        conf = sentinel_buffer((b, 1, h, w))
        nd, best = pk.fused(hidden_d, form, conf, want_best=True)
        plain, plain_best = pk.fused(hidden_d, form[5:], want_best=True)
        e_c = R.maxdiff(conf, ref["conf"])
        print(f"head {tag}: confidence err {e_c:.3e} (bound, floor) {ref['conf_bound']}")
        assert torch.equal(nd, plain) and torch.equal(best, plain_best), tag          # the rider leaves the depth outputs alone
        assert e_c <= ref["conf_bound"][0], tag
        conf2 = sentinel_buffer((b, 1, h, w))
        nd2, best2 = pk.fused(hidden_d, form, conf2, want_best=True)
        assert torch.equal(conf2, conf), tag
    else:
        nd, best = pk.fused(hidden_d, form, want_best=True)
        nd2, best2 = pk.fused(hidden_d, form, want_best=True)
    judge(nd, best, ref, tag)
    assert torch.equal(nd2, nd) and torch.equal(best2, best), tag                     # deterministic
    return nd, best


def check_destinations(hidden_d, pk, form, nd, tag):
    """nd into channel 3 of a 5-channel buffer and channel 32 of a 43-channel one (different batch strides), both pre-filled
    with a sentinel that every other channel must still hold; the copies equal the stand-alone result bit for bit"""
    b, _, h, w = hidden_d.shape
    small, wide = sentinel_buffer((b, 5, h, w)), sentinel_buffer((b, 43, h, w))
    conf = sentinel_buffer((b, 1, h, w)) if form.startswith("conf") else None
    got, best = pk.fused(hidden_d, form, conf, nd_out=[(small, 3), (wide, 32)])
    assert got is None and best is None
    assert torch.equal(small[:, 3:4], nd) and torch.equal(wide[:, 32:33], nd), tag
    assert untouched(small, [3]) and untouched(wide, [32]), tag
    wide2 = sentinel_buffer((b, 43, h, w))
    pk.fused(hidden_d, form, conf, nd_out=[(wide2, 32)])
    assert torch.equal(wide2, wide), tag


@functools.lru_cache(maxsize=None)
def packed_case(shape, kind="random", arg=0):
    hidden, w, ref = H.fused_case(shape, kind, arg)
    return hidden, Packed(w, ref["b2_run"]), ref


def fused_shape(name):
    if not isinstance(name, str):
        return name
    shape = H.device_shape(name)
    if name == H.CROSS:          # more tiles than resident workgroups, split over two images: a second tile in the next item
        resident = 2 * torch.cuda.get_device_properties(0).multi_processor_count
        assert shape[0] == 2 and 2 * shape[1] * ((shape[2] + 15) // 16) == resident + 4
    return shape


# ------------------------------------------------------------------------------------------------------------------------
# a. the fused kernel, random weights
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.FUSED_SHAPES + list(walk_shapes.REGIMES) + [H.CROSS], ids=str)
def test_head_fused_fp32_against_fp64(shape):
    """itermvs_head_fused, fp32 matrix path, random weights scaled to a logit spread of about 4 and hidden = tanh(randn), in
    the three layouts of ``lay_hidden`` (identical bits in all three), nd into two sentinel buffers, and -- the engine's own
    arrangement -- hidden as channels :32 of the 43-channel buffer whose channel 32 receives nd.
    (1,1,1): one tile with a single live pixel; (1,1,16): one whole tile; in both every halo row and column is outside the map;
    (1,1,17): a last tile of one pixel whose halo is the neighbour's; (1,2,18): two rows, both halo rows outside; (2,3,5),
    (1,5,15): maps narrower than a tile; (3,2,33): three items of small maps; (2,23,37); the regimes of tests/walk_shapes.py
    at two workgroups per CU (on 256 CUs: (1,1,47), (3,1,47), (1,46,175), (1,32,255), (1,103,79)).
    The grid is min(tiles, 2 CUs) workgroups, so only walk:C+3 and ``cross:C+4`` give a workgroup a second tile, fetched while
    the first computes: at walk:C+3 in the same image, at cross:C+4 (head_reference.device_shape; (2,43,95) on 256 CUs: two
    images of 258 tiles) the workgroups 0..3 go from image 0 to image 1 -- the next tile's batch decode with every batch
    stride (hidden, both nd destinations).

    Floors: logits 1.7e-6 .. 1.9e-5 (sums of 288 + 32 + 64 rounded terms); nd at most 4.4e-7 -> bound 2e-6 (the project's) for
    every shape; undecided pixels: none up to (2,23,37), 2 of 8050, 0 of 8160, 3 of 8137 and 0 of 8170 at walk:C-6, walk:C,
    walk:C+3 and cross:C+4."""
    shape = fused_shape(shape)
    hidden, pk, ref = packed_case(shape)
    conditions(shape, ref)
    first = None
    for layout in LAYOUTS:
        hd = lay_hidden(hidden, layout)
        assert layout == "plain" or shape[0] == 1 or hd.stride(0) != 32 * shape[1] * shape[2]
        nd, best = run_fused_form(hd, pk, "fp32", ref, (shape, layout))
        first = first or (nd, best)
        assert torch.equal(nd, first[0]) and torch.equal(best, first[1]), layout
        check_destinations(hd, pk, "fp32", nd, (shape, layout))
    b, h, w = shape
    buf = torch.full((b, 43, h, w), SENTINEL, device=DEV)
    buf[:, :32] = cu(hidden)
    pk.fused(buf[:, :32], "fp32", nd_out=[(buf, 32)])
    assert torch.equal(buf[:, 32:33], first[0]) and torch.equal(buf[:, :32].cpu(), hidden) and untouched(buf, range(33))


@pytest.mark.parametrize("form", FUSED_FORMS[1:])
@pytest.mark.parametrize("shape", H.SUBSET_SHAPES + [(2, 23, 37), "walk:9", "walk:C+3", H.CROSS], ids=str)
def test_head_fused_other_forms_against_fp64(shape, form):
    """the bf16x3 last layer, the bf16x3 3x3 layer as well, and the confidence rider with either w2 form, on the one-pixel last
    tile, the two-row map, the three-item map (3,2,33), (2,23,37), walk:9, walk:C+3 and cross:C+4 (a workgroup's second tile in
    the next batch item: also the rider's batch stride); plain and 43-channel layouts.  The rider's depth outputs equal those
    of the same form without it bit for bit; its confidence lands in a sentinel-filled buffer.

    The bf16x3 forms are held to the fp32 bound: each operand is split EXACTLY into three bf16 terms and the three cross
    products left out (m*l, l*m, l*l) are below 2^-24 |a||b| each, i.e. below the rounding an fp32 product already carries.
    Floors: nd as for the fp32 form (bound 2e-6); confidence at most 5.1e-7 -> 2.05e-6 at walk:C+3 and 2.03e-6 at cross:C+4,
    elsewhere 2e-6 (the project's)."""
    shape = fused_shape(shape)
    hidden, pk, ref = packed_case(shape)
    conditions(shape, ref)
    for layout in ("plain", "slice43"):
        hd = lay_hidden(hidden, layout)
        nd, _ = run_fused_form(hd, pk, form, ref, (shape, form, layout))
        check_destinations(hd, pk, form, nd, (shape, form, layout))


@pytest.mark.parametrize("form", FUSED_FORMS)
def test_head_fused_trained_weights_against_fp64(form):
    """the trained dtu weights at (2,23,37) (logit spread 5.7, logits up to some tens: floor 6.0e-5, 8 of 1702 pixels
    undecided; nd floor 2.1e-7 -> bound 2e-6; confidence floor 2.0e-7 -> 2e-6)"""
    hidden, pk, ref = packed_case(H.TRAINED_SHAPE, "trained")
    conditions(H.TRAINED_SHAPE, ref)
    run_fused_form(lay_hidden(hidden, "slice43"), pk, form, ref, ("trained", form))


# ------------------------------------------------------------------------------------------------------------------------
# b. designed weights through every fused form
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FUSED_FORMS)
def test_head_fused_routing_clamps_slices_and_ties(form):
    """(2,3,21), weights that route a lit channel straight to a bin (exact in every arithmetic: floor 0, nothing undecided):
    single peaks at bins 0..4 and 251..255 (every window clamp) and at 63|64, 127|128, 191|192 (both sides of the borders
    between the four waves' 64-bin slices); exact ties across a slice border, across both clamps, within a slice, with the
    lower bin on the higher channel: the lower bin wins.  nd floor 7.6e-8 -> bound 2e-6."""
    shape = H.DESIGNED_SHAPE
    hidden, pk, ref = packed_case(shape, "routing")
    assert ref["logit_floor"] == 0.0 and not bool(ref["undecided"].any())
    _, best = run_fused_form(lay_hidden(hidden, "slice43"), pk, form, ref, ("routing", form))
    assert torch.equal(best.cpu(), H.routing_hidden(shape)[1])


@pytest.mark.parametrize("form", FUSED_FORMS)
@pytest.mark.parametrize("tap", range(9))
def test_head_fused_single_tap_in_closed_form(tap, form):
    """(2,5,19), w0 = one tap alone, every pixel lighting the channel (x + 5 y + 11 b) % 31 with a value of its own: the arg-max
    is the bin of the pixel at (y + 2 (ky - 1), x + 2 (kx - 1)) and bin 250 where that lies in the zero padding -- the
    dilation, the padding at all four borders, and the halo columns of the 3-pixel last tile and of the first tile that are
    the neighbouring tile's pixels.  Exact logits; nd floor at most 1.8e-7 -> bound 2e-6."""
    shape = H.TAP_SHAPE
    hidden, pk, ref = packed_case(shape, "tap", tap)
    _, best = run_fused_form(lay_hidden(hidden, "every_other"), pk, form, ref, ("tap", tap, form))
    assert torch.equal(best.cpu(), H.tap_wanted_best(shape, tap))


@pytest.mark.parametrize("form", FUSED_FORMS)
@pytest.mark.parametrize("shift", [90.0, -90.0])
def test_head_fused_shifted_bias(shift, form):
    """(2,3,21), b2 on the 2^-12 grid plus / minus 90 (exact in fp32): the soft-max must subtract the maximum; judged by the
    UN-shifted float64 result.  Logits near +-90 carry an fp32 ulp of 7.6e-6: logit floor 5.4e-5, nd floor 1.7e-7 -> bound
    2e-6, nothing undecided."""
    hidden, pk, ref = packed_case(H.SHIFT_SHAPE, "shift", shift)
    conditions(H.SHIFT_SHAPE, ref)
    run_fused_form(lay_hidden(hidden, "slice43"), pk, form, ref, ("shift", shift, form))


# ------------------------------------------------------------------------------------------------------------------------
# c. itermvs_head_regress
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.REGRESS_SHAPES, ids=str)
def test_head_regress_against_fp64(shape):
    """B = 2; P = 1, 63, 64, 65, 33 and 145 pixels (a workgroup handles 64, a wave 16: a lone pixel, one short of a workgroup,
    exactly one, one more, 16 k + 1 within a workgroup and across three); x = the float64 first layer of a random hidden
    state rounded once to fp32, in the three layouts; nd into two sentinel buffers.  At P = 145 also b2 +- 90.
    Floors: logits at most 8.9e-6 (5.4e-5 with the shifted bias); nd at most 3.6e-7 -> bound 2e-6; nothing undecided."""
    b, h, w = shape
    for shift in (0.0, 90.0, -90.0) if shape == H.REGRESS_SHAPES[-1] else (0.0,):
        x, wts, ref = H.regress_case(shape, shift)
        conditions(shape, ref)
        pk = Packed(wts, ref["b2_run"])
        first = None
        for layout in LAYOUTS:
            xd = lay_hidden(x, layout)
            nd, best = pk.regress(xd, want_best=True)
            judge(nd, best, ref, ("regress", shape, shift, layout))
            first = first or (nd, best)
            assert torch.equal(nd, first[0]) and torch.equal(best, first[1]), layout
            nd2, best2 = pk.regress(xd, want_best=True)
            assert torch.equal(nd2, nd) and torch.equal(best2, best)
            small, wide = sentinel_buffer((b, 5, h, w)), sentinel_buffer((b, 43, h, w))
            got, _ = pk.regress(xd, nd_out=[(small, 3), (wide, 32)])
            assert got is None and torch.equal(small[:, 3:4], nd) and torch.equal(wide[:, 32:33], nd)
            assert untouched(small, [3]) and untouched(wide, [32])

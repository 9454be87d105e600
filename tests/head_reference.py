"""Float64 reference for the depth and confidence head kernels of itermvs_amd/csrc/head.hip (itermvs_head_regress,
itermvs_head_fused, itermvs_head_fused_conf): plain torch-on-CPU restatements of models/itermvs.py:121-126, 139-151, 171-219.
The soft-max, the first-max arg-max and the window regression are those of tests/update_tail_reference.py.

Every function takes ``dtype``: float64 is the reference, the same function run in float32 is the "fp32 CPU restatement"
whose distance from the reference is the rounding floor a kernel's bound is derived from (``update_tail_reference.bound``).
The layers are written out as sums that start from the bias and add one input channel (and tap) after the other, which is
what a plain fp32 implementation does: the float32 run then carries one rounding per term, at the magnitude of the running
sum -- also where a bias of +-90 lifts that magnitude.

The case builders of tests/test_head_gpu.py live here too, so that tests/test_head_reference_cpu.py can pin the conditions
on those inputs (spread of the logits, decided arg-max, bins reached) without a GPU.  A case is computed once and never
modified."""
import functools
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

import update_tail_reference as R

F64 = torch.float64
F32 = torch.float32
BINS = R.BINS


# ------------------------------------------------------------------------------------------------------------------------
# the layers
# ------------------------------------------------------------------------------------------------------------------------
def _t(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.detach().cpu().to(dtype)


def conv3x3_dil2(x: torch.Tensor, w: torch.Tensor, dtype=F64) -> torch.Tensor:
    """x [B,C,H,W], w [O,C,3,3] -> [B,O,H,W]: dilation 2, zero padding 2, no bias.  Tap (ky, kx) of output pixel (y, x) reads
    input pixel (y + 2 (ky - 1), x + 2 (kx - 1))."""
    x, w = _t(x, dtype), _t(w, dtype)
    b, c, h, wd = x.shape
    o = w.shape[0]
    xp = F.pad(x, (2, 2, 2, 2))
    acc = torch.zeros((b, o, h, wd), dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, 2 * ky:2 * ky + h, 2 * kx:2 * kx + wd]
            for ci in range(c):
                acc = acc + w[:, ci, ky, kx].view(1, o, 1, 1) * win[:, ci:ci + 1]
    return acc


def conv1x1(x: torch.Tensor, w: torch.Tensor, bias, dtype=F64) -> torch.Tensor:
    """x [B,C,H,W], w [O,C,1,1] (or [O,C]), bias [O] | None -> [B,O,H,W]; the sum starts from the bias"""
    x, w = _t(x, dtype), _t(w, dtype).reshape(w.shape[0], -1)
    b, c, h, wd = x.shape
    o = w.shape[0]
    acc = torch.zeros((b, o, h, wd), dtype=dtype)
    if bias is not None:
        acc = acc + _t(bias, dtype).view(1, o, 1, 1)
    for ci in range(c):
        acc = acc + w[:, ci].view(1, o, 1, 1) * x[:, ci:ci + 1]
    return acc


def first_layer(hidden, w0, dtype=F64) -> torch.Tensor:
    """depth_head[0:2]: relu(conv3x3 dil 2 pad 2), 32 -> 32"""
    return torch.relu(conv3x3_dil2(hidden, w0, dtype))


def head_tail(x, w1, w2, b2, dtype=F64):
    """depth_head[2:5] + regression on x = first_layer(hidden): -> (logits [B,256,H,W], nd [B,1,H,W], best int64 [B,1,H,W])"""
    logits = conv1x1(torch.relu(conv1x1(x, w1, None, dtype)), w2, b2, dtype)
    nd, _, best = R.prob_regress(logits, dtype)
    return logits, nd, best


def depth_head(hidden, w0, w1, w2, b2, dtype=F64):
    """relu(conv3x3 dil 2 pad 2) -> relu(1x1 32 -> 64) -> 1x1 64 -> 256 + b2 -> soft-max -> window regression:
    -> (logits, nd, best)"""
    return head_tail(first_layer(hidden, w0, dtype), w1, w2, b2, dtype)


def confidence(hidden, c0, c2w, c2b, dtype=F64) -> torch.Tensor:
    """sigmoid(1x1(relu(conv3x3 dil 2))) [B,1,H,W] (itermvs.py:147-151, 198)"""
    return torch.sigmoid(conv1x1(torch.relu(conv3x3_dil2(hidden, c0, dtype)), c2w, c2b, dtype))


# ------------------------------------------------------------------------------------------------------------------------
# near-ties of the arg-max
# ------------------------------------------------------------------------------------------------------------------------
def undecided(logits64: torch.Tensor, gap: float) -> torch.Tensor:
    """bool [B,1,H,W]: the two largest float64 logits differ by at most ``gap`` and are not exactly equal (exactly equal
    logits are a tie, which IS decided: the lower index wins).  ``gap`` = 8 x max |fp32 restatement - fp64| of the logits of
    the case at hand: the kernel and the reference's reading of it may each be off by 4 x floor."""
    top = logits64.topk(2, dim=1).values
    l1, l2 = top[:, :1], top[:, 1:2]
    return ((l1 - l2) <= gap) & (l1 != l2)


def nd_alternatives(prob64: torch.Tensor):
    """-> (nd1, i1, nd2, i2): the window regression centred on the best bin and on the best among the other bins"""
    _, i1, _, i2 = R.top_two(prob64)
    nd1, _ = R.window_regression(prob64, best=i1)
    nd2, _ = R.window_regression(prob64, best=i2)
    return nd1, i1, nd2, i2


# ------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------
Weights = Dict[str, torch.Tensor]


def random_weights(seed: int) -> Weights:
    """He-style random layers; b2 on the 2^-12 grid (so that b2 +- 90 is exact in fp32).  ``w2`` still has to be scaled to the
    logit spread wanted (``scaled``)."""
    return {"w0": R.randn((32, 32, 3, 3), (2.0 / 288) ** 0.5, seed), "w1": R.randn((64, 32, 1, 1), (2.0 / 32) ** 0.5, seed + 1),
            "w2": R.randn((256, 64, 1, 1), (1.0 / 64) ** 0.5, seed + 2), "b2": R.grid_randn((256,), 0.5, seed + 3),
            "c0": R.randn((32, 32, 3, 3), (2.0 / 288) ** 0.5, seed + 4), "c2w": R.randn((1, 32, 1, 1), 2.0 * (1.0 / 32) ** 0.5, seed + 5),
            "c2b": torch.tensor([0.125])}


def scaled(w: Weights, x64: torch.Tensor, target: float = 4.0) -> Weights:
    """``w`` with w2 multiplied by the power of two that brings the standard deviation of the float64 logits (without their
    bias) on the first layer's output ``x64`` closest to ``target`` (a power of two: the scaled weight is exact)"""
    spread = conv1x1(torch.relu(conv1x1(x64, w["w1"], None)), w["w2"], None).std()
    k = torch.round(torch.log2(torch.tensor(target) / spread)).item()
    out = dict(w)
    out["w2"] = w["w2"] * 2.0 ** k
    return out


def trained_weights(tag: str = "dtu") -> Weights:
    from conftest import load_weights
    wts = load_weights(tag)
    p, c = "iter_mvs.update.depth_head.", "iter_mvs.update.confidence_head."
    return {"w0": wts[p + "0.weight"], "w1": wts[p + "2.weight"], "w2": wts[p + "4.weight"], "b2": wts[p + "4.bias"],
            "c0": wts[c + "0.weight"], "c2w": wts[c + "2.weight"], "c2b": wts[c + "2.bias"]}


# Routing: bin lit by first-layer channel c.  Channels 0..15 sweep every clamp of the window (0..4, 251..255) and both sides
# of the borders between the four 64-bin slices that the fused kernel's waves own; the others serve the ties.
ROUTE_BINS = [0, 1, 2, 3, 4, 251, 252, 253, 254, 255, 63, 64, 127, 128, 191, 192, 100, 101, 35, 10, 77, 200]
ROUTE_SINGLE = 16
# ties as (channel, channel): 63|64, 127|128, 191|192 (neighbours in different slices), 0|255, 4|251 (both clamps), 100|101,
# 35|10 and 35|77 (the lower bin sits on the higher channel / on the lower one), 200|10
ROUTE_TIES = [(10, 11), (12, 13), (14, 15), (0, 9), (4, 5), (16, 17), (18, 19), (18, 20), (21, 19)]
ROUTE_PERIOD = ROUTE_SINGLE + len(ROUTE_TIES)


def routing_weights(seed: int = 77) -> Weights:
    """w0: identity on the centre tap; w1: identity into the first 32 of the 64 channels; w2: 8 from channel c to bin
    ROUTE_BINS[c]; b2: -2 at the routed bins, elsewhere ``prob_background`` (in [-3,-2] on a 1/16 grid, different in
    neighbouring bins).  Every product and sum is exact in fp32 and in bf16x3: a lit bin has the logit 6."""
    w = random_weights(seed)
    w0, w1, w2 = torch.zeros((32, 32, 3, 3)), torch.zeros((64, 32, 1, 1)), torch.zeros((256, 64, 1, 1))
    for c in range(32):
        w0[c, c, 1, 1] = 1.0
        w1[c, c] = 1.0
    b2 = R.prob_background(1, 1, 1).view(BINS).clone()
    for c, k in enumerate(ROUTE_BINS):
        w2[k, c] = 8.0
        b2[k] = -2.0
    w.update(w0=w0, w1=w1, w2=w2, b2=b2)
    return w


def routing_hidden(shape) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hidden [B,32,H,W], wanted arg-max int64 [B,1,H,W]): pixel n (counted through the batch) lights channel n % 25 if that
    is below 16 -- one peak -- and otherwise both channels of tie n % 25 - 16, whose LOWER bin must win"""
    b, h, w = shape
    hidden, want = torch.zeros((b, 32, h * w)), torch.zeros((b, 1, h * w), dtype=torch.int64)
    for n in range(b * h * w):
        r = n % ROUTE_PERIOD
        chans = (r,) if r < ROUTE_SINGLE else ROUTE_TIES[r - ROUTE_SINGLE]
        for c in chans:
            hidden[n // (h * w), c, n % (h * w)] = 1.0
        want[n // (h * w), 0, n % (h * w)] = min(ROUTE_BINS[c] for c in chans)
    return hidden.view(b, 32, h, w), want.view(b, 1, h, w)


TAP_BINS = [5 + 8 * c for c in range(31)]         # bins 5 .. 245, apart by more than a window
TAP_EMPTY_BIN = 250


def tap_weights(tap: int, seed: int = 78) -> Weights:
    """w0: identity on tap ``tap`` = ky*3 + kx alone; w1 / w2: channel c < 31 lights bin TAP_BINS[c] with 8 x its value; b2 as
    for the routing but -4.5 at TAP_EMPTY_BIN, the arg-max of a pixel whose tap falls into the zero padding"""
    w = routing_weights(seed)
    w0, w2 = torch.zeros((32, 32, 3, 3)), torch.zeros((256, 64, 1, 1))
    for c in range(32):
        w0[c, c, tap // 3, tap % 3] = 1.0
    b2 = R.prob_background(1, 1, 1).view(BINS).clone() - 3.0
    for c, k in enumerate(TAP_BINS):
        w2[k, c] = 8.0
    b2[TAP_EMPTY_BIN] = -4.5
    w.update(w0=w0, w2=w2, b2=b2)
    return w


def tap_channel(shape) -> torch.Tensor:
    """int64 [B,H,W]: the channel that pixel (b, y, x) lights: (x + 5 y + 11 b) % 31.  Any two pixels that a wrong tap, a wrong
    row, a wrong tile (16 columns) or a wrong batch item could confuse differ in it."""
    b, h, w = shape
    return (torch.arange(w).view(1, 1, w) + 5 * torch.arange(h).view(1, h, 1) + 11 * torch.arange(b).view(b, 1, 1)) % 31


def tap_hidden(shape) -> torch.Tensor:
    """hidden [B,32,H,W]: pixel p lights its ``tap_channel`` with a value of its own in (0.5, 1] (on a 2^-10 grid: exact in
    the three bf16 terms)"""
    b, h, w = shape
    n = b * h * w
    val = 0.5 + torch.round(512.0 * (torch.arange(n) + 1.0) / n) / 1024.0
    hidden = torch.zeros((b, 32, h, w))
    hidden.scatter_(1, tap_channel(shape).view(b, 1, h, w), val.view(b, 1, h, w))
    return hidden


def tap_wanted_best(shape, tap: int) -> torch.Tensor:
    """the closed form: the bin of the pixel at (y + 2 (ky - 1), x + 2 (kx - 1)), TAP_EMPTY_BIN where that is outside"""
    b, h, w = shape
    ky, kx = tap // 3, tap % 3
    bins = torch.tensor(TAP_BINS)[tap_channel(shape)]
    want = torch.full((b, 1, h, w), TAP_EMPTY_BIN, dtype=torch.int64)
    for y in range(h):
        for x in range(w):
            sy, sx = y + 2 * (ky - 1), x + 2 * (kx - 1)
            if 0 <= sy < h and 0 <= sx < w:
                want[:, 0, y, x] = bins[:, sy, sx]
    return want


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
MI355X_CUS = 256
CROSS = "cross:C+4"                  # see device_shape
FUSED_SHAPES = [(1, 1, 1), (1, 1, 16), (1, 1, 17), (1, 2, 18), (2, 3, 5), (1, 5, 15), (3, 2, 33), (2, 23, 37)]
SUBSET_SHAPES = [(1, 1, 17), (1, 2, 18), (3, 2, 33)]                 # (+ walk:C+3 and CROSS) for the bf16x3 and the rider forms
REGRESS_SHAPES = [(2, 1, 1), (2, 7, 9), (2, 8, 8), (2, 5, 13), (2, 3, 11), (2, 5, 29)]       # P = 1, 63, 64, 65, 33, 145
TRAINED_SHAPE = (2, 23, 37)
DESIGNED_SHAPE = (2, 3, 21)          # two tiles per row, the second of 5 pixels; 126 pixels: five periods of the routing
TAP_SHAPE = (2, 5, 19)               # a last tile of 3 pixels: both of its left halo columns are the neighbour tile's
SHIFT_SHAPE = (2, 3, 21)
SEED_OVERRIDES: Dict[tuple, int] = {}


def seed_of(shape) -> int:
    b, h, w = shape
    return SEED_OVERRIDES.get(tuple(shape), 4000 + 10007 * b + 101 * h + w)


def random_hidden(shape, seed: int) -> torch.Tensor:
    b, h, w = shape
    return torch.tanh(R.randn((b, 32, h, w), 1.0, seed + 9))


def _reference(inp, w: Weights, shift: float, from_x: bool):
    """the reference of one case.  ``inp``: hidden, or -- ``from_x`` -- the first layer's output.  The kernel runs with
    b2 + shift (exact); the float64 reference is that of the UN-shifted bias."""
    f = head_tail if from_x else depth_head
    lead = () if from_x else (w["w0"],)
    b2_run = w["b2"] + shift
    assert torch.equal(b2_run.double(), w["b2"].double() + shift)
    logits, nd, best = f(inp, *lead, w["w1"], w["w2"], w["b2"], F64)
    l32, nd32, best32 = f(inp, *lead, w["w1"], w["w2"], b2_run, F32)
    logit_floor = R.maxdiff(l32, logits + shift)
    und = undecided(logits, 8.0 * logit_floor)
    ok = ~und
    prob = R.softmax_bins(logits)
    nd1, i1, nd2, i2 = nd_alternatives(prob)
    assert torch.equal(nd1, nd) and torch.equal(i1, best)
    ref = {"logits": logits, "nd": nd, "best": best, "alt_nd": nd2, "alt_best": i2, "undecided": und, "b2_run": b2_run,
           "logit_floor": logit_floor, "nd_bound": R.bound(2e-6, nd32[ok], nd[ok]), "best32_ok": torch.equal(best32[ok], best[ok]),
           "std": float(logits.std()), "shift": shift}
    if not from_x:
        conf = confidence(inp, w["c0"], w["c2w"], w["c2b"])
        ref["conf"] = conf
        ref["conf_bound"] = R.bound(2e-6, confidence(inp, w["c0"], w["c2w"], w["c2b"], F32), conf)
    return ref


@functools.lru_cache(maxsize=None)
def fused_case(shape, kind: str = "random", arg=0):
    """(hidden fp32 CPU, weights, reference dict) of one case of the fused kernels.  ``kind``: "random" (random weights scaled
    to a logit spread of about 4), "trained" (the dtu weights), "shift" (random weights, ``arg`` = +-90 added to b2),
    "routing", "tap" (``arg`` = the tap)."""
    seed = seed_of(shape)
    if kind in ("random", "shift", "trained"):
        hidden = random_hidden(shape, seed)
        w = trained_weights() if kind == "trained" else random_weights(seed)
        if kind != "trained":
            w = scaled(w, first_layer(hidden, w["w0"]))
    elif kind == "routing":
        hidden, w = routing_hidden(shape)[0], routing_weights()
    else:
        assert kind == "tap"
        hidden, w = tap_hidden(shape), tap_weights(arg)
    return hidden, w, _reference(hidden, w, float(arg) if kind == "shift" else 0.0, False)


@functools.lru_cache(maxsize=None)
def regress_case(shape, shift: float = 0.0):
    """(x fp32 CPU = the float64 first layer of a random hidden state, rounded once; weights; reference of the tail on x)"""
    seed = seed_of(shape) + 50000
    hidden = random_hidden(shape, seed)
    w = random_weights(seed)
    x64 = first_layer(hidden, w["w0"])
    w = scaled(w, x64)
    x = x64.float()
    return x, w, _reference(x, w, shift, True)


def device_shape(name):
    """(B,H,W) of a shape of the fused head (tile 1 x 16, two workgroups per CU) that depends on the device's CU count: a
    regime of tests/walk_shapes.py, or CROSS.  The grid is min(tiles, 2 CUs) workgroups and workgroup g takes the tiles
    g, g + grid, ...: only with more tiles than that does a workgroup fetch a second tile while the first computes.
    CROSS = two images of CUs + 2 tiles each, 2 CUs + 4 in all: the workgroups 0..3 take their first tile in image 0 and their
    second in image 1, so the double-buffered step decodes another batch item and uses every batch stride."""
    import walk_shapes
    if name != CROSS:
        return walk_shapes.walk_shape(name, 1, 16, per_cu=2)
    per = (walk_shapes.walk_tiles("walk:C+3", 2) + 1) // 2
    tx = max(d for d in range(1, 17) if per % d == 0)
    return 2, per // tx, tx * 16 - 1


def check_depth(nd: torch.Tensor, best: torch.Tensor, ref) -> Tuple[float, int]:
    """Every pixel of one result against the reference: a decided pixel has the reference's arg-max and its nd within the
    bound; an undecided one has either of the two best bins and the nd of the window around THAT bin within the bound.
    -> (largest nd error on the decided pixels, number of undecided pixels)"""
    nd, best = nd.detach().cpu().to(F64), best.detach().cpu()
    assert nd.shape == ref["nd"].shape and best.shape == ref["best"].shape and best.dtype == torch.int64
    bound = ref["nd_bound"][0]
    und = ref["undecided"]
    first = (best == ref["best"]) & ((nd - ref["nd"]).abs() <= bound)
    second = (best == ref["alt_best"]) & ((nd - ref["alt_nd"]).abs() <= bound)
    bad_best = (best != ref["best"]) & ~und
    assert not bool(bad_best.any()), f"arg-max differs at {int(bad_best.sum())} decided pixels, first {bad_best.nonzero()[:4].tolist()}"
    err = R.maxdiff(nd[~und], ref["nd"][~und])
    assert err <= bound, f"nd error {err:.3e} on the decided pixels exceeds {bound:.3e}"
    assert bool((first | second)[und].all()), "an undecided pixel matches neither of its two alternatives"
    assert bool((first | (second & und)).all())
    return err, int(und.sum())

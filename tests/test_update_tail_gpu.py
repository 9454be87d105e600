"""The depth-update tail kernels of itermvs_amd/csrc/update.hip (prob_regress, gru_rh / gru_out, pack_scores,
convex_upsample / final_upsample, bilinear_up / bilinear_up2) against the float64 restatements of
tests/update_tail_reference.py: ragged and degenerate shapes, strided layouts, logits far from zero, closed forms for every
index order.  Needs an MI355X: run with ``-m gpu``.

Bounds.  For every quantity: floor = max |fp32 CPU restatement - fp64 reference| on the very inputs of the case (the
restatement is the reference function run in float32), bound = max(the bound tests/test_kernels_gpu.py already asserts for
that quantity, 4 x floor) -- ``update_tail_reference.bound``; each test prints floor and bound before it asserts.  The
floors measured on an x86-64 host (torch CPU) and the bounds they give are listed in each test's docstring; no number
comes from a kernel's output."""
import functools

import pytest
import torch

import update_tail_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SENTINEL = -7.25
LAYOUTS = ["nchw", "nhwc", "every_other", "wslice"]


def ops():
    from itermvs_amd import ops as _ops
    return _ops


def cu(t):
    return t.to(DEV)


def lay(x: torch.Tensor, kind: str) -> torch.Tensor:
    """the CPU tensor [B,C,H,W] on the device in one of the layouts; the elements that do not belong to it hold 7"""
    b, c, h, w = x.shape
    if kind == "nchw":
        return cu(x).contiguous()
    if kind == "nhwc":
        return cu(x).contiguous(memory_format=torch.channels_last)
    if kind == "every_other":                                  # batch stride 2*C*H*W
        big = torch.full((2 * b, c, h, w), 7.0, device=DEV)
        big[::2] = cu(x)
        return big[::2]
    assert kind == "wslice"                                    # row stride W+1
    big = torch.full((b, c, h, w + 1), 7.0, device=DEV)
    big[..., 1:] = cu(x)
    return big[..., 1:]


def sentinel_buffer(shape):
    return torch.full(shape, SENTINEL, device=DEV)


def untouched(buf: torch.Tensor, written) -> bool:
    """every channel of ``buf`` outside the channel range ``written`` still holds the sentinel, bit for bit"""
    keep = [c for c in range(buf.shape[1]) if c not in written]
    return torch.equal(buf[:, keep], torch.full_like(buf[:, keep], SENTINEL))


# ------------------------------------------------------------------------------------------------------------------------
# a. prob_regress
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prob_case(shape, name):
    """(logits fp32 CPU, reference dict) of one input of one shape; computed once, never modified"""
    b, h, w = shape
    tie = False
    if name in ("randn4", "grid", "grid+90", "grid-90"):
        cases = R.prob_random_inputs(shape)
        x, base = cases[name], cases["grid" if name.startswith("grid") else name]      # shifted: the UN-shifted reference
    elif name == "sweep":
        x = base = R.prob_sweep()
    elif name == "ties":
        x = base = R.prob_ties(b, h, w)
        tie = True
    else:
        assert name == "constant"
        x = base = torch.full((b, R.BINS, h, w), 2.5)
    nd, prob, best = R.prob_regress(base)
    nd32, prob32, _ = R.prob_regress(x, torch.float32)
    _, _, _, second = R.top_two(prob)
    ok = R.decided(prob)
    ref = {"nd": nd, "prob": prob, "best": best, "second": second, "decided": ok, "tie": tie,
           "nd_bound": R.bound(1e-6, nd32[ok], nd[ok]), "prob_bound": R.bound(1e-6, prob32, prob),
           "sum_bound": R.bound(1e-6, prob32.double().sum(1), torch.ones(b, h, w, dtype=F64))}
    return x, ref


def check_prob(got, ref, tag):
    nd, prob, best = got
    ok = ref["decided"]
    best = best.cpu()
    undecided = float((~ok).double().mean())
    e_nd, e_p = R.maxdiff(nd.cpu()[ok], ref["nd"][ok]), R.maxdiff(prob, ref["prob"])
    e_sum = R.maxdiff(prob.double().sum(1), torch.ones_like(ref["prob"][:, 0]))
    print(f"prob_regress {tag}: undecided {undecided:.4f}; nd err {e_nd:.3e} (bound, floor) {ref['nd_bound']}; "
          f"prob err {e_p:.3e} {ref['prob_bound']}; sum err {e_sum:.3e} {ref['sum_bound']}")
    assert best.dtype == torch.int64 and nd.dtype == torch.float32
    assert undecided <= 0.01, tag
    assert torch.equal(best[ok], ref["best"][ok]), tag
    assert bool(((best == ref["best"]) | (best == ref["second"]))[~ok].all()), tag
    if ref["tie"]:
        assert bool(ok.all())
    assert e_p <= ref["prob_bound"][0], tag
    assert e_sum <= ref["sum_bound"][0], tag
    assert e_nd <= ref["nd_bound"][0], tag


def prob_inputs(shape):
    names = ["randn4", "grid", "grid+90", "grid-90", "constant"]
    if shape == (1, 16, 16):
        names.append("sweep")
    if shape == (2, 4, 8):
        names.append("ties")
    return names


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.PROB_SHAPES)
def test_prob_regress(shape, layout):
    """soft-max, first-max arg-max and window regression per (B,H,W) and layout, inputs: randn*4; randn*4 on a 2^-12 grid and
    that grid input shifted by +90 / -90 (exact in fp32, judged by the un-shifted float64 result: the max-subtraction);
    constant logits (arg-max 0, closed form below); at (1,16,16) the sweep "pixel k peaks at bin k" (all window clamps, all
    seven 32-bin group boundaries); at (2,4,8) exact ties at bins (31,32), (0,255), (100,101), lower index wins.
    ``wslice`` makes the wrapper copy the view: its results equal those of the copied tensor bit for bit.

    Floors (fp32 CPU restatement vs fp64; the largest over all shapes and inputs): nd 3.4e-7 -> bound 1.35e-6, probabilities
    3.2e-7 -> 1.28e-6, sum of a pixel's probabilities 4.0e-7 -> 1.62e-6 (256 rounded terms).  Where 4 x floor stays below it
    the bound is the project's 1e-6: all of (1,1,1), the sweep, the ties and the constant logits (floor 4.3e-10 for nd, 0
    for the probabilities, which are exactly 1/256)."""
    for name in prob_inputs(shape):
        x, ref = prob_case(shape, name)
        xd = lay(x, layout)
        got = ops().prob_regress(xd, want_prob=True, want_best=True)
        check_prob(got, ref, (shape, layout, name))
        if layout == "wslice":
            assert xd.stride(2) != xd.shape[3] * xd.stride(3) or shape[1] == 1
            copied = ops().prob_regress(xd.contiguous(), want_prob=True, want_best=True)
            assert all(torch.equal(a, b) for a, b in zip(got, copied)), name
        if name == "constant":
            p = 1.0 / 256
            closed = (10 * p) / (9 * p + 1e-6) / 255                                   # window 0,0,0,0,0,1,2,3,4
            assert int(got[2].abs().max()) == 0
            assert R.maxdiff(got[0], torch.full((1,), closed, dtype=F64)) <= ref["nd_bound"][0]


def test_prob_regress_two_destinations():
    """B = 3; channel 3 of a 5-channel buffer and channel 32 of a 43-channel one (different batch strides), both pre-filled
    with a sentinel that every other channel must still hold; the two copies equal the stand-alone result bit for bit.
    Bound for nd: the project's 1e-6 (floor 2.4e-7)."""
    shape = (3, 5, 7)
    x, ref = prob_case(shape, "randn4")
    b, h, w = shape
    for layout in ("nchw", "nhwc"):
        xd = lay(x, layout)
        small, wide = sentinel_buffer((b, 5, h, w)), sentinel_buffer((b, 43, h, w))
        nd, _, best = ops().prob_regress(xd, nd_out=[(small, 3), (wide, 32)], want_best=True)
        alone, _, best_alone = ops().prob_regress(xd, want_best=True)
        assert nd is None and torch.equal(best, best_alone)
        assert torch.equal(small[:, 3:4], alone) and torch.equal(wide[:, 32:33], alone)
        assert untouched(small, [3]) and untouched(wide, [32])
        ok = ref["decided"]
        assert R.maxdiff(alone.cpu()[ok], ref["nd"][ok]) <= ref["nd_bound"][0]
        # one destination only, in the wide buffer
        wide2 = sentinel_buffer((b, 43, h, w))
        ops().prob_regress(xd, nd_out=[(wide2, 32)])
        assert torch.equal(wide2, wide)


# ------------------------------------------------------------------------------------------------------------------------
# b. gru_rh / gru_out
# ------------------------------------------------------------------------------------------------------------------------
GRU_B, GRU_H, GRU_W, H_CH, RH_CH = 2, 5, 7, 43, 40


def gru_inputs(hid, seed):
    zr = R.randn((GRU_B, 2 * hid, GRU_H, GRU_W), 2.0, seed)
    q = R.randn((GRU_B, hid, GRU_H, GRU_W), 2.0, seed + 1)
    hbuf = R.randn((GRU_B, H_CH, GRU_H, GRU_W), 1.5, seed + 2)
    return zr, q, hbuf


def run_gru(zr, q, hbuf, hid, with_copy):
    """-> (rh buffer, h buffer after gru_out, h_copy | None), all on the device"""
    hd, rhd = cu(hbuf).contiguous(), sentinel_buffer((GRU_B, RH_CH, GRU_H, GRU_W))
    ops().gru_rh(cu(zr), hd, rhd, hid=hid)
    assert torch.equal(hd.cpu(), hbuf)                                                 # gru_rh reads the state only
    copy = torch.full((GRU_B, hid, GRU_H, GRU_W), SENTINEL, device=DEV) if with_copy else None
    ops().gru_out(cu(zr), cu(q), hd, copy, hid=hid)
    return rhd, hd, copy


@pytest.mark.parametrize("hid", [32, 5])
def test_gru_gates_against_fp64(hid):
    """B = 2, 5x7 pixels, state in a 43-channel buffer and r*h into a 40-channel one (h_sb != rh_sb), hid = 32 and 5 (2240 and
    350 elements: several blocks, a partial last one).  Channels hid.. of both buffers keep their bits; with and without
    ``h_copy`` the new state is the same and the copy equals it.

    Floors: new state 2.8e-7 (hid 32) and 2.4e-7 (hid 5) -> bound 2e-5 (the project's).  r*h: the project asserts no bound of
    its own; it is h / (1 + expf(-x)) -- expf, an addition, a division and a product, each within 2 ulp in HIP's documented
    accuracy -- so 8 ulp (8 * 2^-24 relative) of the largest |r*h|: 2.13e-6 (hid 32) and 1.30e-6 (hid 5), which exceed
    4 x floor (floors 4.1e-7 and 2.2e-7)."""
    zr, q, hbuf = gru_inputs(hid, 40 + hid)
    h = hbuf[:, :hid]
    want_rh, want = R.gru_rh(zr, h), R.gru_state(zr, q, h)
    b_rh = R.bound(8 * 2.0 ** -24 * float(want_rh.abs().max()), R.gru_rh(zr, h, torch.float32), want_rh)
    b_st = R.bound(2e-5, R.gru_state(zr, q, h, torch.float32), want)
    rhd, hd, _ = run_gru(zr, q, hbuf, hid, False)
    rhd2, hd2, copy = run_gru(zr, q, hbuf, hid, True)
    e_rh, e_st = R.maxdiff(rhd[:, :hid], want_rh), R.maxdiff(hd[:, :hid], want)
    print(f"gru hid={hid}: rh err {e_rh:.3e} (bound, floor) {b_rh}; state err {e_st:.3e} {b_st}")
    assert e_rh <= b_rh[0] and e_st <= b_st[0]
    assert torch.equal(hd, hd2) and torch.equal(rhd, rhd2) and torch.equal(copy, hd[:, :hid])
    assert untouched(rhd, range(hid))
    assert torch.equal(hd[:, hid:].cpu(), hbuf[:, hid:])


@pytest.mark.parametrize("hid", [32, 5])
def test_gru_saturated_gates(hid):
    """pre-activations of +-100: sample 0 has z = 0 (the state passes through bit for bit) and r = 0 (r*h is exactly 0),
    sample 1 has z = 1 (the new state is tanh(q)) and r = 1 (r*h is h bit for bit).
    Bound for tanh(q): the project's 2e-5 for the state (floor 3.1e-8)."""
    zr, q, hbuf = gru_inputs(hid, 70 + hid)
    zr[0], zr[1] = -100.0, 100.0
    h = hbuf[:, :hid]
    rhd, hd, copy = run_gru(zr, q, hbuf, hid, True)
    assert torch.equal(hd[0, :hid].cpu(), h[0])
    assert bool((rhd[0, :hid] == 0).all()) and torch.equal(rhd[1, :hid].cpu(), h[1])
    want = torch.tanh(q[1].double())
    b_st = R.bound(2e-5, torch.tanh(q[1]), want)
    err = R.maxdiff(hd[1, :hid], want)
    print(f"gru saturated hid={hid}: tanh err {err:.3e} (bound, floor) {b_st}")
    assert err <= b_st[0] and torch.equal(copy, hd[:, :hid])
    assert R.maxdiff(hd[:, :hid], R.gru_state(zr, q, h)) <= b_st[0]
    assert untouched(rhd, range(hid)) and torch.equal(hd[:, hid:].cpu(), hbuf[:, hid:])


# ------------------------------------------------------------------------------------------------------------------------
# c. pack_scores
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("ch0", [0, 33])
@pytest.mark.parametrize("n", [(4, 4, 2), (1, 3, 2)])
def test_pack_scores(n, ch0, second):
    """B = 3, 35 pixels: the written channels ch0 .. ch0+sum(n) equal the inputs exactly, every other channel of the
    43-channel buffers keeps the sentinel"""
    b, h, w = 3, 5, 7
    s = [R.randn((b, c, h, w), 1.0, 20 + i) for i, c in enumerate(n)]
    d0 = sentinel_buffer((b, 43, h, w))
    d1 = sentinel_buffer((b, 43, h, w)) if second else None
    ops().pack_scores([cu(t) for t in s], d0, d1, ch0)
    want, written = torch.cat(s, 1), range(ch0, ch0 + sum(n))
    for d in (d0, d1) if second else (d0,):
        assert torch.equal(d[:, ch0:ch0 + sum(n)].cpu(), want) and untouched(d, written)


# ------------------------------------------------------------------------------------------------------------------------
# d. convex_upsample / final_upsample
# ------------------------------------------------------------------------------------------------------------------------
CONVEX_B = 2
DEPTH_MIN, DEPTH_MAX = torch.tensor([400.0, 425.0]), torch.tensor([900.0, 935.0])


@functools.lru_cache(maxsize=None)
def convex_case(size, name):
    """(nd [B,1,H,W], logits [B,144,H,W], inv_min, inv_max, reference dict); shifted logits: the UN-shifted reference"""
    h, w = size
    seed = 300 + 16 * h + w
    nd = torch.rand((CONVEX_B, 1, h, w), generator=torch.Generator().manual_seed(seed))
    base = R.grid_randn((CONVEX_B, 144, h, w), 3.0, seed + 1)
    x = {"grid": base, "grid+90": base + R.SHIFT, "grid-90": base - R.SHIFT}[name]
    inv_min, inv_max = 1.0 / DEPTH_MIN, 1.0 / DEPTH_MAX
    depth, up = R.convex_upsample(nd, base, inv_min, inv_max)
    depth32, up32 = R.convex_upsample(nd, x, inv_min, inv_max, torch.float32)
    ref = {"depth": depth, "up": up, "up_bound": R.bound(1e-6, up32, up), "depth_bound": R.bound(1e-6, depth32, depth, depth)}
    return nd, x, inv_min, inv_max, ref


def neighbour(nd: torch.Tensor, k: int) -> torch.Tensor:
    """tap k = ky*3 + kx of the replicate-padded 3x3 neighbourhood of every pixel, by clamped indexing"""
    h, w = nd.shape[2:]
    yy = (torch.arange(h) + k // 3 - 1).clamp(0, h - 1)
    xx = (torch.arange(w) + k % 3 - 1).clamp(0, w - 1)
    return nd[:, :, yy][:, :, :, xx]


def nd_buffers(nd):
    """the normalised depth as channel 32 of a 43-channel buffer and as channel 0 of a 1-channel one"""
    b, _, h, w = nd.shape
    wide = sentinel_buffer((b, 43, h, w))
    wide[:, 32:33] = cu(nd)
    return [(wide, 32), (cu(nd).contiguous(), 0)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc", "every_other"])
@pytest.mark.parametrize("size", R.CONVEX_SIZES)
def test_convex_and_final_upsample_against_fp64(size, layout):
    """B = 2 with per-sample depth ranges, randn*3 logits on the 2^-12 grid and the same shifted by +-90 (judged by the
    un-shifted float64 result), nd inside a 43-channel buffer and as a 1-channel tensor; final_upsample (depth + the x4
    bilinear confidence in one launch; 8, 48, 40, 120 and 504 convex threads: never a multiple of 256, at 7x9 the partial second
    convex block sits next to the first bilinear block) equals convex_upsample and bilinear_up(conf, 4) bit for bit.

    Floors: normalised map at most 2.2e-7 -> bound 1e-6 (the project's), except 3.1e-7 -> 1.26e-6 at 1x6; depth at most
    2.0e-7 relative -> 1e-6 relative (the project's); confidence at most 1.0e-7 -> 1e-6."""
    h, w = size
    conf = torch.rand((CONVEX_B, 1, h, w), generator=torch.Generator().manual_seed(900 + 16 * h + w))
    want_conf = R.bilinear_up(conf, 4)
    b_conf = R.bound(1e-6, R.bilinear_up(conf, 4, dtype=torch.float32), want_conf)
    for name in ("grid", "grid+90", "grid-90"):
        nd, x, inv_min, inv_max, ref = convex_case(size, name)
        xd = lay(x, layout)
        for buf, ch in nd_buffers(nd):
            depth, norm = ops().convex_upsample(xd, buf, cu(inv_min), cu(inv_max), nd_channel=ch, want_norm=True)
            e_up = R.maxdiff(norm, ref["up"])
            e_d = float(((depth.cpu().double() - ref["depth"]).abs() / ref["depth"]).max())
            print(f"convex {size} {layout} {name} ch{ch}: up err {e_up:.3e} (bound, floor) {ref['up_bound']}; "
                  f"depth rel err {e_d:.3e} {ref['depth_bound']}")
            assert tuple(depth.shape) == (CONVEX_B, 1, 4 * h, 4 * w)
            assert e_up <= ref["up_bound"][0] and e_d <= ref["depth_bound"][0], (name, ch)
            assert torch.equal(depth, ops().convex_upsample(xd, buf, cu(inv_min), cu(inv_max), nd_channel=ch))
            depth_f, conf_up = ops().final_upsample(xd, buf, cu(inv_min), cu(inv_max), cu(conf), nd_channel=ch)
            assert torch.equal(depth_f, depth), (name, ch)
            assert torch.equal(conf_up, ops().bilinear_up(cu(conf), 4))
            assert R.maxdiff(conf_up, want_conf) <= b_conf[0]


@pytest.mark.parametrize("layout", ["nchw", "nhwc", "every_other"])
@pytest.mark.parametrize("size", R.CONVEX_SIZES)
def test_convex_upsample_index_orders_in_closed_form(size, layout):
    """logits of +60 at one tap and 0 at the other eight make the soft-max a selection (the others weigh e^-60): with tap k
    selected for every sub-pixel the normalised output is the replicate-padded neighbour k = ky*3 + kx of nd, each value
    repeated 4x4; with tap (2i + j) % 9 selected for sub-pixel (i, j) -- a choice that differs between (i, j) and (j, i)
    for every i != j -- the output at row 4y+i, column 4x+j is that neighbour of pixel (y, x).  This fixes the channel order
    k*16 + i*4 + j, the neighbour order and the placement.  1e-6 absolute, as for the normalised map elsewhere."""
    h, w = size
    nd = torch.rand((CONVEX_B, 1, h, w), generator=torch.Generator().manual_seed(700 + 16 * h + w))
    inv_min, inv_max = cu(1.0 / DEPTH_MIN), cu(1.0 / DEPTH_MAX)
    buf, ch = nd_buffers(nd)[0]
    for k in range(9):
        logits = torch.zeros((CONVEX_B, 9, 16, h, w))
        logits[:, k] = 60.0
        _, norm = ops().convex_upsample(lay(logits.view(CONVEX_B, 144, h, w), layout), buf, inv_min, inv_max, nd_channel=ch, want_norm=True)
        want = neighbour(nd, k).repeat_interleave(4, 2).repeat_interleave(4, 3)
        assert R.maxdiff(norm, want) <= 1e-6, k
    logits = torch.zeros((CONVEX_B, 9, 4, 4, h, w))
    for i in range(4):
        for j in range(4):
            logits[:, (2 * i + j) % 9, i, j] = 60.0
    depth, norm = ops().convex_upsample(lay(logits.view(CONVEX_B, 144, h, w), layout), buf, inv_min, inv_max, nd_channel=ch, want_norm=True)
    norm = norm.cpu()
    for i in range(4):
        for j in range(4):
            assert R.maxdiff(norm[:, :, i::4, j::4], neighbour(nd, (2 * i + j) % 9)) <= 1e-6, (i, j)
    # the same closed form through the float64 reference, and the depth it un-normalises to
    want_depth, want = R.convex_upsample(nd, logits.view(CONVEX_B, 144, h, w), 1.0 / DEPTH_MIN, 1.0 / DEPTH_MAX)
    assert R.maxdiff(norm, want) <= 1e-6
    d32, _ = R.convex_upsample(nd, logits.view(CONVEX_B, 144, h, w), 1.0 / DEPTH_MIN, 1.0 / DEPTH_MAX, torch.float32)
    assert float(((depth.cpu().double() - want_depth).abs() / want_depth).max()) <= R.bound(1e-6, d32, want_depth, want_depth)[0]


# ------------------------------------------------------------------------------------------------------------------------
# e. bilinear_up / bilinear_up_into
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(1, 1), (2, 5)])
@pytest.mark.parametrize("size", [(1, 1), (1, 5), (6, 1), (2, 3), (7, 9)])
@pytest.mark.parametrize("scale", [2, 4])
def test_bilinear_up_and_into(scale, size, bc):
    """B*C = 1 and 10, single rows, single columns and a single pixel (the y1 = y0, x1 = x0 clamps), with and without tanh;
    bilinear_up_into writes channels 2.. of a (C+3)-channel buffer and channels 5.. of a (C+9)-channel one, equals
    bilinear_up bit for bit and leaves the surrounding channels alone.
    Floors: at most 3.1e-7 without tanh -> bound 1.23e-6 there (1e-6, the project's, wherever 4 x floor is below it);
    at most 1.1e-7 with tanh -> 1e-6."""
    (b, c), (h, w) = bc, size
    x = R.randn((b, c, h, w), 1.0, 500 + 100 * scale + 16 * h + w + c)
    for act in ("none", "tanh"):
        want = R.bilinear_up(x, scale, act)
        bd = R.bound(1e-6, R.bilinear_up(x, scale, act, torch.float32), want)
        got = ops().bilinear_up(cu(x), scale, act=act)
        err = R.maxdiff(got, want)
        print(f"bilinear x{scale} {size} {bc} {act}: err {err:.3e} (bound, floor) {bd}")
        assert tuple(got.shape) == (b, c, scale * h, scale * w) and err <= bd[0], act
        a, wide = sentinel_buffer((b, c + 3, scale * h, scale * w)), sentinel_buffer((b, c + 9, scale * h, scale * w))
        ops().bilinear_up_into(cu(x), scale, a[:, 2:2 + c], wide[:, 5:5 + c], act=act)
        assert torch.equal(a[:, 2:2 + c], got) and torch.equal(wide[:, 5:5 + c], got), act
        assert untouched(a, range(2, 2 + c)) and untouched(wide, range(5, 5 + c))
        single = sentinel_buffer((b, c + 9, scale * h, scale * w))
        ops().bilinear_up_into(cu(x), scale, single[:, 5:5 + c], act=act)
        assert torch.equal(single, wide)

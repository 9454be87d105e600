"""Pins tests/head_reference.py before any kernel is judged by it: the float64 restatement of the depth and confidence heads
reproduces what the reference recorded in fp32 (tests/golden) and what the oracle computes, and the inputs of
tests/test_head_gpu.py meet the conditions that make its assertions sharp (spread of the logits, decided arg-max, all four
64-bin slices reached, every clamp and tie of the designed sweep).  Prints the floors (fp32 CPU restatement vs float64) that
the docstrings of tests/test_head_gpu.py list.  No GPU needed."""
import pytest
import torch

import head_reference as H
import update_tail_reference as R
from conftest import golden, load_weights
from oracle import itermvs_oracle as O

F64 = torch.float64


def _report(tag, ref):
    n_und, n = int(ref["undecided"].sum()), ref["undecided"].numel()
    line = (f"head floors {tag}: logits {ref['logit_floor']:.2e} (std {ref['std']:.2f}); nd (bound, floor) "
            f"({ref['nd_bound'][0]:.2e}, {ref['nd_bound'][1]:.2e}); undecided {n_und} of {n}")
    if "conf_bound" in ref:
        line += f"; confidence ({ref['conf_bound'][0]:.2e}, {ref['conf_bound'][1]:.2e})"
    print(line)


def _conditions(shape, ref, spread=True):
    """what tests/test_head_gpu.py relies on, for one case"""
    b, h, w = shape
    share = float(ref["undecided"].double().mean())
    assert share == 0.0 if h * w <= 256 else share <= 0.01, (shape, share)
    assert ref["best32_ok"]                       # the fp32 restatement itself has the reference's arg-max where it is decided
    if spread:
        assert 2.0 <= ref["std"] <= 8.0, (shape, ref["std"])


@pytest.mark.parametrize("tag", ["seed0", "dtu"])
def test_restatement_reproduces_the_recorded_head_outputs(tag):
    """every recorded hidden state through the float64 restatement: the recorded fp32 logits lie within the gap of the case
    (8 x floor: two fp32 computations, each within 4 x floor), the recorded arg-max and nd pass the very check the kernels
    get, and so do the oracle's depth_head_logits / window_regression / confidence_logit"""
    g, wts = golden(f"e2e_small_{tag}.npz"), load_weights(tag)
    w = H.trained_weights(tag)
    for it in range(int(g.np("iteration"))):
        hidden = g[f"iter{it}.hidden"]
        ref = H._reference(hidden, w, 0.0, False)
        _report(f"golden {tag} iter{it}", ref)
        gap = 8.0 * ref["logit_floor"]
        assert ref["logits"].dtype == F64 and ref["logit_floor"] > 0.0
        assert R.maxdiff(ref["logits"], g[f"iter{it}.logits"]) <= gap
        H.check_depth(g[f"iter{it}.nd"], g[f"iter{it}.best"], ref)
        if f"iter{it}.conf" in g:
            assert R.maxdiff(ref["conf"], g[f"iter{it}.conf"]) <= ref["conf_bound"][0]
        # the oracle on the same inputs
        lo = O.depth_head_logits(wts, hidden)
        assert R.maxdiff(ref["logits"], lo) <= gap
        H.check_depth(*O.window_regression(torch.softmax(lo, 1)), ref)
        nd_o, best_o = O.window_regression(R.softmax_bins(ref["logits"]))          # its regression on the reference's own probabilities
        assert torch.equal(best_o, ref["best"]) and R.maxdiff(nd_o, ref["nd"]) <= 1e-12
        assert R.maxdiff(ref["conf"], torch.sigmoid(O.confidence_logit(wts, hidden))) <= ref["conf_bound"][0]
        # the float64 run of the library's convolutions agrees with the written-out sums to float64 rounding
        lib = O.depth_head_logits({k: v.double() for k, v in wts.items() if v.dtype.is_floating_point}, hidden.double())
        assert R.maxdiff(ref["logits"], lib) <= 1e-11


def test_designed_weights_reach_every_clamp_and_tie():
    """the routing sweep: exact logits (floor 0), no undecided pixel, the wanted arg-max (the lower bin of every tie), every
    bin of ROUTE_BINS below 16 as a single peak, every tie; the oracle's regression agrees at every clamp"""
    shape = H.DESIGNED_SHAPE
    hidden, w, ref = H.fused_case(shape, "routing")
    _report("routing", ref)
    _, want = H.routing_hidden(shape)
    assert ref["logit_floor"] == 0.0 and not bool(ref["undecided"].any())
    assert torch.equal(ref["best"], want)
    n = shape[0] * shape[1] * shape[2]
    assert n >= 2 * H.ROUTE_PERIOD
    singles = {H.ROUTE_BINS[c] for c in range(H.ROUTE_SINGLE)}
    assert singles == {0, 1, 2, 3, 4, 251, 252, 253, 254, 255, 63, 64, 127, 128, 191, 192}
    l1, i1, l2, i2 = R.top_two(R.softmax_bins(ref["logits"]))            # (equal logits are equal probabilities)
    tied = (l1 == l2).view(-1)
    got_ties = {(int(a), int(b)) for a, b in zip(i1.view(-1)[tied], i2.view(-1)[tied])}
    assert got_ties == {tuple(sorted(H.ROUTE_BINS[c] for c in pair)) for pair in H.ROUTE_TIES}
    assert {int(k) for k in ref["best"].view(-1)[~tied]} == singles
    assert float(ref["logits"].amax(1).min()) == 6.0 and float(ref["logits"].max()) == 6.0
    nd_o, best_o = O.window_regression(torch.softmax(ref["logits"], 1))
    assert torch.equal(best_o, want) and R.maxdiff(nd_o, ref["nd"]) <= 1e-12
    # closed form of a single peak at bin 0 (window 0,0,0,0,0,1,2,3,4) from the probabilities
    p = R.softmax_bins(ref["logits"])[0, :, 0, 0]
    assert int(want[0, 0, 0, 0]) == 0
    closed = (p[1] + 2 * p[2] + 3 * p[3] + 4 * p[4]) / (1e-6 + 5 * p[0] + p[1] + p[2] + p[3] + p[4]) / 255
    assert abs(float(ref["nd"][0, 0, 0, 0] - closed)) <= 1e-15
    _conditions(shape, ref, spread=False)


@pytest.mark.parametrize("tap", range(9))
def test_tap_cases_have_their_closed_form(tap):
    """one non-zero tap: the arg-max of every pixel is the bin of the pixel that tap reads, or TAP_EMPTY_BIN in the padding;
    all nine taps differ, every border is reached, and so are the two halo columns on either side of the tile border"""
    shape = H.TAP_SHAPE
    hidden, w, ref = H.fused_case(shape, "tap", tap)
    _report(f"tap {tap}", ref)
    want = H.tap_wanted_best(shape, tap)
    assert torch.equal(ref["best"], want)
    assert not bool(ref["undecided"].any())
    ky, kx = tap // 3, tap % 3
    empty = want[:, 0] == H.TAP_EMPTY_BIN
    b, h, wd = shape
    rows = {0: [0, 1], 1: [], 2: [h - 2, h - 1]}[ky]
    cols = {0: [0, 1], 1: [], 2: [wd - 2, wd - 1]}[kx]
    expect = torch.zeros((h, wd), dtype=torch.bool)
    expect[rows, :] = True
    expect[:, cols] = True
    assert torch.equal(empty, expect.expand(b, h, wd))
    for other in range(tap):
        assert not torch.equal(want, H.tap_wanted_best(shape, other))
    # values differ per pixel: nd is a function of the lit value, not only of the bin
    assert hidden.amax(1).unique().numel() >= 0.9 * b * h * wd
    _conditions(shape, ref, spread=False)


@pytest.fixture
def mi355x_shapes(monkeypatch):
    """{name: (B,H,W)} of the shapes tests/test_head_gpu.py takes from the device's CU count, for the 256 CUs of an MI355X"""
    import types
    import walk_shapes
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda _=0: types.SimpleNamespace(multi_processor_count=H.MI355X_CUS))
    return {name: H.device_shape(name) for name in walk_shapes.REGIMES + (H.CROSS,)}


def test_random_cases_meet_the_conditions_of_the_gpu_test(mi355x_shapes):
    """every random case and seed of tests/test_head_gpu.py: logit spread in [2, 8], no undecided pixel in maps of at most
    256 pixels and at most 1 % otherwise, and over the set the arg-max falls into all four 64-bin slices"""
    slices = set()
    shapes = [(s, "random", 0) for s in H.FUSED_SHAPES + list(mi355x_shapes.values())]
    shapes += [(H.TRAINED_SHAPE, "trained", 0), (H.SHIFT_SHAPE, "shift", 90.0), (H.SHIFT_SHAPE, "shift", -90.0)]
    for shape, kind, arg in shapes:
        _, _, ref = H.fused_case(shape, kind, arg)
        _report(f"fused {kind} {arg} {shape}", ref)
        _conditions(shape, ref, spread=kind != "trained")
        if kind == "random":
            slices |= {int(k) // 64 for k in ref["best"].view(-1)}
    assert slices == {0, 1, 2, 3}
    # the shifted cases are judged by the un-shifted reference
    base = H.fused_case(H.SHIFT_SHAPE, "random")[2]
    for s in (90.0, -90.0):
        assert torch.equal(H.fused_case(H.SHIFT_SHAPE, "shift", s)[2]["nd"], base["nd"])
    for shape in H.REGRESS_SHAPES:
        for shift in (0.0, 90.0, -90.0) if shape == H.REGRESS_SHAPES[-1] else (0.0,):
            x, _, ref = H.regress_case(shape, shift)
            _report(f"regress {shift} {shape}", ref)
            assert x.dtype == torch.float32
            _conditions(shape, ref)


def _tiles_of_workgroup(shape, g, grid):
    """[(batch item, row, first column)] of the tiles workgroup ``g`` of ``grid`` walks: g, g + grid, ... decoded as the kernel
    does (tile = (item * H + row) * tiles_x + column tile)"""
    b, h, w = shape
    tx = (w + 15) // 16
    return [(t // (h * tx), t % (h * tx) // tx, t % tx * 16) for t in range(g, b * h * tx, grid)]


def test_which_shapes_give_a_workgroup_a_second_tile(mi355x_shapes):
    """the grid of the fused head is min(tiles, 2 CUs): on 256 CUs only walk:C+3 and CROSS give a workgroup a second tile --
    the step that fetches the next tile while this one computes.  At walk:C+3 that tile lies in the same image; at CROSS the
    workgroups 0..3 go from image 0 to image 1.  The fixed small shapes, (3,2,33) included, are one tile per workgroup."""
    resident = 2 * H.MI355X_CUS

    def walks(shape):
        b, h, w = shape
        grid = min(b * h * ((w + 15) // 16), resident)
        return [_tiles_of_workgroup(shape, g, grid) for g in range(grid)]

    for shape in H.FUSED_SHAPES + [H.TRAINED_SHAPE, H.DESIGNED_SHAPE, H.TAP_SHAPE] + [mi355x_shapes[r] for r in ("walk:3", "walk:9", "walk:C-6", "walk:C")]:
        assert all(len(t) == 1 for t in walks(shape)), shape
    two = [t for t in walks(mi355x_shapes["walk:C+3"]) if len(t) > 1]
    assert len(two) == 3 and all(t[0][0] == t[1][0] == 0 for t in two)
    cross = mi355x_shapes[H.CROSS]
    assert cross == (2, 43, 95)
    two = [t for t in walks(cross) if len(t) > 1]
    assert len(two) == 4 and all(len(t) == 2 and t[0][0] == 0 and t[1][0] == 1 for t in two)
    assert sum(len(t) for t in walks(cross)) == resident + 4


def test_undecided_and_alternatives():
    """undecided(): within the gap and not equal; an exact tie is decided.  nd_alternatives(): the second window is the
    regression the runner-up would give."""
    logits = torch.full((1, 256, 1, 3), -4.0, dtype=F64)
    logits[0, 10, 0, 0], logits[0, 200, 0, 0] = 1.0, 1.0                # tie
    logits[0, 10, 0, 1], logits[0, 200, 0, 1] = 1.0, 1.0 + 1e-7         # near-tie, the higher bin ahead
    logits[0, 10, 0, 2], logits[0, 200, 0, 2] = 1.0, 1.1
    assert H.undecided(logits, 1e-6).view(-1).tolist() == [False, True, False]
    assert H.undecided(logits, 0.0).view(-1).tolist() == [False, False, False]
    prob = R.softmax_bins(logits)
    nd1, i1, nd2, i2 = H.nd_alternatives(prob)
    assert i1.view(-1).tolist() == [10, 200, 200] and i2.view(-1).tolist() == [200, 10, 10]
    swapped = logits.clone()
    swapped[0, 10, 0, 1] = 1.0 + 2e-7
    nd_s, _, best_s = R.prob_regress(swapped)
    assert int(best_s[0, 0, 0, 1]) == 10 and abs(float(nd_s[0, 0, 0, 1] - nd2[0, 0, 0, 1])) <= 1e-8
    assert abs(float(nd1[0, 0, 0, 1] - nd2[0, 0, 0, 1])) > 0.5


def test_check_depth_rejects_one_wrong_pixel():
    """the check the kernels get is per pixel: one corner pixel off by 3e-6, or on the neighbouring bin, fails it"""
    shape = (2, 3, 5)
    _, _, ref = H.fused_case(shape)
    nd, best = ref["nd"].float(), ref["best"].clone()
    H.check_depth(nd, best, ref)
    for b, y, x in ((0, 0, 0), (1, 2, 4)):
        bad = nd.clone()
        bad[b, 0, y, x] += 3e-6
        with pytest.raises(AssertionError):
            H.check_depth(bad, best, ref)
        bad_best = best.clone()
        bad_best[b, 0, y, x] += 1
        with pytest.raises(AssertionError):
            H.check_depth(nd, bad_best, ref)
    # an undecided pixel may have the runner-up, but then with the runner-up's window
    logits = ref["logits"].clone()
    i1, i2 = int(ref["best"][0, 0, 0, 0]), (int(ref["best"][0, 0, 0, 0]) + 100) % 256
    logits[0, i2, 0, 0] = logits[0, i1, 0, 0] - 1e-9
    prob = R.softmax_bins(logits)
    nd1, b1, nd2, b2 = H.nd_alternatives(prob)
    und = H.undecided(logits, 1e-6)
    assert und.view(-1).tolist() == [True] + [False] * 29
    ref2 = dict(ref, logits=logits, nd=nd1, best=b1, alt_nd=nd2, alt_best=b2, undecided=und)
    H.check_depth(nd1, b1, ref2)
    swapped_nd, swapped_best = nd1.clone(), b1.clone()
    swapped_nd[0, 0, 0, 0], swapped_best[0, 0, 0, 0] = nd2[0, 0, 0, 0], i2
    H.check_depth(swapped_nd, swapped_best, ref2)
    swapped_nd[0, 0, 0, 0] = nd1[0, 0, 0, 0]                       # the runner-up's bin with the winner's window
    with pytest.raises(AssertionError):
        H.check_depth(swapped_nd, swapped_best, ref2)

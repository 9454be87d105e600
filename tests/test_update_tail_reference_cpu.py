"""Pins tests/update_tail_reference.py before any kernel is judged by it: the float64 restatements reproduce what the
reference recorded in fp32 (tests/golden), the bilinear function is F.interpolate, and the random inputs of
tests/test_update_tail_gpu.py leave an fp32 kernel's arg-max decided at (almost) every pixel.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import update_tail_reference as R
from conftest import golden, load_weights

F64 = torch.float64


def _regress_keys(g):
    return [("logits0", "best0", "nd0")] + [(f"iter{it}.logits", f"iter{it}.best", f"iter{it}.nd")
                                            for it in range(int(g.np("iteration")))]


@pytest.mark.parametrize("tag", ["seed0", "dtu"])
def test_prob_regress_reproduces_the_recorded_outputs(tag):
    g = golden(f"e2e_small_{tag}.npz")
    for lk, bk, nk in _regress_keys(g):
        nd, prob, best = R.prob_regress(g[lk])
        assert torch.equal(best, g[bk]), lk                                  # fp64 arg-max == the recorded fp32 one
        assert R.maxdiff(nd, g[nk]) <= 1e-6, lk
        assert R.maxdiff(prob.sum(1), torch.ones(1, dtype=F64)) <= 1e-12
        # the float32 run of the same function is the recorded computation up to the order of its sums
        nd32, _, best32 = R.prob_regress(g[lk], torch.float32)
        assert nd32.dtype == torch.float32 and torch.equal(best32, g[bk]) and R.maxdiff(nd32, g[nk]) <= 1e-6


@pytest.mark.parametrize("tag", ["seed0", "dtu"])
def test_gru_reproduces_the_recorded_state(tag):
    g, w = golden(f"e2e_small_{tag}.npz"), load_weights(tag)
    h = g["iter0.hidden_in"].to(F64)
    x = torch.cat([g["iter0.nd_in"], g["iter0.score"]], 1).to(F64)
    p = "iter_mvs.update.gru."
    conv = lambda inp, name: F.conv2d(inp, w[p + name + ".weight"].to(F64), w[p + name + ".bias"].to(F64), padding=2, dilation=2)
    hx = torch.cat([h, x], 1)
    zr = torch.cat([conv(hx, "convz"), conv(hx, "convr")], 1)
    rh = R.gru_rh(zr, h)
    assert R.maxdiff(rh, torch.sigmoid(zr[:, 32:]) * h) == 0.0
    state = R.gru_state(zr, conv(torch.cat([rh, x], 1), "convq"), h)
    # the recorded state went through three fp32 convolutions of 387 terms each: the project's bound for this golden
    # (tests/test_kernels_gpu.py:test_gru_gates), not an fp32 ulp
    assert state.dtype == F64 and R.maxdiff(state, g["iter0.hidden"]) <= 2e-5


def test_convex_upsample_reproduces_the_recorded_outputs():
    g = golden("upsample.npz")
    depth, up = R.convex_upsample(g["x"], g["logits"], g["inv_min"].view(-1), g["inv_max"].view(-1))
    assert depth.dtype == F64 and tuple(up.shape) == tuple(g["up"].shape)
    assert R.maxdiff(up, g["up"]) <= 1e-6
    assert float(((depth - g["depth"].to(F64)).abs() / g["depth"].to(F64)).max()) <= 1e-6


def test_convex_upsample_index_orders_in_closed_form():
    """one-hot weights (no soft-max involved: +-inf-free logits of 0 / 800 in float64): tap k = ky*3+kx of the replicate-padded
    neighbourhood lands at row 4y+i, column 4x+j for the channel k*16 + i*4 + j"""
    b, h, w = 2, 3, 5
    nd = R.randn((b, 1, h, w), 1.0, 5).abs()
    one = torch.ones(b)
    ys, xs = torch.arange(h), torch.arange(w)
    logits = torch.zeros(b, 9, 4, 4, h, w)
    for i in range(4):
        for j in range(4):
            logits[:, (2 * i + j) % 9, i, j] = 800.0
    _, up = R.convex_upsample(nd, logits.view(b, 144, h, w), one, 2 * one)
    for i in range(4):
        for j in range(4):
            k = (2 * i + j) % 9
            yy, xx = (ys + k // 3 - 1).clamp(0, h - 1), (xs + k % 3 - 1).clamp(0, w - 1)
            assert torch.equal(up[:, :, i::4, j::4], nd.to(F64)[:, :, yy][:, :, :, xx]), (i, j)


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 5), (2, 5, 6, 1), (2, 5, 2, 3), (2, 5, 7, 9)])
def test_bilinear_up_is_interpolate(shape, scale):
    x = R.randn(shape, 1.0, 7).to(F64)
    want = F.interpolate(x, scale_factor=scale, mode="bilinear")
    got = R.bilinear_up(x, scale)
    assert got.dtype == F64 and got.shape == want.shape and R.maxdiff(got, want) <= 1e-15
    assert R.maxdiff(R.bilinear_up(x, scale, "tanh"), torch.tanh(want)) <= 1e-15
    got32 = R.bilinear_up(x, scale, dtype=torch.float32)
    assert got32.dtype == torch.float32 and R.maxdiff(got32, want) <= 1e-6


@pytest.mark.parametrize("shape", R.PROB_SHAPES)
def test_random_logits_leave_the_argmax_decided(shape):
    """the decidedness condition of the GPU test, on its seeds, for the reference alone: at most 1 % of the pixels are left
    out, and the three grid cases describe the same distribution"""
    cases = R.prob_random_inputs(shape)
    for name, x in cases.items():
        assert x.dtype == torch.float32
        ok = R.decided(R.softmax_bins(x))
        assert float((~ok).double().mean()) <= 0.01, (name, int((~ok).sum()))
    assert R.maxdiff(R.softmax_bins(cases["grid+90"]), R.softmax_bins(cases["grid"])) <= 1e-15
    assert R.maxdiff(R.softmax_bins(cases["grid-90"]), R.softmax_bins(cases["grid"])) <= 1e-15


def test_constructed_logits():
    """sweep: pixel k peaks at bin k; ties: both peaks are the same fp32 number, decided, lower bin wins; constant logits:
    arg-max 0 and the closed form of the clamped window"""
    _, _, best = R.prob_regress(R.prob_sweep())
    assert torch.equal(best.view(-1), torch.arange(256))
    ties = R.prob_ties()
    _, prob, best = R.prob_regress(ties)
    assert bool(R.decided(prob).all())
    want = torch.tensor([R.TIE_PAIRS[p % 3][0] for p in range(32)]).view(1, 1, 4, 8).expand(2, 1, 4, 8)
    assert torch.equal(best, want)
    p1, _, p2, i2 = R.top_two(prob)
    assert torch.equal(p1, p2) and torch.equal(i2.view(2, -1)[0], torch.tensor([R.TIE_PAIRS[p % 3][1] for p in range(32)]))
    nd, _, best = R.prob_regress(torch.full((3, 256, 5, 7), 2.5))
    p = 1.0 / 256
    assert int(best.abs().max()) == 0 and R.maxdiff(nd, torch.full((1,), (10 * p) / (9 * p + 1e-6) / 255, dtype=F64)) <= 1e-15

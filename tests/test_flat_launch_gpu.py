"""The one-thread-per-item launches (csrc/flat_launch.hpp) at totals that are no multiple of the block size, and the seam of the two
launches that carry two pieces of work in one grid: where the first piece does not fill its last block, the second piece must
still start at its own item 0.  Everything is compared bit for bit with the separate entry points, which other tests hold to fp64.
Needs an MI355X: run with ``-m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S, N, H, W = 1, 2, 4, 3, 5                     # 15 pixels: no piece's item count is a multiple of 256


def ops():
    from itermvs_amd import ops as _ops
    return _ops


def rand(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_final_upsample_seam_equals_the_separate_launches():
    logits, nd, conf = 4 * rand(1, B, 144, H, W) - 2, rand(2, B, 43, H, W), rand(3, B, 1, H, W)
    inv_min, inv_max = torch.tensor([1 / 425.0], device=DEV), torch.tensor([1 / 935.0], device=DEV)
    depth, conf_up = ops().final_upsample(logits, nd, inv_min, inv_max, conf, nd_channel=32)          # 60 + 240 items
    assert torch.equal(depth, ops().convex_upsample(logits, nd, inv_min, inv_max, nd_channel=32))
    assert torch.equal(conf_up, ops().bilinear_up(conf, 4))


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("groups_last", [False, True])
def test_view_aggregate_up_seam_equals_the_separate_launches(groups_last, interleaved):
    corr, vw = rand(4, B, S, N, 8, H, W) - 0.5, rand(5, B, S, H, W)                                  # 480 (60 groups last) + 120 items
    arg = corr.permute(0, 1, 2, 4, 5, 3).contiguous().permute(0, 1, 2, 5, 3, 4) if groups_last else corr
    assert arg.is_contiguous() != groups_last and torch.equal(arg, corr)
    agg, up = ops().view_aggregate_up(arg, vw, interleaved=interleaved)
    assert torch.equal(agg, ops().view_aggregate(corr, vw))
    assert up.shape == (B, S, 2 * H, 2 * W) and up.is_contiguous() != interleaved
    assert torch.equal(up, ops().bilinear_up(vw.view(B * S, 1, H, W), 2).view(B, S, 2 * H, 2 * W))


@pytest.mark.parametrize("act", ["none", "tanh"])
@pytest.mark.parametrize("scale", [2, 4])
def test_bilinear_up_into_channel_slices_equals_bilinear_up(scale, act):
    """both kernels call the one bilinear_up_sample: same operations in the same order"""
    x = 4 * rand(6, 1, 3, 3, 5) - 2
    wide_a = torch.full((1, 7, 3 * scale, 5 * scale), 9.0, device=DEV)
    wide_b = torch.full((1, 5, 3 * scale, 5 * scale), 9.0, device=DEV)
    ops().bilinear_up_into(x, scale, wide_a[:, 2:5], wide_b[:, 1:4], act=act)
    want = ops().bilinear_up(x, scale, act=act)
    assert torch.equal(wide_a[:, 2:5], want) and torch.equal(wide_b[:, 1:4], want)
    assert bool((wide_a[:, :2] == 9).all() and (wide_a[:, 5:] == 9).all() and (wide_b[:, :1] == 9).all() and (wide_b[:, 4:] == 9).all())


@pytest.mark.parametrize("n", [5, 33])
def test_softmax_max_at_a_ragged_total(n):
    """15 items in a 64-thread (n <= 32) and a 256-thread launch.  Bound: value <= 1; n exponentials of <= 2 ulp summed in order, one
    division -- (n + 3) * 2^-24 against fp64"""
    x = 6 * rand(7, 1, n, H, W) - 3
    want = torch.softmax(x.double(), 1).max(1, keepdim=True)[0]
    got = ops().softmax_max(x)
    assert got.shape == (1, 1, H, W) and float((got.double() - want).abs().max()) <= (n + 3) * 2.0 ** -24

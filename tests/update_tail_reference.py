"""Float64 reference for the depth-update tail kernels of itermvs_amd/csrc/update.hip (prob_regress, gru_rh / gru_out,
convex_upsample / final_upsample, bilinear_up / bilinear_up2): plain torch-on-CPU restatements of models/itermvs.py:171-219,
262-264 and models/module.py:59-66, 127-152.

Every function takes ``dtype``: float64 is the reference, the same function run in float32 is the "fp32 CPU restatement"
whose distance from the reference is the rounding floor a kernel's bound is derived from (``bound``).  The input builders
of tests/test_update_tail_gpu.py live here too, so that tests/test_update_tail_reference_cpu.py can pin properties of
those inputs (how many pixels have a decided arg-max) without a GPU."""
from typing import Tuple

import torch
import torch.nn.functional as F

F64 = torch.float64
BINS = 256
RADIUS = 4


# ------------------------------------------------------------------------------------------------------------------------
# soft-max over the depth bins, first-max arg-max, +-RADIUS window regression (itermvs.py:171-190 / 201-219)
# ------------------------------------------------------------------------------------------------------------------------
def softmax_bins(logits: torch.Tensor, dtype=F64) -> torch.Tensor:
    """logits [B,K,H,W] -> probabilities over dim 1, written out (subtract the maximum, exp, divide by the sum) so that the
    float32 run does what an fp32 implementation does, whatever short-cuts the library's fused soft-max takes"""
    return _softmax(logits.detach().cpu().to(dtype), 1)


def _softmax(x: torch.Tensor, dim: int) -> torch.Tensor:
    e = (x - x.amax(dim=dim, keepdim=True)).exp()
    return e / e.sum(dim=dim, keepdim=True)


def first_argmax(prob: torch.Tensor) -> torch.Tensor:
    """[B,K,H,W] -> int64 [B,1,H,W]: the LOWEST index holding the maximum, written out instead of relying on argmax"""
    k = prob.shape[1]
    idx = torch.arange(k).view(1, k, 1, 1).expand_as(prob)
    top = prob.amax(dim=1, keepdim=True)
    return torch.where(prob == top, idx, torch.full_like(idx, k)).amin(dim=1, keepdim=True)


def window_regression(prob: torch.Tensor, radius: int = RADIUS, best=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """prob [B,K,H,W] -> (normalised depth [B,1,H,W] in prob's dtype, arg-max int64 [B,1,H,W]).  The window indices are
    clamped to [0, K-1]; a clamped index appears (and is counted) more than once; the denominator starts at 1e-6.
    ``best`` (int64 [B,1,H,W]): centre the window there instead of on the first arg-max (tests/head_reference.py asks what
    the regression would be around the runner-up of a near-tie)."""
    k = prob.shape[1]
    if best is None:
        best = first_argmax(prob)
    num = torch.zeros_like(prob[:, :1])
    den = torch.full_like(prob[:, :1], 1e-6)
    for off in range(-radius, radius + 1):
        idx = (best + off).clamp(0, k - 1)
        p = torch.gather(prob, 1, idx)
        num = num + idx.to(prob.dtype) * p
        den = den + p
    return num / den / (k - 1.0), best


def prob_regress(logits: torch.Tensor, dtype=F64):
    """-> (nd [B,1,H,W], prob [B,K,H,W], best int64 [B,1,H,W])"""
    prob = softmax_bins(logits, dtype)
    nd, best = window_regression(prob)
    return nd, prob, best


def top_two(prob: torch.Tensor):
    """-> (p1, i1, p2, i2): the largest probability with its first index and the largest among the OTHER bins"""
    i1 = first_argmax(prob)
    p1 = torch.gather(prob, 1, i1)
    rest = prob.scatter(1, i1, -1.0)
    i2 = first_argmax(rest)
    return p1, i1, torch.gather(rest, 1, i2), i2


def decided(prob: torch.Tensor, rel: float = 1e-6) -> torch.Tensor:
    """bool [B,1,H,W]: the arg-max of this pixel can be asked of an fp32 kernel -- the two largest float64 probabilities
    differ by more than ``rel`` relative, or they are exactly equal (a tie of identical logits: the lower index wins)"""
    p1, _, p2, _ = top_two(prob)
    return ((p1 - p2) > rel * p1) | (p1 == p2)


# ------------------------------------------------------------------------------------------------------------------------
# ConvGRU gate math (module.py:59-66); zr [B,2*hid,H,W] = pre-activations of z (channels :hid) and r (channels hid:)
# ------------------------------------------------------------------------------------------------------------------------
def gru_rh(zr: torch.Tensor, h: torch.Tensor, dtype=F64) -> torch.Tensor:
    """r * h, [B,hid,H,W]"""
    hid = h.shape[1]
    return torch.sigmoid(zr.detach().cpu().to(dtype)[:, hid:2 * hid]) * h.detach().cpu().to(dtype)


def gru_state(zr: torch.Tensor, q: torch.Tensor, h: torch.Tensor, dtype=F64) -> torch.Tensor:
    """(1 - z) * h + z * tanh(q), [B,hid,H,W]; q is the pre-activation of the candidate state"""
    hid = h.shape[1]
    z = torch.sigmoid(zr.detach().cpu().to(dtype)[:, :hid])
    return (1 - z) * h.detach().cpu().to(dtype) + z * torch.tanh(q.detach().cpu().to(dtype))


# ------------------------------------------------------------------------------------------------------------------------
# convex x4 up-sampling (itermvs.py:262-264, module.py:127-140) and depth un-normalisation (module.py:148-152)
# ------------------------------------------------------------------------------------------------------------------------
def convex_upsample(nd: torch.Tensor, logits: torch.Tensor, inv_min: torch.Tensor, inv_max: torch.Tensor, dtype=F64):
    """nd [B,1,H,W], logits [B,144,H,W] (channel = k*16 + i*4 + j: tap k of the 3x3 neighbourhood, sub-pixel row i and
    column j), inv_min / inv_max [B] -> (depth [B,1,4H,4W], normalised up-sampled map [B,1,4H,4W])"""
    b, _, h, w = nd.shape
    weight = _softmax(logits.detach().cpu().to(dtype).reshape(b, 1, 9, 4, 4, h, w), 2)
    x = F.pad(nd.detach().cpu().to(dtype), (1, 1, 1, 1), mode="replicate")
    x = F.unfold(x, kernel_size=3).view(b, 1, 9, 1, 1, h, w)
    up = (x * weight).sum(dim=2)                                            # [B,1,4(i),4(j),H,W]
    up = up.permute(0, 1, 4, 2, 5, 3).reshape(b, 1, 4 * h, 4 * w)           # row 4y+i, column 4x+j
    imin = inv_min.detach().cpu().to(dtype).view(b, 1, 1, 1)
    imax = inv_max.detach().cpu().to(dtype).view(b, 1, 1, 1)
    return 1.0 / (imax + up * (imin - imax)), up


# ------------------------------------------------------------------------------------------------------------------------
# F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False) for integer s, written out
# ------------------------------------------------------------------------------------------------------------------------
def _taps(n: int, scale: int, dtype):
    src = ((torch.arange(n * scale, dtype=dtype) + 0.5) / scale - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, src - i0.to(dtype)


def bilinear_up(x: torch.Tensor, scale: int, act: str = "none", dtype=F64) -> torch.Tensor:
    """x [B,C,H,W] -> [B,C,sH,sW]; ``act``: "none" or "tanh" """
    x = x.detach().cpu().to(dtype)
    y0, y1, ly = _taps(x.shape[2], scale, dtype)
    x0, x1, lx = _taps(x.shape[3], scale, dtype)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    out = top * (1 - ly) + bot * ly
    return torch.tanh(out) if act == "tanh" else out


# ------------------------------------------------------------------------------------------------------------------------
# bounds and inputs shared by the CPU and the GPU tests
# ------------------------------------------------------------------------------------------------------------------------
def maxdiff(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| in float64 (0 for empty tensors)"""
    d = (a.detach().cpu().to(F64) - b.detach().cpu().to(F64)).abs()
    return float(d.max()) if d.numel() else 0.0


def bound(project_bound: float, fp32_restatement: torch.Tensor, reference: torch.Tensor, scale=None) -> Tuple[float, float]:
    """(bound, floor): floor = max |fp32 CPU restatement - fp64 reference| on the inputs at hand (divided element-wise by
    ``scale`` for a relative quantity); bound = max(the bound the project already asserts, 4 x floor) -- the device's
    expf / tanhf / division may differ from the host's by a few ulp.  Never derived from a kernel's output."""
    d = (fp32_restatement.detach().cpu().to(F64) - reference.to(F64)).abs()
    if scale is not None:
        d = d / scale.to(F64).abs()
    floor = float(d.max()) if d.numel() else 0.0
    return max(project_bound, 4.0 * floor), floor


GRID = 2.0 ** -12
SHIFT = 90.0
PROB_SHAPES = [(3, 5, 7), (1, 1, 1), (2, 4, 8), (1, 16, 16)]
PROB_SEEDS = {(3, 5, 7): 101, (1, 1, 1): 102, (2, 4, 8): 103, (1, 16, 16): 104}
CONVEX_SIZES = [(1, 1), (1, 6), (5, 1), (3, 5), (7, 9)]


def randn(shape, scale: float, seed: int) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def grid_randn(shape, scale: float, seed: int) -> torch.Tensor:
    """randn * scale rounded to multiples of 2^-12.  For |x| < 38 both x + 90 and x - 90 are then exact in fp32 (their ulp is
    at most 2^-17), so the shifted tensor IS the shifted input and the un-shifted float64 result is its exact reference:
    a difference can only come from how the kernel subtracts the maximum, not from rounding the input."""
    x = torch.round(randn(shape, scale, seed) / GRID) * GRID
    assert float(x.abs().max()) < 38.0
    assert torch.equal((x + SHIFT).double(), x.double() + SHIFT) and torch.equal((x - SHIFT).double(), x.double() - SHIFT)
    return x


def prob_random_inputs(shape):
    """{name: logits [B,256,H,W]} of the random cases of one (B,H,W): plain randn * 4, the same on the 2^-12 grid, and the
    grid case shifted by +-90 (all three grid cases share the un-shifted float64 reference)"""
    b, h, w = shape
    seed = PROB_SEEDS[tuple(shape)]
    g = grid_randn((b, BINS, h, w), 4.0, seed + 1000)
    return {"randn4": randn((b, BINS, h, w), 4.0, seed), "grid": g, "grid+90": g + SHIFT, "grid-90": g - SHIFT}


def prob_background(b: int, h: int, w: int) -> torch.Tensor:
    """[B,256,H,W] logits in [-3,-2] on a 1/16 grid, different in neighbouring bins: a window assembled from the wrong bins
    changes the regression by far more than any bound"""
    k = torch.arange(BINS)
    return (-2.0 - ((k * 37 + 11) % 17).float() / 16.0).view(1, BINS, 1, 1).expand(b, BINS, h, w).clone()


def prob_sweep() -> torch.Tensor:
    """[1,256,16,16]: pixel k has its single peak (logit 0) at bin k -- every clamp of the window (k < 4, k > 251), every
    boundary between two 32-bin groups within reach of a window, and both ends of the arg-max reduction"""
    x = prob_background(1, 16, 16).view(1, BINS, 256)
    x[0, torch.arange(BINS), torch.arange(256)] = 0.0
    return x.view(1, BINS, 16, 16)


TIE_PAIRS = [(31, 32), (0, 255), (100, 101)]


def prob_ties(b: int = 2, h: int = 4, w: int = 8) -> torch.Tensor:
    """[B,256,H,W]: pixel p holds two identical peaks (logit 0) at TIE_PAIRS[p % 3]; the lower bin must win"""
    x = prob_background(b, h, w).view(b, BINS, h * w)
    for p in range(h * w):
        for k in TIE_PAIRS[p % 3]:
            x[:, k, p] = 0.0
    return x.view(b, BINS, h, w)

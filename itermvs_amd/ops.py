"""Tensor-level wrappers over the C ABI (one per entry point of include/itermvs_hip.h).

Every function takes CUDA (ROCm) float32 tensors, enqueues the HIP kernel on torch's current
stream and returns freshly allocated outputs (or writes into ``out=`` buffers).  There is no
CPU path: a CPU tensor raises ``RuntimeError``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import MAX_HYP, MAX_SRC, ConvParams, CorrInitParams, CorrIterParams, FMap, LevelSlots, LevelSrc, TapParams, check

Tensor = torch.Tensor


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    return t


_FEATURE_DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
FEATURE_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _feat(t: Tensor, name: str) -> int:
    """a feature map (fp32, or fp16 / bf16 STORAGE -- the kernels compute in fp32) -> its itermvs_dtype"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if t.dtype not in _FEATURE_DTYPES:
        raise RuntimeError(f"{name}: feature maps are float32, float16 or bfloat16, got {t.dtype}")
    return _FEATURE_DTYPES[t.dtype]


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def fmap(t: Tensor, name: str = "fmap") -> FMap:
    """Describe a [B,C,H,W] tensor (any strides; fp32 or 16-bit feature storage) as an ``itermvs_fmap``."""
    dt = _feat(t, name)
    if t.dim() != 4:
        raise RuntimeError(f"{name}: expected [B,C,H,W]")
    sb, sc, sy, sx = t.stride()
    return FMap(t.data_ptr(), sb, sc, sy, sx, t.shape[1], t.shape[2], t.shape[3], dt)


def level_src(views: Sequence[Tensor], name: str = "src") -> LevelSrc:
    """S source-view maps [B,C,H1,W1] sharing shape and strides -> ``itermvs_level_src``."""
    if not 1 <= len(views) <= MAX_SRC:
        raise RuntimeError(f"{name}: need 1..{MAX_SRC} source views, got {len(views)}")
    v0 = views[0]
    ls = LevelSrc()
    ls.dtype = _feat(v0, name)
    for i, v in enumerate(views):
        if _feat(v, name) != ls.dtype or v.shape != v0.shape or v.stride() != v0.stride():
            raise RuntimeError(f"{name}: all source views must share dtype, shape and strides")
        ls.view[i] = v.data_ptr()
    ls.sb, ls.sc, ls.sy, ls.sx = v0.stride()
    ls.C, ls.H, ls.W = v0.shape[1], v0.shape[2], v0.shape[3]
    return ls


class SlotSource:
    """The source views of one pyramid level read through a slot table (scan mode, ``itermvs_level_slots``): ``slab``
    [n_slots,C,H1,W1] channels-last (fp32 / fp16 / bf16 storage) holds cached maps, ``slot`` (int32 device [B,S]) says which
    slot is source view s of batch item b.  ``corr_iter`` / ``corr_init`` take it in place of the list of S views and launch
    the slot form of the kernel (same arithmetic, bit for bit)."""

    def __init__(self, slab: Tensor, slot: Tensor, name: str = "slab"):
        _feat(slab, name)
        if slab.dim() != 4 or slab.stride(1) != 1:
            raise RuntimeError(f"{name}: expected a channels-last [n_slots,C,H,W] slab")
        if not (isinstance(slot, torch.Tensor) and slot.is_cuda and slot.dtype == torch.int32 and slot.dim() == 2
                and slot.is_contiguous()):
            raise RuntimeError(f"{name}: the slot table must be a contiguous int32 device tensor [B,S]")
        if slot.device != slab.device:
            raise RuntimeError(f"{name}: slab and slot table must be on the same device")
        if not 1 <= slot.shape[1] <= MAX_SRC:
            raise RuntimeError(f"{name}: need 1..{MAX_SRC} source views, got {slot.shape[1]}")
        self.slab, self.slot, self.name = slab, slot, name

    @property
    def S(self) -> int:
        return self.slot.shape[1]

    @property
    def B(self) -> int:
        return self.slot.shape[0]

    def struct(self) -> LevelSlots:
        t = self.slab
        ls = LevelSlots()
        ls.slab, ls.slot = t.data_ptr(), self.slot.data_ptr()
        ls.slot_stride, ls.sc, ls.sy, ls.sx = t.stride()
        ls.C, ls.H, ls.W = t.shape[1], t.shape[2], t.shape[3]
        ls.dtype, ls.n_slots = _feat(t, self.name), t.shape[0]
        return ls


def channels_last(t: Tensor) -> Tensor:
    """Return ``t`` in channels-last memory format (no copy if it already is)."""
    return t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------
def compose_proj(mats: Tensor, nan_flag: Optional[Tensor] = None, depth_range=None):
    """module.py:77-90.  mats [n,V,4,4] (view 0 = reference) -> [n,V-1,12] rows of [rot|trans].
    ``depth_range`` = (depth_min [B], depth_max [B]): the same launch also returns (1/depth_min, 1/depth_max)
    (itermvs.py:240-241); the result is then (proj, inv_min, inv_max)."""
    mats = _dev(mats, "mats").contiguous()
    n, v = mats.shape[0], mats.shape[1]
    out = torch.empty((n, v - 1, 12), device=mats.device, dtype=torch.float32)
    dmin = dmax = imin = imax = None
    nb = 0
    if depth_range is not None:
        dmin, dmax = (_dev(t, "depth range").contiguous() for t in depth_range)
        nb = dmin.numel()
        imin, imax = torch.empty_like(dmin), torch.empty_like(dmax)
    check(_lib.load().itermvs_compose_proj(mats.data_ptr(), n, v, out.data_ptr(), _ptr(nan_flag), _ptr(dmin), _ptr(dmax),
                                           nb, _ptr(imin), _ptr(imax), _stream()), "itermvs_compose_proj")
    return out if depth_range is None else (out, imin, imax)


class _WarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, proj12, depth, want_mask):
        b, c, h1, w1 = src.shape
        _, n, h, w = depth.shape
        depth = depth.contiguous()
        out = torch.empty((b, c, n, h, w), device=src.device, dtype=torch.float32)
        mask = torch.empty((b, n, h, w), device=src.device, dtype=torch.uint8) if want_mask else None
        fm = fmap(src, "src_fea")
        check(_lib.load().itermvs_warp(C.byref(fm), proj12.data_ptr(), depth.data_ptr(), b, n, h, w, out.data_ptr(),
                                       _ptr(mask), _stream()), "itermvs_warp")
        ctx.save_for_backward(proj12, depth)
        ctx.src_shape = (b, c, h1, w1)
        ctx.mark_non_differentiable(*([mask] if want_mask else []))
        return (out, mask) if want_mask else out

    @staticmethod
    def backward(ctx, gout, *_):
        proj12, depth = ctx.saved_tensors
        b, c, h1, w1 = ctx.src_shape
        _, n, h, w = depth.shape
        gsrc = torch.zeros((b, c, h1, w1), device=gout.device, dtype=torch.float32)
        gout = gout.contiguous()
        check(_lib.load().itermvs_warp_backward(gout.data_ptr(), proj12.data_ptr(), depth.data_ptr(), b, c, n, h, w,
                                                h1, w1, gsrc.data_ptr(), _stream()), "itermvs_warp_backward")
        return gsrc, None, None, None


def warp(src_fea: Tensor, proj12: Tensor, depth_samples: Tensor, return_mask: bool = False):
    """module.py:68-125 on a pre-composed projection [B,12]: -> [B,C,N,H,W] (and bool mask)."""
    _dev(src_fea, "src_fea"); _dev(depth_samples, "depth_samples")
    proj12 = _dev(proj12, "proj").contiguous()
    res = _WarpFn.apply(src_fea, proj12, depth_samples, return_mask)
    if return_mask:
        return res[0], res[1].bool()
    return res


def ref_quarter(ref1: Tensor, ref2: Tensor, ref3: Tensor) -> Tensor:
    """itermvs.py:95-98: reference features of levels 1..3 on the 1/4 grid, [B,H,W,C1+C2+C3]."""
    b, _, h, w = ref2.shape
    cq = ref1.shape[1] + ref2.shape[1] + ref3.shape[1]
    out = torch.empty((b, h, w, cq), device=ref2.device, dtype=torch.float32)
    f1, f2, f3 = fmap(ref1, "ref1"), fmap(ref2, "ref2"), fmap(ref3, "ref3")
    check(_lib.load().itermvs_ref_quarter(C.byref(f1), C.byref(f2), C.byref(f3), b, out.data_ptr(), _stream()),
          "itermvs_ref_quarter")
    return out


def copy_multi(dst: Sequence[Tensor], src: Sequence[Tensor]) -> None:
    """dst[i].copy_(src[i]) for up to 8 dense tensor pairs of equal dtype and shape in ONE launch (itermvs_copy_multi)"""
    n = len(dst)
    if n == 0:
        return
    if n > 8 or len(src) != n:
        raise RuntimeError("copy_multi: 1..8 tensor pairs")
    for d, t in zip(dst, src):
        if not (isinstance(d, torch.Tensor) and isinstance(t, torch.Tensor) and d.is_cuda and t.is_cuda):
            raise RuntimeError("copy_multi: expected CUDA/ROCm tensors - the IterMVS HIP engine has no CPU path")
        if d.dtype != t.dtype or d.shape != t.shape or not d.is_contiguous() or not t.is_contiguous():
            raise RuntimeError("copy_multi: pairs must be dense tensors of equal dtype and shape")
    sp = (C.c_void_p * n)(*[t.data_ptr() for t in src])
    dp = (C.c_void_p * n)(*[d.data_ptr() for d in dst])
    nb = (C.c_int64 * n)(*[d.numel() * d.element_size() for d in dst])
    check(_lib.load().itermvs_copy_multi(sp, dp, nb, n, _stream()), "itermvs_copy_multi")


def box_probe(sink: Tensor, blocks: int, iters: int, clocks: Optional[Tensor] = None) -> None:
    """itermvs_box_probe: the fixed fp32-MFMA issue loop of bench.py's box calibration (sink: float32[blocks*256];
    clocks: int64[2] -> shader-clock ticks, 100 MHz ticks of workgroup 0)"""
    if not sink.is_cuda or sink.dtype != torch.float32 or sink.numel() < blocks * 256:
        raise RuntimeError("box_probe: sink must be a float32 CUDA/ROCm tensor of blocks*256 elements")
    check(_lib.load().itermvs_box_probe(sink.data_ptr(), blocks, iters, _ptr(clocks), _stream()), "itermvs_box_probe")


def box_chase(ring: Tensor, steps: int, start: int = 0):
    """itermvs_box_chase: (nanoseconds per dependent load along ``ring`` -- an int32 device tensor of indices forming one cycle --,
    shader clock in MHz during the walk, index where it ended)"""
    if not ring.is_cuda or ring.dtype != torch.int32:
        raise RuntimeError("box_chase: ring must be an int32 CUDA/ROCm tensor")
    out = torch.zeros((1,), device=ring.device, dtype=torch.int32)
    clocks = torch.zeros((2,), device=ring.device, dtype=torch.int64)
    check(_lib.load().itermvs_box_chase(ring.data_ptr(), start, steps, out.data_ptr(), clocks.data_ptr(), _stream()), "itermvs_box_chase")
    c = clocks.tolist()
    return float(c[0]) * 10.0 / steps, float(c[1]) / max(c[0], 1) * 100.0, int(out.item())


def clock_stamp(out: Tensor) -> None:
    """itermvs_clock_stamp: every XCD writes {100 MHz counter, shader-clock counter} to out[XCC_ID] (int64[16, 2], zeroed)"""
    if not out.is_cuda or out.dtype != torch.int64 or out.numel() != 32:
        raise RuntimeError("clock_stamp: out must be an int64 CUDA/ROCm tensor [16, 2]")
    check(_lib.load().itermvs_clock_stamp(out.data_ptr(), _stream()), "itermvs_clock_stamp")


def ref_quarter_compose(ref1: Tensor, ref2: Tensor, ref3: Tensor, mats: Tensor, nan_flag: Optional[Tensor], depth_range):
    """ref_quarter and compose_proj (with the inverse depth range) in ONE launch -- two independent pieces of work that both
    precede the correlation kernels.  Returns (ref_q, proj, inv_min, inv_max)."""
    b, _, h, w = ref2.shape
    cq = ref1.shape[1] + ref2.shape[1] + ref3.shape[1]
    out = torch.empty((b, h, w, cq), device=ref2.device, dtype=torch.float32)
    f1, f2, f3 = fmap(ref1, "ref1"), fmap(ref2, "ref2"), fmap(ref3, "ref3")
    mats = _dev(mats, "mats").contiguous()
    n, v = mats.shape[0], mats.shape[1]
    proj = torch.empty((n, v - 1, 12), device=mats.device, dtype=torch.float32)
    dmin, dmax = (_dev(t, "depth range").contiguous() for t in depth_range)
    imin, imax = torch.empty_like(dmin), torch.empty_like(dmax)
    check(_lib.load().itermvs_ref_quarter_compose(C.byref(f1), C.byref(f2), C.byref(f3), b, out.data_ptr(), mats.data_ptr(), n, v,
                                                  proj.data_ptr(), _ptr(nan_flag), dmin.data_ptr(), dmax.data_ptr(), dmin.numel(),
                                                  imin.data_ptr(), imax.data_ptr(), _stream()), "itermvs_ref_quarter_compose")
    return out, proj, imin, imax


@contextlib.contextmanager
def _untimed(bit: int):
    """the launches inside carry no timing events (itermvs_profile_*): mask ``bit`` (0: none) is off, and back on however they end"""
    lib = _lib.load()
    if bit:
        lib.itermvs_profile_set_mask(_PROFILE_MASK[0] & ~bit)
    try:
        yield
    finally:
        if bit:
            lib.itermvs_profile_set_mask(_PROFILE_MASK[0])


def _corr_iter_params(src, ref_q, proj, view_w, inv_min, inv_max, norm_depth, offsets, outs, depth=None, want_out=True):
    """The parameter block of itermvs_corr_iter / _slots / _backward.  ``outs`` None: allocated here; ``want_out=False`` (the
    backward): no output pointers.  The block carries what it points into: ``p.slots`` (the itermvs_level_slots of slot
    sources, else None), ``p.outs``, ``p.norm_depth_tensor`` (as the kernel reads it), ``p.keep`` (copies made here)."""
    b, h, w, _ = ref_q.shape
    p = CorrIterParams()
    p.slots = None
    if isinstance(src[1], SlotSource):          # scan mode: itermvs_corr_iter_slots
        if not all(isinstance(src[l], SlotSource) and src[l].B == b and src[l].S == src[1].S for l in (1, 2, 3)):
            raise RuntimeError("corr_iter: slot sources of all three levels must share the [B,S] table shape")
        s = src[1].S
        p.slots = (LevelSlots * 3)(*[src[l].struct() for l in (1, 2, 3)])
    else:
        s = len(src[1])
    p.B, p.S, p.H, p.W = b, s, h, w
    keep = []
    p.outs = []
    for i, l in enumerate((1, 2, 3)):
        if p.slots is None:
            p.src[i] = level_src(src[l], f"src level {l}")
        if depth is not None and depth.get(l) is not None:
            d = _dev(depth[l], "depth").contiguous()
            keep.append(d)
            n = d.shape[1]
            p.depth[i] = d.data_ptr()
        else:
            if offsets is None or norm_depth is None:
                raise RuntimeError("corr_iter: give either depth[l] or norm_depth + offsets[l]")
            n = len(offsets[l])
            p.depth[i] = None
            for k, o in enumerate(offsets[l]):
                p.offsets[i][k] = o
        if n > MAX_HYP:
            raise RuntimeError(f"corr_iter: at most {MAX_HYP} hypotheses per level")
        p.N[i] = n
        if want_out:
            o = outs[i] if outs is not None else torch.empty((b, n, 8, h, w), device=ref_q.device, dtype=torch.float32)
            p.outs.append(o)
            p.out[i] = o.data_ptr()
    if norm_depth is not None:
        # [B,1,H,W] view, possibly one channel of a wider contiguous [B,Ct,H,W] buffer
        _dev(norm_depth, "norm_depth")
        if norm_depth.stride(3) != 1 or norm_depth.stride(2) != w:
            norm_depth = norm_depth.contiguous()
        p.norm_depth = norm_depth.data_ptr()
        p.norm_depth_sb = norm_depth.stride(0)
    p.norm_depth_tensor = norm_depth
    proj = _dev(proj, "proj").contiguous()
    # [B,S,H,W] with any batch / view / pixel strides whose rows are dense in the pixel stride: contiguous, or the
    # interleaved [B,H,W,S] storage view_aggregate_up(interleaved=True) returns (one vector load per lane quad)
    _dev(view_w, "view_w")
    if tuple(view_w.shape) != (b, s, h, w):
        raise RuntimeError(f"corr_iter: view_w must be [B,S,H,W] = {(b, s, h, w)}, got {tuple(view_w.shape)}")
    if view_w.dtype != torch.float32 or view_w.stride(2) != w * view_w.stride(3) or min(view_w.stride()) < 1:
        view_w = view_w.float().contiguous()
    # a contiguous tensor goes as the all-zero default: the stride of a size-1 dimension is arbitrary, and the backward
    # takes nothing but the canonical contiguous strides
    if not view_w.is_contiguous():
        p.view_w_sb, p.view_w_ss, p.view_w_sp = view_w.stride(0), view_w.stride(1), view_w.stride(3)
    p.ref_q, p.proj, p.view_w = _dev(ref_q, "ref_q").data_ptr(), proj.data_ptr(), view_w.data_ptr()
    p.inv_depth_min, p.inv_depth_max = _dev(inv_min, "inv_min").data_ptr(), _dev(inv_max, "inv_max").data_ptr()
    p.keep = (keep, proj, view_w)
    return p


def _launch_corr(name: str, p) -> None:
    """itermvs_corr_iter / itermvs_corr_init (``name``) on block ``p``: the slot form when its sources are slot sources"""
    lib = _lib.load()
    if p.slots is None:
        check(getattr(lib, name)(C.byref(p), _stream()), name)
    else:
        check(getattr(lib, name + "_slots")(C.byref(p), p.slots, _stream()), name + "_slots")


def corr_iter(src: Dict[int, Sequence[Tensor]], ref_q: Tensor, proj: Tensor, view_w: Tensor,
              inv_min: Tensor, inv_max: Tensor, depth: Optional[Dict[int, Tensor]] = None,
              norm_depth: Optional[Tensor] = None, offsets: Optional[Dict[int, Sequence[float]]] = None,
              out: Optional[List[Tensor]] = None, timed: bool = True) -> List[Tensor]:
    """itermvs.py:84-120 fused (see include/itermvs_hip.h).  ``src[l]`` = S channels-last maps of
    level l; ``proj`` [3,B,S,12]; ``view_w`` [B,S,H,W]; hypotheses either explicit
    ``depth[l]`` [B,N_l,H,W] or generated from ``norm_depth`` [B,1,H,W] + ``offsets[l]``.
    Returns the three aggregated group correlations [B,N_l,8,H,W]."""
    p = _corr_iter_params(src, ref_q, proj, view_w, inv_min, inv_max, norm_depth, offsets, out, depth)
    with _untimed(0 if timed else 1):
        _launch_corr("itermvs_corr_iter", p)
    return p.outs


def _views(feat: Tensor, b: int, v: int):
    """[B*V,C,H,W] dense channels-last pyramid level -> (reference view [B,C,H,W], list of the V-1 source views), all views"""
    pv = feat.view(b, v, *feat.shape[1:])
    return pv[:, 0], [pv[:, i] for i in range(1, v)]


def _need_cl(t: Tensor, name: str) -> Tensor:
    _feat(t, name)
    if not t.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError(f"{name}: expected a dense channels-last [B*V,C,H,W] tensor")
    return t


class FeatureGradPool:
    """Shared accumulators for the feature gradients of ONE training forward.

    Every ``Evaluation`` call of a step (one initialisation + ``iteration`` iteration calls, models/itermvs.py:271-298) sends a
    gradient to the same three pyramid tensors.  As separate autograd outputs that is one zero-filled dense tensor per call
    and level plus autograd's sums (at train_dtu.sh's batch of 4: 177 MB per call, ~3 ms of element-wise kernels per step).
    With a pool the backward kernels of all calls scatter into ONE zero-filled fp32 tensor per level; ``feature_grad_sink``
    hands those to autograd once, after the last call's backward has been enqueued."""

    def __init__(self):
        self.acc = {}

    def get(self, level: int, like: Tensor) -> Tensor:
        a = self.acc.get(level)
        if a is None:
            a = self.acc[level] = torch.zeros_like(like, dtype=torch.float32)     # dense channels-last like the features
        return a


class _FeatGradSink(torch.autograd.Function):
    """identity on the three pyramid levels; its backward adds the pool's accumulators to whatever other consumers of the
    features (reference-view resampling, up-sampling head) sent.  The fused correlation Functions take THESE outputs as their
    feature inputs, so autograd runs this backward only after every one of theirs."""

    @staticmethod
    def forward(ctx, pool, f1, f2, f3):
        ctx.pool = pool
        ctx.set_materialize_grads(False)
        return f1.view_as(f1), f2.view_as(f2), f3.view_as(f3)

    @staticmethod
    def backward(ctx, g1, g2, g3):
        out = []
        for level, g in zip((1, 2, 3), (g1, g2, g3)):
            a = ctx.pool.acc.pop(level, None)
            out.append(g if a is None else (a if g is None else a.add_(g)))
        return (None,) + tuple(out)


def feature_grad_sink(pool: FeatureGradPool, feats: Dict[int, Tensor]) -> Dict[int, Tensor]:
    """route the feature gradients of every fused correlation call given ``pool=`` through ``pool`` (see FeatureGradPool)"""
    pool.acc.clear()            # a new forward: accumulators a previous (partial or failed) backward left behind are not its
    f1, f2, f3 = _FeatGradSink.apply(pool, feats[1], feats[2], feats[3])
    for t in (f1, f2, f3):
        t._itermvs_sink_pool = pool        # corr_*_train(pool=...) accepts only these tensors (_check_sink)
    return {1: f1, 2: f2, 3: f3}


def _check_sink(pool: Optional["FeatureGradPool"], feats: Sequence[Tensor], what: str) -> None:
    """``pool=`` routes the feature gradient through the pool instead of returning it: that is only sound when the features
    ARE the outputs of ``feature_grad_sink(pool, ...)`` -- otherwise the gradient would be dropped silently"""
    if pool is not None and any(getattr(t, "_itermvs_sink_pool", None) is not pool for t in feats):
        raise RuntimeError(f"{what}: pool= needs the feature tensors returned by feature_grad_sink(pool, ...)")


class _CorrIterFn(torch.autograd.Function):
    """itermvs.py:84-120 as one differentiable op: forward = itermvs_corr_iter, backward = itermvs_corr_iter_backward.
    Inputs: ref_q [B,H,W,96], proj, view_w (detached by the caller, itermvs.py:295), inverse depth range, normalised
    depth (no gradient, module.py:77), and the three channels-last pyramid levels [B*V,C_l,H_l,W_l] whose views 1..V-1 are
    the sources.  The gradient w.r.t. each level is one dense tensor the kernel scatter-adds into (view 0 stays zero).
    ``f1..f3`` are the fp32 tensors the gradient is routed to; ``s1..s3`` the tensors the kernels GATHER from -- the same
    objects for fp32 storage, their bf16 / fp16 roundings for 16-bit feature storage (BASELINE cfg 4): the gradient is
    taken at the stored values and handed to the fp32 tensors in fp32 (straight-through rounding, no 16-bit gradient)."""

    @staticmethod
    def forward(ctx, ref_q, proj, view_w, inv_min, inv_max, norm_depth, offsets, b, v, f1, f2, f3, s1, s2, s3, pool=None):
        ctx.pool = pool
        f1, f2, f3 = s1, s2, s3
        src = {l: _views(f, b, v)[1] for l, f in ((1, f1), (2, f2), (3, f3))}
        p = _corr_iter_params(src, ref_q, proj, view_w, inv_min, inv_max, norm_depth, offsets, None)
        _launch_corr("itermvs_corr_iter", p)
        ctx.save_for_backward(ref_q, proj, view_w, inv_min, inv_max, p.norm_depth_tensor, f1, f2, f3)
        ctx.meta = (offsets, b, v)
        return tuple(p.outs)

    @staticmethod
    def backward(ctx, *gouts):
        ref_q, proj, view_w, inv_min, inv_max, nd, f1, f2, f3 = ctx.saved_tensors
        offsets, b, v = ctx.meta
        feats = (f1, f2, f3)
        src = {l: _views(f, b, v)[1] for l, f in zip((1, 2, 3), feats)}
        p = _corr_iter_params(src, ref_q, proj, view_w, inv_min, inv_max, nd, offsets, None, want_out=False)
        gouts = [g.contiguous() for g in gouts]
        # dense channels-last like the features, fp32 whatever their storage type (fp32 atomics); with a pool: the step's
        # shared accumulators (FeatureGradPool), handed to autograd once by the sink
        pool = ctx.pool
        gfeat = [torch.zeros_like(f, dtype=torch.float32) if pool is None else pool.get(l, f) for l, f in zip((1, 2, 3), feats)]
        gref = torch.empty_like(ref_q)
        go = (C.c_void_p * 3)(*[g.data_ptr() for g in gouts])
        lv = [(C.c_void_p * (v - 1))(*[t.data_ptr() for t in _views(gf, b, v)[1]]) for gf in gfeat]
        gs = (C.POINTER(C.c_void_p) * 3)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in lv])
        check(_lib.load().itermvs_corr_iter_backward(C.byref(p), C.byref(go), C.byref(gs), gref.data_ptr(), _stream()),
              "itermvs_corr_iter_backward")
        return (gref, None, None, None, None, None, None, None, None) + (tuple(gfeat) if pool is None else (None, None, None)) + (None, None, None, None)


def corr_iter_train(feats: Dict[int, Tensor], b: int, v: int, ref_q: Tensor, proj: Tensor, view_w: Tensor, inv_min: Tensor,
                    inv_max: Tensor, norm_depth: Tensor, offsets: Dict[int, Sequence[float]],
                    stored: Optional[Dict[int, Tensor]] = None, pool: Optional[FeatureGradPool] = None) -> Tuple[Tensor, ...]:
    """differentiable itermvs_corr_iter: ``feats[l]`` = dense channels-last fp32 [B*V,C_l,H_l,W_l] (gradient to the source
    views) and ``ref_q`` [B,H,W,96] (gradient) -> three [B,N_l,8,H,W] tensors.  ``stored[l]``: the 16-bit copies the kernels
    gather from (feature storage bf16 / fp16); default: ``feats`` themselves.  ``pool``: ``feats`` are the outputs of
    ``feature_grad_sink(pool, ...)`` and their gradient is accumulated there instead of being returned to autograd per call."""
    _check_sink(pool, [feats[l] for l in (1, 2, 3)], "corr_iter_train")
    f = [_need_cl(_dev(feats[l], f"feature level {l}"), f"feature level {l}") for l in (1, 2, 3)]
    st = f if stored is None else [_need_cl(stored[l].detach(), f"stored feature level {l}") for l in (1, 2, 3)]
    if any(a.shape != c.shape for a, c in zip(f, st)):
        raise RuntimeError("corr_iter_train: stored features must have the shapes of the fp32 features")
    return _CorrIterFn.apply(_dev(ref_q, "ref_q").contiguous(), _dev(proj, "proj").contiguous(), _dev(view_w, "view_w").contiguous(),
                             inv_min, inv_max, norm_depth.detach(), {l: tuple(offsets[l]) for l in (1, 2, 3)}, b, v, *f, *st, pool)


def _corr_init_params(src3, ref3, proj, inv_min, inv_max, n, out, depth=None, groups_last=None):
    """The parameter block of itermvs_corr_init / _slots / _backward.  ``out`` None: no output (the backward), or, with
    ``groups_last`` False / True, allocated here in that layout.  Carries ``p.slots``, ``p.out_tensor``, ``p.keep`` likewise."""
    b, _, h, w = ref3.shape
    p = CorrInitParams()
    p.slots = None
    if isinstance(src3, SlotSource):            # scan mode: itermvs_corr_init_slots
        if src3.B != b:
            raise RuntimeError("corr_init: the slot table must have one row per batch item")
        s, p.slots = src3.S, (LevelSlots * 1)(src3.struct())
    else:
        s = len(src3)
    p.B, p.S, p.H, p.W, p.N = b, s, h, w, n
    if p.slots is None:
        p.src = level_src(src3, "src level 3")
    p.ref = fmap(ref3, "ref3")
    proj = _dev(proj, "proj").contiguous()
    p.proj = proj.data_ptr()
    if depth is not None:
        depth = _dev(depth, "depth").contiguous()
        p.N = depth.shape[1]
        p.depth = depth.data_ptr()
    p.inv_depth_min, p.inv_depth_max = _dev(inv_min, "inv_min").data_ptr(), _dev(inv_max, "inv_max").data_ptr()
    if out is None and groups_last is not None:
        out = torch.empty((b, s, p.N, h, w, 8) if groups_last else (b, s, p.N, 8, h, w), device=ref3.device, dtype=torch.float32)
        out = out.permute(0, 1, 2, 5, 3, 4) if groups_last else out
    if out is not None:
        if tuple(out.shape) != (b, s, p.N, 8, h, w) or out.dtype != torch.float32:
            raise RuntimeError(f"corr_init: out must be float32 [B,S,N,8,H,W] = {(b, s, p.N, 8, h, w)}")
        if out.is_contiguous():
            p.out_layout = 0
        elif out.permute(0, 1, 2, 4, 5, 3).is_contiguous():
            p.out_layout = 1
        else:
            raise RuntimeError("corr_init: out must be contiguous [B,S,N,8,H,W] or the view of contiguous [B,S,N,H,W,8] storage")
        p.out = out.data_ptr()
    p.out_tensor = out
    p.keep = (proj, depth)
    return p


class _CorrInitFn(torch.autograd.Function):
    """itermvs.py:48-51 (+ :11-19) as one differentiable op on the level-3 features [B*V,48,H,W] (channels-last):
    per-view group correlation [B,S,N,8,H,W]; gradient = one dense tensor (reference view gathered, sources scattered)"""

    @staticmethod
    def forward(ctx, f3, proj, inv_min, inv_max, n, b, v, s3, pool=None):
        ctx.pool = pool
        f3 = s3                 # the tensor the kernel reads (f3 itself, or its 16-bit rounding); gradient goes to f3 in fp32
        ref3, src3 = _views(f3, b, v)
        p = _corr_init_params(src3, ref3, proj, inv_min, inv_max, n, None, groups_last=False)
        _launch_corr("itermvs_corr_init", p)
        ctx.save_for_backward(f3, proj, inv_min, inv_max)
        ctx.meta = (n, b, v)
        return p.out_tensor

    @staticmethod
    def backward(ctx, gout):
        f3, proj, inv_min, inv_max = ctx.saved_tensors
        n, b, v = ctx.meta
        ref3, src3 = _views(f3, b, v)
        p = _corr_init_params(src3, ref3, proj, inv_min, inv_max, n, None)
        gout = gout.contiguous()
        gf = torch.zeros_like(f3, dtype=torch.float32) if ctx.pool is None else ctx.pool.get(3, f3)
        gref, gsrc = _views(gf, b, v)
        ptrs = (C.c_void_p * (v - 1))(*[t.data_ptr() for t in gsrc])
        check(_lib.load().itermvs_corr_init_backward(C.byref(p), gout.data_ptr(), ptrs, gref.data_ptr(), _stream()),
              "itermvs_corr_init_backward")
        return (gf if ctx.pool is None else None), None, None, None, None, None, None, None, None


def corr_init_train(f3: Tensor, b: int, v: int, proj: Tensor, inv_min: Tensor, inv_max: Tensor, num_samples: int = 32,
                    stored: Optional[Tensor] = None, pool: Optional[FeatureGradPool] = None) -> Tensor:
    """differentiable itermvs_corr_init on the dense channels-last fp32 level-3 features [B*V,48,H,W]: -> [B,S,N,8,H,W];
    ``stored``: the bf16 / fp16 copy the kernel reads (16-bit feature storage), default ``f3`` itself"""
    _check_sink(pool, [f3], "corr_init_train")
    f3 = _need_cl(_dev(f3, "feature level 3"), "feature level 3")
    s3 = f3 if stored is None else _need_cl(stored.detach(), "stored feature level 3")
    return _CorrInitFn.apply(f3, _dev(proj, "proj").contiguous(), inv_min, inv_max, num_samples, b, v, s3, pool)


class _BnReluTrainFn(torch.autograd.Function):
    """torch.nn.BatchNorm2d in train() mode (+ ReLU) as one op on the HIP kernels of csrc/bn.hip -- the ConvBnReLU / ConvBn
    layers of FeatureNet under training (models/module.py:33-50): batch statistics, running stats updated in place, the
    ReLU mask recomputed from x in the backward (nothing but x, two [C] vectors and the affine parameters is saved)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu):
        n, c = x.shape[0], x.shape[1]
        hw = x.numel() // (n * c)
        lib = _lib.load()
        ws = torch.empty((check_count(lib.itermvs_bn_workspace_floats(n, c, hw), "itermvs_bn_workspace_floats"),), device=x.device,
                         dtype=torch.float32)
        y = torch.empty_like(x)
        mean = torch.empty((c,), device=x.device, dtype=torch.float32)
        invstd = torch.empty_like(mean)
        check(lib.itermvs_bn_train_forward(x.data_ptr(), y.data_ptr(), n, c, hw, gamma.data_ptr(), beta.data_ptr(), float(eps),
                                           float(momentum), int(relu), _ptr(running_mean), _ptr(running_var), mean.data_ptr(),
                                           invstd.data_ptr(), ws.data_ptr(), _stream()), "itermvs_bn_train_forward")
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.relu = int(relu)
        for t in (running_mean, running_var):       # written by the kernel: tell autograd's version counters
            if t is not None:                       # (itermvs_amd.net invalidates its packed inference engine on them)
                torch.autograd.graph.increment_version(t)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        n, c = x.shape[0], x.shape[1]
        hw = x.numel() // (n * c)
        lib = _lib.load()
        dy = dy.contiguous()
        ws = torch.empty((check_count(lib.itermvs_bn_workspace_floats(n, c, hw), "itermvs_bn_workspace_floats"),), device=x.device,
                         dtype=torch.float32)
        dx = torch.empty_like(x)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        check(lib.itermvs_bn_train_backward(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, c, hw, gamma.data_ptr(), beta.data_ptr(),
                                            mean.data_ptr(), invstd.data_ptr(), ctx.relu, dgamma.data_ptr(), dbeta.data_ptr(),
                                            ws.data_ptr(), _stream()), "itermvs_bn_train_backward")
        return dx, dgamma, dbeta, None, None, None, None, None


def check_count(value: int, what: str) -> int:
    """a C entry point that returns a non-negative count or a negative error code"""
    if value < 0:
        check(value, what)
    return value


def bn_relu_train(x: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                  eps: float = 1e-5, momentum: float = 0.1, relu: bool = True) -> Tensor:
    """``relu(F.batch_norm(x, running_mean, running_var, gamma, beta, training=True, momentum, eps))`` (``relu=False``: without
    the ReLU) on dense NCHW fp32 ``x``; differentiable w.r.t. x, gamma, beta; the running statistics are updated in place."""
    x = _dev(x, "x")
    if x.dim() < 2:
        raise RuntimeError("bn_relu_train: expected [N,C,...]")
    for t, name in ((gamma, "gamma"), (beta, "beta")):
        if _dev(t, name).shape != (x.shape[1],):
            raise RuntimeError(f"bn_relu_train: {name} must have shape [{x.shape[1]}]")
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and (_dev(t, name).shape != (x.shape[1],) or not t.is_contiguous()):
            raise RuntimeError(f"bn_relu_train: {name} must be a contiguous [{x.shape[1]}] tensor")
    return _BnReluTrainFn.apply(x.contiguous(), gamma.contiguous(), beta.contiguous(), running_mean, running_var, eps, momentum, relu)


def corr_iter_kernel_name() -> str:
    """name of the device kernel itermvs_corr_iter launches (rocprofv3's Kernel_Name contains it)"""
    return "corr_iter_kernel"


def corr_init(src3: Sequence[Tensor], ref3: Tensor, proj: Tensor, inv_min: Tensor, inv_max: Tensor,
              num_samples: int = 32, depth: Optional[Tensor] = None, out: Optional[Tensor] = None,
              timed: bool = True, groups_last: bool = False) -> Tensor:
    """itermvs.py:48-51 (+ :11-19): per-view group correlation, [B,S,N,8,H,W].  ``groups_last``: STORED [B,S,N,H,W,8] and returned
    as the [B,S,N,8,H,W] view of that storage -- as [B*S*N,8,H,W] it is a channels-last tensor, which conv2d's 8-channel bf16x3
    layer stages with two 16-byte loads per pixel, and view_aggregate(_up) reads it as it is."""
    p = _corr_init_params(src3, ref3, proj, inv_min, inv_max, num_samples, out, depth, groups_last=bool(groups_last))
    with _untimed(0 if timed else 2):
        _launch_corr("itermvs_corr_init", p)
    return p.out_tensor


def tap_indices(proj: Tensor, inv_min: Tensor, inv_max: Tensor, grid_hw: Tuple[int, int], src_hw: Tuple[int, int], *,
                depth: Optional[Tensor] = None, norm_depth: Optional[Tensor] = None, offsets: Sequence[float] = (),
                init_samples: int = 0, want_coords: bool = False):
    """Diagnostic (itermvs_tap_indices): floor(ix), floor(iy) and the validity bits of the bilinear footprints exactly as
    the fused correlation kernels compute them (module.py:99-115 + grid_sample's floor).  proj [B,S,12]; hypotheses from
    ``depth`` [B,N,h,w], or ``init_samples`` initial planes, or ``norm_depth`` [B,1,h,w] + ``offsets``.
    -> int32 [B,S,N,3,h,w] (x0, y0, bits)  (+ float [B,S,N,2,h,w] coordinates with ``want_coords``)."""
    proj = _dev(proj, "proj").contiguous()
    b, s = proj.shape[0], proj.shape[1]
    h, w = grid_hw
    p = TapParams()
    p.B, p.S, p.H, p.W, p.H1, p.W1 = b, s, h, w, src_hw[0], src_hw[1]
    p.proj = proj.data_ptr()
    if depth is not None:
        depth = _dev(depth, "depth").contiguous()
        p.N = depth.shape[1]
        p.depth = depth.data_ptr()
    elif init_samples:
        p.N, p.init = init_samples, 1
    else:
        nd = _dev(norm_depth, "norm_depth")
        if nd.stride(-1) != 1 or nd.stride(-2) != w:
            nd = nd.contiguous()
        p.N = len(offsets)
        p.norm_depth, p.norm_depth_sb = nd.data_ptr(), nd.stride(0)
        for i, o in enumerate(offsets):
            p.offsets[i] = o
    p.inv_depth_min, p.inv_depth_max = _dev(inv_min, "inv_min").data_ptr(), _dev(inv_max, "inv_max").data_ptr()
    out = torch.empty((b, s, p.N, 3, h, w), device=proj.device, dtype=torch.int32)
    coords = torch.empty((b, s, p.N, 2, h, w), device=proj.device, dtype=torch.float32) if want_coords else None
    p.out, p.coords = out.data_ptr(), _ptr(coords)
    check(_lib.load().itermvs_tap_indices(C.byref(p), _stream()), "itermvs_tap_indices")
    return (out, coords) if want_coords else out


def view_aggregate(corr: Tensor, w: Tensor) -> Tensor:
    """itermvs.py:59-69.  corr [B,S,N,8,H,W], w [B,S,H,W] -> [B,N,8,H,W]."""
    b, s, n, g, h, wd = corr.shape
    corr = _dev(corr, "corr").contiguous()
    w = _dev(w, "w").contiguous()
    out = torch.empty((b, n, g, h, wd), device=corr.device, dtype=torch.float32)
    check(_lib.load().itermvs_view_aggregate(corr.data_ptr(), w.data_ptr(), s, b, n, h * wd, out.data_ptr(), _stream()),
          "itermvs_view_aggregate")
    return out


def view_aggregate_up(corr: Tensor, w: Tensor, interleaved: bool = False) -> Tuple[Tensor, Tensor]:
    """view_aggregate and, in the same launch, the x2 bilinear up-sampling of the view weights (itermvs.py:56-57,71):
    corr [B,S,N,8,H,W], w [B,S,H,W] -> ([B,N,8,H,W], [B,S,2H,2W]).  ``interleaved``: the up-sampled weights are STORED
    [B,2H,2W,S] and returned as the permuted [B,S,2H,2W] view of that storage -- same values, the layout corr_iter reads with
    one vector load per lane quad.  ``corr`` may be corr_init(..., groups_last=True)'s view of [B,S,N,H,W,8] storage."""
    b, s, n, g, h, wd = corr.shape
    _dev(corr, "corr")
    corr_layout = 1 if (g == 8 and not corr.is_contiguous() and corr.permute(0, 1, 2, 4, 5, 3).is_contiguous()) else 0
    if corr_layout == 0:
        corr = corr.contiguous()
    w = _dev(w, "w").contiguous()
    out = torch.empty((b, n, g, h, wd), device=corr.device, dtype=torch.float32)
    if interleaved:
        store = torch.empty((b, 2 * h, 2 * wd, s), device=corr.device, dtype=torch.float32)
        w_up = store.permute(0, 3, 1, 2)
    else:
        store = w_up = torch.empty((b, s, 2 * h, 2 * wd), device=corr.device, dtype=torch.float32)
    check(_lib.load().itermvs_view_aggregate_up(corr.data_ptr(), corr_layout, w.data_ptr(), s, b, n, h, wd, out.data_ptr(), store.data_ptr(),
                                                1 if interleaved else 0, _stream()), "itermvs_view_aggregate_up")
    return out, w_up


def pvw_tail(x: Tensor, weight: Tensor, bias: Optional[Tensor], n_hyp: int) -> Tensor:
    """itermvs.py:343-348 fused: x [M*N,16,h,w] (after the 3x3 layer + ReLU), weight [1,16,1,1] -> [M,1,h,w]."""
    _dev(x, "x")
    mn, c, h, w = x.shape
    if mn % n_hyp or not x.is_contiguous():
        raise RuntimeError("pvw_tail: x must be contiguous [M*N,C,H,W]")
    m = mn // n_hyp
    out = torch.empty((m, 1, h, w), device=x.device, dtype=torch.float32)
    wv = _dev(weight, "weight").reshape(-1).contiguous()
    check(_lib.load().itermvs_pvw_tail(x.data_ptr(), wv.data_ptr(), _ptr(bias), m, n_hyp, c, h * w, out.data_ptr(), _stream()),
          "itermvs_pvw_tail")
    return out


def softmax_max(x: Tensor) -> Tensor:
    """itermvs.py:347-348.  x [M,N,H,W] -> max over N of softmax over N, [M,1,H,W]."""
    x = _dev(x, "x").contiguous()
    m, n, h, w = x.shape
    out = torch.empty((m, 1, h, w), device=x.device, dtype=torch.float32)
    check(_lib.load().itermvs_softmax_max(x.data_ptr(), m, n, h * w, out.data_ptr(), _stream()), "itermvs_softmax_max")
    return out


def pack_head_weights(w1: Tensor, w2: Tensor) -> Tuple[Tensor, Tensor]:
    """depth_head[2].weight [64,32,1,1], depth_head[4].weight [256,64,1,1] -> the matrix-core operand
    layouts of itermvs_head_regress (include/itermvs_hip.h)."""
    a1 = w1.reshape(4, 16, 2, 4, 4).permute(0, 2, 3, 1, 4).contiguous()     # [mb,i,u,q,s] -> [mb,u,q,i,s]
    a2 = w2.reshape(16, 16, 4, 4, 4).permute(0, 2, 3, 1, 4).contiguous()    # [mb,i,m,q,r] -> [mb,m,q,i,r]
    return a1, a2


def pack_head_w2_split3(w2: Tensor) -> Tensor:
    """depth_head[4].weight [256,64,1,1] -> the bf16x3 A operands of itermvs_head_fused's 64 -> 256 layer (w2_format 3):
    bfloat16 [16][2][3][64][8] whose element (ob, g, p, lane = 16 q + i, j) is term p (h, m, l of ``split_bf16x3``) of
    W2[ob*16 + i][(2g + j//4)*16 + 4q + j%4]."""
    if w2.numel() != 256 * 64:
        raise RuntimeError("pack_head_w2_split3: expects the [256,64,1,1] weight")
    t = w2.reshape(16, 16, 2, 2, 4, 4).float()                    # [ob, i, g, jj, q, r]: channel (2g + jj)*16 + 4q + r
    t = t.permute(0, 2, 4, 1, 3, 5).reshape(16, 2, 64, 8)         # [ob, g, (q, i), (jj, r)]
    return torch.stack(split_bf16x3(t), 2).contiguous()           # [16, 2, 3, 64, 8]


def pack_head_w0_split3(w0: Tensor) -> Tensor:
    """depth_head[0].weight [32,32,3,3] (dilated 3x3) -> the bf16x3 A operands of itermvs_head_fused's first layer (w0_format 3):
    bfloat16 [2][9][3][64][8] whose element (mb, tap, p, lane = 16 q + i, j) is term p of W0[16 mb + i][(j//4)*16 + 4q + j%4][tap]."""
    if tuple(w0.shape) != (32, 32, 3, 3):
        raise RuntimeError("pack_head_w0_split3: expects the [32,32,3,3] weight")
    t = w0.float().reshape(2, 16, 2, 4, 4, 9).permute(0, 5, 3, 1, 2, 4).reshape(2, 9, 64, 8)      # [mb, tap, (q, i), (jj, r)]
    return torch.stack(split_bf16x3(t), 2).contiguous()                                            # [2, 9, 3, 64, 8]


def pack_conv1x1_operand(w1: Tensor, bias: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """Conv2d(64, NO, 1) weight [NO,64,1,1] (+ bias [NO]) -> the matrix-core operand layout of itermvs_conv3x3_conv1x1:
    [NOB][4][4][16][4] with element (ob,m,q,i,r) = W1[ob*16+i][m*16+q*4+r], NO zero-padded to NOB*16 (bias likewise)."""
    no, ci = w1.shape[0], w1.shape[1]
    if ci != 64 or w1.numel() != no * 64:
        raise RuntimeError("pack_conv1x1_operand: expects a [NO,64,1,1] weight")
    nob = (no + 15) // 16
    full = torch.zeros((nob * 16, 64), device=w1.device, dtype=torch.float32)
    full[:no] = w1.reshape(no, 64).float()
    a = full.reshape(nob, 16, 4, 4, 4).permute(0, 2, 3, 1, 4).contiguous()     # [ob,i,m,q,r] -> [ob,m,q,i,r]
    bp = None
    if bias is not None:
        bp = torch.zeros((nob * 16,), device=w1.device, dtype=torch.float32)
        bp[:no] = bias.float()
    return a, bp


def pack_conv3x3_conv1x1_split3(w0: Tensor, w1: Tensor, bias: Optional[Tensor] = None):
    """Conv2d(32, 64, 3) weight [64,32,3,3] and Conv2d(64, NO, 1) weight [NO,64,1,1] (+ bias) -> the bf16x3 operands of
    itermvs_conv3x3_conv1x1 (weight_format 3): (bf16 [4][9][3][64][8], bf16 [NOB][2][3][64][8], fp32 bias [NOB*16] | None).  A lane
    (q, i) holds, as its eight K slots j of a 32-channel group, the channels (j // 4) * 16 + 4 q + j % 4."""
    if tuple(w0.shape) != (64, 32, 3, 3) or w1.shape[1] != 64 or w1.numel() != w1.shape[0] * 64:
        raise RuntimeError("pack_conv3x3_conv1x1_split3: expects [64,32,3,3] and [NO,64,1,1] weights")
    t0 = w0.float().reshape(4, 16, 2, 4, 4, 9)                       # [w, i, jj, q, r, tap]: input channel jj*16 + 4q + r
    t0 = t0.permute(0, 5, 3, 1, 2, 4).reshape(4, 9, 64, 8)           # [w, tap, (q, i), (jj, r)]
    a0 = torch.stack(split_bf16x3(t0), 2).contiguous()               # [4, 9, 3, 64, 8]
    no = w1.shape[0]
    nob = (no + 15) // 16
    full = torch.zeros((nob * 16, 64), device=w1.device, dtype=torch.float32)
    full[:no] = w1.reshape(no, 64).float()
    t1 = full.reshape(nob, 16, 2, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(nob, 2, 64, 8)      # [ob, g, (q, i), (jj, r)]
    a1 = torch.stack(split_bf16x3(t1), 2).contiguous()               # [nob, 2, 3, 64, 8]
    bp = None
    if bias is not None:
        bp = torch.zeros((nob * 16,), device=w1.device, dtype=torch.float32)
        bp[:no] = bias.float()
    return a0, a1, bp


def conv3x3_conv1x1(x: Tensor, w0, w1p: Tensor, bias_p: Optional[Tensor], no: int, out: Optional[Tensor] = None) -> Tensor:
    """itermvs_conv3x3_conv1x1: conv3x3 32 -> 64 + ReLU + conv1x1 64 -> ``no`` in one launch; x [B,32,H,W] -> [B,no,H,W].
    ``w0``: the 3x3 layer's MfmaWeight (fp32 tile format) with ``w1p`` / ``bias_p`` from pack_conv1x1_operand (exact fp32 matrix
    instruction), or both bfloat16 tensors of pack_conv3x3_conv1x1_split3 (bf16x3 arithmetic)."""
    ptr, sb = _planes(x, "conv3x3_conv1x1 input")
    b, c, h, w = x.shape
    nob = (no + 15) // 16
    if isinstance(w0, Tensor):
        if not (w0.is_cuda and w1p.is_cuda and w0.dtype == w1p.dtype == torch.bfloat16 and tuple(w0.shape) == (4, 9, 3, 64, 8)
                and tuple(w1p.shape) == (nob, 2, 3, 64, 8) and w0.is_contiguous() and w1p.is_contiguous()) or c != 32:
            raise RuntimeError("conv3x3_conv1x1: bfloat16 weights must come from pack_conv3x3_conv1x1_split3 for this output width")
        if bias_p is not None and bias_p.numel() != nob * 16:
            raise RuntimeError("conv3x3_conv1x1: bias_p must come from pack_conv3x3_conv1x1_split3")
        if out is None:
            out = torch.empty((b, no, h, w), device=x.device, dtype=torch.float32)
        elif tuple(out.shape) != (b, no, h, w):
            raise RuntimeError(f"conv3x3_conv1x1: output has shape {tuple(out.shape)}, expected {(b, no, h, w)}")
        po, so = _planes(out, "conv3x3_conv1x1 output")
        check(_lib.load().itermvs_conv3x3_conv1x1(ptr, sb, b, h, w, w0.data_ptr(), w1p.data_ptr(), 3, _ptr(bias_p), no, po, so, _stream()),
              "itermvs_conv3x3_conv1x1")
        return out
    if c != 32 or w0.tile is None or w0.cin != 32 or w0.cout != 64 or w0.ksize != 3:
        raise RuntimeError("conv3x3_conv1x1: expects a 32-channel input and the 32 -> 64 3x3 weight")
    if w1p.numel() != nob * 1024 or (bias_p is not None and bias_p.numel() != nob * 16):
        raise RuntimeError("conv3x3_conv1x1: w1p / bias_p must come from pack_conv1x1_operand for this output width")
    if out is None:
        out = torch.empty((b, no, h, w), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (b, no, h, w):
        raise RuntimeError(f"conv3x3_conv1x1: output has shape {tuple(out.shape)}, expected {(b, no, h, w)}")
    po, so = _planes(out, "conv3x3_conv1x1 output")
    check(_lib.load().itermvs_conv3x3_conv1x1(ptr, sb, b, h, w, w0.tile.data_ptr(), _dev(w1p, "w1p").data_ptr(), 0, _ptr(bias_p), no,
                                              po, so, _stream()), "itermvs_conv3x3_conv1x1")
    return out


def pack_gru_conv_split3(w: Tensor) -> Tensor:
    """ConvGRU 3x3 weight [NO,43,3,3] (NO = 64: convz and convr stacked; 32: convq) -> the bf16x3 operands of itermvs_gru_conv:
    bfloat16 [NO/16][9][6][64][8].  Operands 0..2: terms h, m, l of input channel (j // 4) * 16 + 4 q + j % 4 (lane = 16 q + i,
    output channel 16 ob + i); operands 3..5: channel 32 + 8 (q % 2) + j (zero from 43 on), terms h, m and (l if q < 2 else h)."""
    no = w.shape[0]
    if tuple(w.shape[1:]) != (43, 3, 3) or no % 16:
        raise RuntimeError("pack_gru_conv_split3: expects a [16 k, 43, 3, 3] weight")
    nob = no // 16
    wf = w.float().reshape(nob, 16, 43, 9)
    ta = wf[:, :, :32].reshape(nob, 16, 2, 4, 4, 9).permute(0, 5, 3, 1, 2, 4).reshape(nob, 9, 64, 8)      # [ob, tap, (q, i), (jj, r)]
    ah, am, al = split_bf16x3(ta)
    full = torch.zeros((nob, 16, 16, 9), device=w.device, dtype=torch.float32)
    full[:, :, :11] = wf[:, :, 32:]
    tb = full.reshape(nob, 16, 2, 8, 9).permute(0, 4, 2, 1, 3)                                             # [ob, tap, half, i, j]
    tb = torch.stack([tb, tb], 2).reshape(nob, 9, 64, 8)                                                   # q = 2 second + half
    bh, bm, bl = split_bf16x3(tb)
    b3 = torch.cat([bl.reshape(nob, 9, 4, 16, 8)[:, :, :2], bh.reshape(nob, 9, 4, 16, 8)[:, :, 2:]], 2).reshape(nob, 9, 64, 8)
    return torch.stack([ah, am, al, bh, bm, b3], 2).contiguous()


def gru_conv(x: Tensor, wp: Tensor, bias: Optional[Tensor], h: Tensor, out: Tensor, out2: Optional[Tensor] = None,
             z: Optional[Tensor] = None) -> None:
    """itermvs_gru_conv.  ``z`` None: the update / reset gates (``wp`` [4,9,6,64,8]): x = [h | inputs] [B,43,H,W] ->
    out = z, out2 = r * h.  ``z`` given: the candidate state and the update (``wp`` [2,9,6,64,8]): x = [r*h | inputs] ->
    out (= out2 if given) = (1 - z) h + z tanh(convq(x))  (models/module.py:59-66)."""
    px, sx = _planes(x, "gru_conv input")
    b, c, hh, ww = x.shape
    mode = 0 if z is None else 1
    nob = 4 if mode == 0 else 2
    if c != 43 or not (wp.is_cuda and wp.dtype == torch.bfloat16 and tuple(wp.shape) == (nob, 9, 6, 64, 8) and wp.is_contiguous()):
        raise RuntimeError("gru_conv: expects a 43-channel input and the weights of pack_gru_conv_split3")
    if bias is not None and bias.numel() != 16 * nob:
        raise RuntimeError("gru_conv: bias size")
    if mode == 0 and out2 is None:
        raise RuntimeError("gru_conv: the gate form needs both outputs")
    for t in (h, out, out2, z):
        if t is not None and tuple(t.shape) != (b, 32, hh, ww):
            raise RuntimeError(f"gru_conv: expected [B,32,H,W] tensors, got {tuple(t.shape)}")
    ph, sh = _planes(h, "gru_conv h")
    po, so = _planes(out, "gru_conv out")
    po2, so2 = _planes(out2, "gru_conv out2") if out2 is not None else (None, 0)
    pz, sz = _planes(z, "gru_conv z") if z is not None else (None, 0)
    check(_lib.load().itermvs_gru_conv(px, sx, b, hh, ww, mode, wp.data_ptr(), _ptr(bias), ph, sh, pz, sz, po, so, po2, so2, _stream()),
          "itermvs_gru_conv")
    if CONV_FLOP_COUNTER["enabled"]:         # the dilated 3x3 layer(s) over the 43 input channels, one bracketed launch
        CONV_FLOP_COUNTER["flops"] += 2.0 * b * hh * ww * 16 * nob * 43 * 9
        CONV_FLOP_COUNTER["launches"] += 1


def head_regress(x: Tensor, w1p: Tensor, w2p: Tensor, bias2: Tensor,
                 nd_out: Optional[Sequence[Tuple[Tensor, int]]] = None, want_best: bool = False):
    """itermvs_head_regress: x [B,32,H,W] (after depth_head[0:2]) -> normalised depth (and arg-max bin),
    written like prob_regress's ``nd_out``.  Returns (nd | None, best | None)."""
    _dev(x, "x")
    b, c, h, w = x.shape
    if c != 32:
        raise RuntimeError("head_regress: expects the 32-channel depth-head feature")
    ptr, sb = _planes(x, "head input")
    p = h * w
    nd, dests = None, []
    if nd_out is None:
        nd = torch.empty((b, 1, h, w), device=x.device, dtype=torch.float32)
        dests.append((nd.data_ptr(), p))
    else:
        for buf, ch in nd_out:
            _dev(buf, "nd_out")
            assert buf.is_contiguous() and buf.shape[2:] == (h, w)
            dests.append((buf.data_ptr() + 4 * ch * p, buf.shape[1] * p))
    while len(dests) < 2:
        dests.append((None, 0))
    best = torch.empty((b, 1, h, w), device=x.device, dtype=torch.int64) if want_best else None
    check(_lib.load().itermvs_head_regress(ptr, sb, b, p, _dev(w1p, "w1").data_ptr(), _dev(w2p, "w2").data_ptr(),
                                           _dev(bias2, "bias2").data_ptr(), dests[0][0], dests[0][1], dests[1][0],
                                           dests[1][1], _ptr(best), _stream()), "itermvs_head_regress")
    return nd, best


def head_fused(hidden: Tensor, w0, w1p: Tensor, w2p: Tensor, bias2: Tensor,
               nd_out: Optional[Sequence[Tuple[Tensor, int]]] = None, want_best: bool = False, conf=None):
    """itermvs_head_fused: hidden [B,32,H,W] -> normalised depth (and arg-max bin); the dilated 3x3 layer (``w0``: its
    MfmaWeight), both 1x1 layers and the regression in one launch.  Returns (nd | None, best | None).
    ``conf`` = (MfmaWeight of confidence_head[0], its 1x1 layer as 33 floats {w, bias}, out [B,1,H,W]): itermvs_head_fused_conf,
    the confidence head (itermvs.py:147-151,198) rides in the same launch and writes sigmoid(...) to ``out``."""
    _dev(hidden, "hidden")
    b, c, h, w = hidden.shape
    if isinstance(w0, Tensor):               # pack_head_w0_split3: the dilated 3x3 layer in bf16x3 (needs the bf16x3 w2, no conf rider)
        if not (w0.is_cuda and w0.dtype == torch.bfloat16 and tuple(w0.shape) == (2, 9, 3, 64, 8) and w0.is_contiguous()) or c != 32:
            raise RuntimeError("head_fused: a tensor w0 must come from pack_head_w0_split3")
        if conf is not None or not (isinstance(w2p, Tensor) and w2p.dtype == torch.bfloat16):
            raise RuntimeError("head_fused: the bf16x3 3x3 layer needs the bf16x3 last layer (pack_head_w2_split3) and no confidence rider")
        w0_ptr, w0_format = w0.data_ptr(), 3
    else:
        if c != 32 or w0.tile is None or w0.cin != 32 or w0.cout != 32:
            raise RuntimeError("head_fused: expects the 32-channel hidden state and the 32 -> 32 3x3 weight")
        w0_ptr, w0_format = w0.tile.data_ptr(), 0
    ptr, sb = _planes(hidden, "hidden")
    p = h * w
    if not isinstance(w2p, torch.Tensor) or not w2p.is_cuda:
        raise RuntimeError("w2: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if w2p.dtype == torch.bfloat16:          # pack_head_w2_split3: the 64 -> 256 layer in the bf16x3 form
        if tuple(w2p.shape) != (16, 2, 3, 64, 8) or not w2p.is_contiguous():
            raise RuntimeError("head_fused: a bfloat16 w2 must come from pack_head_w2_split3")
        w2_format = 3
    elif w2p.dtype == torch.float32 and w2p.numel() == 256 * 64 and w2p.is_contiguous():
        w2_format = 0
    else:
        raise RuntimeError("head_fused: w2 must come from pack_head_weights (float32) or pack_head_w2_split3 (bfloat16)")
    nd, dests = None, []
    if nd_out is None:
        nd = torch.empty((b, 1, h, w), device=hidden.device, dtype=torch.float32)
        dests.append((nd.data_ptr(), p))
    else:
        for buf, ch in nd_out:
            _dev(buf, "nd_out")
            assert buf.is_contiguous() and buf.shape[2:] == (h, w)
            dests.append((buf.data_ptr() + 4 * ch * p, buf.shape[1] * p))
    while len(dests) < 2:
        dests.append((None, 0))
    best = torch.empty((b, 1, h, w), device=hidden.device, dtype=torch.int64) if want_best else None
    if conf is not None:
        wc, cdot, cout = conf
        if wc.tile is None or wc.cin != 32 or wc.cout != 32 or cdot.numel() != 33 or tuple(cout.shape) != (b, 1, h, w) or not cout.is_contiguous():
            raise RuntimeError("head_fused: conf = (32 -> 32 3x3 MfmaWeight in the fp32 tile format, 33 floats, contiguous [B,1,H,W] output)")
        check(_lib.load().itermvs_head_fused_conf(ptr, sb, b, h, w, w0_ptr, _dev(w1p, "w1").data_ptr(),
                                                  w2p.data_ptr(), w2_format, _dev(bias2, "bias2").data_ptr(), dests[0][0], dests[0][1],
                                                  dests[1][0], dests[1][1], _ptr(best), wc.tile.data_ptr(), _dev(cdot, "conf_dot").data_ptr(),
                                                  _dev(cout, "conf").data_ptr(), p, _stream()), "itermvs_head_fused_conf")
        return nd, best
    check(_lib.load().itermvs_head_fused(ptr, sb, b, h, w, w0_ptr, w0_format, _dev(w1p, "w1").data_ptr(),
                                         w2p.data_ptr(), w2_format, _dev(bias2, "bias2").data_ptr(), dests[0][0], dests[0][1],
                                         dests[1][0], dests[1][1], _ptr(best), _stream()), "itermvs_head_fused")
    return nd, best


def prob_regress(logits: Tensor, nd_out: Optional[Sequence[Tuple[Tensor, int]]] = None, want_prob: bool = False,
                 want_best: bool = False):
    """itermvs.py:171-190 / 201-219.  logits [B,256,H,W] (NCHW or channels-last).
    ``nd_out``: up to two (buffer [B,Ct,H,W] contiguous, channel) destinations written in place;
    default: a fresh [B,1,H,W].  Returns (nd, prob | None, best | None)."""
    _dev(logits, "logits")
    b, k, h, w = logits.shape
    if k != 256:
        raise RuntimeError("prob_regress: expects 256 bins")
    sb, sc, sy, sx = logits.stride()
    if sy != w * sx:
        logits = logits.contiguous()
        sb, sc, sy, sx = logits.stride()
    p = h * w
    nd = None
    dests = []
    if nd_out is None:
        nd = torch.empty((b, 1, h, w), device=logits.device, dtype=torch.float32)
        dests.append((nd.data_ptr(), p))
    else:
        for buf, ch in nd_out:
            _dev(buf, "nd_out")
            assert buf.is_contiguous() and buf.shape[2:] == (h, w)
            dests.append((buf.data_ptr() + 4 * ch * p, buf.shape[1] * p))
    while len(dests) < 2:
        dests.append((None, 0))
    prob = torch.empty((b, 256, h, w), device=logits.device, dtype=torch.float32) if want_prob else None
    best = torch.empty((b, 1, h, w), device=logits.device, dtype=torch.int64) if want_best else None
    check(_lib.load().itermvs_prob_regress(logits.data_ptr(), sb, sc, sx, b, p, dests[0][0], dests[0][1], dests[1][0],
                                           dests[1][1], _ptr(prob), _ptr(best), _stream()), "itermvs_prob_regress")
    return nd, prob, best


def gru_rh(zr: Tensor, h_buf: Tensor, rh_buf: Tensor, hid: int = 32) -> None:
    """module.py:63-64: rh_buf[:, :hid] = sigmoid(zr[:, hid:]) * h_buf[:, :hid]  (buffers [B,Ct,H,W])."""
    b, _, h, w = zr.shape
    p = h * w
    assert zr.is_contiguous() and h_buf.is_contiguous() and rh_buf.is_contiguous()
    check(_lib.load().itermvs_gru_rh(_dev(zr, "zr").data_ptr(), _dev(h_buf, "h").data_ptr(), h_buf.shape[1] * p,
                                     _dev(rh_buf, "rh").data_ptr(), rh_buf.shape[1] * p, b, hid, p, _stream()),
          "itermvs_gru_rh")


def gru_out(zr: Tensor, q: Tensor, h_buf: Tensor, h_copy: Optional[Tensor] = None, hid: int = 32) -> None:
    """module.py:62,65: h_buf[:, :hid] = (1-z)*h + z*tanh(q), in place; ``h_copy`` [B,hid,H,W]
    optionally receives a contiguous copy of the new state."""
    b, _, h, w = zr.shape
    p = h * w
    assert zr.is_contiguous() and q.is_contiguous() and h_buf.is_contiguous()
    assert h_copy is None or (h_copy.is_contiguous() and h_copy.shape == (b, hid, h, w))
    check(_lib.load().itermvs_gru_out(_dev(zr, "zr").data_ptr(), _dev(q, "q").data_ptr(), _dev(h_buf, "h").data_ptr(),
                                      h_buf.shape[1] * p, _ptr(h_copy), b, hid, p, _stream()), "itermvs_gru_out")


def pack_scores(scores: Sequence[Tensor], dst0: Tensor, dst1: Optional[Tensor], ch0: int) -> None:
    """itermvs.py:124,193: write the three CorrNet outputs [B,N_l,H,W] into channels ch0.. of the buffers."""
    b, _, h, w = scores[0].shape
    n = (C.c_int32 * 3)(*[s.shape[1] for s in scores])
    sc = [_dev(s, "score").contiguous() for s in scores]
    assert dst0.is_contiguous() and (dst1 is None or (dst1.is_contiguous() and dst1.shape == dst0.shape))
    check(_lib.load().itermvs_pack_scores(sc[0].data_ptr(), sc[1].data_ptr(), sc[2].data_ptr(), n, b, h * w,
                                          dst0.data_ptr(), _ptr(dst1), dst0.shape[1] * h * w, ch0, _stream()),
          "itermvs_pack_scores")


def convex_upsample(logits: Tensor, nd: Tensor, inv_min: Tensor, inv_max: Tensor, nd_channel: int = 0,
                    want_norm: bool = False):
    """itermvs.py:262-264 + module.py:127-140 + :148-152.  logits [B,144,H,W] (raw, pre-softmax),
    nd = buffer [B,Ct,H,W] whose channel ``nd_channel`` holds the normalised depth.
    -> depth [B,1,4H,4W] (and the normalised up-sampled map if ``want_norm``)."""
    _dev(logits, "logits"); _dev(nd, "nd")
    b, k, h, w = logits.shape
    assert k == 144 and nd.is_contiguous()
    sb, sc, sy, sx = logits.stride()
    depth = torch.empty((b, 1, 4 * h, 4 * w), device=logits.device, dtype=torch.float32)
    norm = torch.empty_like(depth) if want_norm else None
    check(_lib.load().itermvs_convex_upsample(logits.data_ptr(), sb, sc, sy, sx, nd.data_ptr() + 4 * nd_channel * h * w,
                                              nd.shape[1] * h * w, _dev(inv_min, "inv_min").data_ptr(),
                                              _dev(inv_max, "inv_max").data_ptr(), b, h, w, depth.data_ptr(),
                                              _ptr(norm), _stream()), "itermvs_convex_upsample")
    return (depth, norm) if want_norm else depth


def final_upsample(logits: Tensor, nd: Tensor, inv_min: Tensor, inv_max: Tensor, conf: Tensor, nd_channel: int = 0):
    """convex_upsample (depth) and the x4 bilinear up-sampling of the confidence (itermvs.py:321-324) in ONE launch:
    logits [B,144,H,W], nd buffer [B,Ct,H,W], conf [B,1,H,W] -> (depth [B,1,4H,4W], confidence [B,1,4H,4W])."""
    _dev(logits, "logits"); _dev(nd, "nd")
    conf = _dev(conf, "conf").contiguous()
    b, k, h, w = logits.shape
    assert k == 144 and nd.is_contiguous() and tuple(conf.shape[-2:]) == (h, w)
    sb, sc, sy, sx = logits.stride()
    depth = torch.empty((b, 1, 4 * h, 4 * w), device=logits.device, dtype=torch.float32)
    m = conf.numel() // (h * w)
    conf_up = torch.empty(tuple(conf.shape[:-2]) + (4 * h, 4 * w), device=logits.device, dtype=torch.float32)
    check(_lib.load().itermvs_final_upsample(logits.data_ptr(), sb, sc, sy, sx, nd.data_ptr() + 4 * nd_channel * h * w,
                                             nd.shape[1] * h * w, _dev(inv_min, "inv_min").data_ptr(),
                                             _dev(inv_max, "inv_max").data_ptr(), b, h, w, depth.data_ptr(), conf.data_ptr(), m,
                                             conf_up.data_ptr(), _stream()), "itermvs_final_upsample")
    return depth, conf_up


def bilinear_up_into(x: Tensor, scale: int, out: Tensor, out2: Optional[Tensor] = None, act: str = "none") -> Tensor:
    """F.interpolate(x, scale_factor=scale, 'bilinear') (+tanh) written into ``out`` and ``out2`` -- [B,C,sH,sW] views with
    dense planes, e.g. channel slices of wider buffers (itermvs_bilinear_up2)."""
    x = _dev(x, "x").contiguous()
    b, c, h, w = x.shape
    for t in (out, out2):
        if t is not None and tuple(t.shape) != (b, c, h * scale, w * scale):
            raise RuntimeError(f"bilinear_up_into: destination has shape {tuple(t.shape)}")
    po, so = _planes(out, "out")
    p2, s2 = _planes(out2, "out2") if out2 is not None else (None, 0)
    check(_lib.load().itermvs_bilinear_up2(x.data_ptr(), b, c, h, w, scale, 1 if act == "tanh" else 0, po, so, p2, s2, _stream()),
          "itermvs_bilinear_up2")
    return out


def bilinear_up(x: Tensor, scale: int, act: str = "none") -> Tensor:
    """F.interpolate(x, scale_factor=scale, mode='bilinear') (+ tanh): x [B,C,H,W] -> [B,C,sH,sW]."""
    x = _dev(x, "x").contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, c, scale * h, scale * w), device=x.device, dtype=torch.float32)
    check(_lib.load().itermvs_bilinear_up(x.data_ptr(), b * c, h, w, scale, {"none": 0, "tanh": 1}[act], out.data_ptr(),
                                          _stream()), "itermvs_bilinear_up")
    return out


# ------------------------------------------------------------------------------------------
ACT = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3, "gru_rh": 4, "gru_out": 5, "relu_dot": 6, "relu_dot_sigmoid": 7}


def pack_conv_weight(w: Tensor, transposed: bool = False) -> Tensor:
    """VALU-kernel format: [Cout,Cin,k,k] (Conv2d) or [Cin,Cout,k,k] (ConvTranspose2d) -> [Cin,k,k,Cout]."""
    return (w.permute(0, 2, 3, 1) if transposed else w.permute(1, 2, 3, 0)).contiguous()


def tile_k_split(cin: int) -> int:
    """S of the LDS-tiled kernel (conv_tile.hip): consecutive channels held by one k-slot of a chunk."""
    return 1 if cin <= 4 else 2 if cin <= 8 else 4


def split_bf16x3(t: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """fp32 tensor -> (h, m, l) bfloat16 tensors with h + m + l == t EXACTLY (finite t): h = t truncated to bf16's 8
    significant bits, m = (t - h) truncated, l = t - h - m (at most 8 bits left).  The split conv_tile3.hip applies to the
    activations when it stages them."""
    t = t.float().contiguous()
    mask = -65536
    h = (t.view(torch.int32) & mask).view(torch.float32)
    r = t - h
    m = (r.view(torch.int32) & mask).view(torch.float32)
    l = r - m
    return h.to(torch.bfloat16), m.to(torch.bfloat16), l.to(torch.bfloat16)


# Default arithmetic of the 3x3 convolutions with more than 8 input channels (MfmaWeight(split3=None)):
#   True  -> bf16x3 split on v_mfma_f32_16x16x32_bf16 (conv_tile3.hip, weight_format 3): fp32-comparable error, 2.7x less matrix time
#   False -> exact fp32 MFMA (conv_tile.hip, weight_format 2): bit-for-bit an fmaf chain
MFMA_SPLIT3_DEFAULT = True


class MfmaWeight:
    """Matrix-core formats of a Conv2d weight [Cout,Cin,k,k], zero padded:
    ``data`` (weight_format 1, conv_mfma.hip): [k*k, Cin_pad4, Cout_pad16];
    ``tile`` (weight_format 2, conv_tile.hip, 3x3 only): [9, chunks, 4, Cout_pad16, S] whose element
    (tap, ch, q, co, s) is the weight of input channel ch*4*S + q*S + s;
    ``tile3`` (weight_format 3, conv_tile3.hip, 3x3 with Cin > 8, ``split3``): bfloat16 [9, chunks, 3, Cout_pad16, 16] whose
    element (tap, ch, p, co, c) is term p (h, m, l of ``split_bf16x3``) of the weight of input channel ch*16 + c."""

    def __init__(self, w: Tensor, transposed: bool = False, split3: Optional[bool] = None):
        """``transposed``: ``w`` is a ConvTranspose2d weight [Cin,Cout,k,k] (only the tile format is built).
        ``split3``: build (and let conv2d use) the bf16x3 form; None = ``MFMA_SPLIT3_DEFAULT``."""
        self.transposed = transposed
        if transposed:
            w = w.permute(1, 0, 2, 3)
        cout, cin, k, _ = w.shape
        cin_p, cout_p = (cin + 3) // 4 * 4, (cout + 15) // 16 * 16
        packed = torch.zeros((k * k, cin_p, cout_p), device=w.device, dtype=torch.float32)
        packed[:, :cin, :cout] = w.permute(2, 3, 1, 0).reshape(k * k, cin, cout)
        self.data, self.cin, self.cout, self.ksize = packed.contiguous(), cin, cout, k
        self.tile = None
        if k == 3:
            s = tile_k_split(cin)
            nch = (cin + 4 * s - 1) // (4 * s)
            t = torch.zeros((9, nch * 4 * s, cout_p), device=w.device, dtype=torch.float32)
            t[:, :cin, :cout] = w.permute(2, 3, 1, 0).reshape(9, cin, cout)
            self.tile = t.reshape(9, nch, 4, s, cout_p).permute(0, 1, 2, 4, 3).contiguous()
        self.tile3 = None
        # (up to 64 input channels: the split weights of a 16-channel block -- 13.8 KB per input chunk -- share the LDS with the tile)
        if k == 3 and 8 < cin <= 64 and not transposed and (MFMA_SPLIT3_DEFAULT if split3 is None else split3):
            nch = (cin + 15) // 16
            t = torch.zeros((9, nch * 16, cout_p), device=w.device, dtype=torch.float32)
            t[:, :cin, :cout] = w.permute(2, 3, 1, 0).reshape(9, cin, cout)
            t = t.reshape(9, nch, 16, cout_p).permute(0, 1, 3, 2)                      # [9, chunks, Cout_pad, 16]
            self.tile3 = torch.stack(split_bf16x3(t), 2).contiguous()                  # [9, chunks, 3, Cout_pad, 16] bf16
        # 5 .. 8 input channels: the TAP-PAIR form of conv_tile3.hip (stride 1, no dilation): K-step v = 0..4 carries the 8 channels
        # at tap 2v in slots 0..7 and at tap 2v + 1 in slots 8..15 (the tenth tap: zeros) -> [5, 1, 3, Cout_pad, 16] bf16
        elif k == 3 and 4 < cin <= 8 and not transposed and (MFMA_SPLIT3_DEFAULT if split3 is None else split3):
            t = torch.zeros((10, 8, cout_p), device=w.device, dtype=torch.float32)
            t[:9, :cin, :cout] = w.permute(2, 3, 1, 0).reshape(9, cin, cout)
            t = t.reshape(5, 2, 8, cout_p).permute(0, 3, 1, 2).reshape(5, 1, cout_p, 16)      # [pair, chunk, Cout_pad, (tap in pair, ch)]
            self.tile3 = torch.stack(split_bf16x3(t), 2).contiguous()                  # [5, 1, 3, Cout_pad, 16] bf16


_TILE_SHAPES = {(1, 1), (2, 1), (1, 2)}   # (stride, dilation) instantiated in conv_tile.hip


def _use_tile(wt: "MfmaWeight", stride: int, dilation: int) -> bool:
    if wt.tile is None:
        return False
    return (stride, dilation) in _TILE_SHAPES and (wt.cin > 4 or (stride, dilation) == (1, 1))


def _planes(t: Tensor, name: str):
    """[N,C,H,W] view whose channel planes are dense (a channel slice of a contiguous buffer is fine)."""
    _dev(t, name)
    n, c, h, w = t.shape
    if t.stride(3) != 1 or t.stride(2) != w or (c > 1 and t.stride(1) != h * w):
        raise RuntimeError(f"{name}: needs dense [C,H,W] planes (NCHW); got strides {t.stride()}")
    return t.data_ptr(), (t.stride(0) if n > 1 else c * h * w)


def conv2d(x: Tensor, weight, bias=None, *, ksize: int = 3, stride: int = 1, pad: int = 1, dilation: int = 1,
           act: str = "none", add: Optional[Tensor] = None, aux1: Optional[Tensor] = None,
           aux2: Optional[Tensor] = None, out: Optional[Tensor] = None, out2: Optional[Tensor] = None,
           transposed: bool = False, seg_end: Sequence[int] = (), add_up2: bool = False,
           channels_last_out: bool = False, split=None, plan=None) -> Tensor:
    """itermvs_conv2d.  ``weight`` / ``bias``: packed tensor(s) (see pack_conv_weight); pass lists of up to
    three for per-segment weight sets with ``seg_end`` = batch boundaries.  ``add_up2``: ``add`` is the
    half-resolution tensor whose x2 bilinear up-sampling is added (fused F.interpolate).
    ``channels_last_out``: ``out`` is written in channels-last memory format ([N,H,W,C] dense, what the
    correlation kernels read); ``out2`` can still take the planar copy.
    ``split`` = (channel, act_b, out_b): output channels from ``channel`` on are a second result with its own
    activation and destination (two convolutions of one input in one launch).  ``plan`` (a ``_lib.ConvPlan``) receives
    itermvs_conv2d_plan's answer for this call: which kernel runs it.  Returns ``out``."""
    weights = list(weight) if isinstance(weight, (list, tuple)) else [weight]
    biases = list(bias) if isinstance(bias, (list, tuple)) else [bias] * len(weights)
    n, cin, hin, win = x.shape
    mfma, tiled, split3 = isinstance(weights[0], MfmaWeight), False, False
    if mfma:
        if transposed != weights[0].transposed:
            raise RuntimeError("conv2d: weight was packed for the other direction (MfmaWeight(transposed=...))")
        if any(wt.cin != cin or wt.ksize != ksize for wt in weights):
            raise RuntimeError("conv2d: MfmaWeight does not match the input channels / kernel size")
        cout = weights[0].cout
        tiled = transposed or all(_use_tile(wt, stride, dilation) for wt in weights)
        # (stride-2 layers keep the fp32 form here: through this kernel every channel block re-stages and re-splits the halo tile, and
        #  the split form measured 30.2 us per launch against 28.0, profiles/r06/r06l_*; FeatureNet's two stride-2 pairs run in bf16x3
        #  through down_conv, which stages each tile once for all output channels)
        split3 = (tiled and not transposed and stride == 1
                  and all(wt.tile3 is not None for wt in weights)
                  and (cin > 8 or dilation == 1))                    # (the tap-pair form of 5..8 channels: no dilation)
        weights = [(wt.tile3 if split3 else wt.tile) if tiled else wt.data for wt in weights]
    else:
        cout = weights[0].shape[3]
    if transposed:
        hout, wout = 2 * hin, 2 * win
    else:
        span = (ksize - 1) * dilation + 1
        hout, wout = (hin + 2 * pad - span) // stride + 1, (win + 2 * pad - span) // stride + 1
    cout_total = cout
    dot = None
    if act in ("relu_dot", "relu_dot_sigmoid"):
        # ReLU + a 1x1 convolution to ONE channel (+ sigmoid) in the epilogue: aux1 = Cout + 1 floats {w[Cout], bias}
        if not (mfma and tiled and cout in (16, 32) and aux1 is not None and aux1.numel() == cout + 1 and add is None and out2 is None
                and split is None):
            raise RuntimeError("conv2d: act='relu_dot' needs a 16- or 32-channel 3x3 matrix-core layer and aux1 = Cout + 1 floats")
        dot, aux1, cout = _dev(aux1, "aux1").contiguous(), None, 1
    if split is not None:
        if not (mfma and ksize == 3 and not transposed):
            raise RuntimeError("conv2d: split results need the tiled matrix-core kernel (3x3 MfmaWeight)")
        cout = int(split[0])
    if out is None:
        out = torch.empty((n, cout, hout, wout), device=x.device, dtype=torch.float32,
                          memory_format=torch.channels_last if channels_last_out else torch.contiguous_format)
    if not channels_last_out and out.dtype != torch.float32:
        raise RuntimeError("conv2d: 16-bit storage exists for channels-last outputs only")
    p = ConvParams()
    if (cin == 8 and split3 and not transposed and x.dim() == 4 and not x.is_contiguous()
            and x.is_contiguous(memory_format=torch.channels_last)):
        # channels-last input [N,H,W,8] (corr_init's groups-last volume): two 16-byte loads per pixel in the tap-pair kernel
        _dev(x, "conv input")
        p.inp, p.in_sn, p.in_layout = x.data_ptr(), 8 * hin * win, 1
    else:
        p.inp, p.in_sn = _planes(x, "conv input")
    if channels_last_out:
        if not out.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("conv2d: channels_last_out needs a dense channels-last `out`")
        # out_layout 1 / 2 / 3 = fp32 / fp16 / bf16 storage of the feature map (rounded to nearest even from fp32)
        p.out, p.out_sn, p.out_layout = out.data_ptr(), cout * hout * wout, 1 + _feat(out, "conv output")
    else:
        p.out, p.out_sn = _planes(out, "conv output")
    if out.shape != (n, cout, hout, wout):
        raise RuntimeError(f"conv2d: out has shape {tuple(out.shape)}, expected {(n, cout, hout, wout)}")
    if out2 is not None:
        assert out2.is_contiguous() and out2.shape == out.shape
        p.out2 = out2.data_ptr()
    for name, t in (("add", add), ("aux1", aux1), ("aux2", aux2)):
        if t is not None:
            ptr, sn = _planes(t, name)
            want = (n, cout, hout // 2, wout // 2) if (name == "add" and add_up2) else tuple(out.shape)
            if tuple(t.shape) != want:
                raise RuntimeError(f"conv2d: {name} has shape {tuple(t.shape)}, expected {want}")
            setattr(p, name, ptr)
            setattr(p, name + "_sn", sn)
    p.n_seg = len(weights)
    for i, (wt, bs) in enumerate(zip(weights, biases)):
        if not (mfma and split3):
            _dev(wt, "weight")
        elif not wt.is_cuda:
            raise RuntimeError("weight: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
        if not mfma and (not wt.is_contiguous() or wt.shape != (cin, ksize, ksize, cout)):
            raise RuntimeError(f"conv2d: packed weight must be contiguous [{cin},{ksize},{ksize},{cout}], got {tuple(wt.shape)}")
        p.weight[i] = wt.data_ptr()
        p.bias[i] = None if bs is None else _dev(bs, "bias").data_ptr()
    for i, e in enumerate(seg_end):
        p.seg_end[i] = e
    p.N, p.Cin, p.Hin, p.Win, p.Cout = n, cin, hin, win, cout_total
    if dot is not None:
        p.aux1, p.aux1_sn = dot.data_ptr(), 0
    if split is not None:
        ob = split[2]
        if tuple(ob.shape) != (n, cout_total - cout, hout, wout):
            raise RuntimeError(f"conv2d: split output has shape {tuple(ob.shape)}, expected {(n, cout_total - cout, hout, wout)}")
        p.split_cout, p.act_b = cout, ACT[split[1]]
        p.out_b, p.out_b_sn = _planes(ob, "split output")
    p.ksize, p.stride, p.pad, p.dilation = ksize, stride, pad, dilation
    p.transposed, p.act = int(transposed), ACT[act]
    p.weight_format = ((3 if split3 else 2) if tiled else 1) if mfma else 0
    p.add_mode = int(add_up2)
    if CONV_FLOP_COUNTER["enabled"]:
        CONV_FLOP_COUNTER["flops"] += 2.0 * n * hout * wout * cout_total * cin * ksize * ksize / (4.0 if transposed else 1.0)
        CONV_FLOP_COUNTER["launches"] += 1
    if plan is not None:
        check(_lib.load().itermvs_conv2d_plan(C.byref(p), C.byref(plan)), "itermvs_conv2d_plan")
    check(_lib.load().itermvs_conv2d(C.byref(p), _stream()), "itermvs_conv2d")
    return out


# ------------------------------------------------------------------------------------------
CONV_FLOP_COUNTER = {"enabled": False, "flops": 0.0, "launches": 0}


def _fuse_depth(what: str, depth_ref: Tensor, conf_ref: Tensor, depth_src: Sequence[Tensor], mats: Tensor, geo_pixel_thres: float,
                geo_depth_thres: float, photo_thres: float, geo_mask_thres: Optional[int], claim: Optional[tuple] = None,
                dynamic: Optional[tuple] = None):
    """the inputs, outputs and call that itermvs_fuse_depth, itermvs_fuse_depth_claim and itermvs_fuse_depth_dynamic share;
    ``claim``: the two extra pointer arguments of the latter two; ``dynamic``: (pixel step, depth step, n_min, n_max) of the last,
    which takes no ``geo_mask_thres`` and also returns the level map"""
    h, w = depth_ref.shape
    s = len(depth_src)
    depth_ref, conf_ref = _dev(depth_ref, "depth_ref").contiguous(), _dev(conf_ref, "conf_ref").contiguous()
    srcs = [_dev(t, "depth_src").contiguous() for t in depth_src]
    if any(tuple(t.shape) != (h, w) for t in srcs + [conf_ref]) or tuple(mats.shape) != (s, 60):
        raise RuntimeError(f"{what}: all maps must be [H,W] and mats [S,60]")
    mats = _dev(mats, "mats").float().contiguous()
    ptrs = (C.c_void_p * s)(*[t.data_ptr() for t in srcs])
    dev = depth_ref.device
    avg = torch.empty((h, w), device=dev, dtype=torch.float64)
    photo, geo, final = (torch.empty((h, w), device=dev, dtype=torch.uint8) for _ in range(3))
    cnt = torch.empty((h, w), device=dev, dtype=torch.int32)
    count_thres = () if dynamic is not None else (int(geo_mask_thres),)
    level = torch.empty((h, w), device=dev, dtype=torch.uint8) if dynamic is not None else None
    rule = () if dynamic is None else (float(dynamic[0]), float(dynamic[1]), int(dynamic[2]), int(dynamic[3]), level.data_ptr())
    check(getattr(_lib.load(), "itermvs_" + what)(depth_ref.data_ptr(), conf_ref.data_ptr(), ptrs, mats.data_ptr(), s, h, w,
                                                  float(geo_pixel_thres), float(geo_depth_thres), float(photo_thres),
                                                  *count_thres, avg.data_ptr(), photo.data_ptr(), geo.data_ptr(),
                                                  final.data_ptr(), cnt.data_ptr(), *(claim or ()), *rule, _stream()), "itermvs_" + what)
    return (avg, photo, geo, final, cnt) if dynamic is None else (avg, photo, geo, final, cnt, level)


def fuse_depth(depth_ref: Tensor, conf_ref: Tensor, depth_src: Sequence[Tensor], mats: Tensor, geo_pixel_thres: float = 1.0,
               geo_depth_thres: float = 0.01, photo_thres: float = 0.3, geo_mask_thres: int = 3):
    """itermvs_fuse_depth (eval.py:154-269 for one reference view).  depth_ref / conf_ref [H,W], depth_src: S maps [H,W],
    mats [S,60] (itermvs_amd.fusion.pair_matrices).  -> (depth_avg float64 [H,W], photo, geo, final uint8, count int32)."""
    return _fuse_depth("fuse_depth", depth_ref, conf_ref, depth_src, mats, geo_pixel_thres, geo_depth_thres, photo_thres,
                       geo_mask_thres)


def _claim_pointers(what: str, depth_ref: Tensor, depth_src: Sequence[Tensor], claimed_ref: Optional[Tensor],
                    claimed_src: Optional[Sequence[Tensor]]) -> tuple:
    """the checked claim maps of ``fuse_depth_claim`` / ``fuse_depth_dynamic`` -> the two pointer arguments of their entry points"""
    h, w = depth_ref.shape
    maps = ([] if claimed_ref is None else [claimed_ref]) + list(claimed_src or [])
    for t in maps:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: expected CUDA/ROCm tensors - the IterMVS HIP engine has no CPU path")
        if t.dtype != torch.uint8 or tuple(t.shape) != (h, w) or not t.is_contiguous() or t.device != depth_ref.device:
            raise RuntimeError(f"{what}: a claim map must be a contiguous torch.uint8 tensor of shape {(h, w)} on "
                               f"{depth_ref.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if claimed_src is not None and len(claimed_src) != len(depth_src):
        raise RuntimeError(f"{what}: {len(claimed_src)} claim maps for {len(depth_src)} source views")
    ptrs = None if claimed_src is None else (C.c_void_p * len(claimed_src))(*[t.data_ptr() for t in claimed_src])
    return (None if claimed_ref is None else claimed_ref.data_ptr(), ptrs)


def fuse_depth_claim(depth_ref: Tensor, conf_ref: Tensor, depth_src: Sequence[Tensor], mats: Tensor,
                     claimed_ref: Optional[Tensor], claimed_src: Optional[Sequence[Tensor]], geo_pixel_thres: float = 1.0,
                     geo_depth_thres: float = 0.01, photo_thres: float = 0.3, geo_mask_thres: int = 3):
    """itermvs_fuse_depth_claim: ``fuse_depth`` whose ``final`` leaves out the pixels marked in ``claimed_ref`` (uint8 [H,W];
    None: nothing is marked), and whose emitting pixels mark, IN PLACE, the pixel they were verified against in each consistent
    source view's map of ``claimed_src`` (S uint8 [H,W] maps, none of them ``claimed_ref``; None: nothing is marked).  The
    contract is in include/itermvs_hip.h.  -> the tuple of ``fuse_depth``."""
    return _fuse_depth("fuse_depth_claim", depth_ref, conf_ref, depth_src, mats, geo_pixel_thres, geo_depth_thres, photo_thres,
                       geo_mask_thres, claim=_claim_pointers("fuse_depth_claim", depth_ref, depth_src, claimed_ref, claimed_src))


DYN_PIXEL_STEP, DYN_DEPTH_STEP, DYN_N_MIN, DYN_N_MAX = 0.25, 1.0 / 1300.0, 2, 10     # unverified defaults, DESIGN.md section 4c


def fuse_depth_dynamic(depth_ref: Tensor, conf_ref: Tensor, depth_src: Sequence[Tensor], mats: Tensor,
                       claimed_ref: Optional[Tensor] = None, claimed_src: Optional[Sequence[Tensor]] = None,
                       geo_pixel_thres: float = 1.0, geo_depth_thres: float = 0.01, photo_thres: float = 0.3,
                       dyn_pixel_step: float = DYN_PIXEL_STEP, dyn_depth_step: float = DYN_DEPTH_STEP,
                       dyn_n_min: int = DYN_N_MIN, dyn_n_max: int = DYN_N_MAX):
    """itermvs_fuse_depth_dynamic: ``fuse_depth_claim`` (claim maps optional) whose ``geo`` is the level rule of
    include/itermvs_hip.h instead of a count against ``geo_mask_thres``: a source passes level n when its reprojection lies within
    n * dyn_pixel_step pixels and n * dyn_depth_step (rounded to float32) of relative depth, and the pixel is accepted at the
    smallest level n of dyn_n_min..dyn_n_max that at least n sources pass.  The average, the count and the claims stay
    those of the base thresholds.  -> (depth_avg, photo, geo, final, count, level uint8 [H,W]: the accepting level, 0 = none)."""
    return _fuse_depth("fuse_depth_dynamic", depth_ref, conf_ref, depth_src, mats, geo_pixel_thres, geo_depth_thres, photo_thres,
                       None, claim=_claim_pointers("fuse_depth_dynamic", depth_ref, depth_src, claimed_ref, claimed_src),
                       dynamic=(dyn_pixel_step, dyn_depth_step, dyn_n_min, dyn_n_max))


POINT_RECORD_BYTES = 15      # PLY vertex of eval.py:298-308: x, y, z float32, red, green, blue uint8


def fuse_points_workspace_bytes(h: int, w: int) -> int:
    n = _lib.load().itermvs_fuse_points_workspace_bytes(int(h), int(w))
    check(min(n, 0), "itermvs_fuse_points_workspace_bytes")
    return n


def _fuse_points(what: str, record_bytes: int, depth_avg: Tensor, final_mask: Tensor, cam: Tensor, rgb: Tensor, records: Tensor,
                 cursor: Tensor, view_counts: Tensor, view: int, photo_mask: Optional[Tensor], geo_mask: Optional[Tensor],
                 capacity: Optional[int], workspace: Optional[Tensor], extra: tuple = ()) -> None:
    """the checks and the call of fuse_points / fuse_points_normals; ``extra``: the entry point's arguments between W and records"""
    h, w = depth_avg.shape
    want = ((depth_avg, torch.float64, (h, w)), (final_mask, torch.uint8, (h, w)), (cam, torch.float32, (21,)),
            (rgb, torch.uint8, (h, w, 3)), (cursor, torch.int64, (1,)))
    masks = [m for m in (photo_mask, geo_mask) if m is not None]
    for t, dt, shp in want + tuple((m, torch.uint8, (h, w)) for m in masks):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: expected CUDA/ROCm tensors - the IterMVS HIP engine has no CPU path")
        if t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous():
            raise RuntimeError(f"{what}: expected a contiguous {dt} tensor of shape {shp}, got {t.dtype} {tuple(t.shape)}")
    for t, dt, name in ((records, torch.uint8, "records"), (view_counts, torch.int64, "view_counts")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous {dt} CUDA/ROCm tensor")
    if view_counts.dim() != 2 or view_counts.shape[1] != 4 or not 0 <= view < view_counts.shape[0]:
        raise RuntimeError(f"{what}: view_counts must be [n_views,4] with view {view} inside it")
    cap = records.numel() // record_bytes if capacity is None else int(capacity)
    if cap < 0 or cap * record_bytes > records.numel():
        raise RuntimeError(f"{what}: capacity {cap} vertices does not fit records ({records.numel()} bytes)")
    need = fuse_points_workspace_bytes(h, w)
    if workspace is None:
        workspace = torch.empty(need, device=depth_avg.device, dtype=torch.uint8)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: workspace must be a contiguous uint8 CUDA/ROCm tensor of >= {need} bytes")
    ptr = lambda m: None if m is None else m.data_ptr()    # noqa: E731
    check(getattr(_lib.load(), "itermvs_" + what)(depth_avg.data_ptr(), final_mask.data_ptr(), ptr(photo_mask), ptr(geo_mask),
                                                  cam.data_ptr(), rgb.data_ptr(), h, w, *extra, records.data_ptr() if cap else None,
                                                  cap, cursor.data_ptr(), view_counts.data_ptr(), int(view), workspace.data_ptr(),
                                                  _stream()),
          "itermvs_" + what)


def fuse_points(depth_avg: Tensor, final_mask: Tensor, cam: Tensor, rgb: Tensor, records: Tensor, cursor: Tensor,
                view_counts: Tensor, view: int, photo_mask: Optional[Tensor] = None, geo_mask: Optional[Tensor] = None,
                capacity: Optional[int] = None, workspace: Optional[Tensor] = None) -> None:
    """itermvs_fuse_points (eval.py:287-308 for one reference view): appends the vertices of ``final_mask`` to ``records``
    (uint8, 15 bytes per vertex) behind the ``cursor`` (uint64 [1], kept as int64) and fills ``view_counts[view]`` (int64
    [n,4]: photo, geo, final pixels, first vertex); nothing is read back and nothing synchronises.  depth_avg float64 [H,W],
    masks uint8 [H,W], cam float32 [21] = inv(K) | inv(E)[:3], rgb uint8 [H,W,3].  ``capacity`` (vertices) defaults to all of
    ``records``; ``workspace``: uint8 scratch of fuse_points_workspace_bytes(H, W), allocated here when not given."""
    _fuse_points("fuse_points", POINT_RECORD_BYTES, depth_avg, final_mask, cam, rgb, records, cursor, view_counts, view,
                 photo_mask, geo_mask, capacity, workspace)


POINT_NORMAL_RECORD_BYTES = 27      # x, y, z, nx, ny, nz float32, red, green, blue uint8 (the vertex of COLMAP's fused.ply)


def fuse_points_normals(depth_avg: Tensor, final_mask: Tensor, cam: Tensor, rgb: Tensor, records: Tensor, cursor: Tensor,
                        view_counts: Tensor, view: int, photo_mask: Optional[Tensor] = None, geo_mask: Optional[Tensor] = None,
                        capacity: Optional[int] = None, workspace: Optional[Tensor] = None, edge_thres: float = 0.01) -> None:
    """itermvs_fuse_points_normals: ``fuse_points`` with 27-byte records that carry, between the coordinates and the colour, the
    unit normal of the surface at the pixel in world space, facing the reference camera: the cross product of ``depth_avg``'s
    camera-space differences along the row and the column, where a neighbour whose depth differs by ``edge_thres * depth`` or
    more is left out (include/itermvs_hip.h has every step); (0, 0, 0) where it is not defined.  Everything else as there."""
    _fuse_points("fuse_points_normals", POINT_NORMAL_RECORD_BYTES, depth_avg, final_mask, cam, rgb, records, cursor, view_counts,
                 view, photo_mask, geo_mask, capacity, workspace, extra=(float(edge_thres),))


TSDF_VOXEL_BYTES = 12        # sum_t float32 | count uint16 | red, green, blue sums uint16 (include/itermvs_hip.h)
MESH_VERTEX_BYTES = 15       # x, y, z float32, red, green, blue uint8
MESH_FACE_BYTES = 12         # three int32 vertex indices


def _tsdf_tensor(what: str, name: str, t, dtype, shape=None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name}: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} tensor" + (f" of shape {tuple(shape)}" if shape else "") +
                           f", got {t.dtype} {tuple(t.shape)}")


def tsdf_tet_tables() -> Tuple[List[List[int]], List[List[List[Tuple[int, int]]]]]:
    """the two tables of csrc/tsdf_tets.hpp through the library's host functions (no GPU): (corners [6][4] as cube corners,
    cases [16] = list of triangles, each three edges (lower, upper local corner))"""
    lib = _lib.load()
    buf4, buf12 = (C.c_int32 * 4)(), (C.c_int32 * 12)()
    corners, cases = [], []
    for t in range(6):
        check(lib.itermvs_tsdf_tet_corners(t, buf4), "itermvs_tsdf_tet_corners")
        corners.append(list(buf4))
    for m in range(16):
        n = lib.itermvs_tsdf_tet_case(m, buf12)
        check(min(n, 0), "itermvs_tsdf_tet_case")
        cases.append([[(buf12[6 * t + 2 * v], buf12[6 * t + 2 * v + 1]) for v in range(3)] for t in range(n)])
    return corners, cases


def tsdf_volume(dims: Sequence[int], device) -> Tensor:
    """an empty volume state for ``tsdf_integrate``: int32 [nx*ny*nz, 3], all zero"""
    nx, ny, nz = (int(d) for d in dims)
    return torch.zeros((nx * ny * nz, 3), device=device, dtype=torch.int32)


def tsdf_integrate(state: Tensor, dims: Sequence[int], origin: Sequence[float], voxel: float, trunc: float, depth: Tensor,
                   mask: Tensor, cams: Tensor, rgb: Tensor) -> None:
    """itermvs_tsdf_integrate: folds the V views depth float64 [V,H,W] (``depth_avg``), mask uint8 [V,H,W] (photo & geo), cams
    float32 [V,21] = K | E[:3] (world -> camera), rgb uint8 [V,H,W,3] into ``state`` (int32 [nx*ny*nz,3], ``tsdf_volume``) IN PLACE,
    in the given order, one launch; nothing is read back.  The contract is in include/itermvs_hip.h."""
    nx, ny, nz = (int(d) for d in dims)
    what = "tsdf_integrate"
    _tsdf_tensor(what, "depth", depth, torch.float64)
    if depth.dim() != 3:
        raise RuntimeError(f"{what}: depth must be [V,H,W], got {tuple(depth.shape)}")
    v, h, w = depth.shape
    _tsdf_tensor(what, "state", state, torch.int32, (nx * ny * nz, 3))
    _tsdf_tensor(what, "mask", mask, torch.uint8, (v, h, w))
    _tsdf_tensor(what, "cams", cams, torch.float32, (v, 21))
    _tsdf_tensor(what, "rgb", rgb, torch.uint8, (v, h, w, 3))
    check(_lib.load().itermvs_tsdf_integrate(state.data_ptr(), nx, ny, nz, *(float(o) for o in origin), float(voxel), float(trunc),
                                             depth.data_ptr(), mask.data_ptr(), cams.data_ptr(), rgb.data_ptr(), v, h, w, _stream()),
          "itermvs_tsdf_integrate")


def tsdf_mesh_workspace_bytes(dims: Sequence[int]) -> int:
    n = C.c_int64(0)
    check(_lib.load().itermvs_tsdf_mesh_workspace_bytes(*(int(d) for d in dims), C.byref(n)), "itermvs_tsdf_mesh_workspace_bytes")
    return int(n.value)


def tsdf_mesh(state: Tensor, dims: Sequence[int], origin: Sequence[float], voxel: float, min_count: int, vertices: Tensor,
              faces: Tensor, totals: Tensor, workspace: Optional[Tensor] = None, vertex_capacity: Optional[int] = None,
              face_capacity: Optional[int] = None) -> None:
    """itermvs_tsdf_mesh: marching tetrahedra over ``state`` -> ``vertices`` (uint8, 15 bytes each), ``faces`` (int32 [F,3] or flat)
    and ``totals`` (int64 [2]: vertices, triangles that exist, whatever the capacities); nothing is read back.  The capacities
    default to all of the two buffers; ``workspace``: uint8 scratch of tsdf_mesh_workspace_bytes(dims), allocated here when not given."""
    nx, ny, nz = (int(d) for d in dims)
    what = "tsdf_mesh"
    _tsdf_tensor(what, "state", state, torch.int32, (nx * ny * nz, 3))
    _tsdf_tensor(what, "vertices", vertices, torch.uint8)
    _tsdf_tensor(what, "faces", faces, torch.int32)
    _tsdf_tensor(what, "totals", totals, torch.int64, (2,))
    vcap = vertices.numel() // MESH_VERTEX_BYTES if vertex_capacity is None else int(vertex_capacity)
    fcap = faces.numel() // 3 if face_capacity is None else int(face_capacity)
    if vcap < 0 or vcap * MESH_VERTEX_BYTES > vertices.numel() or fcap < 0 or fcap * 3 > faces.numel():
        raise RuntimeError(f"{what}: capacities {vcap} vertices, {fcap} triangles do not fit the buffers "
                           f"({vertices.numel()} bytes, {faces.numel()} indices)")
    need = tsdf_mesh_workspace_bytes(dims)
    if workspace is None:
        workspace = torch.empty(need, device=state.device, dtype=torch.uint8)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: workspace must be a contiguous uint8 CUDA/ROCm tensor of >= {need} bytes")
    check(_lib.load().itermvs_tsdf_mesh(state.data_ptr(), nx, ny, nz, *(float(o) for o in origin), float(voxel), int(min_count),
                                        vertices.data_ptr() if vcap else None, vcap, faces.data_ptr() if fcap else None, fcap,
                                        totals.data_ptr(), workspace.data_ptr(), _stream()),
          "itermvs_tsdf_mesh")


def mesh_components(faces: Tensor, n_vertices: int) -> Tuple[Tensor, Tensor, Tensor]:
    """itermvs_mesh_components: ``faces`` int32 [NF,3] (or flat [NF*3]) of a mesh of ``n_vertices`` vertices -> (label int32 [NV] =
    the smallest vertex index of each vertex's component, face_count int32 [NV] = the valid faces of a component at its label,
    totals int64 [3] = components with a face, largest face_count, valid faces), all on the GPU; nothing is read back."""
    what = "mesh_components"
    _tsdf_tensor(what, "faces", faces, torch.int32)
    nv = int(n_vertices)
    if faces.numel() % 3 or nv < 0:
        raise RuntimeError(f"{what}: faces must hold index triples and n_vertices be >= 0, got {faces.numel()} indices, {nv} vertices")
    nf = faces.numel() // 3
    store = torch.empty((2, max(nv, 1)), device=faces.device, dtype=torch.int32)       # an empty tensor has no address, and the
    label, face_count = store[0, :nv], store[1, :nv]                                   # entry point refuses NULL whatever NV is
    totals = torch.empty(3, device=faces.device, dtype=torch.int64)
    check(_lib.load().itermvs_mesh_components(faces.data_ptr() if nf else None, nf, nv, store[0].data_ptr(), store[1].data_ptr(),
                                              totals.data_ptr(), _stream()), "itermvs_mesh_components")
    return label, face_count, totals


def mesh_keep_workspace_bytes(n_vertices: int, n_faces: int) -> int:
    n = C.c_int64(0)
    check(_lib.load().itermvs_mesh_keep_workspace_bytes(int(n_vertices), int(n_faces), C.byref(n)), "itermvs_mesh_keep_workspace_bytes")
    return int(n.value)


def mesh_keep(vertices: Tensor, record_bytes: int, faces: Tensor, label: Tensor, face_count: Tensor, min_faces: int,
              out_vertices: Tensor, out_faces: Tensor, totals: Tensor, workspace: Optional[Tensor] = None,
              vertex_capacity: Optional[int] = None, face_capacity: Optional[int] = None) -> None:
    """itermvs_mesh_keep: the vertices (uint8, ``record_bytes`` each) and faces (int32 triples) of the components with at least
    ``min_faces`` valid faces -> ``out_vertices``, ``out_faces`` (in their order, faces renumbered) and ``totals`` (int64 [2]: kept
    vertices, kept faces, whatever the capacities); nothing is read back.  ``label``, ``face_count``: ``mesh_components`` of the same
    faces.  The capacities default to all of the two buffers; ``workspace``: uint8 scratch of mesh_keep_workspace_bytes, allocated
    here when not given."""
    what = "mesh_keep"
    rec = int(record_bytes)
    for name, t, dtype in (("vertices", vertices, torch.uint8), ("faces", faces, torch.int32), ("label", label, torch.int32),
                           ("face_count", face_count, torch.int32), ("out_vertices", out_vertices, torch.uint8),
                           ("out_faces", out_faces, torch.int32)):
        _tsdf_tensor(what, name, t, dtype)
    _tsdf_tensor(what, "totals", totals, torch.int64, (2,))
    if rec < 1 or vertices.numel() % rec or faces.numel() % 3:
        raise RuntimeError(f"{what}: {vertices.numel()} vertex bytes are no records of {rec} bytes, or {faces.numel()} indices no triples")
    nv, nf = vertices.numel() // rec, faces.numel() // 3
    if label.numel() != nv or face_count.numel() != nv:
        raise RuntimeError(f"{what}: label and face_count must have one entry per vertex ({nv}), got {label.numel()}, {face_count.numel()}")
    vcap = out_vertices.numel() // rec if vertex_capacity is None else int(vertex_capacity)
    fcap = out_faces.numel() // 3 if face_capacity is None else int(face_capacity)
    if vcap < 0 or vcap * rec > out_vertices.numel() or fcap < 0 or fcap * 3 > out_faces.numel():
        raise RuntimeError(f"{what}: capacities {vcap} vertices, {fcap} triangles do not fit the buffers "
                           f"({out_vertices.numel()} bytes, {out_faces.numel()} indices)")
    need = mesh_keep_workspace_bytes(nv, nf)
    if workspace is None:
        workspace = torch.empty(max(need, 8), device=faces.device, dtype=torch.uint8)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: workspace must be a contiguous uint8 CUDA/ROCm tensor of >= {need} bytes")
    if nv == 0:                                                    # empty tensors have no address: see mesh_components
        label = face_count = torch.empty(1, device=faces.device, dtype=torch.int32)
    check(_lib.load().itermvs_mesh_keep(vertices.data_ptr() if nv else None, nv, rec, faces.data_ptr() if nf else None, nf,
                                        label.data_ptr(), face_count.data_ptr(), int(min_faces),
                                        out_vertices.data_ptr() if vcap else None, vcap, out_faces.data_ptr() if fcap else None, fcap,
                                        totals.data_ptr(), workspace.data_ptr(), _stream()), "itermvs_mesh_keep")


MESH_SIMPLIFY_REG = 1e-3           # include/itermvs_hip.h: ITERMVS_MESH_SIMPLIFY_REG
MESH_SIMPLIFY_MAX_FACES = (2 ** 31 - 1) // 3


def _simplify_sizes(what: str, named: Sequence[tuple]) -> None:
    """the checks the three simplify wrappers share: every (name, tensor, dtype, elements or None) is a contiguous device tensor of
    that dtype and size"""
    for name, t, dtype, n in named:
        _tsdf_tensor(what, name, t, dtype)
        if n is not None and t.numel() != n:
            raise RuntimeError(f"{what}: {name} must have {n} elements, got {t.numel()}")


def mesh_simplify_corners(faces: Tensor, cluster: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """itermvs_mesh_simplify_corners: ``faces`` int32 [NF*3], ``cluster`` int32 [NV] (the cluster of every vertex, -1: not valid) ->
    (pair_cluster int32 [NF*3], key_hi int64 [NF], key_lo int32 [NF]); nothing is read back"""
    what = "mesh_simplify_corners"
    _simplify_sizes(what, (("faces", faces, torch.int32, None), ("cluster", cluster, torch.int32, None)))
    if faces.numel() % 3:
        raise RuntimeError(f"{what}: {faces.numel()} indices are no triples")
    nf, nv, dev = faces.numel() // 3, cluster.numel(), faces.device
    pair = torch.empty(3 * nf, device=dev, dtype=torch.int32)
    hi = torch.empty(nf, device=dev, dtype=torch.int64)
    lo = torch.empty(nf, device=dev, dtype=torch.int32)
    if nf:
        check(_lib.load().itermvs_mesh_simplify_corners(faces.data_ptr(), nf, nv, cluster.data_ptr() if nv else None, pair.data_ptr(),
                                                        hi.data_ptr(), lo.data_ptr(), _stream()), "itermvs_mesh_simplify_corners")
    return pair, hi, lo


def mesh_simplify_clusters(vertices: Tensor, record_bytes: int, faces: Tensor, keys_sorted: Tensor, perm: Tensor, cluster_sorted: Tensor,
                           pair_sorted: Tensor, pair_face: Tensor, grid: "CloudGrid", reps: Optional[Tensor] = None) -> Tensor:
    """itermvs_mesh_simplify_clusters: the representative record of every cluster -> ``reps`` uint8 [NV*record_bytes] (record c =
    cluster c; allocated here when not given).  The arrays are those of the header, sorted stably by the caller."""
    what = "mesh_simplify_clusters"
    rec = int(record_bytes)
    _simplify_sizes(what, (("vertices", vertices, torch.uint8, None), ("faces", faces, torch.int32, None)))
    if rec < 1 or vertices.numel() % rec or faces.numel() % 3:
        raise RuntimeError(f"{what}: {vertices.numel()} vertex bytes are no records of {rec} bytes, or {faces.numel()} indices no triples")
    nv, nf, dev = vertices.numel() // rec, faces.numel() // 3, vertices.device
    if reps is None:
        reps = torch.empty(nv * rec, device=dev, dtype=torch.uint8)
    _simplify_sizes(what, (("keys_sorted", keys_sorted, torch.int64, nv), ("perm", perm, torch.int64, nv),
                           ("cluster_sorted", cluster_sorted, torch.int32, nv), ("pair_sorted", pair_sorted, torch.int32, 3 * nf),
                           ("pair_face", pair_face, torch.int32, 3 * nf), ("reps", reps, torch.uint8, nv * rec)))
    at = lambda t, n: t.data_ptr() if n else None                  # noqa: E731  (an empty tensor has no address)
    check(_lib.load().itermvs_mesh_simplify_clusters(at(vertices, nv), nv, rec, at(faces, nf), nf, at(keys_sorted, nv), at(perm, nv),
                                                     at(cluster_sorted, nv), at(pair_sorted, nf), at(pair_face, nf), *grid.args(),
                                                     at(reps, nv), _stream()), "itermvs_mesh_simplify_clusters")
    return reps


def mesh_simplify_emit_workspace_bytes(n_vertices: int, n_faces: int) -> int:
    n = C.c_int64(0)
    check(_lib.load().itermvs_mesh_simplify_emit_workspace_bytes(int(n_vertices), int(n_faces), C.byref(n)),
          "itermvs_mesh_simplify_emit_workspace_bytes")
    return int(n.value)


def mesh_simplify_emit(reps: Tensor, record_bytes: int, faces: Tensor, cluster: Tensor, key_hi_sorted: Tensor, key_lo_sorted: Tensor,
                       order: Tensor, out_vertices: Tensor, out_faces: Tensor, totals: Tensor, workspace: Optional[Tensor] = None,
                       vertex_capacity: Optional[int] = None, face_capacity: Optional[int] = None) -> None:
    """itermvs_mesh_simplify_emit: the surviving faces (renumbered) and the representatives they reference -> ``out_vertices``,
    ``out_faces`` and ``totals`` (int64 [2]: vertices, faces, whatever the capacities); nothing is read back.  The capacities default
    to all of the two buffers; ``workspace``: uint8 scratch of mesh_simplify_emit_workspace_bytes, allocated here when not given."""
    what = "mesh_simplify_emit"
    rec = int(record_bytes)
    _simplify_sizes(what, (("reps", reps, torch.uint8, None), ("faces", faces, torch.int32, None),
                           ("out_vertices", out_vertices, torch.uint8, None), ("out_faces", out_faces, torch.int32, None),
                           ("totals", totals, torch.int64, 2)))
    if rec < 1 or reps.numel() % rec or faces.numel() % 3:
        raise RuntimeError(f"{what}: {reps.numel()} bytes are no records of {rec} bytes, or {faces.numel()} indices no triples")
    nv, nf = reps.numel() // rec, faces.numel() // 3
    _simplify_sizes(what, (("cluster", cluster, torch.int32, nv), ("key_hi_sorted", key_hi_sorted, torch.int64, nf),
                           ("key_lo_sorted", key_lo_sorted, torch.int32, nf), ("order", order, torch.int32, nf)))
    vcap = out_vertices.numel() // rec if vertex_capacity is None else int(vertex_capacity)
    fcap = out_faces.numel() // 3 if face_capacity is None else int(face_capacity)
    if vcap < 0 or vcap * rec > out_vertices.numel() or fcap < 0 or fcap * 3 > out_faces.numel():
        raise RuntimeError(f"{what}: capacities {vcap} vertices, {fcap} triangles do not fit the buffers "
                           f"({out_vertices.numel()} bytes, {out_faces.numel()} indices)")
    need = mesh_simplify_emit_workspace_bytes(nv, nf)
    if workspace is None:
        workspace = torch.empty(max(need, 8), device=faces.device, dtype=torch.uint8)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: workspace must be a contiguous uint8 CUDA/ROCm tensor of >= {need} bytes")
    at = lambda t, n: t.data_ptr() if n else None                  # noqa: E731
    check(_lib.load().itermvs_mesh_simplify_emit(at(reps, nv), nv, rec, at(faces, nf), nf, at(cluster, nv), at(key_hi_sorted, nf),
                                                 at(key_lo_sorted, nf), at(order, nf), at(out_vertices, vcap), vcap,
                                                 at(out_faces, fcap), fcap, totals.data_ptr(), workspace.data_ptr(), _stream()),
          "itermvs_mesh_simplify_emit")


def _colmap_inputs(what: str, offsets: Tensor, point: Tensor, xyz: Tensor, per_view: Tensor, width: int) -> Tuple[int, int]:
    """shared checks of view_scores / depth_ranges -> (V, P).  ``offsets`` is the one HOST tensor: its values are checked here
    (ascending from offsets[0] >= 0 to offsets[V] <= len(point)), which the kernels rely on for their reads of ``point``."""
    for t, name in ((point, "point"), (xyz, "xyz"), (per_view, "per-view matrix")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: {name}: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if not isinstance(offsets, torch.Tensor) or offsets.is_cuda or offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise RuntimeError(f"{what}: offsets must be a 1-D int64 HOST tensor (it is validated here and uploaded)")
    v = offsets.numel() - 1
    if point.dtype != torch.int32 or point.dim() != 1 or not point.is_contiguous():
        raise RuntimeError(f"{what}: point must be a contiguous 1-D int32 tensor")
    if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3 or not xyz.is_contiguous():
        raise RuntimeError(f"{what}: xyz must be a contiguous float64 [P,3] tensor")
    if per_view.dtype != torch.float64 or tuple(per_view.shape) != (v, width) or not per_view.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous float64 [{v},{width}] per-view tensor, got {tuple(per_view.shape)}")
    if v >= 1 and (int(offsets[0]) < 0 or int(offsets[-1]) > point.numel() or bool((offsets[1:] < offsets[:-1]).any())):
        raise RuntimeError(f"{what}: offsets must ascend from >= 0 to <= len(point) = {point.numel()}")
    return v, int(xyz.shape[0])


def view_scores(offsets: Tensor, point: Tensor, xyz: Tensor, centre: Tensor, theta0: float = 5.0, sigma1: float = 1.0,
                sigma2: float = 10.0, offsets_dev: Optional[Tensor] = None) -> Tensor:
    """itermvs_view_scores (colmap_input.py:336-364): the symmetric float64 [V,V] view-selection score matrix.  offsets: HOST
    int64 [V+1] (CSR of the observation lists), point int32 [total] (dense point index or -1), xyz float64 [P,3], centre
    float64 [V,3] on the device; ``offsets_dev``: a device copy of ``offsets`` the caller already holds (uploaded here otherwise).
    Nothing is read back and nothing synchronises."""
    v, p = _colmap_inputs("view_scores", offsets, point, xyz, centre, 3)
    score = torch.empty((max(v, 0), max(v, 0)), device=point.device, dtype=torch.float64)
    off = offsets.to(point.device) if offsets_dev is None else offsets_dev
    check(_lib.load().itermvs_view_scores(off.data_ptr(), point.data_ptr(), xyz.data_ptr(), centre.data_ptr(), v, p, float(theta0),
                                          float(sigma1), float(sigma2), score.data_ptr(), _stream()), "itermvs_view_scores")
    return score


def depth_ranges(offsets: Tensor, point: Tensor, xyz: Tensor, ext_row2: Tensor, offsets_dev: Optional[Tensor] = None) -> Tensor:
    """itermvs_depth_ranges (colmap_input.py:319-333): float64 [V,2] = the order statistics int(len * .01) and int(len * .99)
    of every image's observation depths; NaN for an image without a valid observation.  ext_row2 float64 [V,4] = row 2 of the
    extrinsics; the other arguments as :func:`view_scores`."""
    v, p = _colmap_inputs("depth_ranges", offsets, point, xyz, ext_row2, 4)
    out = torch.empty((max(v, 0), 2), device=point.device, dtype=torch.float64)
    off = offsets.to(point.device) if offsets_dev is None else offsets_dev
    check(_lib.load().itermvs_depth_ranges(off.data_ptr(), point.data_ptr(), xyz.data_ptr(), ext_row2.data_ptr(), v, p,
                                           out.data_ptr(), _stream()), "itermvs_depth_ranges")
    return out


class CloudGrid(NamedTuple):
    """the uniform grid of the cloud_* searches: cell = floor((p - origin) / edge), key = (cx * ny + cy) * nz + cz"""
    origin: Tuple[float, float, float]
    dims: Tuple[int, int, int]
    edge: float

    def args(self) -> tuple:
        return tuple(float(o) for o in self.origin) + tuple(int(d) for d in self.dims) + (float(self.edge),)


def _cloud(what: str, t: Tensor, name: str, dtype=torch.float32, shape_tail: tuple = (3,)) -> Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name}: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if t.dtype != dtype or tuple(t.shape[1:]) != shape_tail or t.dim() != 1 + len(shape_tail) or not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} [n{''.join(',%d' % s for s in shape_tail)}] tensor, "
                           f"got {t.dtype} {tuple(t.shape)}")
    return t


def _cloud_flat(what: str, m: int, *tensors) -> None:
    """every (tensor, dtype, name) is a contiguous flat device tensor of that dtype with exactly ``m`` elements"""
    for t, dt, name in tensors:
        if _cloud(what, t, name, dt, ()).numel() != m:
            raise RuntimeError(f"{what}: {name} must have {m} elements, got {t.numel()}")


def cloud_cell_keys(xyz: Tensor, grid: CloudGrid) -> Tensor:
    """itermvs_cloud_cell_keys: int64 [n] cell keys of float32 [n,3] points on ``grid``; INT64_MAX for a point that is not
    finite or outside the grid.  An extent that does not fit the key (a dimension above 2^21) raises."""
    _cloud("cloud_cell_keys", xyz, "xyz")
    keys = torch.empty((xyz.shape[0],), device=xyz.device, dtype=torch.int64)
    if xyz.shape[0]:
        check(_lib.load().itermvs_cloud_cell_keys(xyz.data_ptr(), xyz.shape[0], *grid.args(), keys.data_ptr(), _stream()),
              "itermvs_cloud_cell_keys")
    return keys


def cloud_reduce_round(xyz_sorted: Tensor, keys_sorted: Tensor, rank_sorted: Tensor, grid: CloudGrid, dst: float, state: Tensor,
                       undecided: Tensor) -> None:
    """itermvs_cloud_reduce_round: one round of the parallel form of reducePts_haa.m:24-30 over the key-sorted cloud.  state
    int32 [n] (0 undecided, 1 kept, 2 removed) is updated in place; ``undecided`` (int32, one element, zeroed by the caller) counts
    the points the round leaves undecided.  Nothing is read back."""
    n = _cloud("cloud_reduce_round", xyz_sorted, "xyz_sorted").shape[0]
    _cloud_flat("cloud_reduce_round", n, (keys_sorted, torch.int64, "keys_sorted"), (rank_sorted, torch.int32, "rank_sorted"),
                (state, torch.int32, "state"))
    _cloud_flat("cloud_reduce_round", 1, (undecided, torch.int32, "undecided"))
    check(_lib.load().itermvs_cloud_reduce_round(xyz_sorted.data_ptr(), keys_sorted.data_ptr(), rank_sorted.data_ptr(), n,
                                                 *grid.args(), float(dst), state.data_ptr(), undecided.data_ptr(), _stream()),
          "itermvs_cloud_reduce_round")


def cloud_nn_distance(q_from: Tensor, to_sorted: Tensor, keys_sorted: Tensor, grid: CloudGrid, region: Sequence[float], cap: float,
                      rings: int, best_d2: Tensor, done: Tensor, dist: Tensor, index: Optional[Tensor] = None) -> None:
    """itermvs_cloud_nn_distance: one grid's rings of the capped nearest-neighbour search of MaxDistCP.m.  q_from float32 [nq,3];
    to_sorted float32 [nt,3] / keys_sorted int64 [nt] in key order on ``grid``; region = the six floats lo[3], hi[3] of the
    covered queries; best_d2 float64 [nq] (+Inf at first), done uint8 [nq] (0 at first) and dist float64 [nq] are updated in
    place; ``index``: int64 list of the queries to look at (default: all).  Nothing is read back."""
    nq = _cloud("cloud_nn_distance", q_from, "q_from").shape[0]
    nt = _cloud("cloud_nn_distance", to_sorted, "to_sorted").shape[0]
    _cloud_flat("cloud_nn_distance", nt, (keys_sorted, torch.int64, "keys_sorted"))
    _cloud_flat("cloud_nn_distance", nq, (best_d2, torch.float64, "best_d2"), (done, torch.uint8, "done"), (dist, torch.float64, "dist"))
    if index is not None:
        _cloud("cloud_nn_distance", index, "index", torch.int64, ())
    if len(region) != 6:
        raise RuntimeError("cloud_nn_distance: region is lo[3] + hi[3]")
    reg = (C.c_double * 6)(*[float(r) for r in region])
    check(_lib.load().itermvs_cloud_nn_distance(q_from.data_ptr(), nq, _ptr(index), 0 if index is None else index.numel(),
                                                to_sorted.data_ptr(), keys_sorted.data_ptr(), nt, *grid.args(), reg, float(cap),
                                                int(rings), best_d2.data_ptr(), done.data_ptr(), dist.data_ptr(), _stream()),
          "itermvs_cloud_nn_distance")


def cloud_in_mask(xyz: Tensor, mask: Tensor, origin: Sequence[float], res: float) -> Tensor:
    """itermvs_cloud_in_mask (PointCompareMain.m:32-41): uint8 [n] = the point's voxel round(((p - origin) / res) + 1) (half away
    from zero) lies inside the uint8 [sx,sy,sz] ``mask`` and is set there."""
    n = _cloud("cloud_in_mask", xyz, "xyz").shape[0]
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError("cloud_in_mask: mask: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if mask.dtype != torch.uint8 or mask.dim() != 3 or not mask.is_contiguous():
        raise RuntimeError(f"cloud_in_mask: mask must be a contiguous uint8 [sx,sy,sz] tensor, got {mask.dtype} {tuple(mask.shape)}")
    out = torch.empty((n,), device=xyz.device, dtype=torch.uint8)
    if n:
        check(_lib.load().itermvs_cloud_in_mask(xyz.data_ptr(), n, mask.data_ptr(), *[int(s) for s in mask.shape],
                                                *[float(o) for o in origin], float(res), out.data_ptr(), _stream()),
              "itermvs_cloud_in_mask")
    return out


def _transform(what: str, T) -> "C.Array":
    m = np.asarray(T.cpu() if torch.is_tensor(T) else T, dtype=np.float64)
    if m.shape != (4, 4):
        raise RuntimeError(f"{what}: T must be a 4x4 matrix, got shape {m.shape}")
    return (C.c_double * 16)(*[float(v) for v in m.reshape(-1)])


def cloud_crop(xyz: Tensor, T, axis: int, axis_min: float, axis_max: float, polygon) -> Tensor:
    """itermvs_cloud_crop: uint8 [n] = 1 where T * p lies in the prism (orthogonal ``axis`` 0/1/2, axis_min <= c <= axis_max, the
    other two coordinates inside ``polygon``, a host [n_poly,3] fp64 array, by the even-odd rule of the header)."""
    n = _cloud("cloud_crop", xyz, "xyz").shape[0]
    poly = np.ascontiguousarray(np.asarray(polygon, dtype=np.float64))
    if poly.ndim != 2 or poly.shape[1] != 3:
        raise RuntimeError(f"cloud_crop: polygon must be [n_poly,3], got shape {poly.shape}")
    out = torch.empty((n,), device=xyz.device, dtype=torch.uint8)
    if n:
        ws = torch.empty((max(2 * poly.shape[0], 1),), device=xyz.device, dtype=torch.float64)
        check(_lib.load().itermvs_cloud_crop(xyz.data_ptr(), n, _transform("cloud_crop", T), int(axis), float(axis_min),
                                             float(axis_max), poly.ctypes.data_as(C.POINTER(C.c_double)), poly.shape[0],
                                             ws.data_ptr(), out.data_ptr(), _stream()), "itermvs_cloud_crop")
    return out


def cloud_voxel_heads(keys_sorted: Tensor) -> Tensor:
    """itermvs_cloud_voxel_heads: int32 [n] = 1 at the first position of every run of equal keys (INT64_MAX keys: 0)"""
    n = _cloud("cloud_voxel_heads", keys_sorted, "keys_sorted", torch.int64, ()).numel()
    head = torch.empty((n,), device=keys_sorted.device, dtype=torch.int32)
    if n:
        check(_lib.load().itermvs_cloud_voxel_heads(keys_sorted.data_ptr(), n, head.data_ptr(), _stream()), "itermvs_cloud_voxel_heads")
    return head


def cloud_voxel_mean(xyz_sorted: Tensor, keys_sorted: Tensor, rank: Tensor, n_out: int) -> Tensor:
    """itermvs_cloud_voxel_mean: float32 [n_out,3] = per run of equal keys the mean of its points (fp64 sum in sorted order, one
    rounding), at the run's ``rank`` (int64 [n]: inclusive prefix sum of the heads, minus 1)"""
    n = _cloud("cloud_voxel_mean", xyz_sorted, "xyz_sorted").shape[0]
    _cloud_flat("cloud_voxel_mean", n, (keys_sorted, torch.int64, "keys_sorted"), (rank, torch.int64, "rank"))
    out = torch.zeros((max(int(n_out), 0), 3), device=xyz_sorted.device, dtype=torch.float32)
    check(_lib.load().itermvs_cloud_voxel_mean(xyz_sorted.data_ptr(), keys_sorted.data_ptr(), rank.data_ptr(), n, int(n_out),
                                               out.data_ptr(), _stream()), "itermvs_cloud_voxel_mean")
    return out


def cloud_nn_index(q: Tensor, T, to_sorted: Tensor, keys_sorted: Tensor, perm: Tensor, grid: CloudGrid, max_dist: float,
                   rings: int) -> Tuple[Tensor, Tensor]:
    """itermvs_cloud_nn_index: (idx int64 [nq], d2 float64 [nq]) = for every query T * q the nearest target with
    d2 < max_dist^2 (exclusive), as ``perm[position]`` (ties: the lowest) or -1 / +Inf.  to_sorted float32 [nt,3], keys_sorted
    and perm int64 [nt] in key order on ``grid``; nt may be 0."""
    nq = _cloud("cloud_nn_index", q, "q").shape[0]
    nt = _cloud("cloud_nn_index", to_sorted, "to_sorted").shape[0]
    _cloud_flat("cloud_nn_index", nt, (keys_sorted, torch.int64, "keys_sorted"), (perm, torch.int64, "perm"))
    idx = torch.empty((nq,), device=q.device, dtype=torch.int64)
    d2 = torch.empty((nq,), device=q.device, dtype=torch.float64)
    check(_lib.load().itermvs_cloud_nn_index(q.data_ptr(), nq, _transform("cloud_nn_index", T), _ptr(to_sorted) if nt else None,
                                             _ptr(keys_sorted) if nt else None, _ptr(perm) if nt else None, nt, *grid.args(),
                                             float(max_dist), int(rings), idx.data_ptr(), d2.data_ptr(), _stream()),
          "itermvs_cloud_nn_index")
    return idx, d2


def cloud_umeyama_groups(n: int) -> int:
    """itermvs_cloud_umeyama_groups: the number of workgroups (= rows of partials) the sums over n correspondences use"""
    g = _lib.load().itermvs_cloud_umeyama_groups(int(n))
    check(min(g, 0), "itermvs_cloud_umeyama_groups")
    return g


def cloud_umeyama_sums(q: Tensor, T, idx: Tensor, d2: Tensor, target: Tensor) -> Tensor:
    """itermvs_cloud_umeyama_sums: float64 [18] on the device = {count, sum p, sum t, sum t p^T, sum |p|^2, sum d2} over the
    correspondences idx[i] >= 0 with p = T * q_i and t = target[idx[i]] (the unsorted targets).  Nothing is read back."""
    n = _cloud("cloud_umeyama_sums", q, "q").shape[0]
    nt = _cloud("cloud_umeyama_sums", target, "target").shape[0]
    _cloud_flat("cloud_umeyama_sums", n, (idx, torch.int64, "idx"), (d2, torch.float64, "d2"))
    partials = torch.empty((max(cloud_umeyama_groups(n), 1) if n else 1, 18), device=q.device, dtype=torch.float64)
    sums = torch.empty((18,), device=q.device, dtype=torch.float64)
    check(_lib.load().itermvs_cloud_umeyama_sums(q.data_ptr(), n, _transform("cloud_umeyama_sums", T), idx.data_ptr(), d2.data_ptr(),
                                                 _ptr(target) if nt else None, nt, partials.data_ptr(), sums.data_ptr(), _stream()),
          "itermvs_cloud_umeyama_sums")
    return sums


def cloud_knn_mean(xyz_sorted: Tensor, keys_sorted: Tensor, perm: Tensor, grid: CloudGrid, k: int, cap: float, rings: int,
                   mean: Tensor, flag: Tensor, index: Optional[Tensor] = None) -> None:
    """itermvs_cloud_knn_mean: one grid's rings of the k-nearest search of a key-sorted cloud against itself.  mean float64 [n] and
    flag uint8 [n] are written in the caller's order (at perm[position]) for every sorted position, or for the positions of
    ``index`` (int64): flag 0 = settled (mean = the mean distance to the k nearest other points), 1 = isolated (fewer than k within
    ``cap``; mean +Inf), 2 = rings used up (mean +Inf; repeat on a coarser grid).  Nothing is read back."""
    n = _cloud("cloud_knn_mean", xyz_sorted, "xyz_sorted").shape[0]
    _cloud_flat("cloud_knn_mean", n, (keys_sorted, torch.int64, "keys_sorted"), (perm, torch.int64, "perm"),
                (mean, torch.float64, "mean"), (flag, torch.uint8, "flag"))
    if index is not None:
        _cloud("cloud_knn_mean", index, "index", torch.int64, ())
    check(_lib.load().itermvs_cloud_knn_mean(_ptr(xyz_sorted), _ptr(keys_sorted), _ptr(perm), n, _ptr(index),
                                             0 if index is None else index.numel(), *grid.args(), int(k), float(cap), int(rings),
                                             _ptr(mean), _ptr(flag), _stream()), "itermvs_cloud_knn_mean")


def cloud_radius_count(xyz_sorted: Tensor, keys_sorted: Tensor, perm: Tensor, grid: CloudGrid, radius: float, limit: int,
                       count: Tensor) -> None:
    """itermvs_cloud_radius_count: count int32 [n], in the caller's order (at perm[position]) = min(number of other points with
    d2 <= radius * radius, limit) for every point of a key-sorted cloud.  Nothing is read back."""
    n = _cloud("cloud_radius_count", xyz_sorted, "xyz_sorted").shape[0]
    _cloud_flat("cloud_radius_count", n, (keys_sorted, torch.int64, "keys_sorted"), (perm, torch.int64, "perm"),
                (count, torch.int32, "count"))
    check(_lib.load().itermvs_cloud_radius_count(_ptr(xyz_sorted), _ptr(keys_sorted), _ptr(perm), n, *grid.args(), float(radius),
                                                 int(limit), _ptr(count), _stream()), "itermvs_cloud_radius_count")


CORRNET_WEIGHT_FLOATS = 14288
CORRNET_WEIGHT_FLOATS_SPLIT3 = 23120     # bf16x3 form: conv0 + conv2 + the two transposed convolutions as split bf16 operands


def _mfma_operand_order(w_tap_ci_co: Tensor, co_pad: int) -> Tensor:
    """[9, Cin, Cout] -> [9][Cin/4][4][co_pad] (zero padded): the A-operand order of v_mfma_f32_16x16x4_f32 in itermvs_corrnet"""
    taps, cin, cout = w_tap_ci_co.shape
    out = torch.zeros((taps, cin // 4, 4, co_pad), device=w_tap_ci_co.device, dtype=torch.float32)
    out[..., :cout] = w_tap_ci_co.reshape(taps, cin // 4, 4, cout)
    return out.reshape(-1)


def pack_corrnet_weights(w: Dict[str, Tensor], prefix: str, split3: bool = False) -> Tensor:
    """the six layers of one CorrNet (state-dict names ``prefix`` + conv0.conv.weight ... conv5.bias) in the layout of
    itermvs_corrnet (include/itermvs_hip.h): the five matrix-core layers in operand order [tap][k-step][q][co], conv5 as
    [ci][tap], the bias, padding.  ``split3``: the set of itermvs_corrnet_bf16x3 -- conv0 as the bf16 A operands of its 18
    v_mfma_f32_16x16x32_bf16 ([mfma][q][row m][8 channels], three-term split of the fp32 weights), conv1 unchanged (fp32), conv2 and
    the two transposed convolutions in itermvs_conv2d's weight_format 3 (bf16 [tap][chunk][h, m, l][row co][16 ci]; a transposed
    convolution as the convolution weight [co][ci][ky][kx] = w[ci][co][ky][kx]), conv5 and the bias unchanged."""
    conv = lambda name, pad: _mfma_operand_order(w[prefix + name].float().permute(2, 3, 1, 0).reshape(9, w[prefix + name].shape[1], -1), pad)
    # ConvTranspose2d weights are [ci, co, ky, kx]
    dconv = lambda name, pad: _mfma_operand_order(w[prefix + name].float().permute(2, 3, 0, 1).reshape(9, w[prefix + name].shape[0], -1), pad)
    # conv0 computes two output rows per matrix-core tile: rows 0..7 = the 8 channels with the taps in window rows 0..2,
    # rows 8..15 = the same channels with the taps in window rows 1..3 ([window row 4][kx 3][ci 8][16])
    w0 = w[prefix + "conv0.conv.weight"].float()                                   # [co 8, ci 8, ky 3, kx 3]
    two = torch.zeros((4, 3, 8, 16), device=w0.device, dtype=torch.float32)
    two[0:3, :, :, 0:8] = w0.permute(2, 3, 1, 0)
    two[1:4, :, :, 8:16] = w0.permute(2, 3, 1, 0)
    if split3:
        wh, wm, wl = split_bf16x3(two)                                              # each [4, 3, 8 ci, 16 rows] bf16
        wp = lambda t: t.reshape(12, 8, 16).permute(0, 2, 1)                        # [window position 12, row m 16, ci 8]
        h, m_, l = wp(wh), wp(wm), wp(wl)
        ops_a = []
        for v in range(6):                  # MFMA 2v = [h h | h h], 2v + 1 = [m m | m m]: lanes q = 0..3 -> window position 2v + (q & 1)
            for term in (h, m_):
                ops_a.append(torch.stack([term[2 * v], term[2 * v + 1], term[2 * v], term[2 * v + 1]]))       # [q 4, m 16, ci 8]
        for v in range(6):                  # MFMA 12 + v = [l l | h h]
            ops_a.append(torch.stack([l[2 * v], l[2 * v + 1], h[2 * v], h[2 * v + 1]]))
        first = torch.stack(ops_a).contiguous().view(torch.int16).reshape(-1).view(torch.float32)              # 18 x 64 x 8 bf16 = 4608 floats
    else:
        first = _mfma_operand_order(two.reshape(12, 8, 16), 16)
    if split3:
        as_floats = lambda wt: MfmaWeight(wt, split3=True).tile3.contiguous().view(torch.int16).reshape(-1).view(torch.float32)
        mid = [as_floats(w[prefix + "conv2.conv.weight"].float()),                       # [9][1][3][32][16] bf16 = 6912 floats
               as_floats(w[prefix + "conv3.weight"].float().permute(1, 0, 2, 3)),          # [9][2][3][16][16]
               as_floats(w[prefix + "conv4.weight"].float().permute(1, 0, 2, 3))]          # [9][1][3][16 (8 used)][16] = 3456 floats
    else:
        mid = [conv("conv2.conv.weight", 32), dconv("conv3.weight", 16), dconv("conv4.weight", 16)]
    parts = [first, conv("conv1.conv.weight", 16)] + mid + [
             w[prefix + "conv5.weight"].float().permute(1, 2, 3, 0).reshape(-1), w[prefix + "conv5.bias"].float().reshape(-1)]
    flat = torch.cat(parts + [torch.zeros(7, device=parts[0].device)])
    assert flat.numel() == (CORRNET_WEIGHT_FLOATS_SPLIT3 if split3 else CORRNET_WEIGHT_FLOATS)
    return flat.contiguous()


STEM_W0_FLOATS, STEM_W1_FLOATS = 224, 2336


def pack_stem_weights(w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor, wd: Tensor, bd: Tensor) -> Tuple[Tensor, Tensor]:
    """weights of itermvs_stem (BatchNorm already folded): FeatureNet.conv1 (w0 [8,3,3,3], b0) as [ci][ky][kx][co] + biases;
    layer1[0].conv1 (w1 [16,8,3,3], b1) and layer1[0].downsample (wd, bd), output channels concatenated, in matrix-core
    operand order [tap][k-step][q][co 32] + the 32 biases"""
    if tuple(w0.shape) != (8, 3, 3, 3) or tuple(w1.shape) != (16, 8, 3, 3) or tuple(wd.shape) != (16, 8, 3, 3):
        raise RuntimeError("pack_stem_weights: expects conv1 [8,3,3,3] and two stride-2 layers [16,8,3,3]")
    p0 = torch.cat([w0.float().permute(1, 2, 3, 0).reshape(-1), b0.float().reshape(-1)]).contiguous()
    wc = torch.cat([w1, wd]).float()                                              # [32, 8, 3, 3]
    p1 = torch.cat([_mfma_operand_order(wc.permute(2, 3, 1, 0).reshape(9, 8, 32), 32), b1.float().reshape(-1),
                    bd.float().reshape(-1)]).contiguous()
    assert p0.numel() == STEM_W0_FLOATS and p1.numel() == STEM_W1_FLOATS
    return p0, p1


def stem(x: Tensor, w0: Tensor, w1: Tensor, compose=None, quads: bool = False):
    """itermvs_stem: x [M,3,H,W] -> (relu(layer1[0].conv1(f0)), layer1[0].downsample(f0)) with f0 = FeatureNet.conv1(x)
    kept in LDS; both [M,16,H2,W2].  ``w0`` / ``w1`` from pack_stem_weights.
    ``compose`` = (mats [n,V,4,4], nan_flag | None, (depth_min, depth_max)): itermvs_stem_compose -- the camera composition
    (compose_proj + inverse depth range) rides in the same launch; returns (y, sc, proj [n,V-1,12], inv_min, inv_max).
    ``quads``: y and sc are written as channel quads -- tensors of shape [M,4,H2,W2,4] holding channel 4*cq + c at [m,cq,y,x,c] --
    the layout res_chain16(..., quads=True) fetches with 16-byte loads."""
    ptr, x_sn = _planes(x, "stem input")
    m, c, h, w = x.shape
    if c != 3:
        raise RuntimeError("stem: expects [M,3,H,W]")
    if w0.numel() != STEM_W0_FLOATS or w1.numel() != STEM_W1_FLOATS:
        raise RuntimeError("stem: weights must come from pack_stem_weights")
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((m, 4, h2, w2, 4) if quads else (m, 16, h2, w2), device=x.device, dtype=torch.float32)
    sc = torch.empty_like(y)
    if compose is not None:
        mats, nan_flag, depth_range = compose
        mats = _dev(mats, "mats").contiguous()
        n, v = mats.shape[0], mats.shape[1]
        proj = torch.empty((n, v - 1, 12), device=mats.device, dtype=torch.float32)
        dmin, dmax = (_dev(t, "depth range").contiguous() for t in depth_range)
        imin, imax = torch.empty_like(dmin), torch.empty_like(dmax)
        check(_lib.load().itermvs_stem_compose(ptr, x_sn, m, h, w, _dev(w0, "stem weights").data_ptr(), _dev(w1, "stem weights").data_ptr(),
                                               y.data_ptr(), sc.data_ptr(), 16 * h2 * w2, int(quads), mats.data_ptr(), n, v, proj.data_ptr(),
                                               _ptr(nan_flag), dmin.data_ptr(), dmax.data_ptr(), dmin.numel(), imin.data_ptr(),
                                               imax.data_ptr(), _stream()), "itermvs_stem_compose")
        return y, sc, proj, imin, imax
    check(_lib.load().itermvs_stem(ptr, x_sn, m, h, w, _dev(w0, "stem weights").data_ptr(), _dev(w1, "stem weights").data_ptr(),
                             y.data_ptr(), sc.data_ptr(), 16 * h2 * w2, int(quads), _stream()), "itermvs_stem")
    return y, sc


def res_chain16(y1: Tensor, shortcut: Tensor, weights: Sequence["MfmaWeight"], biases: Sequence[Optional[Tensor]],
                out: Optional[Tensor] = None, quads: bool = False) -> Tensor:
    """itermvs_res_chain16: FeatureNet.layer1 behind the stem in one launch -- a = relu(conv(y1; W0) + b0 + shortcut),
    b = relu(conv(a; W1) + b1), out = relu(conv(b; W2) + b2 + a); ``y1`` / ``shortcut`` [N,16,H,W] (ops.stem's results) or,
    with ``quads``, [N,4,H,W,4] (ops.stem(..., quads=True)); ``weights``: the three layers' MfmaWeight (bf16x3 form, 16 -> 16),
    ``biases``: [16] each or None.  ``out`` [N,16,H,W] planes."""
    if quads:
        for t, name in ((y1, "res_chain16 input"), (shortcut, "res_chain16 shortcut")):
            _dev(t, name)
            if t.dim() != 5 or t.shape[1] != 4 or t.shape[4] != 4 or not t.is_contiguous():
                raise RuntimeError(f"{name}: quads layout is a contiguous [N,4,H,W,4] tensor")
        n, _, h, w, _ = y1.shape
        if tuple(shortcut.shape) != tuple(y1.shape):
            raise RuntimeError("res_chain16: input and shortcut differ in shape")
        ptr, y_sn, sp, s_sn = y1.data_ptr(), 16 * h * w, shortcut.data_ptr(), 16 * h * w
    else:
        ptr, y_sn = _planes(y1, "res_chain16 input")
        sp, s_sn = _planes(shortcut, "res_chain16 shortcut")
        n, c, h, w = y1.shape
        if c != 16 or tuple(shortcut.shape) != (n, c, h, w):
            raise RuntimeError("res_chain16: expects two [N,16,H,W] tensors")
    if len(weights) != 3 or len(biases) != 3:
        raise RuntimeError("res_chain16: three layers")
    for wt in weights:
        if not isinstance(wt, MfmaWeight) or wt.tile3 is None or wt.cin != 16 or wt.cout != 16 or wt.ksize != 3:
            raise RuntimeError("res_chain16: weights must be 3x3 16 -> 16 MfmaWeight built with split3=True")
        if not wt.tile3.is_cuda or wt.tile3.dtype != torch.bfloat16:
            raise RuntimeError("res_chain16 weights: expected bfloat16 ROCm tensors (MfmaWeight.tile3)")
    if out is None:
        out = torch.empty((n, 16, h, w), device=y1.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, 16, h, w):
        raise RuntimeError(f"res_chain16: output has shape {tuple(out.shape)}, expected {(n, 16, h, w)}")
    po, o_sn = _planes(out, "res_chain16 output")
    wp = (C.c_void_p * 3)(*[wt.tile3.data_ptr() for wt in weights])
    bl = [None if b is None else _dev(b, "res_chain16 bias").float().contiguous() for b in biases]
    bp = (C.c_void_p * 3)(*[_ptr(b) for b in bl])
    check(_lib.load().itermvs_res_chain16(ptr, y_sn, sp, s_sn, int(quads), n, h, w, wp, bp, po, o_sn, _stream()), "itermvs_res_chain16")
    if CONV_FLOP_COUNTER["enabled"]:         # the three layers' FLOPs (the recomputed halo is not counted), one bracketed launch
        CONV_FLOP_COUNTER["flops"] += 3 * 2.0 * n * h * w * 16 * 16 * 9
        CONV_FLOP_COUNTER["launches"] += 1
    return out


def down_conv(x: Tensor, packed: "MfmaWeight", bias: Optional[Tensor], split_channel: int, out: Optional[Tensor] = None,
              out_b: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """itermvs_down_conv: a residual block's stride-2 pair in one launch -- y = relu(conv3x3_s2(x; W1) + b1) and
    sc = conv3x3_s2(x; Wd) + bd (padding 1); ``x`` [N,Cin,H,W] planes, ``packed`` = MfmaWeight(cat(W1, Wd), split3=True),
    ``bias`` = cat(b1, bd) or None, ``split_channel`` = C, the channels of each result; (Cin, C) = (16, 32) or (32, 48).
    ``out`` / ``out_b``: destinations [N,C,(H-1)//2+1,(W-1)//2+1] (planes).  Returns (y, sc)."""
    ptr, x_sn = _planes(x, "down_conv input")
    n, cin, h, w = x.shape
    c = int(split_channel)
    if not isinstance(packed, MfmaWeight) or packed.ksize != 3 or packed.transposed or packed.cin != cin or packed.cout != 2 * c:
        raise RuntimeError("down_conv: weight must be the 3x3 MfmaWeight of cat(W1, Wd) [2C,Cin,3,3]")
    if packed.tile3 is None:
        raise RuntimeError("down_conv: weight must be built with split3=True (bf16x3 form)")
    if not packed.tile3.is_cuda or packed.tile3.dtype != torch.bfloat16:
        raise RuntimeError("down_conv weights: expected bfloat16 ROCm tensors (MfmaWeight.tile3)")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    res = []
    for t, name in ((out, "down_conv output"), (out_b, "down_conv shortcut output")):
        if t is None:
            t = torch.empty((n, c, ho, wo), device=x.device, dtype=torch.float32)
        elif tuple(t.shape) != (n, c, ho, wo) or t.dtype != torch.float32:
            raise RuntimeError(f"{name}: has shape {tuple(t.shape)}, expected float32 {(n, c, ho, wo)}")
        res.append((t,) + _planes(t, name))
    (y, py, y_sn), (sc, ps, s_sn) = res
    bl = None if bias is None else _dev(bias, "down_conv bias").float().contiguous()
    if bl is not None and bl.numel() != 2 * c:
        raise RuntimeError(f"down_conv: bias has {bl.numel()} elements, expected {2 * c}")
    check(_lib.load().itermvs_down_conv(ptr, x_sn, n, cin, h, w, packed.tile3.data_ptr(), _ptr(bl), c, py, y_sn, ps, s_sn, _stream()),
          "itermvs_down_conv")
    if CONV_FLOP_COUNTER["enabled"]:
        CONV_FLOP_COUNTER["flops"] += 2.0 * n * ho * wo * 2 * c * cin * 9
        CONV_FLOP_COUNTER["launches"] += 1
    return y, sc


def lateral_conv3x3(fine: Tensor, coarse: Tensor, w_lat: "MfmaWeight", b_lat: Optional[Tensor], w_out: "MfmaWeight",
                    b_out: Optional[Tensor], out: Optional[Tensor] = None, channels_last_out: bool = False,
                    out2: Optional[Tensor] = None) -> Tensor:
    """itermvs_lateral_conv3x3: out = conv3x3(F.interpolate(coarse, x2, bilinear) + conv1x1(fine; w_lat) + b_lat; w_out) + b_out
    in one launch (net.py:48-50), the 48-channel intermediate map stays on the chip.  ``fine`` [N,16,H,W], ``coarse``
    [N,48,H/2,W/2] planes; ``w_lat``: MfmaWeight of the 1x1 layer 16 -> 48, ``w_out``: MfmaWeight(split3=True) of the 3x3 layer
    48 -> 16.  ``channels_last_out``: ``out`` in channels-last memory format, fp32 / fp16 / bf16 storage (the feature maps the
    correlation kernels gather from); ``out2``: optional fp32 planar copy."""
    fp, f_sn = _planes(fine, "lateral_conv3x3 fine input")
    cp, c_sn = _planes(coarse, "lateral_conv3x3 coarse input")
    n, cf, h, w = fine.shape
    if h % 2 or w % 2 or tuple(coarse.shape) != (n, 48, h // 2, w // 2):
        raise RuntimeError(f"lateral_conv3x3: coarse input {tuple(coarse.shape)} is not [N,48,H/2,W/2] of fine input {tuple(fine.shape)}")
    if not (isinstance(w_lat, MfmaWeight) and w_lat.ksize == 1 and w_lat.cin == cf and w_lat.cout == 48):
        raise RuntimeError("lateral_conv3x3: w_lat must be the MfmaWeight of a 1x1 layer Cf -> 48")
    if not (isinstance(w_out, MfmaWeight) and w_out.ksize == 3 and w_out.cin == 48 and w_out.tile3 is not None):
        raise RuntimeError("lateral_conv3x3: w_out must be the MfmaWeight (split3=True) of a 3x3 layer 48 -> Cout")
    if not (w_out.tile3.is_cuda and w_lat.data.is_cuda):
        raise RuntimeError("lateral_conv3x3 weights: expected ROCm tensors")
    cout = w_out.cout
    if out is None:
        out = torch.empty((n, cout, h, w), device=fine.device, dtype=torch.float32,
                          memory_format=torch.channels_last if channels_last_out else torch.contiguous_format)
    if tuple(out.shape) != (n, cout, h, w):
        raise RuntimeError(f"lateral_conv3x3: output has shape {tuple(out.shape)}, expected {(n, cout, h, w)}")
    if channels_last_out:
        if not out.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("lateral_conv3x3: channels_last_out needs a dense channels-last `out`")
        po, o_sn, layout = out.data_ptr(), cout * h * w, 1 + _feat(out, "lateral_conv3x3 output")
    else:
        if out.dtype != torch.float32:
            raise RuntimeError("lateral_conv3x3: planar output is fp32")
        po, o_sn = _planes(out, "lateral_conv3x3 output")
        layout = 0
    if out2 is not None and not (out2.dtype == torch.float32 and out2.is_contiguous() and tuple(out2.shape) == (n, cout, h, w)):
        raise RuntimeError("lateral_conv3x3: out2 must be a dense fp32 [N,Cout,H,W] tensor")
    bl = None if b_lat is None else _dev(b_lat, "lateral_conv3x3 bias").float().contiguous()
    bo = None if b_out is None else _dev(b_out, "lateral_conv3x3 bias").float().contiguous()
    check(_lib.load().itermvs_lateral_conv3x3(fp, f_sn, cf, cp, c_sn, n, h, w, w_lat.data.data_ptr(), _ptr(bl), w_out.tile3.data_ptr(),
                                              _ptr(bo), cout, po, o_sn, layout, _ptr(out2), _stream()), "itermvs_lateral_conv3x3")
    if CONV_FLOP_COUNTER["enabled"]:         # 1x1 layer + 3x3 layer (the recomputed halo is not counted), one bracketed launch
        CONV_FLOP_COUNTER["flops"] += 2.0 * n * h * w * (cf * 48 + 48 * cout * 9)
        CONV_FLOP_COUNTER["launches"] += 1
    return out


def corrnet(x: Tensor, weight_sets: Sequence[Tensor], seg_end: Sequence[int] = (), out: Optional[Tensor] = None,
            out2: Optional[Tensor] = None) -> Tensor:
    """itermvs_corrnet: x [M,8,H,W] -> [M,1,H,W]; ``weight_sets`` = 1..3 tensors from pack_corrnet_weights, ``seg_end`` the
    batch boundaries between them; ``out`` / ``out2``: [M,1,H,W] views with dense planes (e.g. channels of the GRU buffers)"""
    ptr, x_sn = _planes(x, "corrnet input")
    m, c, h, w = x.shape
    if c != 8 or h % 4 or w % 4:
        raise RuntimeError("corrnet: expects [M,8,H,W] with H and W multiples of 4")
    if out is None:
        out = torch.empty((m, 1, h, w), device=x.device, dtype=torch.float32)
    po, o_sn = _planes(out, "corrnet output")
    p2, o2_sn = _planes(out2, "corrnet output 2") if out2 is not None else (None, 0)
    for t in (out, out2):
        if t is not None and tuple(t.shape) != (m, 1, h, w):
            raise RuntimeError(f"corrnet: output has shape {tuple(t.shape)}, expected {(m, 1, h, w)}")
    wp = (C.c_void_p * len(weight_sets))(*[_dev(t, "corrnet weights").data_ptr() for t in weight_sets])
    se = (C.c_int32 * 3)(*(list(seg_end) + [m] * (3 - len(seg_end))))
    sizes = {t.numel() for t in weight_sets}
    if sizes == {CORRNET_WEIGHT_FLOATS_SPLIT3}:
        check(_lib.load().itermvs_corrnet_bf16x3(ptr, x_sn, wp, se, len(weight_sets), m, h, w, po, o_sn, p2, o2_sn, _stream()),
              "itermvs_corrnet_bf16x3")
        return out
    if sizes != {CORRNET_WEIGHT_FLOATS}:
        raise RuntimeError("corrnet: weight sets must all come from pack_corrnet_weights (one arithmetic)")
    check(_lib.load().itermvs_corrnet(ptr, x_sn, wp, se, len(weight_sets), m, h, w, po, o_sn, p2, o2_sn, _stream()), "itermvs_corrnet")
    return out


def image_pyramid(raw: Tensor, height: int, width: int, all_levels: bool = True, out0: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """datasets/dtu_yao_eval.py:61-74 on the GPU: raw [V,Hs,Ws,3] uint8 RGB (device) -> {'level_0': [V,3,H,W] float32 in
    -1..1, resized like cv2.resize(INTER_LINEAR), 'level_1'..'level_3': the reference's lower pyramid levels}"""
    if not raw.is_cuda or raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[3] != 3:
        raise RuntimeError("image_pyramid: expected a CUDA uint8 tensor [V,Hs,Ws,3]")
    raw = raw.contiguous()
    v, hs, ws, _ = raw.shape
    if out0 is not None and (tuple(out0.shape) != (v, 3, height, width) or not out0.is_contiguous() or out0.dtype != torch.float32):
        raise RuntimeError("image_pyramid: out0 must be a contiguous float32 [V,3,H,W] tensor")
    out = {"level_0": out0 if out0 is not None else torch.empty((v, 3, height, width), device=raw.device, dtype=torch.float32)}
    if all_levels:
        for l in (1, 2, 3):
            out[f"level_{l}"] = torch.empty((v, 3, height >> l, width >> l), device=raw.device, dtype=torch.float32)
    check(_lib.load().itermvs_image_pyramid(raw.data_ptr(), v, hs, ws, height, width, out["level_0"].data_ptr(),
                                            _ptr(out.get("level_1")), _ptr(out.get("level_2")), _ptr(out.get("level_3")), _stream()),
          "itermvs_image_pyramid")
    return out


_RESIZE_TABLES: Dict[tuple, Tuple[Tensor, Tensor, Tensor, Tensor]] = {}


def resize_rgb8(raw: Tensor, height: int, width: int) -> Tensor:
    """itermvs_resize_rgb8: raw [V,Hs,Ws,3] uint8 RGB (device) -> uint8 [V,H,W,3], view for view the bytes of
    ``np.array(Image.fromarray(raw[v]).resize((width, height), Image.BILINEAR))`` (the fusion's vertex colours,
    fusion.read_scan_image(as_uint8=True)).  Pillow's coefficient tables come from ``resize.resize_tables`` (host doubles) and
    stay on the device per (Hs, Ws, H, W); a resize to the same size returns a copy of the input bytes."""
    if not raw.is_cuda or raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[3] != 3:
        raise RuntimeError("resize_rgb8: expected a CUDA uint8 tensor [V,Hs,Ws,3]")
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise RuntimeError(f"resize_rgb8: the output size must be positive, got {height} x {width}")
    raw = raw.contiguous()
    v, hs, ws, _ = raw.shape
    if (hs, ws) == (height, width):
        return raw.clone()
    key = (hs, ws, height, width, raw.device)
    tables = _RESIZE_TABLES.get(key)
    if tables is None:
        from .resize import resize_tables
        tables = _RESIZE_TABLES[key] = tuple(torch.from_numpy(np.array(t)).to(raw.device)     # (the cached arrays are read-only)
                                             for t in resize_tables(hs, ws, height, width))
    xb, xk, yb, yk = tables
    out = torch.empty((v, height, width, 3), device=raw.device, dtype=torch.uint8)
    check(_lib.load().itermvs_resize_rgb8(raw.data_ptr(), v, hs, ws, height, width, xb.data_ptr(), xk.data_ptr(), xk.shape[1],
                                          yb.data_ptr(), yk.data_ptr(), yk.shape[1], out.data_ptr(), _stream()),
          "itermvs_resize_rgb8")
    return out


def undistort_rgb8(raw: Tensor, model, params, out_camera, out_hw: Tuple[int, int], want_map: bool = False):
    """itermvs_undistort_rgb8: raw [Hs,Ws,3] uint8 RGB (device), an image of the COLMAP camera (``model``: name or id, ``params``
    in COLMAP's order) -> uint8 [Ho,Wo,3], the image of the pinhole camera ``out_camera`` = (fx, fy, cx, cy) of size ``out_hw``
    = (Ho, Wo); pixels whose source coordinate leaves the image are (0, 0, 0).  ``want_map``: also float64 [Ho,Wo,2], the source
    coordinates (sx, sy) the kernel sampled at.  FOV and THIN_PRISM_FISHEYE are a ValueError naming the model."""
    from .colmap import CAMERA_MODELS, CAMERA_MODEL_NAMES
    from .undistort import SUPPORTED_MODELS
    name = CAMERA_MODELS[model][0] if model in CAMERA_MODELS else model
    if name not in CAMERA_MODEL_NAMES or name not in SUPPORTED_MODELS:
        raise ValueError(f"undistort_rgb8: camera model {name} is not supported")
    mid, count = CAMERA_MODEL_NAMES[name]
    values = [float(x) for x in params]
    if len(values) != count:
        raise ValueError(f"undistort_rgb8: camera model {name} has {count} parameters, got {len(values)}")
    if not raw.is_cuda or raw.dtype != torch.uint8 or raw.dim() != 3 or raw.shape[2] != 3:
        raise RuntimeError("undistort_rgb8: expected a CUDA uint8 tensor [Hs,Ws,3]")
    height, width = int(out_hw[0]), int(out_hw[1])
    if height < 1 or width < 1:
        raise RuntimeError(f"undistort_rgb8: the output size must be positive, got {height} x {width}")
    raw = raw.contiguous()
    hs, ws, _ = raw.shape
    fx, fy, cx, cy = (float(x) for x in out_camera)
    out = torch.empty((height, width, 3), device=raw.device, dtype=torch.uint8)
    coords = torch.empty((height, width, 2), device=raw.device, dtype=torch.float64) if want_map else None
    check(_lib.load().itermvs_undistort_rgb8(raw.data_ptr(), hs, ws, mid, (C.c_double * count)(*values), count, fx, fy, cx, cy,
                                             height, width, out.data_ptr(), _ptr(coords), _stream()), "itermvs_undistort_rgb8")
    return (out, coords) if want_map else out


JITTER_BYTES = 16      # sizeof(itermvs_jitter): brightness f32, contrast f32, contrast_first i32, enabled i32


def image_pyramid_jitter(raw: Tensor, height: int, width: int, jitter: Tensor, all_levels: bool = True) -> Dict[str, Tensor]:
    """datasets/dtu_yao.py:64-77 / blendedmvs.py:85-101 in train mode on the GPU: Pillow's ColorJitter(brightness=0.5,
    contrast=0.5) per view, then ``image_pyramid``.  raw [V,Hs,Ws,3] uint8 (device); jitter: uint8 device tensor of V
    itermvs_jitter records (train_dataset.jitter_records)."""
    if not raw.is_cuda or raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[3] != 3:
        raise RuntimeError("image_pyramid_jitter: expected a CUDA uint8 tensor [V,Hs,Ws,3]")
    raw = raw.contiguous()
    v, hs, ws, _ = raw.shape
    if not jitter.is_cuda or jitter.dtype != torch.uint8 or not jitter.is_contiguous() or jitter.numel() != v * JITTER_BYTES:
        raise RuntimeError(f"image_pyramid_jitter: jitter must be a contiguous CUDA uint8 tensor of {v} x {JITTER_BYTES} bytes")
    if jitter.data_ptr() % 4:
        raise RuntimeError("image_pyramid_jitter: the jitter records must start on a 4-byte boundary (float / int32 fields)")
    out = {"level_0": torch.empty((v, 3, height, width), device=raw.device, dtype=torch.float32)}
    if all_levels:
        for l in (1, 2, 3):
            out[f"level_{l}"] = torch.empty((v, 3, height >> l, width >> l), device=raw.device, dtype=torch.float32)
    lsum = torch.empty((v,), device=raw.device, dtype=torch.int64)
    check(_lib.load().itermvs_image_pyramid_jitter(raw.data_ptr(), v, hs, ws, height, width, jitter.data_ptr(), lsum.data_ptr(),
                                                   out["level_0"].data_ptr(), _ptr(out.get("level_1")), _ptr(out.get("level_2")),
                                                   _ptr(out.get("level_3")), _stream()),
          "itermvs_image_pyramid_jitter")
    return out


def gt_pyramid(depth_rows: Tensor, mask_src: Optional[Tensor], params: Tensor, height: int, width: int, recipe: int,
               levels: Sequence[int] = (0, 1, 2, 3)) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """itermvs_gt_pyramid: datasets/dtu_yao.py:80-119 (recipe _lib.GT_DTU) or blendedmvs.py:62-83 (_lib.GT_BLENDEDMVS) for a
    batch.  depth_rows [B,Hs,Ws] float32 PFM payload (rows bottom-up), mask_src [B,Hs,Ws] uint8 depth_visual (DTU) or None,
    params [B,4] float32 (device) -> ({'level_l': [B,1,H>>l,W>>l]} depth, same for the mask) for l in ``levels``"""
    if not depth_rows.is_cuda or depth_rows.dtype != torch.float32 or depth_rows.dim() != 3 or not depth_rows.is_contiguous():
        raise RuntimeError("gt_pyramid: depth_rows must be a contiguous CUDA float32 tensor [B,Hs,Ws]")
    b, hs, ws = depth_rows.shape
    if mask_src is not None and (not mask_src.is_cuda or mask_src.dtype != torch.uint8 or tuple(mask_src.shape) != (b, hs, ws)
                                 or not mask_src.is_contiguous()):
        raise RuntimeError("gt_pyramid: mask_src must be a contiguous CUDA uint8 tensor [B,Hs,Ws]")
    if not params.is_cuda or params.dtype != torch.float32 or tuple(params.shape) != (b, 4) or not params.is_contiguous():
        raise RuntimeError("gt_pyramid: params must be a contiguous CUDA float32 tensor [B,4]")
    dev = depth_rows.device
    depth = {f"level_{l}": torch.empty((b, 1, height >> l, width >> l), device=dev, dtype=torch.float32) for l in levels}
    mask = {f"level_{l}": torch.empty((b, 1, height >> l, width >> l), device=dev, dtype=torch.float32) for l in levels}
    check(_lib.load().itermvs_gt_pyramid(depth_rows.data_ptr(), _ptr(mask_src), params.data_ptr(), b, hs, ws, height, width, recipe,
                                         *[_ptr(depth.get(f"level_{l}")) for l in range(4)],
                                         *[_ptr(mask.get(f"level_{l}")) for l in range(4)], _stream()),
          "itermvs_gt_pyramid")
    return depth, mask


_PROFILE_MASK = [0x3]


def profile_enable(capacity: int, mask: int = 0x3) -> None:
    """mask: bit 0 corr_iter, bit 1 corr_init, bit 2 every itermvs_conv2d launch"""
    _PROFILE_MASK[0] = mask
    check(_lib.load().itermvs_profile_set_mask(mask), "itermvs_profile_set_mask")
    check(_lib.load().itermvs_profile_enable(capacity), "itermvs_profile_enable")


def profile_graph_count() -> int:
    """event pairs embedded so far in captured hipGraphs (see itermvs_profile_graph_read)"""
    return _lib.load().itermvs_profile_graph_count()


def profile_graph_read(first: int, count: int):
    """-> list of (kind, milliseconds) of pairs [first, first+count) for the latest replay of their graph (waits)"""
    kinds = (C.c_int32 * max(count, 1))()
    ms = (C.c_float * max(count, 1))()
    n = _lib.load().itermvs_profile_graph_read(first, count, kinds, ms)
    return [(kinds[i], ms[i]) for i in range(n)]


def profile_collect(max_samples: int = 4096):
    """-> list of (kind, milliseconds); kind 1 = corr_iter, 2 = corr_init."""
    kinds = (C.c_int32 * max_samples)()
    ms = (C.c_float * max_samples)()
    n = _lib.load().itermvs_profile_collect(kinds, ms, max_samples)
    return [(kinds[i], ms[i]) for i in range(n)]

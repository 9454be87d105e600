"""Float64 reference for the gradients of the fused correlation kernels (itermvs_corr_iter_backward,
itermvs_corr_init_backward): the oracle's forward restated in float64 and differentiated by torch autograd on the CPU.

The sampling positions come from ``O.warp_source_coords`` in fp32 exactly as the oracle computes them (so the bilinear taps
are the kernels' taps); the bilinear weights, the gather, the group correlation and the view-weighted mean are evaluated
in float64.  Features are taken as given: for 16-bit storage the caller passes the stored values (held in fp32)."""
from typing import Dict, List, Sequence, Tuple

import torch

from oracle import itermvs_oracle as O

CHANS = {1: 16, 2: 32, 3: 48}
REF_Q_OFFSET = {1: 0, 2: 16, 3: 48}          # channel offsets of the three levels in ref_q [B,H,W,96]
F64 = torch.float64


def proj44(p12_s: torch.Tensor) -> torch.Tensor:
    """[B,12] rows of [rot|trans] -> the [B,4,4] matrix warp_source_coords takes"""
    b = p12_s.shape[0]
    return torch.cat([p12_s.float().view(b, 3, 4), torch.zeros(b, 1, 4)], 1)


def source_coords(p12_s: torch.Tensor, depth: torch.Tensor, size: Tuple[int, int]):
    """fp32 sampling positions (the oracle's, module.py:89-115) -> float64 tensors holding the same values"""
    with torch.no_grad():
        ix, iy, _ = O.warp_source_coords(proj44(p12_s), depth.float(), size[0], size[1])
    return ix.to(F64), iy.to(F64)


def view_correlations(src_pv: torch.Tensor, ref: torch.Tensor, p12_l: torch.Tensor, depth: torch.Tensor,
                      dtype=F64) -> List[torch.Tensor]:
    """per-view group correlations [B,G,N,h,w] of one level: src_pv [B,V,C,H1,W1] (view 0 is skipped), ref [B,C,h,w]"""
    size = tuple(src_pv.shape[-2:])
    out = []
    for s in range(1, src_pv.shape[1]):
        ix, iy = source_coords(p12_l[:, s - 1], depth, size)
        out.append(O.group_correlation(O.bilinear_gather(src_pv[:, s].to(dtype), ix.to(dtype), iy.to(dtype)), ref.to(dtype)))
    return out


def iter_outputs(feats: Dict[int, torch.Tensor], ref_q: torch.Tensor, p12: torch.Tensor, view_w: torch.Tensor,
                 depth: Dict[int, torch.Tensor], b: int, v: int, dtype=F64) -> List[torch.Tensor]:
    """itermvs.py:84-120 per level: the view-weighted mean of the group correlations, [B,N_l,8,h,w] for l = 1, 2, 3.
    feats[l] [B*V,C_l,H_l,W_l] (views 1..V-1 are the sources), ref_q [B,h,w,96], p12 [3,B,S,12], view_w [B,S,h,w]."""
    h, w = ref_q.shape[1:3]
    outs = []
    for i, l in enumerate((1, 2, 3)):
        refl = ref_q[..., REF_Q_OFFSET[l]:REF_Q_OFFSET[l] + CHANS[l]].permute(0, 3, 1, 2)
        acc, wsum = 0, 1e-5
        pv = feats[l].view(b, v, *feats[l].shape[1:])
        for s, corr in enumerate(view_correlations(pv, refl, p12[i], depth[l], dtype)):
            wv = view_w[:, s].to(dtype).view(b, 1, 1, h, w)
            acc, wsum = acc + corr * wv, wsum + wv
        outs.append((acc / wsum).permute(0, 2, 1, 3, 4))
    return outs


def corr_iter_grads(feats: Dict[int, torch.Tensor], ref_q: torch.Tensor, p12: torch.Tensor, view_w: torch.Tensor,
                    depth: Dict[int, torch.Tensor], gout: Sequence[torch.Tensor], b: int, v: int, dtype=F64):
    """gradients of sum_l <gout[l], iter_outputs[l]> -> ({l: d/dfeats[l]}, d/dref_q), in ``dtype``"""
    f = {l: feats[l].detach().to(dtype).requires_grad_(True) for l in (1, 2, 3)}
    rq = ref_q.detach().to(dtype).requires_grad_(True)
    outs = iter_outputs(f, rq, p12, view_w, depth, b, v, dtype)
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, gout)).backward()
    return {l: f[l].grad for l in (1, 2, 3)}, rq.grad


def init_outputs(f3: torch.Tensor, p12_3: torch.Tensor, depth: torch.Tensor, b: int, v: int, dtype=F64) -> torch.Tensor:
    """itermvs.py:48-51: per-view group correlations [B,S,N,8,h,w] of the level-3 features f3 [B*V,48,h,w]"""
    pv = f3.view(b, v, *f3.shape[1:])
    return torch.stack([c.permute(0, 2, 1, 3, 4) for c in view_correlations(pv, pv[:, 0], p12_3, depth, dtype)], 1)


def corr_init_grads(f3: torch.Tensor, p12_3: torch.Tensor, depth: torch.Tensor, gout: torch.Tensor, b: int, v: int,
                    dtype=F64) -> torch.Tensor:
    """d/df3 of <gout, init_outputs> (reference view gathered, source views scattered), in ``dtype``"""
    f = f3.detach().to(dtype).requires_grad_(True)
    (init_outputs(f, p12_3, depth, b, v, dtype) * gout.to(dtype)).sum().backward()
    return f.grad


def parity(got: torch.Tensor, want: torch.Tensor) -> Tuple[float, float]:
    """(max |got - want|, max(1, max |want|)) in float64"""
    want = want.detach().cpu().to(F64)
    err = float((got.detach().cpu().to(F64) - want).abs().max()) if want.numel() else 0.0
    return err, max(1.0, float(want.abs().max())) if want.numel() else 1.0

"""Pillow's 8-bit bilinear resample (``Image.resize(size, Image.BILINEAR)`` on an RGB image), the part that involves floating
point: the per-axis coefficient tables.  Pillow (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) computes
them in C doubles and rounds them to integers with 22 fractional bits; the two passes over the pixels are integer arithmetic
on those tables.  Python floats are the same doubles, so the tables below are Pillow's, and a kernel that follows the integer
passes (``itermvs_resize_rgb8``) reproduces Pillow's bytes by construction.  No GPU is needed here.

Per axis, input size n, output size m, output index xx:
    scale = n / m;  fs = max(scale, 1.0);  support = fs  (the triangle filter's support of 1, widened when shrinking)
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0);  count = min(int(center + support + 0.5), n) - xmin
    w[x] = max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|) for x < count, divided by their sum when it is not zero
    k[x] = int(0.5 + w[x] * 2**22)                                  (the weights are never negative)
A pass computes clip(((1 << 21) + sum(pixel[xmin + x] * k[x])) >> 22, 0, 255); the horizontal pass runs first and its
rounded uint8 result feeds the vertical pass.  Pillow skips the pass of an axis that keeps its size; the table of such an
axis is the identity here (one tap of 2**22), which gives the same bytes.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2          # Resample.c: 8 bits for the pixel, 2 spare, the rest for the coefficient


@lru_cache(maxsize=64)
def bilinear_coefficients(n: int, m: int) -> Tuple[np.ndarray, np.ndarray]:
    """one axis resized from ``n`` to ``m`` samples -> (bounds int32 [m,2] = (first input sample, tap count),
    coefficients int32 [m,ksize], zero past the tap count).  The arrays are cached: do not write to them."""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"bilinear_coefficients: sizes must be >= 1, got {n} -> {m}")
    if n == m:
        bounds = np.stack([np.arange(m, dtype=np.int32), np.ones(m, np.int32)], 1)
        kk = np.full((m, 1), 1 << PRECISION_BITS, np.int32)
        bounds.setflags(write=False)
        kk.setflags(write=False)
        return bounds, kk
    scale = n / m
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((m, 2), np.int32)
    kk = np.zeros((m, ksize), np.int32)
    for xx in range(m):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, count)
        kk[xx, :count] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def resize_tables(hs: int, ws: int, h: int, w: int):
    """the tables of an [hs,ws] -> [h,w] resize: (xbounds [w,2], xk [w,kx], ybounds [h,2], yk [h,ky]) int32"""
    xb, xk = bilinear_coefficients(ws, w)
    yb, yk = bilinear_coefficients(hs, h)
    return xb, xk, yb, yk

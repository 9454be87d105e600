"""numpy restatement of the outlier-removal searches (csrc/cloud_filter.hip, itermvs_amd/cloud_filter.py) with the kernels' dtypes
and order of operations: brute-force fp64 squared distances ((dx*dx) + (dy*dy)) + (dz*dz) on the float32 coordinates, the point
itself excluded BY INDEX (a duplicate at distance 0 is a neighbour), non-finite points nobody's neighbour and themselves isolated,
the k smallest sorted, isolated <=> !(d2_k <= cap * cap), m = (((0.0 + sqrt(d2_1)) + ...) + sqrt(d2_k)) / k.  The statistics use
math.fsum (exact to the last rounding): the GPU side's torch sums are held to ``cloud_filter.threshold_bound`` of them."""
import math

import numpy as np

ROWS = 512                                 # rows of the distance matrix held at once


def _d2_rows(x: np.ndarray, a: int, b: int, finite: np.ndarray) -> np.ndarray:
    """fp64 [b - a, n]: squared distances from the points a .. b - 1 to all; +Inf to itself and to every non-finite point"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = x[a:b, None, 0] - x[None, :, 0]
        dy = x[a:b, None, 1] - x[None, :, 1]
        dz = x[a:b, None, 2] - x[None, :, 2]
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
    d2[:, ~finite] = np.inf
    d2[np.arange(b - a), np.arange(a, b)] = np.inf
    return d2


def knn_mean(pts: np.ndarray, k: int, cap: float):
    """(m float64 [n] (+Inf where isolated), isolated bool [n])"""
    x = np.asarray(pts, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    assert 1 <= k < n
    finite = np.isfinite(x).all(1)
    m = np.full((n,), np.inf)
    isolated = np.ones((n,), dtype=bool)
    cap2 = float(cap) * float(cap)
    for a in range(0, n, ROWS):
        b = min(a + ROWS, n)
        near = np.sort(_d2_rows(x, a, b, finite), axis=1)[:, :k]
        ok = (near[:, k - 1] <= cap2) & finite[a:b]
        s = np.zeros((b - a,))
        for t in range(k):
            s = s + np.sqrt(near[:, t])
        isolated[a:b] = ~ok
        m[a:b] = np.where(ok, s / float(k), np.inf)
    return m, isolated


def radius_count(pts: np.ndarray, r: float, limit: int) -> np.ndarray:
    """int32 [n] = min(number of other points with d2 <= r * r, limit); 0 for a non-finite point"""
    x = np.asarray(pts, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    finite = np.isfinite(x).all(1)
    out = np.zeros((n,), dtype=np.int32)
    r2 = float(r) * float(r)
    for a in range(0, n, ROWS):
        b = min(a + ROWS, n)
        c = (_d2_rows(x, a, b, finite) <= r2).sum(1)
        out[a:b] = np.where(finite[a:b], np.minimum(c, limit), 0)
    return out


def statistics(m: np.ndarray, isolated: np.ndarray, std_ratio: float):
    """(mu, sigma, t) over the non-isolated points with math.fsum; sigma = 0 for one point, NaN mu for none"""
    mm = [float(v) for v in m[~isolated]]
    n = len(mm)
    if n == 0:
        return float("nan"), 0.0, float("nan")
    mu = math.fsum(mm) / n
    sigma = math.sqrt(math.fsum((v - mu) ** 2 for v in mm) / (n - 1)) if n > 1 else 0.0
    return mu, sigma, mu + float(std_ratio) * sigma


def statistical_mask(pts: np.ndarray, k: int, std_ratio: float, cap: float):
    """(keep bool [n], m, isolated, t)"""
    m, isolated = knn_mean(pts, k, cap)
    _, _, t = statistics(m, isolated, std_ratio)
    return ~isolated & (m <= t), m, isolated, t


def default_cap(pts: np.ndarray) -> float:
    """0.02 x the diagonal of the 1 % .. 99 % quantile box (fusion.mesh_bounds(xyz, 0.01): sorted[k], sorted[n - 1 - k])"""
    p = np.asarray(pts, dtype=np.float32)
    s = np.sort(p[np.isfinite(p).all(1)], axis=0)
    n = s.shape[0]
    k = int(math.floor(0.01 * (n - 1)))
    lo, hi = [float(v) for v in s[k]], [float(v) for v in s[n - 1 - k]]
    return 0.02 * math.sqrt(sum((hi[a] - lo[a]) ** 2 for a in range(3)))


def make_cloud(seed: int, n_surface: int = 3600, n_floaters: int = 160, n_far: int = 6, n_duplicates: int = 30) -> np.ndarray:
    """the census input of the GPU tests: a wavy noisy surface over the unit square, floaters in the box around it, a few points
    far from everything (isolated at any sensible cap) and exact duplicates of surface points; float32 [n,3], shuffled"""
    g = np.random.default_rng(seed)
    u, v = g.random(n_surface), g.random(n_surface)
    surf = np.stack([u, v, 0.08 * np.sin(6.0 * u) * np.cos(5.0 * v) + g.normal(0.0, 0.002, n_surface)], 1)
    floaters = g.random((n_floaters, 3)) * [1.2, 1.2, 0.8] + [-0.1, -0.1, -0.4]
    far = g.random((n_far, 3)) * 0.5 + [3.0, -2.0, 2.0] + np.arange(n_far)[:, None] * 0.9
    dup = surf[g.integers(0, n_surface, n_duplicates)]
    pts = np.concatenate([surf, floaters, far, dup]).astype(np.float32)
    return pts[g.permutation(pts.shape[0])]


CENSUS = [(11, 20, 2.0, 0.15), (12, 8, 2.0, 0.15), (13, 4, 1.0, None)]         # (seed, k, std_ratio, cap; None = default_cap: about 10 surface points lie within it)
_CENSUS_CACHE = {}


def census(case):
    """the case's cloud and the restatement's answer, computed once and shared: dict(pts, k, std_ratio, cap, keep, m, isolated, t)"""
    if case not in _CENSUS_CACHE:
        seed, k, std_ratio, cap = case
        pts = make_cloud(seed)
        cap = default_cap(pts) if cap is None else cap
        keep, m, isolated, t = statistical_mask(pts, k, std_ratio, cap)
        for a in (pts, keep, m, isolated):
            a.setflags(write=False)
        _CENSUS_CACHE[case] = dict(pts=pts, k=k, std_ratio=std_ratio, cap=cap, keep=keep, m=m, isolated=isolated, t=t)
    return _CENSUS_CACHE[case]

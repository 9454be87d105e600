"""Outlier removal of a fused point cloud on the GPU (csrc/cloud_filter.hip): the statistical rule of Open3D's
``remove_statistical_outlier`` / PCL's ``StatisticalOutlierRemoval`` and the count rule of PCL's ``RadiusOutlierRemoval``, plus
the file side that applies a mask to a PLY without touching the kept records.

The searches run over the sorted uniform grid of ``cloud_grid`` (``sort_into_cells``, ``two_grid_plan``) with the cloud as its own
target set: all arithmetic is fp64 on the float32 coordinates, the squared distance ((dx*dx) + (dy*dy)) + (dz*dz), the distance
its IEEE sqrt.  A point is never its own neighbour; another point at the same place is.  A point with a non-finite coordinate is
nobody's neighbour and is itself isolated (statistical) or has count 0 (radius): it is always removed.

What is a choice here and not a measured optimum: k = 20 and std_ratio = 2.0 (Open3D's usual values), and the default search cap
of ``CAP_SHARE`` = 0.02 times the diagonal of the cloud's 1 % .. 99 % quantile box."""
from __future__ import annotations

import math
import os
import re
import time
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from .cloud_grid import finite_extent, floor_edge, grid_for, points, sort_into_cells, two_grid_plan
from .data_io import _PLY_TYPES

Tensor = torch.Tensor

MAX_K = 32                                 # csrc/cloud_filter.hip: kKnnMaxK
CAP_SHARE = 0.02                           # default cap = this share of the quantile box's diagonal
CAP_QUANTILE = 0.01                        # ... the box of fusion.mesh_bounds(xyz, 0.01)
TRIAL_CELLS = 128                          # default edge: the occupancy is measured on a grid of this many cells along the box
RADIUS_EDGE = 1.0 + 2.0 ** -19             # radius search: cells this much wider than r, so ring 2's bound reaches r (27 cells)
SETTLED, ISOLATED, RINGS_USED_UP = 0, 1, 2


def threshold_bound(n: int, t: float) -> float:
    """how far the threshold computed by ``statistical_outlier_mask`` (sums in torch fp64, reduction order unspecified) may lie
    from its exact value: 2 * (n + 8) * 2^-53 * |t|.  A sum of n non-negative fp64 terms in ANY order has relative error at most
    (n - 1) u / (1 - (n - 1) u), u = 2^-53; that bounds mu (plus one division) and the sum of squares (each term (m - mu)^2 adds
    three roundings and, to first order, nothing from mu's own error, because sum(m - mu) = 0); the square root halves the
    second.  (n + 8) u covers either, and the factor 2 the second-order terms for every n below 2^40."""
    return 2.0 * (n + 8) * 2.0 ** -53 * abs(t)


def default_edge(pts: Tensor, k: int, cap: float) -> float:
    """the cell edge ``knn_mean_distance`` uses when none is given: the edge at which an occupied cell holds about ``k`` points.
    The occupancy o = finite points / occupied cells is measured on a trial grid of edge e0 = longest side of the 1 % .. 99 %
    quantile box / 128; a fused cloud is a surface, so the occupancy grows with the square of the edge and
    edge = e0 * sqrt(k / o), held inside [what the cell key allows, cap].  Rings 0 and 1 then hold about 9 k points of a
    surface and the k-th neighbour lies about 0.56 edge away: most queries stop before ring 2."""
    from .fusion import mesh_bounds
    p, side = finite_extent(pts)
    if p.shape[0] == 0 or side == 0.0:
        return float(cap)
    b = mesh_bounds(p, CAP_QUANTILE)
    e0 = max(b[3 + a] - b[a] for a in range(3)) / TRIAL_CELLS
    e0 = floor_edge(e0 if e0 > 0.0 else side / TRIAL_CELLS, side)
    keys = ops.cloud_cell_keys(p, grid_for(p, e0, "knn_mean_distance"))
    occupancy = p.shape[0] / max(int(torch.unique(keys).numel()), 1)
    return floor_edge(min(e0 * math.sqrt(k / occupancy), float(cap)), side)


def knn_mean_distance(xyz: Tensor, k: int, cap: float, edge: Optional[float] = None, info: Optional[dict] = None) -> Tuple[Tensor, Tensor]:
    """(m float64 [n], isolated bool [n]) for a float32 [n,3] cloud on the GPU, n > k, 1 <= k <= 32: a point is isolated iff
    fewer than k OTHER points lie at d2 <= cap * cap; otherwise m is the mean distance to its k nearest other points, the
    square roots added in ascending order in fp64 (m is +Inf for an isolated point).  Two grids like ``capped_nn_distance``: the
    cloud is sorted into cells of ``edge`` (default: ``default_edge``) and searched ``FINE_RINGS`` rings far; the queries whose
    rings run out restart, with no state carried over, on the coarse grid of ``cloud_grid.two_grid_plan``, whose rings reach
    ``cap``.  The result does not depend on ``edge``.  ``info`` receives edge, coarse_edge, second_pass (queries), isolated,
    non_finite, seconds_sort, seconds_search."""
    pts = points("knn_mean_distance", xyz)
    n, dev = pts.shape[0], pts.device
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn_mean_distance: k must lie in 1 .. {MAX_K}, got {k}")
    if n <= k:
        raise ValueError(f"knn_mean_distance: a cloud of {n} points has no {k} other points per query (n must exceed k)")
    if not (cap > 0 and math.isfinite(cap)):
        raise ValueError(f"knn_mean_distance: cap must be positive and finite, got {cap}")
    if edge is not None and not (edge > 0 and math.isfinite(edge)):
        raise ValueError(f"knn_mean_distance: edge must be positive and finite, got {edge}")
    t0 = time.perf_counter()
    mean = torch.full((n,), float("inf"), device=dev, dtype=torch.float64)
    flag = torch.full((n,), ISOLATED, device=dev, dtype=torch.uint8)
    p, side = finite_extent(pts)
    stats = {"edge": None, "coarse_edge": None, "second_pass": 0, "isolated": n, "non_finite": n - int(p.shape[0]),
             "seconds_sort": 0.0, "seconds_search": 0.0}
    if p.shape[0]:
        fine = floor_edge(default_edge(pts, k, cap) if edge is None else float(edge), side)
        sc = sort_into_cells(pts, fine, "knn_mean_distance", extent=p)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        plan = two_grid_plan(cap, fine)
        ops.cloud_knn_mean(sc.xyz, sc.keys, sc.perm, sc.grid, k, cap, plan.fine_rings, mean, flag)
        stats["edge"] = fine
        if plan.coarse_edge is not None:
            todo = torch.nonzero(flag == RINGS_USED_UP).squeeze(1)
            stats["second_pass"] = int(todo.numel())
            if todo.numel():
                t2 = time.perf_counter()
                # plan.coarse_edge >= fine, which floor_edge has already raised to what the key allows: no second floor_edge
                sc2 = sort_into_cells(pts, plan.coarse_edge, "knn_mean_distance", extent=p)
                where = torch.empty_like(sc2.perm)
                where[sc2.perm] = torch.arange(n, device=dev, dtype=torch.int64)          # original index -> sorted position
                index = torch.sort(where[todo]).values.contiguous()                     # neighbouring lanes, neighbouring cells
                torch.cuda.synchronize(dev)
                t1 += time.perf_counter() - t2                                           # the second sort counts as sort time
                ops.cloud_knn_mean(sc2.xyz, sc2.keys, sc2.perm, sc2.grid, k, cap, plan.coarse_rings, mean, flag, index=index)
                stats["coarse_edge"] = plan.coarse_edge
        torch.cuda.synchronize(dev)
        stats["seconds_sort"] = t1 - t0
        stats["seconds_search"] = time.perf_counter() - t1
        if bool((flag == RINGS_USED_UP).any()):
            raise RuntimeError("knn_mean_distance: a query is unsettled after the coarse grid (state corrupted?)")
    isolated = flag != SETTLED
    stats["isolated"] = int(isolated.sum())
    if info is not None:
        info.update(stats)
    return mean, isolated


def default_cap(xyz: Tensor) -> float:
    """0.02 x the diagonal of ``fusion.mesh_bounds(xyz, 0.01)``: the quantile box, so that the floaters do not set their own
    scale.  0.02 is a choice, not a measured optimum."""
    from .fusion import mesh_bounds
    b = mesh_bounds(xyz, CAP_QUANTILE)
    diag = math.sqrt(sum((b[3 + a] - b[a]) ** 2 for a in range(3)))
    if not diag > 0.0:
        raise ValueError("statistical_outlier_mask: the cloud's quantile box is empty; give cap")
    return CAP_SHARE * diag


def statistical_outlier_mask(xyz: Tensor, k: int = 20, std_ratio: float = 2.0, cap: Optional[float] = None,
                             info: Optional[dict] = None) -> Tensor:
    """bool [n] keep mask: with m and isolated of ``knn_mean_distance(xyz, k, cap)`` and the n' non-isolated points,
    mu = sum(m) / n', sigma = sqrt(sum((m - mu)^2) / (n' - 1)) (0 for n' = 1), t = mu + std_ratio * sigma; a point is kept iff it
    is not isolated and m <= t.  The sums are torch fp64 sums on the GPU (their order is torch's; ``threshold_bound`` bounds what
    any order can do to t).  ``cap`` defaults to ``default_cap``.  k = 20 and std_ratio = 2.0 are Open3D's usual values, 0.02 a
    choice; none of the three is a measured optimum.  ``info`` receives what knn_mean_distance reports plus cap, mean, std,
    threshold, kept, removed."""
    if not (std_ratio >= 0 and math.isfinite(std_ratio)):
        raise ValueError(f"statistical_outlier_mask: std_ratio must be finite and >= 0, got {std_ratio}")
    cap = default_cap(points("statistical_outlier_mask", xyz)) if cap is None else float(cap)
    stats: Dict[str, object] = {}
    m, isolated = knn_mean_distance(xyz, k, cap, info=stats)
    ok = ~isolated
    mm = m[ok]
    n_ok = int(mm.numel())
    mu = float(mm.sum() / n_ok) if n_ok else float("nan")
    sigma = math.sqrt(float(((mm - mu) ** 2).sum() / (n_ok - 1))) if n_ok > 1 else 0.0
    t = mu + float(std_ratio) * sigma
    keep = ok & (m <= t)                                        # NaN threshold (no point left): nothing is kept
    kept = int(keep.sum())
    stats.update(cap=cap, mean=mu, std=sigma, threshold=t, kept=kept, removed=int(keep.numel()) - kept)
    if info is not None:
        info.update(stats)
    return keep


def radius_neighbour_count(xyz: Tensor, radius: float, limit: int, info: Optional[dict] = None) -> Tensor:
    """int32 [n] = min(number of OTHER points with d2 <= radius * radius, limit), on a grid whose cells are a hair wider than
    ``radius`` (27 cells per query; the walk leaves early once ``limit`` is reached)"""
    pts = points("radius_neighbour_count", xyz)
    if not (radius > 0 and math.isfinite(radius)):
        raise ValueError(f"radius_neighbour_count: radius must be positive and finite, got {radius}")
    if int(limit) < 1:
        raise ValueError(f"radius_neighbour_count: limit must be at least 1, got {limit}")
    n, dev = pts.shape[0], pts.device
    t0 = time.perf_counter()
    count = torch.zeros((n,), device=dev, dtype=torch.int32)
    p, side = finite_extent(pts)
    stats = {"edge": None, "non_finite": n - int(p.shape[0]), "seconds_sort": 0.0, "seconds_search": 0.0}
    if p.shape[0]:
        edge = floor_edge(radius * RADIUS_EDGE, side)
        sc = sort_into_cells(pts, edge, "radius_neighbour_count", extent=p)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        ops.cloud_radius_count(sc.xyz, sc.keys, sc.perm, sc.grid, radius, int(limit), count)
        torch.cuda.synchronize(dev)
        stats.update(edge=edge, seconds_sort=t1 - t0, seconds_search=time.perf_counter() - t1)
    if info is not None:
        info.update(stats)
    return count


def radius_outlier_mask(xyz: Tensor, radius: float, min_neighbours: int, info: Optional[dict] = None) -> Tensor:
    """bool [n] keep mask of PCL's RadiusOutlierRemoval: a point is kept iff at least ``min_neighbours`` other points lie at
    d2 <= radius * radius.  ``info`` receives edge, non_finite, the seconds, kept and removed."""
    if int(min_neighbours) < 1:
        raise ValueError(f"radius_outlier_mask: min_neighbours must be at least 1, got {min_neighbours}")
    stats: Dict[str, object] = {}
    keep = radius_neighbour_count(xyz, radius, int(min_neighbours), info=stats) >= int(min_neighbours)
    kept = int(keep.sum())
    stats.update(kept=kept, removed=int(keep.numel()) - kept)
    if info is not None:
        info.update(stats)
    return keep


def method_problem(method: Optional[str], k, std_ratio, max_dist, radius, min_neighbours) -> Optional[str]:
    """what is wrong with the options of a cleaning run, as one sentence about option NAMES (k, std_ratio, max_dist, radius,
    min_neighbours), or None: the drivers turn it into their own flags' error"""
    if method == "radius":
        if radius is None:
            return "radius is needed by the radius method"
        if not (radius > 0 and math.isfinite(radius)):
            return f"radius must be positive and finite, got {radius}"
        if min_neighbours is not None and min_neighbours < 1:
            return f"min_neighbours must be at least 1, got {min_neighbours}"
    if method == "statistical":
        if k is not None and not 1 <= k <= MAX_K:
            return f"k must lie in 1 .. {MAX_K}, got {k}"
        if std_ratio is not None and not (std_ratio >= 0 and math.isfinite(std_ratio)):
            return f"std_ratio must be finite and >= 0, got {std_ratio}"
        if max_dist is not None and not (max_dist > 0 and math.isfinite(max_dist)):
            return f"max_dist must be positive and finite, got {max_dist}"
    return None


def mask_function(method: str, k: Optional[int] = None, std_ratio: Optional[float] = None, max_dist: Optional[float] = None,
                  radius: Optional[float] = None, min_neighbours: Optional[int] = None, device="cuda",
                  info: Optional[dict] = None) -> Callable[[np.ndarray], np.ndarray]:
    """the ``mask_fn`` of ``clean_ply`` for a method and its options (None = the default: k 20, std_ratio 2.0, max_dist =
    ``default_cap``, min_neighbours 2): uploads the coordinates, runs the mask on ``device``, returns it as a numpy array"""
    problem = method_problem(method, k, std_ratio, max_dist, radius, min_neighbours)
    if method not in ("statistical", "radius") or problem:
        raise ValueError(problem or f"unknown method {method!r} (statistical or radius)")

    def fn(xyz: np.ndarray) -> np.ndarray:
        pts = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(device)
        if method == "radius":
            keep = radius_outlier_mask(pts, float(radius), 2 if min_neighbours is None else int(min_neighbours), info=info)
        else:
            keep = statistical_outlier_mask(pts, 20 if k is None else int(k), 2.0 if std_ratio is None else float(std_ratio),
                                            max_dist, info=info)
        return keep.cpu().numpy()

    return fn


def _read_vertex_records(filename: str):
    """(header lines, index of the vertex count line, record dtype, records) of a binary little-endian PLY whose only element
    with entries is the vertex element of scalar properties; the errors of ``read_ply_xyz`` plus those of a file it could read
    but a mask cannot be applied to (ascii, faces)"""
    def bad(why: str) -> ValueError:
        return ValueError(f"{filename}: {why}")

    with open(filename, "rb") as f:
        lines = [f.readline()]
        if lines[0].strip() != b"ply":
            raise bad("not a PLY file")
        fmt, elements, props, current, count_line = None, [], [], None, None
        while True:
            raw = f.readline()
            if not raw:
                raise bad("PLY header without end_header")
            lines.append(raw)
            words = raw.decode("ascii", "replace").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "end_header":
                break
            if words[0] == "format" and len(words) >= 2:
                fmt = words[1]
            elif words[0] == "element" and len(words) == 3:
                current = words[1]
                elements.append((current, int(words[2])))
                if current == "vertex" and count_line is None:
                    count_line = len(lines) - 1
            elif words[0] == "property" and current == "vertex":
                if words[1] == "list":
                    raise bad("list property inside the vertex element")
                if len(words) != 3 or words[1] not in _PLY_TYPES:
                    raise bad(f"unknown vertex property {' '.join(words[1:])!r}")
                props.append((words[2], _PLY_TYPES[words[1]]))
        if fmt != "binary_little_endian":
            raise bad(f"format {fmt!r} is not supported (clean_ply copies binary_little_endian records)")
        if not elements or elements[0][0] != "vertex":
            raise bad("the first element must be the vertices")
        if any(c for _, c in elements[1:]):
            raise bad("elements after the vertices (faces) would lose their vertices")
        n = elements[0][1]
        names = [p[0] for p in props]
        if len(set(names)) != len(names) or any(a not in names for a in "xyz"):
            raise bad(f"the vertex element needs x, y and z once each, has {names}")
        dtype = np.dtype([(name, "<" + t) for name, t in props])
        data = np.fromfile(f, dtype=dtype, count=n)
        if data.shape[0] != n:
            raise bad(f"{data.shape[0]} of {n} vertices: the file is short")
    return lines, count_line, dtype, data


def clean_ply(src: str, dst: str, mask_fn: Callable[[np.ndarray], object]) -> Dict[str, int]:
    """apply ``mask_fn(xyz float32 [n,3]) -> keep [n]`` (a bool array or tensor) to the vertices of the binary little-endian PLY
    ``src`` and write ``dst``: the same header with only the vertex count changed, then the kept records, byte for byte, in their
    original order (15-byte records, 27-byte records with normals, or any scalar vertex properties).  A file without vertices, or
    a mask that keeps nothing, gives a valid PLY of 0 vertices (``mask_fn`` is not called for an empty file).  -> {"vertices",
    "kept", "removed", "record_bytes"}"""
    lines, count_line, dtype, data = _read_vertex_records(src)
    n = int(data.shape[0])
    keep = np.zeros((0,), dtype=bool)
    if n:
        xyz = np.stack([data["x"].astype(np.float32), data["y"].astype(np.float32), data["z"].astype(np.float32)], 1)
        got = mask_fn(xyz)
        keep = np.asarray(got.cpu() if torch.is_tensor(got) else got)
        if keep.shape != (n,) or keep.dtype != np.bool_:
            raise ValueError(f"clean_ply: mask_fn must return a bool mask of {n} elements, got {keep.dtype} {keep.shape}")
    kept = int(keep.sum())
    lines = list(lines)
    lines[count_line] = re.sub(rb"\d+(\s*)$", lambda mo: str(kept).encode("ascii") + mo.group(1), lines[count_line], count=1)
    try:
        with open(dst, "wb") as f:
            f.write(b"".join(lines))
            f.write(data[keep].tobytes())
    except BaseException:
        if os.path.exists(dst):
            os.remove(dst)
        raise
    return {"vertices": n, "kept": kept, "removed": n - kept, "record_bytes": int(dtype.itemsize)}

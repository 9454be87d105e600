"""The DTU evaluation of a fused point cloud (evaluations/dtu/*.m of the reference: BaseEvalMain_web.m, PointCompareMain.m,
reducePts_haa.m, MaxDistCP.m, ComputeStat_web.m) with the searches on the GPU (csrc/cloud_eval.hip): accuracy = distance from
the reduced prediction to the ground truth inside the observability mask, completeness = distance from the ground truth above
the table plane to the reduced prediction, both in mm, outliers beyond 20 mm discarded.

All arithmetic is fp64 on the float32 coordinates of the PLY files, the squared distance ((dx*dx) + (dy*dy)) + (dz*dz), the
distance its IEEE sqrt.  Sorting by cell key (``cloud_grid.sort_into_cells``), compaction and the statistics are torch; the
fixed-radius search, the ring search and the mask lookup are HIP.  Differences from the MATLAB scripts: the visiting order of the
reduction is an explicit input (``randperm`` is not reproducible); a distance is capped at ``cap`` where MATLAB returns the
distance to the nearest point of the block enlarged by ``cap`` (every consumer discards >= 20); the one-ulp seams between
neighbouring blocks are not reproduced; non-finite points are never kept."""
from __future__ import annotations

import math
import os
import time
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .cloud_grid import points, sort_into_cells, two_grid_plan

Tensor = torch.Tensor

EDGE_SLACK = 1.0 + 2.0 ** -20              # the reduction's cells are this much wider than dst: the 27 cells hold the radius
USED_SETS = (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)     # BaseEvalMain_web.m:24


def _bb(bb) -> np.ndarray:
    b = np.asarray(bb.cpu() if torch.is_tensor(bb) else bb, dtype=np.float64)
    if b.shape != (2, 3) or not np.isfinite(b).all():
        raise ValueError(f"bb must be a finite [2,3] array (BB of ObsMask<N>_10.mat), got shape {b.shape}")
    return b


def inverse_permutation(order: Tensor, n: int) -> Tensor:
    """rank[order[i]] = i as int32 on ``order``'s device; raises unless ``order`` is a permutation of 0 .. n - 1"""
    if order.dtype not in (torch.int64, torch.int32) or order.dim() != 1 or order.numel() != n:
        raise ValueError(f"order must be a 1-D integer permutation of {n} elements, got {order.dtype} {tuple(order.shape)}")
    order = order.long()
    if n and (int(order.min()) < 0 or int(order.max()) >= n):
        raise ValueError("order holds an index outside 0 .. n - 1")
    rank = torch.full((n,), -1, device=order.device, dtype=torch.int32)
    rank[order] = torch.arange(n, device=order.device, dtype=torch.int32)
    if n and bool((rank < 0).any()):
        raise ValueError("order is not a permutation (an index occurs twice)")
    return rank


def default_order(n: int, seed: int = 0) -> Tensor:
    """the visiting order when none is given: torch.randperm on a CPU generator seeded with ``seed`` (the stand-in for
    reducePts_haa.m:9, whose randperm is not reproducible)"""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))


def reduce_points(pts: Tensor, dst: float = 0.2, order: Optional[Tensor] = None, seed: int = 0, rounds_per_sync: int = 4,
                  info: Optional[dict] = None) -> Tensor:
    """reducePts_haa.m: bool [n] keep mask such that no two kept points are within ``dst``: the points are visited in the order
    ``order`` (a permutation of 0 .. n - 1; default ``default_order(n, seed)``) and a point that is still kept removes every
    other point with d2 <= dst*dst.  For a given order the mask equals the sequential loop's exactly; it is computed by rounds
    of ``itermvs_cloud_reduce_round`` (``rounds_per_sync`` launches per read-back of the undecided count).  Non-finite points
    are never kept and remove nobody.  ``info`` receives rounds, non_finite, kept, and the seconds of sort and rounds."""
    pts = points("reduce_points", pts)
    n = pts.shape[0]
    if not (dst > 0 and math.isfinite(dst)):
        raise ValueError(f"reduce_points: dst must be positive, got {dst}")
    dev = pts.device
    keep = torch.zeros((n,), device=dev, dtype=torch.bool)
    order = default_order(n, seed) if order is None else order
    rank = inverse_permutation(order.to(dev), n)
    t0 = time.perf_counter()
    sc = sort_into_cells(pts, dst * EDGE_SLACK, "reduce_points")
    m = int(sc.perm.numel())
    stats = {"rounds": 0, "non_finite": n - m, "kept": 0, "seconds_sort": 0.0, "seconds_rounds": 0.0}
    if m:
        rank_sorted = rank[sc.perm].contiguous()
        state = torch.zeros((m,), device=dev, dtype=torch.int32)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        stats["seconds_sort"] = t1 - t0
        per = max(1, int(rounds_per_sync))
        while True:                                   # bounded: every round decides at least the earliest undecided point
            counts = torch.zeros((per,), device=dev, dtype=torch.int32)
            for r in range(per):
                ops.cloud_reduce_round(sc.xyz, sc.keys, rank_sorted, sc.grid, dst, state, counts[r:r + 1])
            left = counts.cpu().tolist()
            done_at = next((r for r, c in enumerate(left) if c == 0), None)
            stats["rounds"] += per if done_at is None else done_at + 1
            if done_at is not None:
                break
            if stats["rounds"] > m + per:
                raise RuntimeError("reduce_points: the rounds did not converge (state corrupted?)")
        stats["seconds_rounds"] = time.perf_counter() - t1
        keep[sc.perm] = state == 1
        stats["kept"] = int(keep.sum())
    if info is not None:
        info.update(stats)
    return keep


def covered_region(bb, cap: float) -> Tuple[np.ndarray, np.ndarray]:
    """MaxDistCP.m:5,10-18: the queries some block looks at are lo <= x < hi per axis; an empty region when a Range is negative"""
    b = _bb(bb)
    rng = np.floor((b[1] - b[0]) / cap)
    lo = b[0].copy()
    hi = (b[0] + rng * cap) + cap
    if (rng < 0).any():
        hi = lo.copy()
    return lo, hi


def capped_nn_distance(q_from: Tensor, q_to: Tensor, bb, cap: float = 60.0, cell: float = 1.0, info: Optional[dict] = None) -> Tensor:
    """MaxDistCP.m (Qto, Qfrom, BB, MaxDist): float64 [n_from] = min(distance to the nearest ``q_to`` point, cap) for every
    ``q_from`` point inside the region the script's blocks cover; ``cap`` for every other point and when no target lies within
    ``cap``.  Targets are sorted into a grid of ``cell``-wide cells and, for the queries that do not settle there, into a
    coarser one (``cloud_grid.two_grid_plan``); targets farther than ``cap`` from the region cannot matter and are dropped, like
    the script's enlarged blocks do."""
    q_from, q_to = points("capped_nn_distance", q_from), points("capped_nn_distance", q_to)
    if not (cap > 0 and cell > 0 and math.isfinite(cap) and math.isfinite(cell)):
        raise ValueError(f"capped_nn_distance: cap and cell must be positive, got {cap}, {cell}")
    lo, hi = covered_region(bb, cap)
    nq, dev = q_from.shape[0], q_from.device
    dist = torch.full((nq,), float(cap), device=dev, dtype=torch.float64)
    stats = {"targets": 0, "second_pass": 0, "seconds_sort": 0.0, "seconds_search": 0.0}
    t0 = time.perf_counter()
    # a target farther than cap from the region is at least cap from every covered query (1.001: room for the rounding of lo - cap)
    tlo = torch.tensor(lo - 1.001 * cap, device=dev, dtype=torch.float64)
    thi = torch.tensor(hi + 1.001 * cap, device=dev, dtype=torch.float64)
    near = ((q_to.double() >= tlo) & (q_to.double() <= thi)).all(1)             # NaN: false
    t = q_to[near]
    stats["targets"] = int(t.shape[0])
    if nq and t.shape[0] and bool((hi > lo).all()):
        best = torch.full((nq,), float("inf"), device=dev, dtype=torch.float64)
        done = torch.zeros((nq,), device=dev, dtype=torch.uint8)
        region = list(lo) + list(hi)
        plan = two_grid_plan(cap, cell)
        fine = sort_into_cells(t, cell, "capped_nn_distance", extent=t)              # t is finite: nothing is dropped or keyless
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        stats["seconds_sort"] = t1 - t0
        ops.cloud_nn_distance(q_from, fine.xyz, fine.keys, fine.grid, region, cap, plan.fine_rings, best, done, dist)
        if plan.coarse_edge is not None:
            todo = torch.nonzero(done == 0).squeeze(1)
            stats["second_pass"] = int(todo.numel())
            if todo.numel():                           # best / done carry the search over; the second sort counts as search time
                coarse = sort_into_cells(t, plan.coarse_edge, "capped_nn_distance", extent=t)
                ops.cloud_nn_distance(q_from, coarse.xyz, coarse.keys, coarse.grid, region, cap, plan.coarse_rings, best, done, dist,
                                      index=todo)
        torch.cuda.synchronize(dev)
        stats["seconds_search"] = time.perf_counter() - t1
    if info is not None:
        info.update(stats)
    return dist


def points_in_mask(pts: Tensor, obs_mask: Tensor, bb, res: float) -> Tensor:
    """PointCompareMain.m:32-41: bool [n] = the point's voxel round(((p - bb[0]) / res) + 1) (MATLAB's round: half away from
    zero) lies inside ``obs_mask`` (uint8 [sx,sy,sz], indexed [x-1, y-1, z-1]) and is set"""
    pts = points("points_in_mask", pts)
    b = _bb(bb)
    if not isinstance(obs_mask, torch.Tensor) or obs_mask.dim() != 3:
        raise RuntimeError("points_in_mask: obs_mask must be a [sx,sy,sz] tensor")
    mask = obs_mask.to(pts.device).ne(0).to(torch.uint8).contiguous()
    return ops.cloud_in_mask(pts, mask, b[0], float(res)).bool()


def above_plane(pts: Tensor, plane) -> Tensor:
    """PointCompareMain.m:53: ((P0*x + P1*y) + P2*z) + P3 > 0 in fp64 (torch arithmetic, any device)"""
    p = [float(v) for v in np.asarray(plane.cpu() if torch.is_tensor(plane) else plane, dtype=np.float64).reshape(-1)]
    if len(p) != 4:
        raise ValueError("plane must hold 4 coefficients (P of Plane<N>.mat)")
    x, y, z = pts[:, 0].double(), pts[:, 1].double(), pts[:, 2].double()
    return (((p[0] * x + p[1] * y) + p[2] * z) + p[3]) > 0


def compare_points(pred: Tensor, gt: Tensor, obs_mask: Tensor, bb, res: float, plane, dst: float = 0.2,
                   order: Optional[Tensor] = None, seed: int = 0, cap: float = 60.0, cell: float = 1.0) -> Dict[str, object]:
    """PointCompareMain.m: reduce the prediction to ``dst`` density, then Ddata (reduced prediction -> ground truth), Dstl
    (ground truth -> reduced prediction), DataInMask, StlAbovePlane; plus keep (the mask over ``pred``), Qdata, the reduced
    size, the downsample factor (reducePts_haa.m:35) and the seconds per stage."""
    red, nn1, nn2 = {}, {}, {}
    keep = reduce_points(pred, dst, order, seed, info=red)
    qdata = points("compare_points", pred)[keep].contiguous()
    gt = points("compare_points", gt)
    ddata = capped_nn_distance(qdata, gt, bb, cap, cell, info=nn1)               # MaxDistCP(Qstl, Qdata, BB, MaxDist)
    dstl = capped_nn_distance(gt, qdata, bb, cap, cell, info=nn2)                # MaxDistCP(Qdata, Qstl, BB, MaxDist)
    t0 = time.perf_counter()
    in_mask = points_in_mask(qdata, obs_mask, bb, res)
    above = above_plane(gt, plane)
    torch.cuda.synchronize(pred.device)
    n_red = int(qdata.shape[0])
    return {"Ddata": ddata, "Dstl": dstl, "DataInMask": in_mask, "StlAbovePlane": above, "keep": keep, "Qdata": qdata,
            "n_pred": int(pred.shape[0]), "n_reduced": n_red, "downsample_factor": (pred.shape[0] / n_red) if n_red else float("nan"),
            "rounds": red["rounds"], "non_finite": red["non_finite"],
            "seconds": {"reduce_sort": red["seconds_sort"], "reduce_rounds": red["seconds_rounds"],
                        "data_to_stl": nn1["seconds_sort"] + nn1["seconds_search"],
                        "stl_to_data": nn2["seconds_sort"] + nn2["seconds_search"], "mask_plane": time.perf_counter() - t0}}


def matlab_median(x: Tensor) -> float:
    """median as MATLAB takes it: the mean of the two middle values of an even count (torch.median returns the lower one);
    NaN for an empty selection"""
    n = x.numel()
    if n == 0:
        return float("nan")
    s = torch.sort(x.double()).values
    return float(s[n // 2]) if n % 2 else float((s[n // 2 - 1] + s[n // 2]) / 2)


def _mean_var(x: Tensor) -> Tuple[float, float]:
    n = x.numel()
    if n == 0:
        return float("nan"), float("nan")
    x = x.double()
    mean = x.sum() / n
    var = ((x - mean) ** 2).sum() / (n - 1) if n > 1 else torch.zeros(())         # MATLAB: var of one value is 0
    return float(mean), float(var)


def scan_statistics(ddata: Tensor, dstl: Tensor, data_in_mask: Tensor, stl_above_plane: Tensor, max_dist: float = 20.0) -> Dict[str, float]:
    """ComputeStat_web.m:52-68 / BaseEvalMain_web.m:63-76: the mask (or plane) first, then ``< max_dist``; count, mean, median
    and variance (n - 1) of both directions.  Torch arithmetic on any device; an empty selection gives NaN."""
    d = ddata[data_in_mask.bool()]
    d = d[d < max_dist]
    s = dstl[stl_above_plane.bool()]
    s = s[s < max_dist]
    (md, vd), (ms, vs) = _mean_var(d), _mean_var(s)
    return {"nData": int(d.numel()), "nStl": int(s.numel()), "MeanData": md, "MedData": matlab_median(d), "VarData": vd,
            "MeanStl": ms, "MedStl": matlab_median(s), "VarStl": vs}


def summary(per_scan: Sequence[Dict[str, float]]) -> Dict[str, float]:
    """BaseEvalMain_web.m:99-100: the mean over scans of the per-scan means; overall = (acc + comp) / 2"""
    if not per_scan:
        return {"acc": float("nan"), "comp": float("nan"), "overall": float("nan")}
    acc = float(np.mean([s["MeanData"] for s in per_scan]))
    comp = float(np.mean([s["MeanStl"] for s in per_scan]))
    return {"acc": acc, "comp": comp, "overall": (acc + comp) / 2}


def _load_keys(path: str, keys: Sequence[str]) -> Dict[str, np.ndarray]:
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in keys if k not in z.files]
            if missing:
                raise ValueError(f"{path}: no {missing} among {z.files}")
            return {k: z[k] for k in keys}
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError(f"{path}: reading a .mat file needs scipy (scipy.io.loadmat); without scipy convert the file to an "
                          f".npz with the keys {list(keys)}") from e
    m = loadmat(path)
    missing = [k for k in keys if k not in m]
    if missing:
        raise ValueError(f"{path}: no {missing} in the file")
    return {k: np.asarray(m[k]) for k in keys}


def load_obs_mask(path: str) -> Tuple[Tensor, np.ndarray, float]:
    """``ObsMask<N>_10.mat`` (or an .npz with the same keys) -> (ObsMask uint8 [sx,sy,sz] CPU tensor, BB float64 [2,3], Res)"""
    d = _load_keys(path, ("ObsMask", "BB", "Res"))
    mask = np.ascontiguousarray(d["ObsMask"] != 0).astype(np.uint8)
    if mask.ndim != 3:
        raise ValueError(f"{path}: ObsMask must have three axes, got {mask.shape}")
    bb = np.asarray(d["BB"], dtype=np.float64).reshape(2, 3)
    return torch.from_numpy(mask), bb, float(np.asarray(d["Res"], dtype=np.float64).reshape(-1)[0])


def load_plane(path: str) -> np.ndarray:
    """``Plane<N>.mat`` (or .npz) -> P float64 [4]"""
    p = np.asarray(_load_keys(path, ("P",))["P"], dtype=np.float64).reshape(-1)
    if p.size != 4:
        raise ValueError(f"{path}: P must hold 4 coefficients, got {p.size}")
    return p


def resolve_file(folder: str, stem: str) -> str:
    """``<stem>.mat`` or ``<stem>.npz`` under ``folder`` (the .mat first, like the scripts)"""
    for ext in (".mat", ".npz"):
        if os.path.isfile(os.path.join(folder, stem + ext)):
            return os.path.join(folder, stem + ext)
    raise FileNotFoundError(os.path.join(folder, stem + ".mat") + " (or .npz)")


def prediction_path(ply_path: str, scan: int, method: str = "itermvs", light: str = "l3") -> str:
    """BaseEvalMain_web.m:34: ``<method><scan:03d>_<light>.ply``; falling back to this project's ``scan<N>.ply``"""
    first = os.path.join(ply_path, "{}{:03d}_{}.ply".format(method.lower(), scan, light))
    for cand in (first, os.path.join(ply_path, "scan{}.ply".format(scan))):
        if os.path.isfile(cand):
            return cand
    raise FileNotFoundError(f"{first} (or scan{scan}.ply)")


def evaluate_scan(data_path: str, ply_path: str, scan: int, method: str = "itermvs", light: str = "l3", dst: float = 0.2,
                  max_dist: float = 20.0, seed: int = 0, device: str = "cuda") -> Dict[str, object]:
    """BaseEvalMain_web.m:30-76 for one scan: read the prediction, the ground truth ``Points/stl/stl<scan:03d>_total.ply``,
    ``ObsMask/ObsMask<scan>_10`` and ``ObsMask/Plane<scan>``; compare; filter -> every field of scan_statistics plus the
    sizes, the file, the seconds per stage"""
    from .data_io import read_ply_xyz
    t0 = time.perf_counter()
    pred_file = prediction_path(ply_path, scan, method, light)
    pred = torch.from_numpy(read_ply_xyz(pred_file)).to(device)
    gt = torch.from_numpy(read_ply_xyz(os.path.join(data_path, "Points", "stl", "stl{:03d}_total.ply".format(scan)))).to(device)
    mask, bb, res = load_obs_mask(resolve_file(os.path.join(data_path, "ObsMask"), "ObsMask{}_10".format(scan)))
    plane = load_plane(resolve_file(os.path.join(data_path, "ObsMask"), "Plane{}".format(scan)))
    t1 = time.perf_counter()
    cmp_ = compare_points(pred, gt, mask.to(device), bb, res, plane, dst=dst, seed=seed)
    stat = scan_statistics(cmp_["Ddata"], cmp_["Dstl"], cmp_["DataInMask"], cmp_["StlAbovePlane"], max_dist)
    seconds = dict(cmp_["seconds"], read=t1 - t0, total=time.perf_counter() - t0)
    return dict(stat, scan=int(scan), file=pred_file, n_pred=cmp_["n_pred"], n_reduced=cmp_["n_reduced"], n_stl=int(gt.shape[0]),
                downsample_factor=cmp_["downsample_factor"], rounds=cmp_["rounds"], non_finite=cmp_["non_finite"], seconds=seconds)

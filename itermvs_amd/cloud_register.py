"""The Tanks and Temples evaluation of a fused point cloud -- precision, recall and F-score against the laser scan of a
training scene -- with every pass over points on the GPU (csrc/cloud_register.hip, csrc/cloud_eval.hip).  It follows the order of
the benchmark's scoring script (align, crop to the scene's polygon volume, voxel-downsample, three rounds of ICP with scale,
nearest-neighbour distances in both directions, counts below tau) without Open3D.

All geometry is fp64 on the float32 coordinates of the PLY files.  Sorting by cell key (``cloud_grid.sort_into_cells``, for the
voxels and for the ICP targets alike), prefix sums, compaction and the transform of a kept cloud are torch plumbing; the crop, the voxel mean, the nearest-neighbour index, the sums of the similarity
fit and the capped distances are HIP.  The 3x3 SVD runs in numpy on the host, from 18 doubles read back per ICP iteration.

Differences from the Open3D script: voxel means come out in ascending voxel-key order (Open3D: a hash
map's order); a tie between two targets goes to the lowest index; a correspondence needs d < max_dist (exclusive); distances
are capped at plot_stretch * tau (nothing beyond is ever counted); each ICP round runs from identity on the transformed, cropped
and down-sampled source; the trajectory alignment is a plain Umeyama fit of the camera centres (no noise-perturbed RANSAC, no
mapping file for differing camera counts); normals are not estimated.  Agreement with the official toolbox on real scenes is
unverified."""
from __future__ import annotations

import json
import math
import os
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import cloud_eval, ops
from .cloud_grid import max_ring, points, sort_into_cells
from .ops import CloudGrid

Tensor = torch.Tensor

# tau per training scene.  Written from memory of the official toolbox, which was not available when this was written:
# check them against the benchmark's own table before quoting a score (``--tau`` overrides).
SCENE_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}
PLOT_STRETCH = 5
CURVE_BINS = 500
UNIFORM_LIMIT = 16e6                       # round 3 strides a source larger than this
GRID_FRACTION = 8.0                        # cells of the ICP search grid: max_dist / 8, at least the voxel


class SelectionVolume(NamedTuple):
    """Open3D's SelectionPolygonVolume"""
    axis: int                              # 0, 1, 2 = X, Y, Z
    axis_min: float
    axis_max: float
    polygon: np.ndarray                    # float64 [n,3]


class TargetGrid(NamedTuple):
    """a target cloud prepared for nearest-neighbour index searches"""
    target: Tensor                         # float32 [nt,3], the caller's order
    sorted: Tensor                         # float32 [nt,3] in key order
    keys: Tensor                           # int64 [nt]
    perm: Tensor                           # int64 [nt]: sorted position -> index into target
    grid: CloudGrid


def read_selection_volume(json_path: str) -> SelectionVolume:
    """Open3D's ``SelectionPolygonVolume`` JSON (``<Scene>.json``): axis_max, axis_min, bounding_polygon, orthogonal_axis"""
    with open(json_path) as f:
        d = json.load(f)
    missing = [k for k in ("axis_max", "axis_min", "bounding_polygon", "orthogonal_axis") if k not in d]
    if missing:
        raise ValueError(f"{json_path}: no {missing} in the file")
    axis = str(d["orthogonal_axis"]).strip().upper()
    if axis not in ("X", "Y", "Z"):
        raise ValueError(f"{json_path}: orthogonal_axis must be X, Y or Z, got {d['orthogonal_axis']!r}")
    poly = np.asarray(d["bounding_polygon"], dtype=np.float64)
    if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= poly.shape[0] <= 1024:
        raise ValueError(f"{json_path}: bounding_polygon must hold 3 .. 1024 vertices of 3 coordinates, got shape {poly.shape}")
    return SelectionVolume("XYZ".index(axis), float(d["axis_min"]), float(d["axis_max"]), poly)


def read_trajectory_log(path: str) -> np.ndarray:
    """a ``.log`` trajectory: records of one metadata line and four matrix lines (camera-to-world) -> float64 [N,4,4]"""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if len(lines) % 5:
        raise ValueError(f"{path}: {len(lines)} non-empty lines are not records of 1 + 4 lines")
    out = np.empty((len(lines) // 5, 4, 4), dtype=np.float64)
    for r in range(out.shape[0]):
        rows = [ln.split() for ln in lines[r * 5 + 1:r * 5 + 5]]
        if any(len(row) != 4 for row in rows):
            raise ValueError(f"{path}: record {r} has a matrix line without 4 numbers")
        out[r] = np.array(rows, dtype=np.float64)
    return out


def crop(pts: Tensor, volume: SelectionVolume, T=None) -> Tensor:
    """bool [n]: T * p (T = identity when None) lies inside ``volume``; a non-finite point is outside"""
    pts = points("crop", pts)
    if pts.shape[0] == 0:
        return torch.zeros((0,), device=pts.device, dtype=torch.bool)
    return ops.cloud_crop(pts, np.eye(4) if T is None else T, volume.axis, volume.axis_min, volume.axis_max, volume.polygon).bool()


def transform_points(pts: Tensor, T) -> Tensor:
    """float32 [n,3] = T * p per row as ((m0*x + m1*y) + m2*z) + m3 in fp64, rounded once (torch arithmetic)"""
    m = np.asarray(T, dtype=np.float64)
    x, y, z = pts[:, 0].double(), pts[:, 1].double(), pts[:, 2].double()
    return torch.stack([((float(m[r, 0]) * x + float(m[r, 1]) * y) + float(m[r, 2]) * z) + float(m[r, 3]) for r in range(3)], 1).float()


def voxel_down_sample(pts: Tensor, voxel: float) -> Tensor:
    """Open3D's ``voxel_down_sample``: float32 [m,3], one point per occupied voxel floor((p - origin) / voxel) with
    origin = min_bound - voxel / 2: the mean of the voxel's points (fp64 sum in index order, one rounding).  Output order:
    ascending voxel key (x-major), not Open3D's hash-map order.  Non-finite points are dropped.  The prefix sum of the segment
    heads is torch.cumsum (plumbing); keys, heads and means are HIP."""
    pts = points("voxel_down_sample", pts)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"voxel_down_sample: voxel must be positive, got {voxel}")
    sc = sort_into_cells(pts, voxel, "voxel_down_sample", pad=voxel / 2, stable=True)       # stable: the sums run in index order
    if sc.xyz.shape[0] == 0:
        return sc.xyz
    head = ops.cloud_voxel_heads(sc.keys)
    rank = torch.cumsum(head, 0, dtype=torch.int64) - 1
    n_out = int(rank[-1]) + 1
    if n_out < 1:
        return sc.xyz[:0]
    return ops.cloud_voxel_mean(sc.xyz, sc.keys, rank, n_out)


def uniform_down_sample(pts: Tensor, every_k: int) -> Tensor:
    """Open3D's ``uniform_down_sample``: every ``every_k``-th point, starting with the first"""
    if every_k < 1:
        raise ValueError(f"uniform_down_sample: every_k must be >= 1, got {every_k}")
    return pts[::int(every_k)].contiguous()


def umeyama(sums, with_scale: bool = True) -> np.ndarray:
    """the similarity transform (float64 [4,4]) that maps p onto t in the least-squares sense, from the 18 sums of
    ``ops.cloud_umeyama_sums`` {count, sum p, sum t, sum t p^T, sum |p|^2, sum d2} (Umeyama 1991, as Eigen::umeyama):
    cov = sum t p^T / N - mu_t mu_p^T = U D V^T, S = diag(1, 1, det(U) det(V)), R = U S V^T, scale = tr(D S) / var_p,
    translation = mu_t - scale * R mu_p.  numpy fp64 on the host."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1)
    if s.size != 18 or not s[0] >= 1:
        raise ValueError("umeyama: needs the 18 sums of at least one correspondence")
    n = s[0]
    mu_p, mu_t = s[1:4] / n, s[4:7] / n
    cov = s[7:16].reshape(3, 3) / n - np.outer(mu_t, mu_p)
    var_p = s[16] / n - float(mu_p @ mu_p)
    u, d, vt = np.linalg.svd(cov)
    sgn = np.array([1.0, 1.0, 1.0 if np.linalg.det(u) * np.linalg.det(vt) >= 0 else -1.0])
    rot = (u * sgn) @ vt
    scale = float((d * sgn).sum() / var_p) if with_scale else 1.0
    out = np.eye(4)
    out[:3, :3] = scale * rot
    out[:3, 3] = mu_t - scale * (rot @ mu_p)
    return out


def build_target_grid(target: Tensor, edge: float) -> TargetGrid:
    """sort the finite points of float32 [nt,3] ``target`` into cells of ``edge`` for ``icp``"""
    target = points("build_target_grid", target)
    sc = sort_into_cells(target, edge, "build_target_grid")
    return TargetGrid(target, sc.xyz, sc.keys, sc.perm, sc.grid)


def icp(source: Tensor, target_grid: TargetGrid, init=None, max_dist: float = 1.0, max_iter: int = 20, rel_fitness: float = 1e-6,
        rel_rmse: float = 1e-6, info: Optional[dict] = None) -> Tuple[np.ndarray, float, float, int]:
    """point-to-point ICP with scale (Open3D's registration_icp with TransformationEstimationPointToPoint(True)).  Every
    iteration: nearest target of T * q within ``max_dist`` (HIP), the 18 sums (HIP), one read-back of 18 doubles, fitness =
    matches / n, rmse = sqrt(sum d2 / matches); stop when both changed by less than their thresholds since the previous
    evaluation, after ``max_iter`` updates, or with fewer than 3 matches; else T <- umeyama(sums) @ T.  Returns (T, fitness,
    rmse, updates applied); fitness and rmse belong to the returned T."""
    source = points("icp", source)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    n = source.shape[0]
    if n == 0:
        return T, 0.0, 0.0, 0
    tg = target_grid
    rings = max_ring(max_dist, tg.grid.edge)
    prev, it, trace = None, 0, []
    while True:
        idx, d2 = ops.cloud_nn_index(source, T, tg.sorted, tg.keys, tg.perm, tg.grid, max_dist, rings)
        s = ops.cloud_umeyama_sums(source, T, idx, d2, tg.target).cpu().numpy()
        m = s[0]
        fitness, rmse = float(m / n), (float(math.sqrt(s[17] / m)) if m > 0 else 0.0)
        trace.append((fitness, rmse))
        if prev is not None and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            break
        if it >= max_iter or m < 3:
            break
        T = umeyama(s, True) @ T
        prev, it = (fitness, rmse), it + 1
    if info is not None:
        info.update(trace=trace)
    return T, fitness, rmse, it


def trajectory_alignment(user_log: Optional[np.ndarray], ref_log: np.ndarray, gt_trans: np.ndarray) -> np.ndarray:
    """the initial transform from the user's frame to the ground truth's: gt_trans @ (Umeyama fit with scale of the user's camera
    centres onto the reference log's).  Both logs are float64 [N,4,4] camera-to-world with the same N (no mapping file, no
    RANSAC).  ``user_log`` None: the cloud was built from the provided COLMAP cameras and the transform is ``gt_trans``."""
    gt_trans = np.asarray(gt_trans, dtype=np.float64).reshape(4, 4)
    if user_log is None:
        return gt_trans.copy()
    a, b = np.asarray(user_log, dtype=np.float64)[:, :3, 3], np.asarray(ref_log, dtype=np.float64)[:, :3, 3]
    if a.shape != b.shape or a.shape[0] < 3:
        raise ValueError(f"trajectory_alignment: the logs hold {a.shape[0]} and {b.shape[0]} cameras; equal counts >= 3 are required")
    s = np.zeros(18)
    s[0], s[1:4], s[4:7] = a.shape[0], a.sum(0), b.sum(0)
    s[7:16] = (b[:, :, None] * a[:, None, :]).sum(0).reshape(-1)
    s[16] = (a * a).sum()
    return gt_trans @ umeyama(s, True)


def _prepare(pts: Tensor, volume: SelectionVolume, T, voxel: Optional[float]) -> Tensor:
    """T * p for the points whose image lies in the volume, then the voxel down-sampling or, with ``voxel`` None, the uniform one
    at the stride of the cropped cloud's own size (registration_unif)"""
    kept = pts[crop(pts, volume, T)]
    if T is not None:
        kept = transform_points(kept, T)
    kept = kept.contiguous()
    return voxel_down_sample(kept, voxel) if voxel is not None else uniform_down_sample(kept, uniform_stride(kept.shape[0]))


def _register(pred: Tensor, gt: Tensor, T: np.ndarray, volume: SelectionVolume, voxel: Optional[float], max_dist: float,
              max_iter: int) -> Tuple[np.ndarray, dict]:
    s, t = _prepare(pred, volume, T, voxel), _prepare(gt, volume, None, voxel)
    edge = max(max_dist / GRID_FRACTION, voxel if voxel is not None else 0.0)
    step, fitness, rmse, it = icp(s, build_target_grid(t, edge), None, max_dist, max_iter)
    return step @ T, {"n_source": int(s.shape[0]), "n_target": int(t.shape[0]), "fitness": fitness, "rmse": rmse, "iterations": it}


def uniform_stride(n: int) -> int:
    """registration_unif: round(n / 16e6) when the cropped cloud holds more than 16e6 points, else 1; each cloud gets its own"""
    return max(int(round(n / UNIFORM_LIMIT)), 1) if n > UNIFORM_LIMIT else 1


def cumulative_curve(dist: Tensor, cap: float) -> Tensor:
    """float64 [500]: the fraction of distances below edge k + 1, edges = cap * (k / 500)"""
    edges = cap * (torch.arange(1, CURVE_BINS + 1, dtype=torch.float64) / CURVE_BINS)
    n = dist.numel()
    if n == 0:
        return torch.zeros((CURVE_BINS,), dtype=torch.float64)
    below = torch.searchsorted(torch.sort(dist).values, edges.to(dist.device), right=False)      # the number of d < edge
    return below.double().cpu() / n


def evaluate_scene(pred: Tensor, gt: Tensor, volume: SelectionVolume, init: np.ndarray, tau: float, refine: bool = True,
                   plot_stretch: int = PLOT_STRETCH) -> Dict[str, object]:
    """the scoring script's ``run_evaluation`` for one scene: three refinement rounds (voxel tau / max_dist 80 tau, tau / 2 /
    20 tau, uniform (each cropped cloud strided by its own size) / 2 tau; 20 iterations each; skipped when ``refine`` is
    False), then crop both clouds, voxel-downsample both
    at tau / 2, distances in both directions capped at plot_stretch * tau, precision = #(d_pred->gt < tau) / n_pred, recall =
    #(d_gt->pred < tau) / n_gt, F = 2PR / (P + R) (0 when both are 0) and both cumulative curves on 500 bins."""
    pred, gt = points("evaluate_scene", pred), points("evaluate_scene", gt)
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"evaluate_scene: tau must be positive, got {tau}")
    T = np.array(init, dtype=np.float64).reshape(4, 4)
    rounds = []
    if refine:
        for voxel, max_dist in ((tau, 80 * tau), (tau / 2, 20 * tau)):
            T, r = _register(pred, gt, T, volume, voxel, max_dist, 20)
            rounds.append(r)
        T, r = _register(pred, gt, T, volume, None, 2 * tau, 20)
        rounds.append(r)
    s, t = _prepare(pred, volume, T, tau / 2), _prepare(gt, volume, None, tau / 2)
    cap = plot_stretch * tau
    n_s, n_t = int(s.shape[0]), int(t.shape[0])
    if n_s and n_t:
        both = torch.cat([s, t])
        bb = np.stack([both.min(0).values.double().cpu().numpy() - cap, both.max(0).values.double().cpu().numpy() + cap])
        d_s = cloud_eval.capped_nn_distance(s, t, bb, cap, cap / 2)
        d_t = cloud_eval.capped_nn_distance(t, s, bb, cap, cap / 2)
    else:
        d_s = torch.full((n_s,), cap, device=pred.device, dtype=torch.float64)
        d_t = torch.full((n_t,), cap, device=pred.device, dtype=torch.float64)
    precision = float((d_s < tau).sum()) / n_s if n_s else 0.0
    recall = float((d_t < tau).sum()) / n_t if n_t else 0.0
    f = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return {"precision": precision, "recall": recall, "fscore": f, "tau": float(tau), "n_pred": n_s, "n_gt": n_t,
            "n_pred_below": int((d_s < tau).sum()), "n_gt_below": int((d_t < tau).sum()), "transform": T.tolist(),
            "rounds": rounds, "curve_pred": cumulative_curve(d_s, cap).tolist(), "curve_gt": cumulative_curve(d_t, cap).tolist()}


def scene_files(gt_dir: str, scene: str) -> Dict[str, str]:
    """``<Scene>.ply``, ``<Scene>.json``, ``<Scene>_trans.txt`` and ``<Scene>_COLMAP_SfM.log`` under ``gt_dir``"""
    files = {"ply": scene + ".ply", "json": scene + ".json", "trans": scene + "_trans.txt", "log": scene + "_COLMAP_SfM.log"}
    out = {k: os.path.join(gt_dir, v) for k, v in files.items()}
    for k, v in out.items():
        if not os.path.isfile(v):
            raise FileNotFoundError(v)
    return out


def evaluate_scene_files(gt_dir: str, ply_path: str, scene: str, traj_path: Optional[str] = None, tau: Optional[float] = None,
                         refine: bool = True, device: str = "cuda") -> Dict[str, object]:
    """read one scene's files and the cloud (``ply_path``: the file, or a folder holding ``<Scene>.ply``) and score it"""
    from .data_io import read_ply_xyz
    files = scene_files(gt_dir, scene)
    if tau is None:
        if scene not in SCENE_TAU:
            raise ValueError(f"no tau known for scene {scene!r}: pass --tau (known: {sorted(SCENE_TAU)})")
        tau = SCENE_TAU[scene]
    cloud = ply_path if os.path.isfile(ply_path) else os.path.join(ply_path, scene + ".ply")
    pred = torch.from_numpy(read_ply_xyz(cloud)).to(device)
    gt = torch.from_numpy(read_ply_xyz(files["ply"])).to(device)
    gt_trans = np.loadtxt(files["trans"], dtype=np.float64).reshape(4, 4)
    user = read_trajectory_log(traj_path) if traj_path else None
    init = trajectory_alignment(user, read_trajectory_log(files["log"]), gt_trans)
    res = evaluate_scene(pred, gt, read_selection_volume(files["json"]), init, float(tau), refine)
    return dict(res, scene=scene, file=cloud, n_pred_raw=int(pred.shape[0]), n_gt_raw=int(gt.shape[0]))

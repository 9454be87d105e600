"""The host side of the sorted uniform grid of the cloud searches: the counterpart of csrc/cloud_grid.hpp, shared by
``cloud_eval`` (DTU), ``cloud_register`` (Tanks and Temples) and ``cloud_filter`` (outlier removal).

A cloud is boxed, its points get the key of their cell (``ops.cloud_cell_keys``), and the cloud is sorted by key
(``sort_into_cells``); the kernels then walk rings of cells around a query.  ``max_ring`` says how many rings reach a distance
and ``two_grid_plan`` how a search with a large cap splits into a fine grid and a coarse one.  Sorting, gathering and the box are
torch plumbing; the keys are HIP."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import ops
from .ops import CloudGrid

Tensor = torch.Tensor

MAX_CELL_DIM = 1 << 21                     # csrc/cloud_grid.hpp: kMaxCellDim
RING_SHRINK = 1.0 - 2.0 ** -20             # csrc/cloud_grid.hpp: kRingShrink
FINE_RINGS = 4                             # rings of the fine grid before the unsettled queries move to the coarse one
COARSE_SHARE = 8.0                         # coarse edge = cap / 8 (or the fine edge if that is larger)


class SortedCloud(NamedTuple):
    """a cloud in key order on ``grid``"""
    xyz: Tensor                            # float32 [m,3] in key order
    keys: Tensor                           # int64 [m], ascending
    perm: Tensor                           # int64 [m]: sorted position -> row of the tensor that was sorted
    grid: CloudGrid


class TwoGridPlan(NamedTuple):
    fine_rings: int                        # rings to search on the fine grid
    coarse_edge: Optional[float]           # None: the fine grid's rings reach the cap
    coarse_rings: int


def points(what: str, pts: Tensor) -> Tensor:
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
        raise RuntimeError(f"{what}: expected a CUDA/ROCm tensor - the IterMVS HIP engine has no CPU path")
    if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError(f"{what}: points must be float32 [n,3], got {pts.dtype} {tuple(pts.shape)}")
    return pts.contiguous()


def grid_for(pts: Tensor, edge: float, what: str, pad: float = 0.0) -> CloudGrid:
    """the grid of cells of edge ``edge`` over the extent of finite float32 [n,3] points, its origin ``pad`` below their minimum
    (one synchronisation: the extent comes to the host); an extent of more than 2^21 cells on an axis raises"""
    lo, hi = pts.min(0).values.double().cpu(), pts.max(0).values.double().cpu()
    origin = [float(lo[a]) - pad for a in range(3)]
    dims = [int(math.floor((float(hi[a]) - origin[a]) / edge)) + 1 for a in range(3)]
    if max(dims) > MAX_CELL_DIM:
        raise ValueError(f"{what}: the cloud spans {dims} cells of edge {edge}; at most {MAX_CELL_DIM} per axis fit the cell key "
                         "(remove the far outliers, or work in the dataset's units)")
    return CloudGrid(tuple(origin), tuple(dims), float(edge))


def max_ring(cap: float, edge: float) -> int:
    """the first ring r whose lower bound (r - 1) * edge * RING_SHRINK reaches ``cap``: rings 0 .. r - 1 finish every search"""
    r = int(math.ceil(cap / (edge * RING_SHRINK))) + 1
    while (r - 1) * edge * RING_SHRINK < cap:
        r += 1
    return r


def floor_edge(edge: float, side: float) -> float:
    """``edge``, or the smallest edge whose grid over a box of longest side ``side`` still fits the cell key"""
    return max(float(edge), side / float(MAX_CELL_DIM // 2))


def finite_extent(pts: Tensor) -> Tuple[Tensor, float]:
    """the finite points (the cloud itself when all are) and the longest side of their bounding box"""
    finite = torch.isfinite(pts).all(1)
    p = pts if bool(finite.all()) else pts[finite]
    side = float((p.max(0).values.double() - p.min(0).values.double()).max()) if p.shape[0] else 0.0
    return p, side


def sort_into_cells(pts: Tensor, edge: float, what: str, extent: Optional[Tensor] = None, pad: float = 0.0,
                    stable: bool = False) -> SortedCloud:
    """float32 [n,3] ``pts`` in key order on a grid of cells of ``edge``; ``perm`` maps a sorted position to a row of ``pts``.
    Without ``extent`` the non-finite rows are dropped and the grid is the box of the rest (``grid_for`` with ``pad``).  With
    ``extent`` (finite points the caller already has) the grid is their box and every row of ``pts`` is sorted: a row that is
    not finite or lies outside the box has key INT64_MAX and sorts last.  No finite row, or an empty ``extent``: an empty cloud on
    a grid of one cell.  ``stable``: rows of one cell keep their order (torch.sort's default does not promise it)."""
    rows = None                                        # the rows of pts that are sorted; None: all of them
    if extent is None:
        rows = torch.nonzero(torch.isfinite(pts).all(1)).squeeze(1)
        pts = extent = pts[rows]
    if extent.shape[0] == 0:
        e = torch.zeros((0,), device=pts.device, dtype=torch.int64)
        return SortedCloud(pts[:0], e, e, CloudGrid((0.0, 0.0, 0.0), (1, 1, 1), float(edge)))
    grid = grid_for(extent, edge, what, pad)
    keys, perm = torch.sort(ops.cloud_cell_keys(pts, grid), stable=stable)
    return SortedCloud(pts[perm].contiguous(), keys, perm if rows is None else rows[perm], grid)


def two_grid_plan(cap: float, fine: float) -> TwoGridPlan:
    """how a search up to ``cap`` over cells of ``fine`` is split: ``FINE_RINGS`` rings on the fine grid, then what is unsettled
    goes on with a grid of cap / ``COARSE_SHARE`` (at least the fine edge) whose rings reach ``cap``; no coarse grid when the
    fine one's rings reach ``cap`` by themselves"""
    full = max_ring(cap, fine)
    if full <= FINE_RINGS:
        return TwoGridPlan(full, None, 0)
    coarse = max(cap / COARSE_SHARE, fine)
    return TwoGridPlan(FINE_RINGS, coarse, max_ring(cap, coarse))

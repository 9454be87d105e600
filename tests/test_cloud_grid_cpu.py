"""The host side of the cloud searches' grid (itermvs_amd/cloud_grid.py) without a GPU: the two-grid plan against values worked
out by hand from its rule, the ring count's defining property, and the box arithmetic of ``grid_for`` on CPU tensors."""
import math

import numpy as np
import pytest
import torch

from itermvs_amd import cloud_grid as CG


def reaches(rings, cap, edge):
    """the defining property of max_ring: ``rings`` is the first ring whose lower bound reaches ``cap``"""
    return (rings - 1) * edge * CG.RING_SHRINK >= cap > (rings - 2) * edge * CG.RING_SHRINK


# cap, fine edge -> fine rings, coarse edge, coarse rings.  By hand: full = the first r with (r - 1) * fine * (1 - 2^-20) >= cap,
# i.e. ceil(cap / fine) + 2 for these integer ratios (the shrink costs one ring): 3, 4, 6, 62, 8.  Up to FINE_RINGS = 4 there is
# no coarse grid; beyond, coarse = max(cap / 8, fine) and its rings follow the same rule: 4 / 1 -> 6, 60 / 7.5 -> 10, 60 / 10 -> 8.
PLANS = [
    (1.0, 1.0, (3, None, 0)),
    (2.0, 1.0, (4, None, 0)),
    (4.0, 1.0, (4, 1.0, 6)),
    (60.0, 1.0, (4, 7.5, 10)),
    (60.0, 10.0, (4, 10.0, 8)),            # cap / 8 = 7.5 is below the fine edge: the coarse grid keeps the fine edge
]


@pytest.mark.parametrize("cap,fine,want", PLANS)
def test_two_grid_plan_equals_the_rule_worked_by_hand(cap, fine, want):
    plan = CG.two_grid_plan(cap, fine)
    assert tuple(plan) == want and (plan.fine_rings, plan.coarse_edge, plan.coarse_rings) == want
    assert CG.FINE_RINGS == 4 and CG.COARSE_SHARE == 8.0
    full = CG.max_ring(cap, fine)
    assert reaches(full, cap, fine)
    assert plan.fine_rings == min(full, 4)
    if plan.coarse_edge is not None:
        assert reaches(plan.coarse_rings, cap, plan.coarse_edge)


def test_max_ring_is_the_first_ring_whose_bound_reaches_the_cap():
    for cap, edge in ((60.0, 1.0), (60.0, 7.5), (4.0, 1.0), (1.0, 3.0)):
        r = CG.max_ring(cap, edge)
        assert (r - 1) * edge * CG.RING_SHRINK >= cap > (r - 2) * edge * CG.RING_SHRINK
    assert CG.MAX_CELL_DIM == 1 << 21 and CG.RING_SHRINK == 1.0 - 1.0 / 1048576.0          # cloud_grid.hpp's constants


@pytest.mark.parametrize("edge,pad", [(0.37, 0.0), (0.37, 0.185), (3.0, 0.0), (0.011, 0.0055)])
def test_grid_for_is_the_hand_written_box(edge, pad):
    pts = torch.from_numpy(np.random.default_rng(5).uniform(-3.0, 7.0, (257, 3)).astype(np.float32))
    lo, hi = pts.numpy().min(0).astype(np.float64), pts.numpy().max(0).astype(np.float64)
    origin = lo - pad
    dims = [int(math.floor((hi[a] - origin[a]) / edge)) + 1 for a in range(3)]
    grid = CG.grid_for(pts, edge, "test", pad)
    assert grid.origin == tuple(float(v) for v in origin) and grid.dims == tuple(dims) and grid.edge == edge
    assert all(isinstance(v, float) for v in grid.origin) and all(isinstance(d, int) for d in grid.dims)
    if pad == 0.0:
        assert grid == CG.grid_for(pts, edge, "test")


def test_grid_for_one_point_and_the_key_limit():
    one = torch.tensor([[1.5, -2.0, 0.25]])
    assert CG.grid_for(one, 0.1, "test") == CG.CloudGrid((1.5, -2.0, 0.25), (1, 1, 1), 0.1)
    assert CG.grid_for(one, 0.1, "test", 0.05).dims == (1, 1, 1)
    fits = torch.tensor([[0.0, 0.0, 0.0], [float(2 ** 21) - 0.5, 1.0, 1.0]])                # floor(2^21 - 0.5) + 1 = 2^21 cells
    assert CG.grid_for(fits, 1.0, "test").dims == (1 << 21, 2, 2)
    over = torch.tensor([[0.0, 0.0, 0.0], [1.0, float(2 ** 21), 1.0]])                      # 2^21 + 1 cells on y
    with pytest.raises(ValueError):
        CG.grid_for(over, 1.0, "test")


def test_floor_edge_and_the_device_check():
    assert CG.floor_edge(0.5, 100.0) == 0.5
    assert CG.floor_edge(1e-9, float(1 << 20)) == 1.0                                        # side / 2^20 cells
    with pytest.raises(RuntimeError, match="no CPU path"):
        CG.points("test", torch.zeros(4, 3))
